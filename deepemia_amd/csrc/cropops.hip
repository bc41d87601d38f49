// Crop-framed mask sets: the stages after the tile -> global mapping (inference.py:2399-2472, 2552-2719;
// spatial_constraints.py:143,186) on masks kept in the GLOBAL frame as (room, cropped packed words) instead of full-frame
// planes [M, H, W/32] -- one 8192^2 plane is 8 MiB, a mask's room a few hundred words.
//
// Layout (that of demia_mask_crop_pack): mask m owns the rectangle room[m] = (y0, x0, y1, x1), inclusive, -1 = empty; its
// words are rows y0 .. y1 x word columns (x0 >> 5) .. (x1 >> 5) of the GLOBAL word grid, row-major at payload[offsets[m]].
// Bit (x & 31) of word (x >> 5), as in the planes: two sets over one frame share the word alignment, so |a & b| needs
// no shifts.  bbox[m] is the TIGHT box (inside the room); bits outside it and beyond column W - 1 are zero.
//
// Here: what exists only for crops -- placing tile masks into rooms, moving rooms between sets, and storing a mask for another room.  The stages that only READ
// a set (pair counts, gray histogram, pooled unpack) are the plane kernels of maskops.hip instantiated for
// mwords::CropWords (maskwords.h), the contour trace is contours.hip's CropContourP.
#include "common.h"
#include "maskwords.h"

namespace {

using mwords::CropWords;

// ---- tile mask -> room of the global frame: place_tile_kernel's nearest resize + paste + clip (mwords::placed_word: the two
// are bit-identical at every scale), one workgroup per mask, area and tight box reduced on the way out.  Writes
// payload[offsets[m] .. + rows * cols) and nothing else.  One float64 index and one source-bit load per pixel: cheap next to the
// planes it replaces (a room is a few hundred words, place_tile_kernel walks H x W/32 words per mask), but not tuned -- a
// word-copy path for the identity resize is the obvious next step.
__global__ __launch_bounds__(256) void crop_place_kernel(const uint32_t* __restrict__ src, const int* __restrict__ x_off,
                                                         const int* __restrict__ y_off, int sh, int sw, int tile_h, int tile_w,
                                                         int H, int W, const int* __restrict__ room, const long* __restrict__ offsets,
                                                         uint32_t* __restrict__ payload, int* __restrict__ area, int* __restrict__ bbox) {
    __shared__ int s_area, s_y0, s_y1, s_x0, s_x1;
    const long m = blockIdx.x;
    const int tid = threadIdx.x;
    const mwords::View g = CropWords{payload, room, offsets}.view(m);
    if (tid == 0) { s_area = 0; s_y0 = 1 << 30; s_x0 = 1 << 30; s_y1 = -1; s_x1 = -1; }
    __syncthreads();
    const uint32_t* tile = src + m * sh * ((sw + 31) >> 5);
    const int xo = x_off[m], yo = y_off[m];
    uint32_t* dst = payload + offsets[m];
    int a = 0, y0 = 1 << 30, y1 = -1, x0 = 1 << 30, x1 = -1;
    for (int t = tid; t < g.rows * g.cols; t += 256) {
        const int ly = t / g.cols, lx = t - ly * g.cols;
        const int y = g.y0 + ly, wx = g.c0 + lx;
        const uint32_t bits = mwords::placed_word(tile, sh, sw, tile_h, tile_w, xo, yo, H, W, y, wx);
        dst[t] = bits;
        if (bits) {
            a += __popc(bits);
            y0 = min(y0, y); y1 = max(y1, y);
            x0 = min(x0, wx * 32 + __ffs((int)bits) - 1);
            x1 = max(x1, wx * 32 + 31 - __clz((int)bits));
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o, 64);
        y0 = min(y0, __shfl_down(y0, o, 64)); x0 = min(x0, __shfl_down(x0, o, 64));
        y1 = max(y1, __shfl_down(y1, o, 64)); x1 = max(x1, __shfl_down(x1, o, 64));
    }
    if ((tid & 63) == 0 && a) {
        atomicAdd(&s_area, a);
        atomicMin(&s_y0, y0); atomicMin(&s_x0, x0);
        atomicMax(&s_y1, y1); atomicMax(&s_x1, x1);
    }
    __syncthreads();
    if (tid == 0) {
        const bool e = s_area == 0;
        area[m] = s_area;
        reinterpret_cast<int4*>(bbox)[m] = e ? make_int4(-1, -1, -1, -1) : make_int4(s_y0, s_x0, s_y1, s_x1);
    }
}

// ---- dst[i] = src[index[i]]: the words of a room move as they are (the destination's room IS the source's) ----------
__global__ __launch_bounds__(256) void crop_gather_kernel(const uint32_t* __restrict__ src, const long* __restrict__ src_off,
                                                          const long* __restrict__ index, const int* __restrict__ dst_room,
                                                          const long* __restrict__ dst_off, uint32_t* __restrict__ dst) {
    const long i = blockIdx.x;
    const mwords::View g = CropWords{dst, dst_room, dst_off}.view(i);
    const uint32_t* s = src + src_off[index[i]];
    uint32_t* d = dst + dst_off[i];
    for (int t = threadIdx.x; t < g.rows * g.cols; t += 256) d[t] = s[t];
}

// ---- dst[i] = src[index[i]] stored for ANOTHER room: both rooms lie on the global word grid, so a destination word inside the
// source room is that source word and every other one is zero -- a dword copy with a stride change, no shifts.  The grid is
// masks x slabs of REROOM_SLAB destination words (a frame-filling 8192^2 mask is 2 M words: not one workgroup's job); a slab
// past the end of its mask's room has nothing to do.  Writes dst[dst_off[i] .. + rows * cols) and nothing else.
constexpr int REROOM_SLAB = 256 * 16;

__global__ __launch_bounds__(256) void crop_reroom_kernel(const uint32_t* __restrict__ src, const int* __restrict__ src_room,
                                                          const long* __restrict__ src_off, const long* __restrict__ index,
                                                          const int* __restrict__ dst_room, const long* __restrict__ dst_off,
                                                          uint32_t* __restrict__ dst) {
    const long i = blockIdx.x;
    const mwords::View d = CropWords{dst, dst_room, dst_off}.view(i);
    const int n = d.rows * d.cols;
    const int t0 = (int)blockIdx.y * REROOM_SLAB;
    if (t0 >= n) return;
    const mwords::View s = CropWords{src, src_room, src_off}.view(index ? index[i] : i);
    uint32_t* out = dst + dst_off[i];
    const int t1 = min(n, t0 + REROOM_SLAB);
    for (int t = t0 + threadIdx.x; t < t1; t += 256) {
        const int ly = t / d.cols, lx = t - ly * d.cols;
        const int sy = d.y0 + ly - s.y0, sx = d.c0 + lx - s.c0;
        out[t] = (sy >= 0 && sy < s.rows && sx >= 0 && sx < s.cols) ? s.p[(long)sy * s.cols + sx] : 0u;
    }
}

}  // namespace

extern "C" int demia_crop_place_tiles(const uint32_t* src, const int32_t* x_off, const int32_t* y_off, int64_t M, int src_h, int src_w,
                                      int tile_h, int tile_w, int H, int W, const int32_t* room, const int64_t* offsets,
                                      uint32_t* payload, int32_t* area, int32_t* bbox, void* stream) {
    DEMIA_REQUIRE(M >= 0 && W > 0 && H > 0 && src_w > 0 && src_h > 0 && tile_w > 0 && tile_h > 0, "shapes");
    if (M == 0) return DEMIA_OK;
    DEMIA_REQUIRE(src && x_off && y_off && room && offsets && payload && area && bbox, "args");
    DEMIA_REQUIRE(M <= 0x7fffffffL, "M");
    hipLaunchKernelGGL(crop_place_kernel, dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, src, x_off, y_off, src_h, src_w, tile_h,
                       tile_w, H, W, room, reinterpret_cast<const long*>(offsets), payload, area, bbox);
    DEMIA_CHECK_LAUNCH("crop_place_kernel");
    return DEMIA_OK;
}

extern "C" int demia_crop_gather(const uint32_t* src, const int64_t* src_offsets, const int64_t* index, const int32_t* dst_room,
                                 const int64_t* dst_offsets, int64_t M, uint32_t* dst, void* stream) {
    DEMIA_REQUIRE(M >= 0, "M");
    if (M == 0) return DEMIA_OK;
    DEMIA_REQUIRE(src && src_offsets && index && dst_room && dst_offsets && dst, "args");
    DEMIA_REQUIRE(M <= 0x7fffffffL, "M");
    hipLaunchKernelGGL(crop_gather_kernel, dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, src,
                       reinterpret_cast<const long*>(src_offsets), reinterpret_cast<const long*>(index), dst_room,
                       reinterpret_cast<const long*>(dst_offsets), dst);
    DEMIA_CHECK_LAUNCH("crop_gather_kernel");
    return DEMIA_OK;
}

extern "C" int demia_crop_reroom(const uint32_t* src, const int32_t* src_room, const int64_t* src_offsets, const int64_t* index,
                                 const int32_t* dst_room, const int64_t* dst_offsets, int64_t M, int64_t max_dst_words, uint32_t* dst,
                                 void* stream) {
    DEMIA_REQUIRE(M >= 0 && max_dst_words >= 0, "M");
    if (M == 0 || max_dst_words == 0) return DEMIA_OK;
    DEMIA_REQUIRE(src && src_room && src_offsets && dst_room && dst_offsets && dst, "args");
    DEMIA_REQUIRE(src != dst, "src and dst must not alias");
    DEMIA_REQUIRE(M <= 0x7fffffffL, "M");
    const long slabs = (max_dst_words + REROOM_SLAB - 1) / REROOM_SLAB;
    DEMIA_REQUIRE(slabs <= 65535, "max_dst_words");
    hipLaunchKernelGGL(crop_reroom_kernel, dim3((unsigned)M, (unsigned)slabs), dim3(256), 0, (hipStream_t)stream, src, src_room,
                       reinterpret_cast<const long*>(src_offsets), reinterpret_cast<const long*>(index), dst_room,
                       reinterpret_cast<const long*>(dst_offsets), dst);
    DEMIA_CHECK_LAUNCH("crop_reroom_kernel");
    return DEMIA_OK;
}

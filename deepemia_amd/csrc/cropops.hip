// Crop-framed mask sets: the stages after the tile -> global mapping (inference.py:2399-2472, 2552-2719;
// spatial_constraints.py:143,186) on masks kept in the GLOBAL frame as (room, cropped packed words) instead of full-frame
// planes [M, H, W/32] -- one 8192^2 plane is 8 MiB, a mask's room a few hundred words.
//
// Layout (that of demia_mask_crop_pack): mask m owns the rectangle room[m] = (y0, x0, y1, x1), inclusive, -1 = empty; its
// words are rows y0 .. y1 x word columns (x0 >> 5) .. (x1 >> 5) of the GLOBAL word grid, row-major at payload[offsets[m]].
// Bit (x & 31) of word (x >> 5), as in the planes: two sets over one frame share the word alignment, so |a & b| needs
// no shifts.  bbox[m] is the TIGHT box (inside the room); bits outside it and beyond column W - 1 are zero.
#include "common.h"

namespace {

struct Room {
    int y0, c0, rows, cols;          // first row, first word column, extent (rows == 0: empty)
};

__device__ __forceinline__ Room room_of(const int* __restrict__ room, long m) {
    const int4 r = reinterpret_cast<const int4*>(room)[m];        // y0, x0, y1, x1
    Room g;
    g.y0 = r.x;
    g.c0 = r.y >> 5;
    g.rows = r.x < 0 ? 0 : r.z - r.x + 1;
    g.cols = r.x < 0 ? 0 : (r.w >> 5) - g.c0 + 1;
    return g;
}

// popcount(a & b) over the intersection of two tight boxes, each operand addressed with its own room stride; the lanes
// of ONE wave share the words (the caller reduces `c` over the wave).  The window is clipped to both rooms, so a box
// that is not inside its room cannot make a thread read outside its mask's words.
__device__ __forceinline__ int pair_count(const uint32_t* __restrict__ pa, const Room ra, const int4 ba,
                                          const uint32_t* __restrict__ pb, const Room rb, const int4 bb, int lane, int nlanes) {
    if (ba.x < 0 || bb.x < 0 || ra.rows == 0 || rb.rows == 0) return 0;
    const int y0 = max(max(ba.x, bb.x), max(ra.y0, rb.y0));
    const int y1 = min(min(ba.z, bb.z), min(ra.y0 + ra.rows, rb.y0 + rb.rows) - 1);
    const int x0 = max(ba.y, bb.y), x1 = min(ba.w, bb.w);
    if (y0 > y1 || x0 > x1) return 0;
    const int wx0 = max(x0 >> 5, max(ra.c0, rb.c0));
    const int wx1 = min(x1 >> 5, min(ra.c0 + ra.cols, rb.c0 + rb.cols) - 1);
    if (wx0 > wx1) return 0;
    const int rw = wx1 - wx0 + 1, rh = y1 - y0 + 1;
    const uint32_t* qa = pa + (long)(y0 - ra.y0) * ra.cols + (wx0 - ra.c0);
    const uint32_t* qb = pb + (long)(y0 - rb.y0) * rb.cols + (wx0 - rb.c0);
    int c = 0;
    for (int t = lane; t < rh * rw; t += nlanes) {
        const int ly = t / rw, lx = t - ly * rw;
        c += __popc(qa[(long)ly * ra.cols + lx] & qb[(long)ly * rb.cols + lx]);
    }
    return c;
}

// ---- tile mask -> room of the global frame: place_tile_kernel's nearest resize + paste + clip, one workgroup per mask,
// area and tight box reduced on the way out.  Writes payload[offsets[m] .. + rows * cols) and nothing else.
// The per-bit loop is place_tile_kernel's own (one float64 index and one source-bit load per pixel): it keeps the two kernels
// bit-identical at every scale and is cheap next to the planes it replaces (a room is a few hundred words, the twin walks
// H x W/32 words per mask), but it is not tuned -- a word-copy path for the identity resize is the obvious next step.
__global__ __launch_bounds__(256) void crop_place_kernel(const uint32_t* __restrict__ src, const int* __restrict__ x_off,
                                                         const int* __restrict__ y_off, int sh, int sw, int tile_h, int tile_w,
                                                         int H, int W, const int* __restrict__ room, const long* __restrict__ offsets,
                                                         uint32_t* __restrict__ payload, int* __restrict__ area, int* __restrict__ bbox) {
    __shared__ int s_area, s_y0, s_y1, s_x0, s_x1;
    const long m = blockIdx.x;
    const int tid = threadIdx.x;
    const Room g = room_of(room, m);
    if (tid == 0) { s_area = 0; s_y0 = 1 << 30; s_x0 = 1 << 30; s_y1 = -1; s_x1 = -1; }
    __syncthreads();
    const int swpr = (sw + 31) >> 5;
    const int xo = x_off[m], yo = y_off[m];
    uint32_t* dst = payload + offsets[m];
    const double fy = 1.0 / ((double)tile_h / (double)sh), fx = 1.0 / ((double)tile_w / (double)sw);
    int a = 0, y0 = 1 << 30, y1 = -1, x0 = 1 << 30, x1 = -1;
    for (int t = tid; t < g.rows * g.cols; t += 256) {
        const int ly = t / g.cols, lx = t - ly * g.cols;
        const int y = g.y0 + ly, wx = g.c0 + lx;
        const int ty = y - yo;
        uint32_t bits = 0u;
        if (y >= 0 && y < H && ty >= 0 && ty < tile_h) {
            const int sy = min((int)floor((double)ty * fy), sh - 1);
            const uint32_t* srow = src + ((long)m * sh + sy) * swpr;
            for (int bb = 0; bb < 32; ++bb) {
                const int x = wx * 32 + bb;
                if (x >= W) break;                                 // padding bits of the frame's last word stay 0
                const int tx = x - xo;
                if (x < 0 || tx < 0 || tx >= tile_w) continue;
                const int sx = min((int)floor((double)tx * fx), sw - 1);
                bits |= ((srow[sx >> 5] >> (sx & 31)) & 1u) << bb;
            }
        }
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
    const Room g = room_of(dst_room, i);
    const uint32_t* s = src + src_off[index[i]];
    uint32_t* d = dst + dst_off[i];
    for (int t = threadIdx.x; t < g.rows * g.cols; t += 256) d[t] = s[t];
}

// ---- |a_i & a_j| for EVERY pair of a segment: pair_matrix_kernel's contract and output layout on cropped words --------
__global__ __launch_bounds__(256) void crop_pair_matrix_kernel(const uint32_t* __restrict__ payload, const int* __restrict__ room,
                                                               const long* __restrict__ offsets, const int* __restrict__ bbox,
                                                               const int* __restrict__ first, const int* __restrict__ count,
                                                               const int* __restrict__ label, int* __restrict__ out, int ld) {
    const int i = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = first[i], end = f + count[i];
    const int4 bi = reinterpret_cast<const int4*>(bbox)[i];          // y0, x0, y1, x1
    if (bi.x < 0) return;
    const int li = label ? label[i] : 0;
    const Room ri = room_of(room, i);
    const uint32_t* pi = payload + offsets[i];
    for (int j = i + 1 + wave; j < end; j += 4) {
        if (j - f >= ld) break;
        if (label && label[j] != li) continue;
        const int4 bj = reinterpret_cast<const int4*>(bbox)[j];
        if (bj.x < 0 || max(bi.x, bj.x) > min(bi.z, bj.z) || max(bi.y, bj.y) > min(bi.w, bj.w)) continue;
        int c = pair_count(pi, ri, bi, payload + offsets[j], room_of(room, j), bj, lane, 64);
        for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
        if (lane == 0) out[(long)i * ld + (j - f)] = c;
    }
}

// ---- |a_i & b_j| for a list of pairs: block per pair ---------------------------------------------------------------
__global__ __launch_bounds__(256) void crop_pair_intersections_kernel(
    const uint32_t* __restrict__ pay_a, const int* __restrict__ room_a, const long* __restrict__ off_a, const int* __restrict__ bbox_a,
    const uint32_t* __restrict__ pay_b, const int* __restrict__ room_b, const long* __restrict__ off_b, const int* __restrict__ bbox_b,
    const int* __restrict__ pi, const int* __restrict__ pj, int* __restrict__ out) {
    __shared__ int acc;
    const int p = blockIdx.x;
    const int i = pi[p], j = pj[p];
    if (threadIdx.x == 0) acc = 0;
    __syncthreads();
    int c = pair_count(pay_a + off_a[i], room_of(room_a, i), reinterpret_cast<const int4*>(bbox_a)[i],
                       pay_b + off_b[j], room_of(room_b, j), reinterpret_cast<const int4*>(bbox_b)[j], threadIdx.x, 256);
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&acc, c);
    __syncthreads();
    if (threadIdx.x == 0) out[p] = acc;
}

// ---- masks [first, first + n) -> the slots 0 .. n - 1 of a plane pool that stays zero outside per-slot boxes: the rule of
// gather_regions_pooled_kernel (write the union of the slot's previous box and the new one, record the new one grown by
// `grow`).  The new box is the mask's TIGHT box (its words are zero outside it); words are read only inside its room.
__global__ __launch_bounds__(256) void crop_unpack_pooled_kernel(const uint32_t* __restrict__ payload, const int* __restrict__ room,
                                                                 const long* __restrict__ offsets, const int* __restrict__ bbox, long first,
                                                                 uint32_t* __restrict__ pool, int* __restrict__ prev, int H, int W, int grow) {
    const int s = blockIdx.x;
    const long m = first + s;
    const int wpr = (W + 31) >> 5;
    int4 nb = reinterpret_cast<const int4*>(bbox)[m];             // y0, x0, y1, x1 (inclusive), -1: empty
    const int4 pb = reinterpret_cast<const int4*>(prev)[s];
    __syncthreads();                                              // every thread has read prev before thread 0 rewrites it
    const Room g = room_of(room, m);
    bool has_n = nb.x >= 0 && g.rows > 0;
    if (has_n) {                                                  // a box never leaves the frame (nor a plane its pool)
        nb = make_int4(max(nb.x, 0), max(nb.y, 0), min(nb.z, H - 1), min(nb.w, W - 1));
        has_n = nb.x <= nb.z && nb.y <= nb.w;
    }
    const bool has_p = pb.x >= 0 && pb.x <= pb.z && pb.z < H && pb.y >= 0 && pb.y <= pb.w && pb.w < W;
    if (threadIdx.x == 0) {
        int4 q = make_int4(-1, -1, -1, -1);
        if (has_n) q = make_int4(max(nb.x - grow, 0), max(nb.y - grow, 0), min(nb.z + grow, H - 1), min(nb.w + grow, W - 1));
        reinterpret_cast<int4*>(prev)[s] = q;
    }
    if (!has_n && !has_p) return;
    const int ry0 = min(has_n ? nb.x : 1 << 30, has_p ? pb.x : 1 << 30), ry1 = max(has_n ? nb.z : -1, has_p ? pb.z : -1);
    const int c0 = min(has_n ? nb.y >> 5 : 1 << 30, has_p ? pb.y >> 5 : 1 << 30), c1 = max(has_n ? nb.w >> 5 : -1, has_p ? pb.w >> 5 : -1);
    const int nc0 = nb.y >> 5, nc1 = nb.w >> 5;
    const uint32_t* sp = payload + offsets[m];
    uint32_t* dp = pool + (long)s * H * wpr;
    const int cols = c1 - c0 + 1, rows = ry1 - ry0 + 1;
    for (int t = threadIdx.x; t < rows * cols; t += 256) {
        const int ry = ry0 + t / cols, cx = c0 + t % cols;
        const int ly = ry - g.y0, lx = cx - g.c0;
        const bool in = has_n && ry >= nb.x && ry <= nb.z && cx >= nc0 && cx <= nc1 && ly >= 0 && ly < g.rows && lx >= 0 && lx < g.cols;
        dp[(long)ry * wpr + cx] = in ? sp[(long)ly * g.cols + lx] : 0u;
    }
}

// ---- gray_hist_kernel (maskops.hip) on a room's words: same bins, same BGR -> gray fixed point.  One workgroup per mask over
// the words of its tight box that lie in its room; bits beyond column W - 1 are masked off before they index the image.
__global__ __launch_bounds__(256) void crop_gray_hist_kernel(const uint32_t* __restrict__ payload, const int* __restrict__ room,
                                                             const long* __restrict__ offsets, const int* __restrict__ bbox,
                                                             const uint8_t* __restrict__ img, int channels, int H, int W,
                                                             int* __restrict__ hist) {
    __shared__ int s_h[256];
    const long m = blockIdx.x;
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const int4 b4 = reinterpret_cast<const int4*>(bbox)[m];       // y0, x0, y1, x1
    const Room g = room_of(room, m);
    if (b4.x >= 0 && g.rows > 0) {
        const int ry0 = max(max(b4.x, 0), g.y0), ry1 = min(min(b4.z, H - 1), g.y0 + g.rows - 1);
        const int wx0 = max(max(b4.y, 0) >> 5, g.c0), wx1 = min(min(b4.w, W - 1) >> 5, g.c0 + g.cols - 1);
        const int rh = ry1 - ry0 + 1, rw = wx1 - wx0 + 1;
        const int last = (W - 1) >> 5;
        const uint32_t* src = payload + offsets[m];
        for (int i = threadIdx.x; i < rh * rw && rw > 0; i += blockDim.x) {
            const int ly = i / rw, lx = i - ly * rw;
            const int y = ry0 + ly, wx = wx0 + lx;
            uint32_t b = src[(long)(y - g.y0) * g.cols + (wx - g.c0)];
            if (wx == last && (W & 31)) b &= (1u << (W & 31)) - 1u;
            while (b) {
                const int bit = __ffs((int)b) - 1;
                b &= b - 1;
                const long px = (long)y * W + (wx << 5) + bit;
                int gr;
                if (channels == 3) {
                    const uint8_t* q = img + px * 3;
                    gr = (q[0] * 1868 + q[1] * 9617 + q[2] * 4899 + (1 << 13)) >> 14;
                } else {
                    gr = img[px];
                }
                atomicAdd(&s_h[gr], 1);
            }
        }
    }
    __syncthreads();
    hist[m * 256 + threadIdx.x] = s_h[threadIdx.x];
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

extern "C" int demia_crop_pair_matrix(const uint32_t* payload, const int32_t* room, const int64_t* offsets, const int32_t* bbox,
                                      const int32_t* first, const int32_t* count, const int32_t* label, int32_t* out, int64_t M, int ld,
                                      void* stream) {
    DEMIA_REQUIRE(M >= 0 && ld > 0, "shapes");
    if (M == 0) return DEMIA_OK;
    DEMIA_REQUIRE(payload && room && offsets && bbox && first && count && out, "args");
    DEMIA_REQUIRE(M <= 0x7fffffffL, "M");
    hipLaunchKernelGGL(crop_pair_matrix_kernel, dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, payload, room,
                       reinterpret_cast<const long*>(offsets), bbox, first, count, label, out, ld);
    DEMIA_CHECK_LAUNCH("crop_pair_matrix_kernel");
    return DEMIA_OK;
}

extern "C" int demia_crop_pair_intersections(const uint32_t* payload_a, const int32_t* room_a, const int64_t* offsets_a, const int32_t* bbox_a,
                                             const uint32_t* payload_b, const int32_t* room_b, const int64_t* offsets_b, const int32_t* bbox_b,
                                             const int32_t* pi, const int32_t* pj, int32_t* out, int64_t P, void* stream) {
    DEMIA_REQUIRE(P >= 0, "P");
    if (P == 0) return DEMIA_OK;
    DEMIA_REQUIRE(payload_a && room_a && offsets_a && bbox_a && payload_b && room_b && offsets_b && bbox_b && pi && pj && out, "args");
    DEMIA_REQUIRE(P <= 0x7fffffffL, "P");
    hipLaunchKernelGGL(crop_pair_intersections_kernel, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, payload_a, room_a,
                       reinterpret_cast<const long*>(offsets_a), bbox_a, payload_b, room_b, reinterpret_cast<const long*>(offsets_b), bbox_b,
                       pi, pj, out);
    DEMIA_CHECK_LAUNCH("crop_pair_intersections_kernel");
    return DEMIA_OK;
}

extern "C" int demia_crop_unpack_pooled(const uint32_t* payload, const int32_t* room, const int64_t* offsets, const int32_t* bbox,
                                        int64_t first, int64_t n, int H, int W, uint32_t* pool, int32_t* prev, int grow, void* stream) {
    DEMIA_REQUIRE(first >= 0 && n >= 0 && W > 0 && H > 0 && grow >= 0, "shapes");
    if (n == 0) return DEMIA_OK;
    DEMIA_REQUIRE(payload && room && offsets && bbox && pool && prev, "args");
    DEMIA_REQUIRE(n <= 0x7fffffffL, "n");
    hipLaunchKernelGGL(crop_unpack_pooled_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, payload, room,
                       reinterpret_cast<const long*>(offsets), bbox, (long)first, pool, prev, H, W, grow);
    DEMIA_CHECK_LAUNCH("crop_unpack_pooled_kernel");
    return DEMIA_OK;
}

extern "C" int demia_crop_gray_histogram(const uint32_t* payload, const int32_t* room, const int64_t* offsets, const int32_t* bbox,
                                         const uint8_t* image, int channels, int64_t M, int H, int W, int32_t* hist, void* stream) {
    DEMIA_REQUIRE(M >= 0 && W > 0 && H > 0 && (channels == 1 || channels == 3), "shapes");
    if (M == 0) return DEMIA_OK;
    DEMIA_REQUIRE(payload && room && offsets && bbox && image && hist, "args");
    DEMIA_REQUIRE(M <= 0x7fffffffL, "M");
    hipLaunchKernelGGL(crop_gray_hist_kernel, dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, payload, room,
                       reinterpret_cast<const long*>(offsets), bbox, image, channels, H, W, hist);
    DEMIA_CHECK_LAUNCH("crop_gray_hist_kernel");
    return DEMIA_OK;
}

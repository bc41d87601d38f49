// The boundary band of a packed mask (demia_mask_boundary_band / demia_crop_boundary_band; definition: include/deepemia_hip.h):
// band(m, d) = m & ~eroded(m, d), the erosion by the (2d + 1) x (2d + 1) square with everything outside the frame counting as 0.
// One kernel over a word source (maskwords.h), one workgroup per mask, on the words of the mask's box.
//
// The erosion is separable and runs on 32 pixels per lane-operation.  With n = 2d + 1, the AND over a window of n bits of a row is
// built by doubling: r[x] &= r[x + p] for p = 1, 2, 4, ... while 2p <= n makes r[x] the AND of the p pixels from x on; one more
// step with the offset n - p covers n of them, and reading it at x - d centres the window.  The last step and the centring are
// one pass: out[x] = r[x - d] & r[x - d + (n - p)].  Every pass makes a word from a funnel shift of two words of the pass before,
// so a pass reads one buffer and writes the other.  The same doubling over ROWS (whole words, no shift) finishes the square:
// about 2 log2(n) passes over the region in all, whatever d is.
//
// Every word outside the region is a zero operand and is never fetched; the region is the box, outside which the mask is zero,
// so a window that leaves the box, the frame or column W - 1 sees a zero as the definition asks.  A box narrower or lower than n
// holds no window at all: the band is the mask, copied and counted without a buffer.
//
// Where the two buffers P, Q live:
//   a region of at most wreg::LARGE_WORDS words   both in LDS
//   a larger one                                  P = the region's words of the OUTPUT (the last pass is elementwise, so the band
//                                                 may overwrite the eroded words it is made from), Q = scratch (planes: the same
//                                                 words of the mask's scratch plane; crops: the mask's share, sized from its room)
// Boolean word operations and popcounts only; plain vector stores.
#include "wordregion.h"

namespace {

using mwords::CropWords;
using mwords::PlaneWords;

constexpr int BAND_LDS = 2 * wreg::LARGE_WORDS * 4;

template <class S>
struct BandP {
    S src;
    const int* bbox;                 // [M, 4]
    uint32_t* out;                   // laid out like the source words; zero on entry
    int* band_area;                  // [M]
    uint32_t* scratch;               // planes: [M, H, wpr]; crops: the shares demia_crop_boundary_scratch sizes
    const long* scratch_off;         // crops: [M] words into scratch
    int H, W, d;
};

// rh x rw words, row-major with `stride`
struct Buf {
    uint32_t* p;
    int stride;
};

// Word lx of row ly of X read s pixels further on: bit b is pixel 32 * lx + b + s of the row, 0 where that lies outside the region.
__device__ __forceinline__ uint32_t shifted(const Buf X, int rw, int ly, int lx, int s) {
    const int a = lx + (s >> 5), t = s & 31;                 // (>> of a negative offset rounds down: the word that holds the pixel)
    const uint32_t* row = X.p + ly * X.stride;
    const uint32_t lo = (unsigned)a < (unsigned)rw ? row[a] : 0u;
    const uint32_t hi = t && (unsigned)(a + 1) < (unsigned)rw ? row[a + 1] : 0u;
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> t);
}

// Y[x] = X[x + s1] & X[x + s2] along the rows (pixel offsets), then a barrier
__device__ __forceinline__ void row_pass(const Buf X, const Buf Y, int rh, int rw, int s1, int s2) {
    const int n = rh * rw;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int ly = i / rw, lx = i - ly * rw;
        Y.p[ly * Y.stride + lx] = shifted(X, rw, ly, lx, s1) & shifted(X, rw, ly, lx, s2);
    }
    __syncthreads();
}

// Y[y] = X[y + s1] & X[y + s2] down the columns (row offsets), then a barrier
__device__ __forceinline__ void col_pass(const Buf X, const Buf Y, int rh, int rw, int s1, int s2) {
    const int n = rh * rw;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int ly = i / rw, lx = i - ly * rw;
        const int y1 = ly + s1, y2 = ly + s2;
        const uint32_t a = (unsigned)y1 < (unsigned)rh ? X.p[y1 * X.stride + lx] : 0u;
        const uint32_t b = (unsigned)y2 < (unsigned)rh ? X.p[y2 * X.stride + lx] : 0u;
        Y.p[ly * Y.stride + lx] = a & b;
    }
    __syncthreads();
}

template <class S>
__global__ __launch_bounds__(256) void boundary_band_kernel(const BandP<S> p) {
    constexpr bool PLANE = std::is_same<S, PlaneWords>::value;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    __shared__ long long s_red[wreg::WAVES];
    const int tid = threadIdx.x, nt = blockDim.x;
    const long m = blockIdx.x;
    const int wpr = (p.W + 31) >> 5;
    const mwords::View v = p.src.view(m);
    const int4 b = reinterpret_cast<const int4*>(p.bbox)[m];
    int y0, y1, c0, c1;
    if (!mwords::clipped_box(v, b, p.H, p.W, y0, y1, c0, c1)) {          // block-uniform
        if (tid == 0) p.band_area[m] = 0;
        return;
    }
    const int rh = y1 - y0 + 1, rw = c1 - c0 + 1, n = rh * rw;
    // the region's words of the source and of the output: both inside the view, which is the whole plane or the mask's room
    long base;
    if constexpr (PLANE) base = m * (long)p.H * wpr;
    else base = p.src.offsets[m];
    const long first = (long)(y0 - v.y0) * v.cols + (c0 - v.c0);
    const uint32_t* A = v.p + first;
    uint32_t* O = p.out + base + first;
    const int astride = v.cols;
    const uint32_t last_valid = (p.W & 31) ? ((1u << (p.W & 31)) - 1u) : 0xFFFFFFFFu;
    const int last_lx = wpr - 1 - c0;                                     // the region's column that holds the padding bits, if any
    const int win = 2 * p.d + 1;
    const int bw = min(b.w, p.W - 1) - max(b.y, 0) + 1, bh = min(b.z, p.H - 1) - max(b.x, 0) + 1;
    long long cnt[1] = {0};
    if (win > bw || win > bh) {
        // no window fits the box: nothing survives the erosion and the band is the mask
        for (int i = tid; i < n; i += nt) {
            const int ly = i / rw, lx = i - ly * rw;
            const uint32_t w = A[(long)ly * astride + lx] & (lx == last_lx ? last_valid : 0xFFFFFFFFu);
            O[(long)ly * astride + lx] = w;
            cnt[0] += __popc(w);
        }
    } else {
        Buf X, Y;
        if (n <= wreg::LARGE_WORDS) {
            X = Buf{smem, rw};
            Y = Buf{smem + wreg::LARGE_WORDS, rw};
        } else if constexpr (PLANE) {
            X = Buf{O, astride};
            Y = Buf{p.scratch + base + first, astride};
        } else {
            X = Buf{O, astride};
            Y = Buf{p.scratch + p.scratch_off[m], rw};
        }
        for (int i = tid; i < n; i += nt) {
            const int ly = i / rw, lx = i - ly * rw;
            X.p[ly * X.stride + lx] = A[(long)ly * astride + lx] & (lx == last_lx ? last_valid : 0xFFFFFFFFu);
        }
        __syncthreads();
        int have = 1;
        for (; 2 * have <= win; have *= 2) {
            row_pass(X, Y, rh, rw, 0, have);
            const Buf t = X; X = Y; Y = t;
        }
        row_pass(X, Y, rh, rw, -p.d, win - have - p.d);
        { const Buf t = X; X = Y; Y = t; }
        for (have = 1; 2 * have <= win; have *= 2) {
            col_pass(X, Y, rh, rw, 0, have);
            const Buf t = X; X = Y; Y = t;
        }
        col_pass(X, Y, rh, rw, -p.d, win - have - p.d);
        // Y is the eroded mask.  Elementwise: where Y is the output's own words, a thread reads its word before it writes it.
        for (int i = tid; i < n; i += nt) {
            const int ly = i / rw, lx = i - ly * rw;
            const uint32_t a = A[(long)ly * astride + lx] & (lx == last_lx ? last_valid : 0xFFFFFFFFu);
            const uint32_t w = a & ~Y.p[ly * Y.stride + lx];
            O[(long)ly * astride + lx] = w;
            cnt[0] += __popc(w);
        }
    }
    wreg::block_sum(cnt, s_red);
    if (tid == 0) p.band_area[m] = (int)cnt[0];
}

}  // namespace

// what both entries require, around the arguments that are the entry's own
#define BAND_REQUIRE(own_args)                                                                                                \
    DEMIA_REQUIRE(M >= 0 && M < (1L << 31) && H > 0 && W > 0, "shapes");                                                      \
    DEMIA_REQUIRE(d >= 1 && d < (1 << 24), "d");                                                                              \
    if (M == 0) return DEMIA_OK;                                                                                              \
    DEMIA_REQUIRE((own_args) && bbox && band && band_area && scratch, "args");                                                \
    DEMIA_REQUIRE((long)H * ((W + 31) >> 5) < (1L << 26), "sizes") /* the words of a region fit the loops' arithmetic */

extern "C" int demia_mask_boundary_band(const uint32_t* masks, const int32_t* bbox, int64_t M, int H, int W, int d, uint32_t* band,
                                        int32_t* band_area, uint32_t* scratch, void* stream) {
    BAND_REQUIRE(masks && masks != band && masks != scratch && band != scratch);
    BandP<PlaneWords> p{PlaneWords{masks, H, (W + 31) >> 5, nullptr}, bbox, band, band_area, scratch, nullptr, H, W, d};
    return wreg::launch<boundary_band_kernel<PlaneWords>>(p, (unsigned)M, BAND_LDS, (hipStream_t)stream, "boundary_band_kernel");
}

// Words of scratch the bands of a crop-framed set need, from the host's room table alone: a mask whose ROOM has more words than the
// large buffer (an upper bound of the region of its box) gets as many at off[m].
extern "C" int64_t demia_crop_boundary_scratch(const int32_t* room_host, int64_t M, int H, int W, int64_t* scratch_off) {
    int64_t total = 0;
    for (int64_t m = 0; m < M; ++m) {
        const int32_t* r = room_host + 4 * m;
        scratch_off[m] = total;
        if (r[0] < 0) continue;
        const int64_t words = (int64_t)(r[2] - r[0] + 1) * ((r[3] >> 5) - (r[1] >> 5) + 1);
        if (words > wreg::LARGE_WORDS) total += words;
    }
    return total;
}

extern "C" int demia_crop_boundary_band(const uint32_t* payload, const int32_t* room, const int64_t* offsets, const int32_t* bbox,
                                        int64_t M, int H, int W, int d, uint32_t* band, int32_t* band_area, uint32_t* scratch,
                                        const int64_t* scratch_off, void* stream) {
    BAND_REQUIRE(payload && room && offsets && scratch_off && payload != band);
    BandP<CropWords> p{CropWords{payload, room, reinterpret_cast<const long*>(offsets)}, bbox, band, band_area, scratch,
                       reinterpret_cast<const long*>(scratch_off), H, W, d};
    return wreg::launch<boundary_band_kernel<CropWords>>(p, (unsigned)M, BAND_LDS, (hipStream_t)stream, "boundary_band_kernel<crop>");
}

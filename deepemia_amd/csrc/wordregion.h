// The region STAGE of the kernels that measure on the packed words of a mask (inscribed.hip, skeleton.hip; the reductions and
// the launch also serve neighbours.hip): one workgroup of 256 threads per mask, over a word source (maskwords.h), on the region
// machinery of maskregion.h.  What such kernels have in common is stated here ONCE: the buffer size that decides where a region
// lives and its host sizer, the clip / region / placement / staging of a mask (stage), the component of a contour (component),
// the block reductions and the launch.
#pragma once
#include <type_traits>
#include "common.h"
#include "maskregion.h"
#include "maskwords.h"

namespace wreg {

// Words of the large region buffer.  A region whose PADDED size pn = (rh + 2) * (rw + 2) -- the tracer's image with its zero ring,
// the unit of its rule -- fits lives in LDS; a larger one lives in memory, for crops in shares of the caller's scratch that the
// host sizes by the same rule.
constexpr int LARGE_WORDS = 8192;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int COLS = 8;                                      // values per contour in `out`

// dynamic LDS of a kernel with K work buffers, in words: A and the K buffers; what follows is the kernel's own
constexpr int lds_words(int K) { return (K + 1) * LARGE_WORDS; }

// Words of scratch a crop-framed set needs for `buffers` padded regions per large mask, from the host's room table alone: a mask
// whose ROOM's region (+ 1 ring, clipped to the frame: an upper bound of the region of its tight box) exceeds the large buffer gets
// them at off[m].
inline int64_t room_scratch_words(const int32_t* room_host, int64_t M, int H, int W, int buffers, int64_t* off) {
    int64_t total = 0;
    for (int64_t m = 0; m < M; ++m) {
        const int32_t* r = room_host + 4 * m;
        off[m] = total;
        if (r[0] < 0) continue;
        int ry0, wx0, rh, rw;
        mreg::region_of(r[0], r[1], r[2], r[3], 1, H, W, ry0, wx0, rh, rw);
        const int64_t pn = (int64_t)(rh + 2) * (rw + 2);
        if (pn > LARGE_WORDS) total += buffers * pn;
    }
    return total;
}

// ---- block reductions over the THREADS threads.  s: WAVES slots of LDS per value.  Each ends with a barrier behind its reads, so
// the slots -- and whatever buffer the caller read to make its value -- are free when it returns.  Integers only: any order gives
// the same bits.

// a[j] <- the sum of a[j] over the workgroup, in THREAD 0 (every use writes one row of results from there; combining the wave sums
// in every thread holds WAVES x N more values in registers beside the caller's)
template <int N>
__device__ __forceinline__ void block_sum(long long (&a)[N], long long* s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < N; ++j)
        for (int d = 32; d > 0; d >>= 1) a[j] += __shfl_xor(a[j], d, 64);
    if (lane == 0)
        for (int j = 0; j < N; ++j) s[wave * N + j] = a[j];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < WAVES; ++w)
            for (int j = 0; j < N; ++j) a[j] += s[w * N + j];
    __syncthreads();
}

// the minimum / the maximum of v over the workgroup, in every thread
__device__ __forceinline__ long long block_min(long long v, long long* s) {
    for (int d = 32; d > 0; d >>= 1) v = min(v, (long long)__shfl_xor(v, d, 64));
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    long long r = s[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r = min(r, s[w]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ unsigned long long block_max(unsigned long long v, long long* s) {
    for (int d = 32; d > 0; d >>= 1) v = max(v, (unsigned long long)__shfl_xor(v, d, 64));
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = (long long)v;
    __syncthreads();
    unsigned long long r = (unsigned long long)s[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r = max(r, (unsigned long long)s[w]);
    __syncthreads();
    return r;
}

// What a kernel on this stage is given; its own parameters derive from it.
template <class S>
struct Params {
    S src;
    const int* select;           // [M] or NULL: position t reads the words of mask select[t]
    uint32_t* scratch;           // planes: one plane per mask; crops: the tracer's scratch
    const long* scratch_off;     // crops: [set] words into scratch (demia_crop_contour_scratch)
    uint32_t* scratch2;          // K == 2.  planes: one more plane per mask; crops: one more padded region per large room
    const long* scratch2_off;    // crops: [set] words into scratch2 (demia_crop_skeleton_scratch)
    const int* bbox;             // [M, 4]
    const int* count;            // [M] (not read where out == NULL)
    const int* info;             // [M, C, 4]
    int H, W, C;
    double um;
    double* out;                 // [M, out_c, COLS], or NULL: nothing to measure
    int out_c;
};

// The staged region of the workgroup's mask: rows ry0 .. ry0 + rh - 1 x word columns wx0 .. wx0 + rw - 1 of the frame, row-major
// with `stride` at A (the mask, which stays as it is) and at each B[k].  Everything outside the region is background: the ring
// is, and where the region ends on the frame the definitions say so.
template <int K>
struct Stage {
    long mw;                     // the mask whose words these are
    mwords::View v;
    int nc;                      // contours to measure
    const int4* info;            // theirs: sx, sy, npts, offset
    double* out;                 // their rows
    int ry0, wx0, rh, rw, n, stride;
    const uint32_t* A;
    uint32_t* B[K];
};

// Position t of the launch: zeroes the output rows no contour fills, and stages the region unless there is nothing to do -- an empty
// mask, or no contour and not `always` (false is returned; block-uniform).  The three homes:
//   LDS (pn <= LARGE_WORDS)   A at smem, B[k] at smem + (k + 1) * LARGE_WORDS
//   planes beyond that        A is the plane itself, read in place; B[k] the same words of the k-th scratch plane; stride = wpr
//   crops beyond that         A staged at scratch + scratch_off[mw], B[0] behind it at + pn, B[1] at scratch2 + scratch2_off[mw]
// The staged words are written, not yet synchronised: the caller's first barrier does that (component() starts with one).
template <int K, class S>
__device__ __forceinline__ bool stage(const Params<S>& p, const long t, const bool always, uint32_t* smem, Stage<K>& g) {
    static_assert(K == 1 || K == 2, "one scratch per work buffer");
    constexpr bool PLANE = std::is_same<S, mwords::PlaneWords>::value;
    const int tid = threadIdx.x, nt = blockDim.x;
    const long mw = p.select ? p.select[t] : t;
    const int wpr = (p.W + 31) >> 5;
    const mwords::View v = p.src.view(mw);
    const int4 b4 = reinterpret_cast<const int4*>(p.bbox)[t];
    int y0 = max(b4.x, 0), x0 = max(b4.y, 0), y1 = min(b4.z, p.H - 1), x1 = min(b4.w, p.W - 1);
    if constexpr (!PLANE) {
        // the box is inside the room by contract; clipped to it, the region lies inside the ROOM's region, which is what the
        // host sized the scratches from (as the tracer does)
        const int4 r = reinterpret_cast<const int4*>(p.src.room)[mw];
        y0 = max(y0, r.x); x0 = max(x0, r.y); y1 = min(y1, r.z); x1 = min(x1, r.w);
    }
    const bool empty = b4.x < 0 || v.rows == 0 || y0 > y1 || x0 > x1;
    g.mw = mw; g.v = v;
    g.nc = 0;
    g.info = nullptr;
    g.out = nullptr;
    if (p.out) {
        g.info = reinterpret_cast<const int4*>(p.info) + t * p.C;
        g.out = p.out + t * p.out_c * COLS;
        g.nc = empty ? 0 : min(max(p.count[t], 0), min(p.out_c, p.C));
        for (int i = g.nc * COLS + tid; i < p.out_c * COLS; i += nt) g.out[i] = 0.0;
    }
    if (empty || (g.nc == 0 && !always)) return false;
    mreg::region_of(y0, x0, y1, x1, 1, p.H, p.W, g.ry0, g.wx0, g.rh, g.rw);
    const int pn = (g.rh + 2) * (g.rw + 2);
    g.n = g.rh * g.rw;
    g.stride = g.rw;
    g.A = nullptr;
    uint32_t* staged = nullptr;
    if (pn <= LARGE_WORDS) {
        staged = smem;
        for (int k = 0; k < K; ++k) g.B[k] = smem + (k + 1) * LARGE_WORDS;
    } else if constexpr (PLANE) {
        uint32_t* const planes[2] = {p.scratch, p.scratch2};
        const long o = (long)g.ry0 * wpr + g.wx0;
        g.A = v.p + o;
        for (int k = 0; k < K; ++k) g.B[k] = planes[k] + mw * p.H * wpr + o;
        g.stride = wpr;
    } else {
        staged = p.scratch + p.scratch_off[mw];
        g.B[0] = staged + pn;
        if constexpr (K == 2) g.B[1] = p.scratch2 + p.scratch2_off[mw];
    }
    if (staged) {
        // a word of the region outside the view (the ring of a box on the room's edge) is zero and is NEVER fetched: behind
        // a room lie the next mask's words
        for (int i = tid; i < g.n; i += nt) {
            const int ly = i / g.rw, lx = i - ly * g.rw;
            const int vy = g.ry0 + ly - v.y0, vx = g.wx0 + lx - v.c0;
            const bool in = (unsigned)vy < (unsigned)v.rows && (unsigned)vx < (unsigned)v.cols;
            staged[i] = in ? v.p[(long)vy * v.cols + vx] : 0u;
        }
        g.A = staged;
    }
    return true;
}

// The component of contour c (c < g.nc) into g.B[0]: clear, plant the contour's seed, mreg::flood<true> through A.  Block-uniform;
// false: the seed is not a pixel of A -- not a trace of these words -- and the contour's row is zero.
//
// Safe to call in a loop, and behind any work of the caller's on the buffers, because it STARTS with a barrier: whatever a thread
// read from B[0] for the contour before (or wrote there, or to A's staged home) it did before it arrived here, so no clear
// overtakes a reader.  The flood leaves s_changed behind a barrier of its own, and the block reductions leave their slots behind
// theirs, so neither is still being read when the next contour writes it.  The barrier at the end publishes the component.
template <int K>
__device__ __forceinline__ bool component(const Stage<K>& g, const int c, int* s_changed) {
    const int tid = threadIdx.x, nt = blockDim.x;
    uint32_t* B = g.B[0];
    const int4 inf = g.info[c];
    const int ly = inf.y - g.ry0, px = inf.x - 32 * g.wx0;
    __syncthreads();
    for (int i = tid; i < g.n; i += nt) B[(i / g.rw) * g.stride + i % g.rw] = 0u;
    __syncthreads();
    const bool ok = (unsigned)ly < (unsigned)g.rh && (unsigned)px < (unsigned)(32 * g.rw) && ((g.A[ly * g.stride + (px >> 5)] >> (px & 31)) & 1u);
    if (!ok) {
        if (tid < COLS) g.out[c * COLS + tid] = 0.0;
        return false;
    }
    if (tid == 0) B[ly * g.stride + (px >> 5)] = 1u << (px & 31);
    __syncthreads();
    mreg::flood<true>(g.A, 0u, B, g.stride, g.rh, g.rw, s_changed);
    __syncthreads();
    return true;
}

// Launches Kern (a __global__ over P) with `lds` bytes of dynamic LDS, raising the kernel's limit when the request grows.
template <auto Kern, class P>
int launch(const P& p, unsigned grid, int lds, hipStream_t st, const char* name) {
    static int lds_set = 0;                                  // per instantiation, so per kernel
    if (lds > lds_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        lds_set = lds;
    }
    hipLaunchKernelGGL(Kern, dim3(grid), dim3(THREADS), lds, st, p);
    DEMIA_CHECK_LAUNCH(name);
    return DEMIA_OK;
}

}  // namespace wreg

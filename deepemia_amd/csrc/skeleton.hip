// Morphological skeleton and its descriptors per external contour (demia_mask_skeleton / demia_crop_skeleton; definition:
// include/deepemia_hip.h).  One kernel over a word source (maskwords.h), one workgroup per mask, the region machinery of
// maskregion.h as it is -- the second measurement on the mask WORDS, built like the first (inscribed.hip).
//
// Per mask the region (tight box + 1 ring, clipped to the frame; mreg::region_of) is staged as the inscribed kernel stages it.
// Three buffers of the region: A, the mask, which stays as it is, and P, Q, which the thinning plays ping-pong in -- in LDS up to
// the tracer's large buffer; beyond it the planes read A in place and work in two scratch planes, the crops stage A and P in the
// tracer's share and Q in a share of a second scratch.  Everything outside the region is background: the ring is, and where the
// region ends on the frame the definition says so.
//
// Thinning (Guo-Hall A1) is a Boolean function of a pixel's 3 x 3 neighbourhood, so it runs on 32 pixels per lane-operation:
// lane = WORD, the eight neighbour planes of a word come from the three rows and the carry bits of the words left and right of
// them, and C == 1, 2 <= min(N1, N2) <= 3 are Boolean expressions of bit-sliced sums.  A sub-iteration reads one buffer and writes
// the other, so every pixel sees the state before it; a pair after the first works on the window of words that can still change
// (the rectangle the pair before it changed, grown by two).  Then per contour: mreg::flood<true> of its component K into P, and six
// popcount reductions over S & K.  Integer sums do not depend on which thread saw which word.  No per-pixel loop, no f32, plain
// vector stores.
#include <type_traits>
#include "common.h"
#include "maskregion.h"
#include "maskwords.h"

namespace {

using mwords::CropWords;
using mwords::PlaneWords;

constexpr int SKEL_COLS = 8;
constexpr int SKEL_WORDS = 8192;        // LDS words per region buffer: the tracer's TRACE_WORDS (contours.hip) -- its scratch contract
constexpr int SKEL_LDS = 3 * SKEL_WORDS * 4;

template <class S>
struct SkelP {
    S src;
    const int* select;           // [M] or NULL: position t reads the words of mask select[t]
    uint32_t* scratch;           // the tracer's scratch
    const long* scratch_off;     // crops: [set] words into scratch (demia_crop_contour_scratch)
    uint32_t* scratch2;          // planes: one more plane per mask; crops: one more padded region per large room
    const long* scratch2_off;    // crops: [set] words into scratch2 (demia_crop_skeleton_scratch)
    const int* bbox;             // [M, 4]
    const int* count;            // [M] or NULL (with out == NULL: thin only)
    const int* info;             // [M, C, 4]
    int H, W, C;
    double um;
    double* out;                 // [M, out_c, 8] or NULL
    int out_c;
    uint32_t* skel_out;          // NULL, or laid out like the source words
};

// The eight neighbour planes of word (ly, lx) of X, named as the definition names them (y downwards): p2 = N, p3 = NE, p4 = E,
// p5 = SE, p6 = S, p7 = SW, p8 = W, p9 = NW.  Bit b of a word is pixel 32 * lx + b, so the EAST neighbour of every pixel of a row
// word r is (r >> 1) with bit 0 of the word to its right carried into bit 31, the WEST neighbour (r << 1) with bit 31 of the word
// to its left carried into bit 0.  Words outside the region are background.
struct Nb {
    uint32_t p2, p3, p4, p5, p6, p7, p8, p9;
};

__device__ __forceinline__ Nb neighbours(const uint32_t* X, int stride, int rh, int rw, int ly, int lx, uint32_t mid) {
    const bool up = ly > 0, dn = ly < rh - 1, lf = lx > 0, rt = lx < rw - 1;
    const uint32_t* r = X + ly * stride + lx;
    const uint32_t u = up ? r[-stride] : 0u, d = dn ? r[stride] : 0u;
    const uint32_t ul = up && lf ? r[-stride - 1] : 0u, ur = up && rt ? r[-stride + 1] : 0u;
    const uint32_t ml = lf ? r[-1] : 0u, mr = rt ? r[1] : 0u;
    const uint32_t dl = dn && lf ? r[stride - 1] : 0u, dr = dn && rt ? r[stride + 1] : 0u;
    Nb n;
    n.p2 = u;
    n.p3 = (u >> 1) | (ur << 31);
    n.p4 = (mid >> 1) | (mr << 31);
    n.p5 = (d >> 1) | (dr << 31);
    n.p6 = d;
    n.p7 = (d << 1) | (dl >> 31);
    n.p8 = (mid << 1) | (ml >> 31);
    n.p9 = (u << 1) | (ul >> 31);
    return n;
}

// at least two of four
__device__ __forceinline__ uint32_t ge2of4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return (a & b) | (c & d) | ((a | b) & (c | d)); }

// A window of the region's words, rows y0 .. y1 x word columns x0 .. x1, inclusive (y1 < y0: empty).
struct Win {
    int y0, y1, x0, x1;
};

// One sub-iteration over the window w of the region: Y <- X less the pixels it deletes, for the words of w.  c grows to hold the
// words in which this thread deleted a pixel.  (All nine words are asked for together, and X and Y are different buffers, so the
// loads of one trip need not wait for the store of the trip before: in the scratch path a trip is one round to memory.)
template <int SUB>
__device__ __forceinline__ void thin_pass(const uint32_t* __restrict__ X, uint32_t* __restrict__ Y, int stride, int rh, int rw, const Win w,
                                          Win& c) {
    const int ww = w.x1 - w.x0 + 1, cnt = (w.y1 - w.y0 + 1) * ww;
#pragma unroll 2
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
        const int dy = i / ww, ly = w.y0 + dy, lx = w.x0 + (i - dy * ww);
        const uint32_t mid = X[ly * stride + lx];
        const Nb q = neighbours(X, stride, rh, rw, ly, lx, mid);
        uint32_t del = 0u;
        if (mid) {
            // C = (!p2 & (p3|p4)) + (!p4 & (p5|p6)) + (!p6 & (p7|p8)) + (!p8 & (p9|p2)) == 1: an odd sum with no pair of ones
            const uint32_t c1 = ~q.p2 & (q.p3 | q.p4), c2 = ~q.p4 & (q.p5 | q.p6), c3 = ~q.p6 & (q.p7 | q.p8), c4 = ~q.p8 & (q.p9 | q.p2);
            const uint32_t c_is_1 = ((c1 ^ c2) ^ (c3 ^ c4)) & ~(c1 & c2) & ~(c3 & c4);
            // 2 <= min(N1, N2) <= 3: both sums at least 2, not both 4
            const uint32_t a1 = q.p9 | q.p2, a2 = q.p3 | q.p4, a3 = q.p5 | q.p6, a4 = q.p7 | q.p8;
            const uint32_t b1 = q.p2 | q.p3, b2 = q.p4 | q.p5, b3 = q.p6 | q.p7, b4 = q.p8 | q.p9;
            const uint32_t n_ok = ge2of4(a1, a2, a3, a4) & ge2of4(b1, b2, b3, b4) & ~(a1 & a2 & a3 & a4 & b1 & b2 & b3 & b4);
            const uint32_t m = SUB == 0 ? (q.p6 | q.p7 | ~q.p9) & q.p8 : (q.p2 | q.p3 | ~q.p5) & q.p4;
            del = mid & c_is_1 & n_ok & ~m;
        }
        Y[ly * stride + lx] = mid & ~del;
        if (del) {
            c.y0 = min(c.y0, ly); c.y1 = max(c.y1, ly);
            c.x0 = min(c.x0, lx); c.x1 = max(c.x1, lx);
        }
    }
}

template <class S>
__global__ __launch_bounds__(256) void mask_skeleton_kernel(const SkelP<S> p) {
    constexpr bool PLANE = std::is_same<S, PlaneWords>::value;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    __shared__ int s_changed;
    __shared__ int s_win[4];
    __shared__ long long s_acc[4][6];
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const long t = blockIdx.x;
    const long mw = p.select ? p.select[t] : t;
    const int wpr = (p.W + 31) >> 5;
    const mwords::View v = p.src.view(mw);
    const int4 b4 = reinterpret_cast<const int4*>(p.bbox)[t];
    int y0 = max(b4.x, 0), x0 = max(b4.y, 0), y1 = min(b4.z, p.H - 1), x1 = min(b4.w, p.W - 1);
    if constexpr (!PLANE) {
        // the box is inside the room by contract; clipped to it, the region lies inside the ROOM's region, which is what the
        // host sized both scratches from
        const int4 r = reinterpret_cast<const int4*>(p.src.room)[mw];
        y0 = max(y0, r.x); x0 = max(x0, r.y); y1 = min(y1, r.z); x1 = min(x1, r.w);
    }
    const bool empty = b4.x < 0 || v.rows == 0 || y0 > y1 || x0 > x1;
    double* out = p.out ? p.out + t * p.out_c * SKEL_COLS : nullptr;
    int nc = 0;
    if (out) {
        nc = empty ? 0 : min(max(p.count[t], 0), min(p.out_c, p.C));
        for (int i = nc * SKEL_COLS + tid; i < p.out_c * SKEL_COLS; i += nt) out[i] = 0.0;
    }
    if (empty || (nc == 0 && !p.skel_out)) return;
    int ry0, wx0, rh, rw;
    mreg::region_of(y0, x0, y1, x1, 1, p.H, p.W, ry0, wx0, rh, rw);
    const int pn = (rh + 2) * (rw + 2), n = rh * rw;        // pn: the tracer's padded image, the unit of its LDS / scratch rule
    const uint32_t* A = nullptr;
    uint32_t *P, *Q;
    int stride = rw;
    uint32_t* stage = nullptr;
    if (pn <= SKEL_WORDS) { stage = smem; P = smem + SKEL_WORDS; Q = smem + 2 * SKEL_WORDS; }
    else if constexpr (PLANE) {                             // the plane itself and the two scratch planes, region in place
        const long o = mw * p.H * wpr + (long)ry0 * wpr + wx0;
        A = v.p + (long)ry0 * wpr + wx0;
        P = p.scratch + o;
        Q = p.scratch2 + o;
        stride = wpr;
    } else { stage = p.scratch + p.scratch_off[mw]; P = stage + pn; Q = p.scratch2 + p.scratch2_off[mw]; }
    if (stage) {
        // a word of the region outside the view (the ring of a box on the room's edge) is zero and is NEVER fetched: behind
        // a room lie the next mask's words
        for (int i = tid; i < n; i += nt) {
            const int ly = i / rw, lx = i - ly * rw;
            const int vy = ry0 + ly - v.y0, vx = wx0 + lx - v.c0;
            const bool in = (unsigned)vy < (unsigned)v.rows && (unsigned)vx < (unsigned)v.cols;
            stage[i] = in ? v.p[(long)vy * v.cols + vx] : 0u;
        }
        A = stage;
    }
    // Pairs of sub-iterations (A -> P -> Q, then Q -> P -> Q, ...) until a whole pair deletes nothing: the skeleton is in Q.  Every
    // pair that continues the loop deletes at least one pixel and none comes back, and the region has 32 * rh * rw of them: that
    // many pairs plus one always suffice, so the limit only bounds the loop and never cuts the thinning short.  (No smaller
    // constant: maskregion.h records what a tight round limit once did to the flood.)
    //
    // A pair works on a WINDOW of the region: the first on all of it, a later one on the bounding rectangle of the words the pair
    // before it changed, grown by TWO rows and two word columns.  A pixel that survived sub-iteration s of pair j is deleted by
    // sub-iteration s of pair j + 1 only if its 3 x 3 neighbourhood changed in between.  For s = 0 that is during pair j: within one
    // row and one word of a word pair j changed.  For s = 1 it is during sub-iteration 1 of pair j or sub-iteration 0 of pair
    // j + 1, whose own deletions lie within one row and one word of pair j's: two in all.  (A pixel outside a window was not looked
    // at, but by the same argument would have survived.)  Outside the window P and Q both hold the current state: a word's last
    // change, in pair j, puts it into the window of pair j + 1, which writes it into P and into Q once more, and nothing changes
    // it afterwards.  So a sub-iteration reads current words all around its window, and Q is the skeleton everywhere at the end.
    const long max_pairs = 32L * n + 1;
    const uint32_t* cur = A;
    Win w{0, rh - 1, 0, rw - 1};
    for (long pair = 0; pair < max_pairs; ++pair) {
        if (tid == 0) { s_changed = 0; s_win[0] = rh; s_win[1] = -1; s_win[2] = rw; s_win[3] = -1; }
        __syncthreads();                                     // (also: the staged words / the previous pair's Q are written)
        Win c{rh, -1, rw, -1};
        thin_pass<0>(cur, P, stride, rh, rw, w, c);
        __syncthreads();
        thin_pass<1>(P, Q, stride, rh, rw, w, c);
        if (c.y1 >= 0) {
            s_changed = 1;
            atomicMin(&s_win[0], c.y0); atomicMax(&s_win[1], c.y1);
            atomicMin(&s_win[2], c.x0); atomicMax(&s_win[3], c.x1);
        }
        __syncthreads();
        cur = Q;
        if (!s_changed) break;
        w = Win{max(s_win[0] - 2, 0), min(s_win[1] + 2, rh - 1), max(s_win[2] - 2, 0), min(s_win[3] + 2, rw - 1)};
        __syncthreads();
    }
    if (p.skel_out) {
        for (int i = tid; i < n; i += nt) {
            const int ly = i / rw, lx = i - ly * rw;
            const uint32_t s = Q[ly * stride + lx];
            if constexpr (PLANE) p.skel_out[mw * p.H * wpr + (long)(ry0 + ly) * wpr + wx0 + lx] = s;
            else {
                const int vy = ry0 + ly - v.y0, vx = wx0 + lx - v.c0;
                if ((unsigned)vy < (unsigned)v.rows && (unsigned)vx < (unsigned)v.cols) p.skel_out[p.src.offsets[mw] + (long)vy * v.cols + vx] = s;
            }
        }
    }
    const int rpx = 32 * rw;
    for (int c = 0; c < nc; ++c) {
        const int4 inf = reinterpret_cast<const int4*>(p.info)[t * p.C + c];      // sx, sy, npts, offset
        const int sy = inf.y - ry0, px = inf.x - 32 * wx0;
        __syncthreads();                                     // P: the thinning's / the previous contour's readers are done
        for (int i = tid; i < n; i += nt) P[(i / rw) * stride + i % rw] = 0u;
        __syncthreads();
        const bool ok = (unsigned)sy < (unsigned)rh && (unsigned)px < (unsigned)rpx && ((A[sy * stride + (px >> 5)] >> (px & 31)) & 1u);
        double* o = out + c * SKEL_COLS;
        if (!ok) {                                           // not a trace of these words: no component to measure
            if (tid < SKEL_COLS) o[tid] = 0.0;
            continue;
        }
        if (tid == 0) P[sy * stride + (px >> 5)] = 1u << (px & 31);
        __syncthreads();
        mreg::flood<true>(A, 0u, P, stride, rh, rw, &s_changed);
        __syncthreads();
        // Sk = S & K.  Two components are never 8-adjacent and S is a subset of the mask, so every neighbour in S of a pixel of
        // Sk is in K: the neighbour planes are taken from S as they are.
        long long a[6] = {0, 0, 0, 0, 0, 0};                 // n, n4, nd, ends, branches, Npix
        for (int i = tid; i < n; i += nt) {
            const int ly = i / rw, lx = i - ly * rw;
            const uint32_t k = P[ly * stride + lx];
            a[5] += __popc(k);
            const uint32_t s = Q[ly * stride + lx], mid = s & k;
            if (!mid) continue;
            const Nb q = neighbours(Q, stride, rh, rw, ly, lx, s);
            a[0] += __popc(mid);
            a[1] += __popc(mid & q.p4) + __popc(mid & q.p6);                        // each pair at its left / upper pixel
            a[2] += __popc(mid & q.p5 & ~q.p4 & ~q.p6) + __popc(mid & q.p7 & ~q.p8 & ~q.p6);
            const uint32_t nb[8] = {q.p2, q.p3, q.p4, q.p5, q.p6, q.p7, q.p8, q.p9};
            uint32_t g1 = 0u, g2 = 0u, t1 = 0u, t2 = 0u, t3 = 0u;                   // at least 1, 2 neighbours; 1, 2, 3 transitions
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                g2 |= g1 & nb[j];
                g1 |= nb[j];
                const uint32_t tr = ~nb[j] & nb[(j + 1) & 7];                       // 0 -> 1 in the cyclic sequence p2 .. p9, p2
                t3 |= t2 & tr;
                t2 |= t1 & tr;
                t1 |= tr;
            }
            a[3] += __popc(mid & g1 & ~g2);
            a[4] += __popc(mid & t3);
        }
#pragma unroll
        for (int j = 0; j < 6; ++j)
            for (int s = 32; s > 0; s >>= 1) a[j] += __shfl_xor(a[j], s, 64);
        if (lane == 0)
            for (int j = 0; j < 6; ++j) s_acc[wave][j] = a[j];
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w)
                for (int j = 0; j < 6; ++j) a[j] += s_acc[w][j];
            for (int j = 0; j < 6; ++j) o[j] = (double)a[j];
            o[6] = ((double)a[1] + sqrt(2.0) * (double)a[2]) * p.um;
            o[7] = a[0] > 0 ? (double)a[5] / (double)a[0] * p.um : 0.0;
        }
    }
}

template <class S>
int launch_skeleton(const SkelP<S>& p, int M, hipStream_t st, const char* name) {
    auto k = mask_skeleton_kernel<S>;
    static bool lds_set = false;                            // per instantiation
    if (!lds_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, SKEL_LDS);
        lds_set = true;
    }
    hipLaunchKernelGGL(k, dim3(M), dim3(256), SKEL_LDS, st, p);
    DEMIA_CHECK_LAUNCH(name);
    return DEMIA_OK;
}

}  // namespace

extern "C" int demia_mask_skeleton(const int32_t* select, const uint32_t* masks, uint32_t* scratch, const int32_t* bbox, const int32_t* count,
                                   const int32_t* info, int M, int H, int W, int C, double um_pix, double* out, int out_c,
                                   uint32_t* scratch2, uint32_t* skel_out, void* stream) {
    const bool measure = count || info || out;
    DEMIA_REQUIRE(M >= 0 && H > 0 && W > 0 && (!measure || (C > 0 && out_c > 0)), "shapes");
    if (M == 0) return DEMIA_OK;
    DEMIA_REQUIRE(masks && scratch && scratch2 && bbox && masks != scratch && masks != scratch2 && scratch != scratch2, "args");
    DEMIA_REQUIRE(measure ? (count && info && out) : skel_out != nullptr, "args");
    DEMIA_REQUIRE(skel_out != masks && skel_out != scratch && skel_out != scratch2, "args");
    DEMIA_REQUIRE((long)H * ((W + 31) >> 5) < (1L << 26), "sizes");       // 32 x the words of a region fit the loops' arithmetic
    SkelP<PlaneWords> p{PlaneWords{masks, H, (W + 31) >> 5, nullptr}, select, scratch, nullptr, scratch2, nullptr, bbox, count, info, H, W,
                        measure ? C : 1, um_pix, out, measure ? out_c : 0, skel_out};
    return launch_skeleton(p, M, (hipStream_t)stream, "mask_skeleton_kernel");
}

// Words of the SECOND scratch a crop-framed skeleton needs, from the host's room table alone: a mask whose ROOM's region (the rule
// of demia_crop_contour_scratch) exceeds the large LDS buffer gets one more padded region buffer.
extern "C" int64_t demia_crop_skeleton_scratch(const int32_t* room_host, int64_t M, int H, int W, int64_t* scratch2_off) {
    int64_t total = 0;
    for (int64_t m = 0; m < M; ++m) {
        const int32_t* r = room_host + 4 * m;
        scratch2_off[m] = total;
        if (r[0] < 0) continue;
        int ry0, wx0, rh, rw;
        mreg::region_of(r[0], r[1], r[2], r[3], 1, H, W, ry0, wx0, rh, rw);
        const int64_t pn = (int64_t)(rh + 2) * (rw + 2);
        if (pn > SKEL_WORDS) total += pn;
    }
    return total;
}

extern "C" int demia_crop_skeleton(const int32_t* select, const uint32_t* payload, const int32_t* room, const int64_t* offsets,
                                   const int32_t* bbox, const int32_t* count, const int32_t* info, int M, int H, int W, int C, double um_pix,
                                   double* out, int out_c, uint32_t* scratch, const int64_t* scratch_off, uint32_t* scratch2,
                                   const int64_t* scratch2_off, uint32_t* skel_out, void* stream) {
    const bool measure = count || info || out;
    DEMIA_REQUIRE(M >= 0 && H > 0 && W > 0 && (!measure || (C > 0 && out_c > 0)), "shapes");
    if (M == 0) return DEMIA_OK;
    DEMIA_REQUIRE(payload && room && offsets && bbox && scratch && scratch_off && scratch2 && scratch2_off, "args");
    DEMIA_REQUIRE(measure ? (count && info && out) : skel_out != nullptr, "args");
    DEMIA_REQUIRE(skel_out != payload, "args");
    DEMIA_REQUIRE((long)H * ((W + 31) >> 5) < (1L << 26), "sizes");
    SkelP<CropWords> p{CropWords{payload, room, reinterpret_cast<const long*>(offsets)}, select, scratch,
                       reinterpret_cast<const long*>(scratch_off), scratch2, reinterpret_cast<const long*>(scratch2_off), bbox, count, info,
                       H, W, measure ? C : 1, um_pix, out, measure ? out_c : 0, skel_out};
    return launch_skeleton(p, M, (hipStream_t)stream, "mask_skeleton_kernel<crop>");
}

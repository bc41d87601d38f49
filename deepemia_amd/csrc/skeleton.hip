// Morphological skeleton and its descriptors per external contour (demia_mask_skeleton / demia_crop_skeleton; definition:
// include/deepemia_hip.h).  One kernel over a word source (maskwords.h), one workgroup per mask, on the region stage of
// wordregion.h with TWO work buffers -- the second measurement on the mask WORDS.
//
// The stage hands over the region of the mask (tight box + 1 ring, clipped to the frame) as A, which stays as it is, and the
// buffers P, Q, which the thinning plays ping-pong in; per contour it floods the contour's component K into P.  What is this
// file's: the thinning, the skeleton written out, and the six sums over S & K.
//
// Thinning (Guo-Hall A1) is a Boolean function of a pixel's 3 x 3 neighbourhood, so it runs on 32 pixels per lane-operation:
// lane = WORD, the eight neighbour planes of a word come from the three rows and the carry bits of the words left and right of
// them, and C == 1, 2 <= min(N1, N2) <= 3 are Boolean expressions of bit-sliced sums.  A sub-iteration reads one buffer and writes
// the other, so every pixel sees the state before it; a pair after the first works on the window of words that can still change
// (the rectangle the pair before it changed, grown by two).  Then per contour: mreg::flood<true> of its component K into P, and six
// popcount reductions over S & K.  Integer sums do not depend on which thread saw which word.  No per-pixel loop, no f32, plain
// vector stores.
#include "wordregion.h"

namespace {

using mwords::CropWords;
using mwords::PlaneWords;

constexpr int SKEL_LDS = wreg::lds_words(2) * 4;

template <class S>
struct SkelP : wreg::Params<S> {     // out == NULL (count, info too): thin only
    uint32_t* skel_out;              // NULL, or laid out like the source words
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
    __shared__ long long s_red[wreg::WAVES * 6];
    const int tid = threadIdx.x, nt = blockDim.x;
    wreg::Stage<2> r;
    if (!wreg::stage(p, blockIdx.x, p.skel_out != nullptr, smem, r)) return;
    const int rh = r.rh, rw = r.rw, n = r.n, stride = r.stride;
    const uint32_t* A = r.A;
    uint32_t *P = r.B[0], *Q = r.B[1];
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
        const mwords::View v = r.v;
        const int wpr = (p.W + 31) >> 5;
        for (int i = tid; i < n; i += nt) {
            const int ly = i / rw, lx = i - ly * rw;
            const uint32_t s = Q[ly * stride + lx];
            if constexpr (PLANE) p.skel_out[r.mw * p.H * wpr + (long)(r.ry0 + ly) * wpr + r.wx0 + lx] = s;
            else {
                const int vy = r.ry0 + ly - v.y0, vx = r.wx0 + lx - v.c0;
                if ((unsigned)vy < (unsigned)v.rows && (unsigned)vx < (unsigned)v.cols) p.skel_out[p.src.offsets[r.mw] + (long)vy * v.cols + vx] = s;
            }
        }
    }
    for (int c = 0; c < r.nc; ++c) {
        if (!wreg::component(r, c, &s_changed)) continue;    // K into P, which the thinning has left
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
        wreg::block_sum(a, s_red);
        if (tid == 0) {
            double* o = r.out + c * wreg::COLS;
            for (int j = 0; j < 6; ++j) o[j] = (double)a[j];
            o[6] = ((double)a[1] + sqrt(2.0) * (double)a[2]) * p.um;
            o[7] = a[0] > 0 ? (double)a[5] / (double)a[0] * p.um : 0.0;
        }
    }
}

}  // namespace

// what both entries require, around the arguments that are the entry's own (distinct: no buffer of the call is another one)
#define SKEL_REQUIRE(own_args, distinct)                                                                                      \
    const bool measure = count || info || out;                                                                                \
    DEMIA_REQUIRE(M >= 0 && H > 0 && W > 0 && (!measure || (C > 0 && out_c > 0)), "shapes");                                  \
    if (M == 0) return DEMIA_OK;                                                                                              \
    DEMIA_REQUIRE((own_args) && bbox && scratch && scratch2, "args");                                                         \
    DEMIA_REQUIRE(measure ? (count && info && out) : skel_out != nullptr, "args");                                            \
    DEMIA_REQUIRE(distinct, "args");                                                                                          \
    DEMIA_REQUIRE((long)H * ((W + 31) >> 5) < (1L << 26), "sizes") /* 32 x the words of a region fit the loops' arithmetic */

extern "C" int demia_mask_skeleton(const int32_t* select, const uint32_t* masks, uint32_t* scratch, const int32_t* bbox, const int32_t* count,
                                   const int32_t* info, int M, int H, int W, int C, double um_pix, double* out, int out_c,
                                   uint32_t* scratch2, uint32_t* skel_out, void* stream) {
    SKEL_REQUIRE(masks && masks != scratch && masks != scratch2 && scratch != scratch2,
                 skel_out != masks && skel_out != scratch && skel_out != scratch2);
    SkelP<PlaneWords> p{{PlaneWords{masks, H, (W + 31) >> 5, nullptr}, select, scratch, nullptr, scratch2, nullptr, bbox, count, info, H, W,
                         measure ? C : 1, um_pix, out, measure ? out_c : 0}, skel_out};
    return wreg::launch<mask_skeleton_kernel<PlaneWords>>(p, M, SKEL_LDS, (hipStream_t)stream, "mask_skeleton_kernel");
}

// Words of the SECOND scratch a crop-framed skeleton needs: one more padded region buffer per large room.
extern "C" int64_t demia_crop_skeleton_scratch(const int32_t* room_host, int64_t M, int H, int W, int64_t* scratch2_off) {
    return wreg::room_scratch_words(room_host, M, H, W, 1, scratch2_off);
}

extern "C" int demia_crop_skeleton(const int32_t* select, const uint32_t* payload, const int32_t* room, const int64_t* offsets,
                                   const int32_t* bbox, const int32_t* count, const int32_t* info, int M, int H, int W, int C, double um_pix,
                                   double* out, int out_c, uint32_t* scratch, const int64_t* scratch_off, uint32_t* scratch2,
                                   const int64_t* scratch2_off, uint32_t* skel_out, void* stream) {
    SKEL_REQUIRE(payload && room && offsets && scratch_off && scratch2_off, skel_out != payload);
    SkelP<CropWords> p{{CropWords{payload, room, reinterpret_cast<const long*>(offsets)}, select, scratch,
                        reinterpret_cast<const long*>(scratch_off), scratch2, reinterpret_cast<const long*>(scratch2_off), bbox, count, info,
                        H, W, measure ? C : 1, um_pix, out, measure ? out_c : 0}, skel_out};
    return wreg::launch<mask_skeleton_kernel<CropWords>>(p, M, SKEL_LDS, (hipStream_t)stream, "mask_skeleton_kernel<crop>");
}


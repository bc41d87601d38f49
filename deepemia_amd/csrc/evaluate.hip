// The device side of the evaluate task (COCO box / mask AP on a test split).
//
//   poly_rasterize   ground-truth polygons -> packed masks with pycocotools' rleFrPoly rule (frPyObjects + merge for a mask
//                    made of several polygons), built in two kernels: the boundary points of every edge, then the packed
//                    words, each written by exactly one thread; only the words of a polygon's columns walk its points.
//                    The words go to full-frame planes (PlaneDest) or to the rooms of a crop-framed set (RoomDest)
//   cross_matrix     |det_i & gt_j| for every detection x ground-truth pair of one image segment with equal labels
//   rle_colmajor     column-major run lengths of each mask (pycocotools' encode order: the background run first)
//
// Packed layout as everywhere in the library: [M, H, ceil(W / 32)] uint32, bit (x & 31) of word (x >> 5) = pixel (y, x);
// boxes int32 y0, x0, y1, x1 inclusive, y0 = -1 for an empty mask.  The two kernels that only READ masks are written over a word
// source (maskwords.h) and instantiated for planes and for crop-framed sets (room, offsets, payload: cropops.hip has the
// layout); a crop set is scored without any [M, H, wpr] tensor.  The rasteriser's double arithmetic must be the C
// reference's expression by expression: this file is built with -ffp-contract=off (no fused multiply-adds).
#include <climits>

#include "common.h"
#include "maskwords.h"

namespace {

using mwords::CropWords;
using mwords::PlaneWords;

struct IPt {
    int u, v;
};

// (int)(5 * c + .5) of the reference: C truncation toward zero
__device__ __forceinline__ int scale5(double c) { return (int)(5.0 * c + 0.5); }

// Walk point d of the edge (xs, ys) -> (xe, ye) of the x5 lattice, as rleFrPoly's inner loops produce it.  A degenerate
// edge (dx == dy == 0) divides 0 by 0 there: the one point's v is (int)NaN, INT_MIN on the x86 hosts pycocotools runs on.
__device__ IPt walk_point(int xs, int ys, int xe, int ye, int d) {
    const int dx = abs(xe - xs), dy = abs(ys - ye);
    const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
    if (flip) {
        int t = xs; xs = xe; xe = t;
        t = ys; ys = ye; ye = t;
    }
    IPt p;
    if (dx >= dy) {
        const int t = flip ? dx - d : d;
        p.u = t + xs;
        if (dx == 0) {
            p.v = INT_MIN;
        } else {
            const double s = (double)(ye - ys) / dx;
            p.v = (int)(ys + s * t + .5);
        }
    } else {
        const int t = flip ? dy - d : d;
        const double s = (double)(xe - xs) / dy;
        p.v = t + ys;
        p.u = (int)(xs + s * t + .5);
    }
    return p;
}

__device__ __forceinline__ int edge_points(int xs, int ys, int xe, int ye) { return max(abs(xe - xs), abs(ye - ys)) + 1; }

// One thread per polygon edge: the y-boundary points (column x, row y in [0, h]) that rleFrPoly keeps from this edge's walk
// (each walk point compared with the one before it in the polygon's whole walk list; the very first point has none).
// Points go to the polygon's list at bnd_off[p] through a per-polygon counter: the fill only needs them as a multiset.
// edge_poly [E] / edge_idx [E]: polygon and edge index of every edge; vert_off [P + 1]: the polygon's vertices in xy.
__global__ __launch_bounds__(256) void poly_boundary_kernel(const double* __restrict__ xy, const int* __restrict__ vert_off,
                                                            const int* __restrict__ edge_poly, const int* __restrict__ edge_idx,
                                                            const long* __restrict__ bnd_off, int2* __restrict__ bnd,
                                                            int* __restrict__ bnd_cnt, int* __restrict__ err, int E, int h, int w) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int p = edge_poly[e], j = edge_idx[e];
    const int v0 = vert_off[p], k = vert_off[p + 1] - v0;
    const double* c = xy + 2L * v0;
    const int j1 = (j + 1 == k) ? 0 : j + 1;
    const int xs = scale5(c[2 * j]), ys = scale5(c[2 * j + 1]), xe = scale5(c[2 * j1]), ye = scale5(c[2 * j1 + 1]);
    const int n = edge_points(xs, ys, xe, ye);
    IPt prev;
    int d0 = 0;
    if (j == 0) {
        prev = walk_point(xs, ys, xe, ye, 0);
        d0 = 1;
    } else {
        const int jp = j - 1;
        const int pxs = scale5(c[2 * jp]), pys = scale5(c[2 * jp + 1]);
        prev = walk_point(pxs, pys, xs, ys, edge_points(pxs, pys, xs, ys) - 1);
    }
    const long cap = bnd_off[p + 1] - bnd_off[p];
    for (int d = d0; d < n; ++d) {
        const IPt q = walk_point(xs, ys, xe, ye, d);
        if (q.u != prev.u) {
            double xd = (double)(q.u < prev.u ? q.u : q.u - 1);
            xd = (xd + .5) / 5.0 - .5;
            if (!(floor(xd) != xd || xd < 0 || xd > w - 1)) {
                double yd = (double)(q.v < prev.v ? q.v : prev.v);
                yd = (yd + .5) / 5.0 - .5;
                if (yd < 0) yd = 0;
                else if (yd > h) yd = h;
                yd = ceil(yd);
                const int slot = atomicAdd(&bnd_cnt[p], 1);
                if (slot < cap) bnd[bnd_off[p] + slot] = make_int2((int)xd, (int)yd);
                else atomicOr(err, 1);
            }
        }
        prev = q;
    }
}

// Output word (mask m, row y, word wx): pixel (x, y) of a polygon is set iff an odd number of its boundary points lie at
// column-major positions <= x * h + y -- the toggles of rleFrPoly's run list, counted over ALL columns, so a point clamped
// to y = h toggles row 0 of the next column.  A point (px, py) covers the pixels of row y from column px + (y < py) on.  The
// mask is the OR of its polygons (merge); bits at x >= W stay zero.
// Work is restricted to the polygon's columns: left of its first point's column no point covers a pixel (0), from the column
// after its last point's on every point does (all ones when the count is odd, as rleFrPoly's closing run) -- only the words
// of the columns lo .. hi walk the point list, so a frame of thousands of small polygons costs their boxes, not M planes.
// A block of 256 threads writes 256 * PER_THREAD consecutive words of one mask, each by exactly one thread.
//
// Where the words go is a type.  A destination hands out, per mask, the rectangle of the global word grid it stores (first row,
// first word column, word columns, words) and the address of its word 0; word t is row y0 + t / cols, word column c0 + t % cols.
//   PlaneDest   mask m's plane of [M, H, wpr]: the whole frame, 8 words per thread (a block covers 2048 words of a plane)
//   RoomDest    mask m's room of a crop-framed set, at payload[offsets[m]]: 1 word per thread -- a typical room is a few
//               hundred words, one or two blocks with most threads busy; the grid is masks x slabs of the LARGEST room, and a
//               slab past the end of its mask's room (block-uniform) has nothing to do.  No word outside a room is written.
struct FillRect {
    uint32_t* p;
    int y0, c0, cols;
    long words;
};

struct PlaneDest {
    uint32_t* out;
    int H, wpr;
    __device__ __forceinline__ FillRect rect(int m) const { return FillRect{out + (long)m * H * wpr, 0, 0, wpr, (long)H * wpr}; }
};

struct RoomDest {
    uint32_t* payload;
    const int* room;                 // [M, 4] y0, x0, y1, x1 (inclusive), -1: empty
    const long* offsets;
    __device__ __forceinline__ FillRect rect(int m) const {
        const int4 r = reinterpret_cast<const int4*>(room)[m];
        const int c0 = r.y >> 5, cols = (r.w >> 5) - c0 + 1;
        return FillRect{payload + offsets[m], r.x, c0, cols, r.x < 0 ? 0L : (long)(r.z - r.x + 1) * cols};
    }
};

constexpr int FILL_PER_THREAD = 8;
constexpr int FILL_WORDS = 256 * FILL_PER_THREAD;
constexpr int ROOM_FILL_WORDS = 256;

template <class D, int PER_THREAD>
__global__ __launch_bounds__(256) void poly_fill_kernel(const int2* __restrict__ bnd, const long* __restrict__ bnd_off,
                                                        const int* __restrict__ bnd_cnt, const int* __restrict__ mask_poly,
                                                        const D dst, int W) {
    __shared__ int red_lo[4], red_hi[4];
    const int m = blockIdx.y;
    const FillRect r = dst.rect(m);
    const long total = r.words;
    if (blockIdx.x * (long)(256 * PER_THREAD) >= total) return;      // (block-uniform: a slab past this mask's room)
    const long base = blockIdx.x * (long)(256 * PER_THREAD) + threadIdx.x;
    uint32_t word[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) word[k] = 0u;
    for (int p = mask_poly[m]; p < mask_poly[m + 1]; ++p) {          // (block-uniform)
        const long b0 = bnd_off[p];
        const int n = (int)min((long)bnd_cnt[p], bnd_off[p + 1] - b0);
        int lo = INT_MAX, hi = -1;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int px = bnd[b0 + i].x;
            lo = min(lo, px);
            hi = max(hi, px);
        }
        for (int o = 32; o > 0; o >>= 1) {
            lo = min(lo, __shfl_down(lo, o, 64));
            hi = max(hi, __shfl_down(hi, o, 64));
        }
        __syncthreads();                                             // (the previous polygon's reads of red_* are done)
        if ((threadIdx.x & 63) == 0) {
            red_lo[threadIdx.x >> 6] = lo;
            red_hi[threadIdx.x >> 6] = hi;
        }
        __syncthreads();
        lo = min(min(red_lo[0], red_lo[1]), min(red_lo[2], red_lo[3]));
        hi = max(max(red_hi[0], red_hi[1]), max(red_hi[2], red_hi[3]));
        const uint32_t tail = (n & 1) ? ~0u : 0u;
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) {
            const long t = base + (long)k * 256;
            if (t >= total) continue;
            const int y = r.y0 + (int)(t / r.cols), x0 = (r.c0 + (int)(t % r.cols)) << 5;
            uint32_t par = 0u;
            if (x0 > hi) {
                par = tail;                                          // every point's first column is <= hi + 1 <= x0
            } else if (x0 + 31 >= lo) {
                for (int i = 0; i < n; ++i) {
                    const int2 q = bnd[b0 + i];
                    const int first = q.x + (y < q.y ? 1 : 0) - x0;
                    if (first <= 0) par = ~par;
                    else if (first < 32) par ^= ~0u << first;
                }
            }
            word[k] |= par;
        }
    }
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const long t = base + (long)k * 256;
        if (t >= total) continue;
        const int valid = W - ((r.c0 + (int)(t % r.cols)) << 5);
        r.p[t] = valid < 32 ? (word[k] & ((1u << valid) - 1u)) : word[k];
    }
}

// After the room fill, one block per mask: the pixel count and the tight box of the room's words (as crop_place_kernel
// reduces them), and the check that the host's rooms lost no pixel.  The rooms come from the vertices alone; what the fill
// sets comes from the kept boundary points.  Per polygon every column holds an EVEN number of them (the walk's lattice column
// u moves in steps of at most one and returns to where it began, so it crosses every kept column's threshold an even number
// of times), so every run of set pixels starts at one point of a column and ends at another of the SAME column: a set pixel
// (x, y) has points (x, py <= y) and (x, qy > y).  All set pixels therefore lie in the points' own rectangle, columns
// min px .. max px and rows min py .. max py - 1, over the mask's polygons.  THE TEST: if that rectangle is not empty and
// not inside the room, or a polygon kept an odd number of points (the closing run to the end of the frame), bit 2 of the
// error word is set.  Conservative: it may object to a room that in fact holds every pixel, never pass one that does not.
__global__ __launch_bounds__(256) void room_finish_kernel(const int2* __restrict__ bnd, const long* __restrict__ bnd_off,
                                                          const int* __restrict__ bnd_cnt, const int* __restrict__ mask_poly,
                                                          const uint32_t* __restrict__ payload, const int* __restrict__ room,
                                                          const long* __restrict__ offsets, int* __restrict__ area,
                                                          int* __restrict__ bbox, int* __restrict__ err) {
    __shared__ int s_area, s_y0, s_y1, s_x0, s_x1, s_py0, s_py1, s_px0, s_px1, s_odd;
    const int m = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        s_area = 0; s_y0 = 1 << 30; s_x0 = 1 << 30; s_y1 = -1; s_x1 = -1;
        s_py0 = 1 << 30; s_px0 = 1 << 30; s_py1 = -1; s_px1 = -1; s_odd = 0;
    }
    __syncthreads();
    int py0 = 1 << 30, py1 = -1, px0 = 1 << 30, px1 = -1;
    for (int p = mask_poly[m]; p < mask_poly[m + 1]; ++p) {
        const long b0 = bnd_off[p];
        const int n = (int)min((long)bnd_cnt[p], bnd_off[p + 1] - b0);
        if (tid == 0 && (n & 1)) s_odd = 1;
        for (int i = tid; i < n; i += 256) {
            const int2 q = bnd[b0 + i];
            px0 = min(px0, q.x); px1 = max(px1, q.x);
            py0 = min(py0, q.y); py1 = max(py1, q.y);
        }
    }
    const mwords::View g = CropWords{payload, room, offsets}.view(m);
    int a = 0, y0 = 1 << 30, y1 = -1, x0 = 1 << 30, x1 = -1;
    for (int t = tid; t < g.rows * g.cols; t += 256) {
        const uint32_t bits = g.p[t];
        if (bits) {
            const int ly = t / g.cols, wx = g.c0 + t - ly * g.cols;
            a += __popc(bits);
            y0 = min(y0, g.y0 + ly); y1 = max(y1, g.y0 + ly);
            x0 = min(x0, wx * 32 + __ffs((int)bits) - 1);
            x1 = max(x1, wx * 32 + 31 - __clz((int)bits));
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o, 64);
        y0 = min(y0, __shfl_down(y0, o, 64)); x0 = min(x0, __shfl_down(x0, o, 64));
        y1 = max(y1, __shfl_down(y1, o, 64)); x1 = max(x1, __shfl_down(x1, o, 64));
        py0 = min(py0, __shfl_down(py0, o, 64)); px0 = min(px0, __shfl_down(px0, o, 64));
        py1 = max(py1, __shfl_down(py1, o, 64)); px1 = max(px1, __shfl_down(px1, o, 64));
    }
    if ((tid & 63) == 0) {
        if (a) {
            atomicAdd(&s_area, a);
            atomicMin(&s_y0, y0); atomicMin(&s_x0, x0);
            atomicMax(&s_y1, y1); atomicMax(&s_x1, x1);
        }
        atomicMin(&s_py0, py0); atomicMin(&s_px0, px0);
        atomicMax(&s_py1, py1); atomicMax(&s_px1, px1);
    }
    __syncthreads();
    if (tid == 0) {
        area[m] = s_area;
        reinterpret_cast<int4*>(bbox)[m] = s_area == 0 ? make_int4(-1, -1, -1, -1) : make_int4(s_y0, s_x0, s_y1, s_x1);
        const int4 r = reinterpret_cast<const int4*>(room)[m];
        const bool can_set = s_py1 > s_py0;                          // (rows min py .. max py - 1 are not empty)
        const bool inside = r.x >= 0 && s_py0 >= r.x && s_py1 - 1 <= r.z && s_px0 >= r.y && s_px1 <= r.w;
        if (s_odd || (can_set && !inside)) atomicOr(err, 2);
    }
}

// ---- |det_i & gt_j| for the pairs of one image segment: block per detection, one wave per candidate gt in turn ----------
// Row i of `out` ([D, ld]) holds column j - gt_first[i] for j in [gt_first[i], gt_first[i] + gt_count[i]) (columns >= ld are
// not stored).  Pairs with different labels, an empty box or disjoint boxes are written as 0 without a mask read.  The two
// sides are word sources (maskwords.h); the count is mwords::pair_count, one WAVE per pair as the pair matrix of maskops.hip
// uses it, CROSS_UNROLL trips of its window loop issued together (DESIGN section 4 has what the compiler makes of 1 and 8).
constexpr int CROSS_UNROLL = 8;

template <class SA, class SB>
__global__ __launch_bounds__(256) void cross_matrix_kernel(const SA det, const int* __restrict__ det_bbox, const int* __restrict__ det_label,
                                                           const SB gt, const int* __restrict__ gt_bbox, const int* __restrict__ gt_label,
                                                           const int* __restrict__ gt_first, const int* __restrict__ gt_count,
                                                           int* __restrict__ out, int ld) {
    const int i = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = gt_first[i], n = min(gt_count[i], ld);
    const int4 bi = reinterpret_cast<const int4*>(det_bbox)[i];
    const int li = det_label ? det_label[i] : 0;
    const mwords::View vi = det.view(i);
    for (int c = wave; c < n; c += 4) {
        const int j = f + c;
        const int4 bj = reinterpret_cast<const int4*>(gt_bbox)[j];
        int s = 0;
        if (bi.x >= 0 && bj.x >= 0 && max(bi.x, bj.x) <= min(bi.z, bj.z) && max(bi.y, bj.y) <= min(bi.w, bj.w) &&
            (!det_label || gt_label[j] == li)) {
            s = mwords::pair_count<CROSS_UNROLL>(vi, bi, gt.view(j), bj, lane, 64);
            for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        }
        if (lane == 0) out[(long)i * ld + c] = s;
    }
}

// ---- column-major run lengths ---------------------------------------------------------------------------------------------
// A transition sits at column-major position q = x * H + y where pixel q differs from pixel q - 1 (pixel -1 = 0); positions
// >= H * W are not transitions.  Every transition of a mask lies in its box or right after a box pixel.  Column x's thread
// reports those at rows y0 .. y1 of its column (pixel q - 1 of row 0 is the last row of column x - 1) and the end of its last
// run: at row y1 + 1, or at row 0 of column x + 1 when that row is not visited by column x + 1's thread.  The runs are the gaps of
// 0, t_1 .. t_k, H * W: k + 1 counts, the first the background run (0 when pixel 0 is set).
// The masks are a word source; pixels are read with mwords::pixel, 0 outside the mask's view.  That matters for a room: with
// a tight box that starts at row 0 the row H - 1 read below lies outside any room that ends above the last row -- behind its
// last word are the NEXT mask's words.
template <bool EMIT>
__device__ int column_transitions(const mwords::View m, int4 bb, int x, int H, int W, uint32_t* dst) {
    int k = 0;
    uint32_t prev = (bb.x == 0 && x > bb.y) ? mwords::pixel(m, H - 1, x - 1) : 0u;
    for (int y = bb.x; y <= bb.z; ++y) {
        const uint32_t b = mwords::pixel(m, y, x);
        if (b != prev) {
            if (EMIT) dst[k] = (uint32_t)x * H + y;
            ++k;
        }
        prev = b;
    }
    if (prev) {
        if (bb.z < H - 1) {
            if (EMIT) dst[k] = (uint32_t)x * H + bb.z + 1;
            ++k;
        } else if (x + 1 < W && (x == bb.w || bb.x > 0)) {     // else column x + 1 visits its row 0 with prev = this pixel
            if (EMIT) dst[k] = (uint32_t)(x + 1) * H;
            ++k;
        }
    }
    return k;
}

__device__ __forceinline__ int block_sum(int v, int* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
    return s;
}

// count pass: n_counts[m] = 1 + transitions of mask m
template <class S>
__global__ __launch_bounds__(256) void rle_count_kernel(const S masks, const int* __restrict__ bbox, int* __restrict__ n_counts, int H,
                                                        int W) {
    __shared__ int red[4];
    const int m = blockIdx.x;
    const int4 bb = reinterpret_cast<const int4*>(bbox)[m];
    const mwords::View src = masks.view(m);
    int c = 0;
    if (bb.x >= 0)
        for (int x = bb.y + (int)threadIdx.x; x <= bb.w; x += (int)blockDim.x) c += column_transitions<false>(src, bb, x, H, W, nullptr);
    const int s = block_sum(c, red);
    if (threadIdx.x == 0) n_counts[m] = 1 + s;
}

// write pass: mask m's counts go to counts[off[m] .. off[m] + n_counts[m]).  The transitions are written in column order
// (a block scan per chunk of columns), then turned into run lengths in place, last chunk first.
template <class S>
__global__ __launch_bounds__(256) void rle_write_kernel(const S masks, const int* __restrict__ bbox, const long* __restrict__ off,
                                                        uint32_t* __restrict__ counts, int H, int W) {
    __shared__ int scan[256];
    const int m = blockIdx.x;
    const int4 bb = reinterpret_cast<const int4*>(bbox)[m];
    const mwords::View src = masks.view(m);
    uint32_t* dst = counts + off[m];
    const long cap = off[m + 1] - off[m];
    const uint32_t total = (uint32_t)H * (uint32_t)W;
    int k = 0;                                              // transitions written so far (block-uniform)
    if (bb.x >= 0) {
        for (int xb = bb.y; xb <= bb.w; xb += (int)blockDim.x) {
            const int x = xb + threadIdx.x;
            const int c = (x <= bb.w) ? column_transitions<false>(src, bb, x, H, W, nullptr) : 0;
            scan[threadIdx.x] = c;
            __syncthreads();
            for (int o = 1; o < (int)blockDim.x; o <<= 1) {           // inclusive Hillis-Steele scan
                const int v = threadIdx.x >= (unsigned)o ? scan[threadIdx.x - o] : 0;
                __syncthreads();
                scan[threadIdx.x] += v;
                __syncthreads();
            }
            const int excl = scan[threadIdx.x] - c, chunk = scan[blockDim.x - 1];
            if (c && k + excl + c < cap) column_transitions<true>(src, bb, x, H, W, dst + k + excl);
            k += chunk;
            __syncthreads();
        }
    }
    if (k + 1 != cap) return;                               // sizes disagree with the count pass: leave the slot alone
    // run lengths: dst[i] = t_{i+1} - t_i with t_0 = 0 and t_{k+1} = H * W; dst[i] reads slots i - 1 and i
    for (int hi = k + 1; hi > 0; hi -= (int)blockDim.x) {
        const int i = hi - 1 - (int)threadIdx.x;
        uint32_t v = 0;
        if (i >= 0) {
            const uint32_t a = (i == 0) ? 0u : dst[i - 1];
            const uint32_t b = (i == k) ? total : dst[i];
            v = b - a;
        }
        __syncthreads();
        if (i >= 0) dst[i] = v;
        __syncthreads();
    }
}

}  // namespace

static int launch_poly_boundary(const double* xy, const int32_t* vert_off, const int32_t* edge_poly, const int32_t* edge_idx,
                                const int64_t* bnd_off, int32_t* bnd, int32_t* bnd_cnt, int32_t* err, int64_t E, int H, int W, hipStream_t s) {
    if (E > 0) {
        hipLaunchKernelGGL(poly_boundary_kernel, dim3(cdiv(E, 256)), dim3(256), 0, s, xy, vert_off, edge_poly, edge_idx,
                           (const long*)bnd_off, (int2*)bnd, bnd_cnt, err, (int)E, H, W);
        DEMIA_CHECK_LAUNCH("poly_boundary_kernel");
    }
    return DEMIA_OK;
}

extern "C" int demia_poly_rasterize(const double* xy, const int32_t* vert_off, const int32_t* edge_poly, const int32_t* edge_idx,
                                    const int64_t* bnd_off, int32_t* bnd, int32_t* bnd_cnt, int32_t* err, int64_t E,
                                    const int32_t* mask_poly, int64_t M, int H, int W, uint32_t* out, int32_t* area,
                                    int32_t* bbox, void* stream) {
    DEMIA_REQUIRE(xy && vert_off && edge_poly && edge_idx && bnd_off && bnd && bnd_cnt && err && mask_poly && out, "args");
    DEMIA_REQUIRE(H > 0 && W > 0 && E >= 0 && M >= 0 && M <= 65535 && E <= 0x7fffffffL, "sizes");
    DEMIA_REQUIRE((int64_t)H * W <= 0xffffffffLL, "H * W must fit 32 bits (column-major positions)");
    if (M == 0) return DEMIA_OK;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = launch_poly_boundary(xy, vert_off, edge_poly, edge_idx, bnd_off, bnd, bnd_cnt, err, E, H, W, s)) return rc;
    const int wpr = (W + 31) / 32;
    const long words = (long)H * wpr;
    hipLaunchKernelGGL((poly_fill_kernel<PlaneDest, FILL_PER_THREAD>), dim3(cdiv(words, FILL_WORDS), (unsigned)M), dim3(256), 0, s,
                       (const int2*)bnd, (const long*)bnd_off, bnd_cnt, mask_poly, PlaneDest{out, H, wpr}, W);
    DEMIA_CHECK_LAUNCH("poly_fill_kernel");
    if (area || bbox) {
        DEMIA_REQUIRE(area && bbox, "area and bbox go together");
        return demia_mask_area_bbox(out, nullptr, area, bbox, M, H, W, stream);
    }
    return DEMIA_OK;
}

extern "C" int demia_crop_poly_rasterize(const double* xy, const int32_t* vert_off, const int32_t* edge_poly, const int32_t* edge_idx,
                                         const int64_t* bnd_off, int32_t* bnd, int32_t* bnd_cnt, int32_t* err, int64_t E,
                                         const int32_t* mask_poly, int64_t M, int H, int W, const int32_t* room, const int64_t* offsets,
                                         int64_t max_room_words, uint32_t* payload, int32_t* area, int32_t* bbox, void* stream) {
    DEMIA_REQUIRE(xy && vert_off && edge_poly && edge_idx && bnd_off && bnd && bnd_cnt && err && mask_poly, "args");
    DEMIA_REQUIRE(H > 0 && W > 0 && E >= 0 && M >= 0 && M <= 65535 && E <= 0x7fffffffL && max_room_words >= 0, "sizes");
    DEMIA_REQUIRE((int64_t)H * W <= 0xffffffffLL, "H * W must fit 32 bits (column-major positions)");
    if (M == 0) return DEMIA_OK;
    DEMIA_REQUIRE(room && offsets && payload && area && bbox, "room args");
    const long slabs = (max_room_words + ROOM_FILL_WORDS - 1) / ROOM_FILL_WORDS;
    DEMIA_REQUIRE(slabs <= 0x7fffffffL, "max_room_words");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = launch_poly_boundary(xy, vert_off, edge_poly, edge_idx, bnd_off, bnd, bnd_cnt, err, E, H, W, s)) return rc;
    if (slabs > 0) {
        hipLaunchKernelGGL((poly_fill_kernel<RoomDest, 1>), dim3((unsigned)slabs, (unsigned)M), dim3(256), 0, s, (const int2*)bnd,
                           (const long*)bnd_off, bnd_cnt, mask_poly, RoomDest{payload, room, (const long*)offsets}, W);
        DEMIA_CHECK_LAUNCH("poly_fill_kernel (rooms)");
    }
    hipLaunchKernelGGL(room_finish_kernel, dim3((unsigned)M), dim3(256), 0, s, (const int2*)bnd, (const long*)bnd_off, bnd_cnt, mask_poly,
                       payload, room, (const long*)offsets, area, bbox, err);
    DEMIA_CHECK_LAUNCH("room_finish_kernel");
    return DEMIA_OK;
}

extern "C" int demia_mask_cross_matrix(const uint32_t* det, const int32_t* det_bbox, const int32_t* det_label, const uint32_t* gt,
                                       const int32_t* gt_bbox, const int32_t* gt_label, const int32_t* gt_first,
                                       const int32_t* gt_count, int32_t* out, int64_t D, int ld, int H, int W, void* stream) {
    DEMIA_REQUIRE(det && det_bbox && gt && gt_bbox && gt_first && gt_count && out && W > 0 && H > 0 && ld > 0, "args");
    DEMIA_REQUIRE(!det_label == !gt_label, "labels on both sides or on neither");
    if (D == 0) return DEMIA_OK;
    DEMIA_REQUIRE(D <= 0x7fffffffL, "D");
    const int wpr = (W + 31) >> 5;
    hipLaunchKernelGGL((cross_matrix_kernel<PlaneWords, PlaneWords>), dim3((int)D), dim3(256), 0, (hipStream_t)stream,
                       PlaneWords{det, H, wpr, nullptr}, det_bbox, det_label, PlaneWords{gt, H, wpr, nullptr}, gt_bbox, gt_label, gt_first,
                       gt_count, out, ld);
    DEMIA_CHECK_LAUNCH("cross_matrix_kernel");
    return DEMIA_OK;
}

extern "C" int demia_crop_cross_matrix(const uint32_t* det_payload, const int32_t* det_room, const int64_t* det_offsets,
                                       const int32_t* det_bbox, const int32_t* det_label, const uint32_t* gt_payload,
                                       const int32_t* gt_room, const int64_t* gt_offsets, const int32_t* gt_bbox, const int32_t* gt_label,
                                       const int32_t* gt_first, const int32_t* gt_count, int32_t* out, int64_t D, int ld, void* stream) {
    DEMIA_REQUIRE(D >= 0 && ld > 0, "sizes");
    if (D == 0) return DEMIA_OK;
    DEMIA_REQUIRE(det_payload && det_room && det_offsets && det_bbox && gt_payload && gt_room && gt_offsets && gt_bbox && gt_first &&
                  gt_count && out, "args");
    DEMIA_REQUIRE(!det_label == !gt_label, "labels on both sides or on neither");
    DEMIA_REQUIRE(D <= 0x7fffffffL, "D");
    hipLaunchKernelGGL((cross_matrix_kernel<CropWords, CropWords>), dim3((unsigned)D), dim3(256), 0, (hipStream_t)stream,
                       CropWords{det_payload, det_room, (const long*)det_offsets}, det_bbox, det_label,
                       CropWords{gt_payload, gt_room, (const long*)gt_offsets}, gt_bbox, gt_label, gt_first, gt_count, out, ld);
    DEMIA_CHECK_LAUNCH("cross_matrix_kernel (crops)");
    return DEMIA_OK;
}

// both passes of the run-length encoder over a word source
template <class S>
static int launch_rle(const S src, const int32_t* bbox, int32_t* n_counts, const int64_t* offsets, uint32_t* counts, int64_t M, int H, int W,
                      void* stream, const char* who) {
    if (!offsets) {
        if (!n_counts) {
            demia_set_error("%s: count pass needs n_counts", who);
            return DEMIA_EINVAL;
        }
        hipLaunchKernelGGL(rle_count_kernel<S>, dim3((int)M), dim3(256), 0, (hipStream_t)stream, src, bbox, n_counts, H, W);
        DEMIA_CHECK_LAUNCH("rle_count_kernel");
        return DEMIA_OK;
    }
    if (!counts) {
        demia_set_error("%s: write pass needs counts", who);
        return DEMIA_EINVAL;
    }
    hipLaunchKernelGGL(rle_write_kernel<S>, dim3((int)M), dim3(256), 0, (hipStream_t)stream, src, bbox, (const long*)offsets, counts, H, W);
    DEMIA_CHECK_LAUNCH("rle_write_kernel");
    return DEMIA_OK;
}

extern "C" int demia_mask_rle_colmajor(const uint32_t* masks, const int32_t* bbox, int32_t* n_counts, const int64_t* offsets,
                                       uint32_t* counts, int64_t M, int H, int W, void* stream) {
    DEMIA_REQUIRE(masks && bbox && W > 0 && H > 0, "args");
    DEMIA_REQUIRE((int64_t)H * W <= 0xffffffffLL, "H * W must fit 32 bits");
    if (M == 0) return DEMIA_OK;
    DEMIA_REQUIRE(M <= 0x7fffffffL, "M");
    return launch_rle(PlaneWords{masks, H, (W + 31) >> 5, nullptr}, bbox, n_counts, offsets, counts, M, H, W, stream, __func__);
}

extern "C" int demia_crop_rle_colmajor(const uint32_t* payload, const int32_t* room, const int64_t* room_offsets, const int32_t* bbox,
                                       int32_t* n_counts, const int64_t* offsets, uint32_t* counts, int64_t M, int H, int W, void* stream) {
    DEMIA_REQUIRE(M >= 0 && W > 0 && H > 0, "sizes");
    DEMIA_REQUIRE((int64_t)H * W <= 0xffffffffLL, "H * W must fit 32 bits");
    if (M == 0) return DEMIA_OK;
    DEMIA_REQUIRE(payload && room && room_offsets && bbox, "args");
    DEMIA_REQUIRE(M <= 0x7fffffffL, "M");
    return launch_rle(CropWords{payload, room, (const long*)room_offsets}, bbox, n_counts, offsets, counts, M, H, W, stream, __func__);
}

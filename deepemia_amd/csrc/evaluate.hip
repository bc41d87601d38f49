// The device side of the evaluate task (COCO box / mask AP on a test split).
//
//   poly_rasterize   ground-truth polygons -> packed masks with pycocotools' rleFrPoly rule (frPyObjects + merge for a mask
//                    made of several polygons), built in two kernels: the boundary points of every edge, then the packed
//                    words, each written by exactly one thread; only the words of a polygon's columns walk its points
//   cross_matrix     |det_i & gt_j| for every detection x ground-truth pair of one image segment with equal labels
//   rle_colmajor     column-major run lengths of each mask (pycocotools' encode order: the background run first)
//
// Packed layout as everywhere in the library: [M, H, ceil(W / 32)] uint32, bit (x & 31) of word (x >> 5) = pixel (y, x);
// boxes int32 y0, x0, y1, x1 inclusive, y0 = -1 for an empty mask.  The rasteriser's double arithmetic must be the C
// reference's expression by expression: this file is built with -ffp-contract=off (no fused multiply-adds).
#include <climits>

#include "common.h"

namespace {

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
// A block of 256 threads writes FILL_WORDS consecutive words of one mask, each by exactly one thread.
constexpr int FILL_PER_THREAD = 8;
constexpr int FILL_WORDS = 256 * FILL_PER_THREAD;

__global__ __launch_bounds__(256) void poly_fill_kernel(const int2* __restrict__ bnd, const long* __restrict__ bnd_off,
                                                        const int* __restrict__ bnd_cnt, const int* __restrict__ mask_poly,
                                                        uint32_t* __restrict__ out, int H, int W) {
    __shared__ int red_lo[4], red_hi[4];
    const int wpr = (W + 31) >> 5;
    const int m = blockIdx.y;
    const long total = (long)H * wpr;
    const long base = blockIdx.x * (long)FILL_WORDS + threadIdx.x;
    uint32_t word[FILL_PER_THREAD];
#pragma unroll
    for (int k = 0; k < FILL_PER_THREAD; ++k) word[k] = 0u;
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
        for (int k = 0; k < FILL_PER_THREAD; ++k) {
            const long t = base + (long)k * 256;
            if (t >= total) continue;
            const int y = (int)(t / wpr), x0 = (int)(t % wpr) << 5;
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
    for (int k = 0; k < FILL_PER_THREAD; ++k) {
        const long t = base + (long)k * 256;
        if (t >= total) continue;
        const int valid = W - ((int)(t % wpr) << 5);
        out[(long)m * total + t] = valid < 32 ? (word[k] & ((1u << valid) - 1u)) : word[k];
    }
}

// ---- |det_i & gt_j| for the pairs of one image segment: block per detection, one wave per candidate gt in turn ----------
// Row i of `out` ([D, ld]) holds column j - gt_first[i] for j in [gt_first[i], gt_first[i] + gt_count[i]) (columns >= ld are
// not stored).  Pairs with different labels or disjoint boxes are written as 0 without a mask read.
__global__ __launch_bounds__(256) void cross_matrix_kernel(const uint32_t* __restrict__ det, const int* __restrict__ det_bbox,
                                                           const int* __restrict__ det_label, const uint32_t* __restrict__ gt,
                                                           const int* __restrict__ gt_bbox, const int* __restrict__ gt_label,
                                                           const int* __restrict__ gt_first, const int* __restrict__ gt_count,
                                                           int* __restrict__ out, int ld, int H, int W) {
    const int i = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = gt_first[i], n = min(gt_count[i], ld);
    const int4 bi = reinterpret_cast<const int4*>(det_bbox)[i];
    const int li = det_label ? det_label[i] : 0;
    const int wpr = (W + 31) >> 5;
    const uint32_t* ma = det + (long)i * H * wpr;
    for (int c = wave; c < n; c += 4) {
        const int j = f + c;
        const int4 bj = reinterpret_cast<const int4*>(gt_bbox)[j];
        const int y0 = max(bi.x, bj.x), y1 = min(bi.z, bj.z), x0 = max(bi.y, bj.y), x1 = min(bi.w, bj.w);
        int s = 0;
        if (bi.x >= 0 && bj.x >= 0 && y0 <= y1 && x0 <= x1 && (!det_label || gt_label[j] == li)) {
            const int wx0 = x0 >> 5, rw = (x1 >> 5) - wx0 + 1, rh = y1 - y0 + 1;
            const uint32_t* mb = gt + (long)j * H * wpr;
            for (int t = lane; t < rh * rw; t += 64) {
                const long o = (long)(y0 + t / rw) * wpr + wx0 + t % rw;
                s += __popc(ma[o] & mb[o]);
            }
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
__device__ __forceinline__ uint32_t px_at(const uint32_t* m, int wpr, int y, int x) { return (m[(long)y * wpr + (x >> 5)] >> (x & 31)) & 1u; }

template <bool EMIT>
__device__ int column_transitions(const uint32_t* m, int wpr, int4 bb, int x, int H, int W, uint32_t* dst) {
    int k = 0;
    uint32_t prev = (bb.x == 0 && x > bb.y) ? px_at(m, wpr, H - 1, x - 1) : 0u;
    for (int y = bb.x; y <= bb.z; ++y) {
        const uint32_t b = px_at(m, wpr, y, x);
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
__global__ __launch_bounds__(256) void rle_count_kernel(const uint32_t* __restrict__ masks, const int* __restrict__ bbox,
                                                        int* __restrict__ n_counts, int H, int W) {
    __shared__ int red[4];
    const int m = blockIdx.x, wpr = (W + 31) >> 5;
    const int4 bb = reinterpret_cast<const int4*>(bbox)[m];
    const uint32_t* src = masks + (long)m * H * wpr;
    int c = 0;
    if (bb.x >= 0)
        for (int x = bb.y + (int)threadIdx.x; x <= bb.w; x += (int)blockDim.x) c += column_transitions<false>(src, wpr, bb, x, H, W, nullptr);
    const int s = block_sum(c, red);
    if (threadIdx.x == 0) n_counts[m] = 1 + s;
}

// write pass: mask m's counts go to counts[off[m] .. off[m] + n_counts[m]).  The transitions are written in column order
// (a block scan per chunk of columns), then turned into run lengths in place, last chunk first.
__global__ __launch_bounds__(256) void rle_write_kernel(const uint32_t* __restrict__ masks, const int* __restrict__ bbox,
                                                        const long* __restrict__ off, uint32_t* __restrict__ counts, int H, int W) {
    __shared__ int scan[256];
    const int m = blockIdx.x, wpr = (W + 31) >> 5;
    const int4 bb = reinterpret_cast<const int4*>(bbox)[m];
    const uint32_t* src = masks + (long)m * H * wpr;
    uint32_t* dst = counts + off[m];
    const long cap = off[m + 1] - off[m];
    const uint32_t total = (uint32_t)H * (uint32_t)W;
    int k = 0;                                              // transitions written so far (block-uniform)
    if (bb.x >= 0) {
        for (int xb = bb.y; xb <= bb.w; xb += (int)blockDim.x) {
            const int x = xb + threadIdx.x;
            const int c = (x <= bb.w) ? column_transitions<false>(src, wpr, bb, x, H, W, nullptr) : 0;
            scan[threadIdx.x] = c;
            __syncthreads();
            for (int o = 1; o < (int)blockDim.x; o <<= 1) {           // inclusive Hillis-Steele scan
                const int v = threadIdx.x >= (unsigned)o ? scan[threadIdx.x - o] : 0;
                __syncthreads();
                scan[threadIdx.x] += v;
                __syncthreads();
            }
            const int excl = scan[threadIdx.x] - c, chunk = scan[blockDim.x - 1];
            if (c && k + excl + c < cap) column_transitions<true>(src, wpr, bb, x, H, W, dst + k + excl);
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

extern "C" int demia_poly_rasterize(const double* xy, const int32_t* vert_off, const int32_t* edge_poly, const int32_t* edge_idx,
                                    const int64_t* bnd_off, int32_t* bnd, int32_t* bnd_cnt, int32_t* err, int64_t E,
                                    const int32_t* mask_poly, int64_t M, int H, int W, uint32_t* out, int32_t* area,
                                    int32_t* bbox, void* stream) {
    DEMIA_REQUIRE(xy && vert_off && edge_poly && edge_idx && bnd_off && bnd && bnd_cnt && err && mask_poly && out, "args");
    DEMIA_REQUIRE(H > 0 && W > 0 && E >= 0 && M >= 0 && M <= 65535 && E <= 0x7fffffffL, "sizes");
    DEMIA_REQUIRE((int64_t)H * W <= 0xffffffffLL, "H * W must fit 32 bits (column-major positions)");
    if (M == 0) return DEMIA_OK;
    hipStream_t s = (hipStream_t)stream;
    if (E > 0) {
        hipLaunchKernelGGL(poly_boundary_kernel, dim3(cdiv(E, 256)), dim3(256), 0, s, xy, vert_off, edge_poly, edge_idx,
                           (const long*)bnd_off, (int2*)bnd, bnd_cnt, err, (int)E, H, W);
        DEMIA_CHECK_LAUNCH("poly_boundary_kernel");
    }
    const long words = (long)H * ((W + 31) / 32);
    hipLaunchKernelGGL(poly_fill_kernel, dim3(cdiv(words, FILL_WORDS), (unsigned)M), dim3(256), 0, s, (const int2*)bnd,
                       (const long*)bnd_off, bnd_cnt, mask_poly, out, H, W);
    DEMIA_CHECK_LAUNCH("poly_fill_kernel");
    if (area || bbox) {
        DEMIA_REQUIRE(area && bbox, "area and bbox go together");
        return demia_mask_area_bbox(out, nullptr, area, bbox, M, H, W, stream);
    }
    return DEMIA_OK;
}

extern "C" int demia_mask_cross_matrix(const uint32_t* det, const int32_t* det_bbox, const int32_t* det_label, const uint32_t* gt,
                                       const int32_t* gt_bbox, const int32_t* gt_label, const int32_t* gt_first,
                                       const int32_t* gt_count, int32_t* out, int64_t D, int ld, int H, int W, void* stream) {
    DEMIA_REQUIRE(det && det_bbox && gt && gt_bbox && gt_first && gt_count && out && W > 0 && H > 0 && ld > 0, "args");
    DEMIA_REQUIRE(!det_label == !gt_label, "labels on both sides or on neither");
    if (D == 0) return DEMIA_OK;
    DEMIA_REQUIRE(D <= 0x7fffffffL, "D");
    hipLaunchKernelGGL(cross_matrix_kernel, dim3((int)D), dim3(256), 0, (hipStream_t)stream, det, det_bbox, det_label, gt, gt_bbox,
                       gt_label, gt_first, gt_count, out, ld, H, W);
    DEMIA_CHECK_LAUNCH("cross_matrix_kernel");
    return DEMIA_OK;
}

extern "C" int demia_mask_rle_colmajor(const uint32_t* masks, const int32_t* bbox, int32_t* n_counts, const int64_t* offsets,
                                       uint32_t* counts, int64_t M, int H, int W, void* stream) {
    DEMIA_REQUIRE(masks && bbox && W > 0 && H > 0, "args");
    DEMIA_REQUIRE((int64_t)H * W <= 0xffffffffLL, "H * W must fit 32 bits");
    if (M == 0) return DEMIA_OK;
    DEMIA_REQUIRE(M <= 0x7fffffffL, "M");
    if (!offsets) {
        DEMIA_REQUIRE(n_counts, "count pass needs n_counts");
        hipLaunchKernelGGL(rle_count_kernel, dim3((int)M), dim3(256), 0, (hipStream_t)stream, masks, bbox, n_counts, H, W);
        DEMIA_CHECK_LAUNCH("rle_count_kernel");
        return DEMIA_OK;
    }
    DEMIA_REQUIRE(counts, "write pass needs counts");
    hipLaunchKernelGGL(rle_write_kernel, dim3((int)M), dim3(256), 0, (hipStream_t)stream, masks, bbox, (const long*)offsets, counts,
                       H, W);
    DEMIA_CHECK_LAUNCH("rle_write_kernel");
    return DEMIA_OK;
}

// Outline agreement of matched pairs (demia_mask_outline_agreement / demia_crop_outline_agreement; definition:
// include/deepemia_hip.h): surface distances between the border of a detection and the border of its annotation, in both
// directions, as integers.  Two stages over word sources (maskwords.h), planes or crop-framed sets, one source type per entry:
//
// mask_border_kernel       (maskborder.h, shared with neighbours.hip and agglomerates.hip) once over ALL detections and once over
//                          ALL annotations: the border points of every mask, compacted behind the host's point_off.
// outline_distance_kernel  over the pair list [P, 2], each pair in both directions (2p: detection -> annotation, 2p + 1 the
//                          reverse).  For every border point of the SOURCE mask, d2 = the minimum squared distance to the border
//                          points of the TARGET mask, exact in 64 bits (|dx|, |dy| <= 65535: each square fits 32 unsigned bits,
//                          their sum does not).
//
// Work split.  The source points of one pair-direction are cut into SHARES of OA_SHARE = 256 threads x OA_SRC points, one
// workgroup per share; the host's chunk table (demia_outline_chunks, from the pixel counts -- border <= pixels -- and capped)
// says which workgroup works on which share, and a workgroup strides over the shares beyond the table's, so every count of
// workgroups >= 1 gives the same sums.  A thread holds its OA_SRC source points and their running minima in registers; the
// target points pass through LDS in tiles of OA_TILE, read back four at a time (one ds_read_b128, every lane the same address).
//
// Reduction.  Per workgroup first: the sums by shuffles and LDS (wreg::block_sum / block_max), the histogram in LDS.  Across the
// workgroups of a pair-direction with INTEGER vector atomics on the caller-zeroed record (add, unsigned max): any order gives the
// same bits.  No f32 / f64 on the device: q and the bin come from an integer square root.
#include "maskborder.h"

namespace {

using mwords::CropWords;
using mwords::PlaneWords;

constexpr int OA_THREADS = wreg::THREADS;
constexpr int OA_SRC = 4;                            // source points a thread holds in registers
constexpr int OA_SHARE = OA_THREADS * OA_SRC;        // source points of one workgroup's share
constexpr int OA_TILE = 2048;                        // target points per LDS tile (8 KiB)
constexpr int OA_MAX_CHUNKS = 256;                   // workgroups per pair-direction at most; the shares beyond are strided over
constexpr int OA_BINS = 128;
constexpr int OA_REC = 8 + OA_BINS;                  // i32 words of a record: n, max_d2, sum_d2, sum_q as i64, then hist[128] i32

static_assert(OA_TILE % 4 == 0 && OA_TILE >= 4, "the tile is read four points at a time");

struct Side {
    const uint32_t* points;
    const long* point_off;       // [count + 1]
    const int* nborder;          // [count]
    long count;
};

struct OutlineP {
    Side side[2];                // 0: detections, 1: annotations
    const int* pairs;            // [P, 2] detection, annotation
    long P;
    const long* chunk_off;       // [2 P + 1]: the first workgroup of every pair-direction; the grid is chunk_off[2 P]
    int* out;                    // [P, 2, OA_REC], zero on entry
};

// floor(sqrt(x)), x < 2^62, by integers alone
__device__ __forceinline__ unsigned long long isqrt64(unsigned long long x) {
    unsigned long long r = 0, bit = 1ULL << 60;
    while (bit > x) bit >>= 2;
    while (bit) {
        if (x >= r + bit) {
            x -= r + bit;
            r = (r >> 1) + bit;
        } else
            r >>= 1;
        bit >>= 2;
    }
    return r;
}

// the running minima of NK source points against tn4 (a multiple of 4) staged target points
template <int NK>
__device__ __forceinline__ void scan_tile(const uint32_t* tile, int tn4, const int (&sy)[OA_SRC], const int (&sx)[OA_SRC],
                                          unsigned long long (&best)[OA_SRC]) {
    for (int j = 0; j < tn4; j += 4) {
        const uint4 q4 = *reinterpret_cast<const uint4*>(tile + j);
        const uint32_t q[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int qy = (int)(q[e] >> 16), qx = (int)(q[e] & 0xffffu);
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                // (unsigned)(a - b) squared modulo 2^32 is (a - b)^2 itself: |a - b| <= 65535
                const unsigned dy = (unsigned)(sy[k] - qy), dx = (unsigned)(sx[k] - qx);
                const unsigned long long d = (unsigned long long)(dx * dx) + (unsigned long long)(dy * dy);
                best[k] = min(best[k], d);
            }
        }
    }
}

__global__ __launch_bounds__(OA_THREADS) void outline_distance_kernel(const OutlineP p) {
    __shared__ __attribute__((aligned(16))) uint32_t s_tile[OA_TILE];
    __shared__ unsigned s_hist[OA_BINS];
    __shared__ long long s_red[wreg::WAVES * 2];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    // the pair-direction whose chunks hold workgroup b: chunk_off[pd] <= b < chunk_off[pd + 1]
    long lo = 0, hi = 2 * p.P;
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if (p.chunk_off[mid] <= b) lo = mid;
        else hi = mid;
    }
    const long pd = lo, first = p.chunk_off[pd], nchunks = p.chunk_off[pd + 1] - first, c = b - first;
    if (nchunks < 1 || c < 0 || c >= nchunks) return;        // (a table that is not one: nothing is read or written)
    const int dir = (int)(pd & 1);
    const Side S = p.side[dir], T = p.side[dir ^ 1];
    const long is = p.pairs[2 * (pd >> 1) + dir], it = p.pairs[2 * (pd >> 1) + (dir ^ 1)];
    if (is < 0 || is >= S.count || it < 0 || it >= T.count) return;
    const long offs = S.point_off[is], offt = T.point_off[it];
    const long ns = max(0L, min((long)S.nborder[is], S.point_off[is + 1] - offs));
    const long nt = max(0L, min((long)T.nborder[it], T.point_off[it + 1] - offt));
    int* rec = p.out + pd * OA_REC;
    if (c == 0 && tid == 0) reinterpret_cast<long long*>(rec)[0] = ns;
    if (ns == 0 || nt == 0) return;                          // nothing to measure: the record stays n, 0, 0, 0 and an empty histogram
    if (c * OA_SHARE >= ns) return;                          // a share the border does not reach (the table counted pixels)
    const uint32_t* sp = S.points + offs;
    const uint32_t* tp = T.points + offt;
    if (tid < OA_BINS) s_hist[tid] = 0u;

    long long acc[2] = {0, 0};                               // sum_d2, sum_q
    unsigned long long mx = 0;
    for (long s0 = c * OA_SHARE; s0 < ns; s0 += nchunks * OA_SHARE) {
        const int cnt = (int)min((long)OA_SHARE, ns - s0);
        const int nk = (cnt + OA_THREADS - 1) / OA_THREADS;
        int sy[OA_SRC], sx[OA_SRC];
        unsigned long long best[OA_SRC];
#pragma unroll
        for (int k = 0; k < OA_SRC; ++k) {
            const int i = k * OA_THREADS + tid;
            const uint32_t v = sp[s0 + (i < cnt ? i : 0)];   // (a thread without a point repeats the first: its minimum is dropped)
            sy[k] = (int)(v >> 16);
            sx[k] = (int)(v & 0xffffu);
            best[k] = ~0ULL;
        }
        for (long t0 = 0; t0 < nt; t0 += OA_TILE) {
            const int tn = (int)min((long)OA_TILE, nt - t0), tn4 = (tn + 3) & ~3;
            __syncthreads();                                 // the tile before is read; s_hist is zero (first trip)
            for (int i = tid; i < tn4; i += OA_THREADS) s_tile[i] = tp[t0 + (i < tn ? i : 0)];      // padded with a point of the tile
            __syncthreads();
            switch (nk) {                                    // block-uniform
                case 1: scan_tile<1>(s_tile, tn4, sy, sx, best); break;
                case 2: scan_tile<2>(s_tile, tn4, sy, sx, best); break;
                case 3: scan_tile<3>(s_tile, tn4, sy, sx, best); break;
                default: scan_tile<4>(s_tile, tn4, sy, sx, best); break;
            }
        }
#pragma unroll
        for (int k = 0; k < OA_SRC; ++k) {
            if (k * OA_THREADS + tid >= cnt) continue;
            const unsigned long long d2 = best[k];
            mx = max(mx, d2);
            acc[0] += (long long)d2;
            acc[1] += (long long)isqrt64(d2 << 16);
            int bin = OA_BINS - 1;
            if (d2 <= (unsigned long long)((OA_BINS - 2) * (OA_BINS - 2))) {
                bin = (int)isqrt64(d2);
                if ((unsigned long long)bin * bin < d2) ++bin;
            }
            atomicAdd(&s_hist[bin], 1u);                     // LDS
        }
    }
    mx = wreg::block_max(mx, s_red);
    wreg::block_sum(acc, s_red);                             // (its barriers: s_hist is final)
    unsigned long long* r64 = reinterpret_cast<unsigned long long*>(rec);
    if (tid == 0) {
        atomicMax(r64 + 1, mx);
        atomicAdd(r64 + 2, (unsigned long long)acc[0]);
        atomicAdd(r64 + 3, (unsigned long long)acc[1]);
    }
    if (tid < OA_BINS && s_hist[tid]) atomicAdd(reinterpret_cast<unsigned*>(rec) + 8 + tid, s_hist[tid]);
}

template <class S>
int launch_outline(const mborder::BorderP<S>& det, const mborder::BorderP<S>& gt, const int32_t* pairs, int64_t P,
                   const int64_t* chunk_off, int64_t n_chunks, int32_t* out, hipStream_t st, const char* name) {
    int e = mborder::launch_border<S>(det, st, name);
    if (e != DEMIA_OK) return e;
    e = mborder::launch_border<S>(gt, st, name);
    if (e != DEMIA_OK) return e;
    OutlineP p{{Side{det.points, det.point_off, det.nborder, det.M}, Side{gt.points, gt.point_off, gt.nborder, gt.M}},
               pairs, (long)P, reinterpret_cast<const long*>(chunk_off), out};
    return wreg::launch<outline_distance_kernel>(p, (unsigned)n_chunks, 0, st, name);
}

}  // namespace

extern "C" int demia_outline_source_share(void) { return OA_SHARE; }
extern "C" int demia_outline_target_tile(void) { return OA_TILE; }

// The chunk table of a pair list, from the HOST copies of the pixel counts: pair-direction 2p (source: the detection) and 2p + 1
// (source: the annotation) get ceil(pixels of the source / share) workgroups each, at least 1 and at most OA_MAX_CHUNKS.
extern "C" int64_t demia_outline_chunks(const int64_t* det_area_host, int64_t D, const int64_t* gt_area_host, int64_t G,
                                        const int32_t* pairs_host, int64_t P, int64_t* chunk_off) {
    int64_t total = 0;
    for (int64_t i = 0; i < 2 * P; ++i) {
        chunk_off[i] = total;
        const int64_t m = pairs_host[i], cnt = (i & 1) ? G : D;
        const int64_t a = (m >= 0 && m < cnt) ? ((i & 1) ? gt_area_host[m] : det_area_host[m]) : 0;
        const int64_t k = (a + OA_SHARE - 1) / OA_SHARE;
        total += k < 1 ? 1 : (k > OA_MAX_CHUNKS ? OA_MAX_CHUNKS : k);
    }
    chunk_off[2 * P] = total;
    return total;
}

// what both entries require, around the arguments that are the entry's own
#define OA_REQUIRE(own_args)                                                                                                  \
    DEMIA_REQUIRE(D >= 0 && G >= 0 && P >= 0 && D < (1L << 31) && G < (1L << 31) && P < (1L << 30), "counts");               \
    DEMIA_REQUIRE(H > 0 && W > 0 && H <= 65535 && W <= 65535, "shapes");                                                      \
    if (P == 0 || D == 0 || G == 0) return DEMIA_OK;                                                                          \
    DEMIA_REQUIRE(n_chunks >= 2 * P && n_chunks <= 2 * P * OA_MAX_CHUNKS && n_chunks < (1L << 31), "n_chunks");              \
    DEMIA_REQUIRE((own_args) && det_bbox && gt_bbox && det_point_off && gt_point_off && det_points && gt_points && det_nborder && \
                      gt_nborder && det_sums && gt_sums && pairs && chunk_off && out, "args")

extern "C" int demia_mask_outline_agreement(const uint32_t* det, const int32_t* det_bbox, int64_t D, const uint32_t* gt,
                                            const int32_t* gt_bbox, int64_t G, int H, int W, const int64_t* det_point_off,
                                            uint32_t* det_points, int32_t* det_nborder, int64_t* det_sums,
                                            const int64_t* gt_point_off, uint32_t* gt_points, int32_t* gt_nborder, int64_t* gt_sums,
                                            const int32_t* pairs, int64_t P, const int64_t* chunk_off, int64_t n_chunks,
                                            int32_t* out, void* stream) {
    OA_REQUIRE(det && gt);
    const int wpr = (W + 31) >> 5;
    mborder::BorderP<PlaneWords> d{PlaneWords{det, H, wpr, nullptr}, det_bbox, (long)D, H, W, reinterpret_cast<const long*>(det_point_off),
                                   det_points, det_nborder, reinterpret_cast<long long*>(det_sums)};
    mborder::BorderP<PlaneWords> g{PlaneWords{gt, H, wpr, nullptr}, gt_bbox, (long)G, H, W, reinterpret_cast<const long*>(gt_point_off),
                                   gt_points, gt_nborder, reinterpret_cast<long long*>(gt_sums)};
    return launch_outline(d, g, pairs, P, chunk_off, n_chunks, out, (hipStream_t)stream, "outline_distance_kernel");
}

extern "C" int demia_crop_outline_agreement(const uint32_t* det_payload, const int32_t* det_room, const int64_t* det_offsets,
                                            const int32_t* det_bbox, int64_t D, const uint32_t* gt_payload, const int32_t* gt_room,
                                            const int64_t* gt_offsets, const int32_t* gt_bbox, int64_t G, int H, int W,
                                            const int64_t* det_point_off, uint32_t* det_points, int32_t* det_nborder,
                                            int64_t* det_sums, const int64_t* gt_point_off, uint32_t* gt_points, int32_t* gt_nborder,
                                            int64_t* gt_sums, const int32_t* pairs, int64_t P, const int64_t* chunk_off,
                                            int64_t n_chunks, int32_t* out, void* stream) {
    OA_REQUIRE(det_payload && det_room && det_offsets && gt_payload && gt_room && gt_offsets);
    mborder::BorderP<CropWords> d{CropWords{det_payload, det_room, reinterpret_cast<const long*>(det_offsets)}, det_bbox, (long)D, H, W,
                                  reinterpret_cast<const long*>(det_point_off), det_points, det_nborder,
                                  reinterpret_cast<long long*>(det_sums)};
    mborder::BorderP<CropWords> g{CropWords{gt_payload, gt_room, reinterpret_cast<const long*>(gt_offsets)}, gt_bbox, (long)G, H, W,
                                  reinterpret_cast<const long*>(gt_point_off), gt_points, gt_nborder,
                                  reinterpret_cast<long long*>(gt_sums)};
    return launch_outline(d, g, pairs, P, chunk_off, n_chunks, out, (hipStream_t)stream, "outline_distance_kernel<crop>");
}

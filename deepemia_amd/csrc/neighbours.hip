// Neighbour statistics per instance (demia_mask_neighbours / demia_crop_neighbours; definition: include/deepemia_hip.h): the first
// RELATION between masks -- nearest edge-to-edge gaps and contact counts -- on the mask WORDS, two kernels over a word source
// (maskwords.h: views, word_at, clipped_box, pair_count), one workgroup per mask each; the block reductions and the launch are
// those of wordregion.h.
//
// mask_border_kernel    (maskborder.h, shared with agglomerates.hip) the border points, the pixel count and the coordinate sums.
// mask_neighbour_kernel for mask a, d2(a, b) over the masks b that can still matter.  gap(a, b), the squared distance of the two
//                       boxes, never exceeds d2(a, b), so b is evaluated only while gap <= max(best so far, r2, 2) -- in ascending
//                       (gap, b), which makes `best` shrink after the first few.  A pair whose boxes meet is first asked for a shared
//                       pixel (mwords::pair_count over the box intersection: d2 = 0); otherwise d2 is the minimum over a's border
//                       points x b's border points: for disjoint masks the closest pair of pixels is a pair of border pixels.
//
// Every decision is an integer comparison and every minimum and sum is order-free, so the result does not depend on which thread
// saw which word or point.  No f32 / f64, no global atomics, plain vector stores.
#include "maskborder.h"

namespace {

using mwords::CropWords;
using mwords::PlaneWords;
using mwords::View;

// a's border points staged in LDS; the points beyond are read from global memory where the border kernel left them
constexpr int NB_LDS_POINTS = 8192;
// candidates (gap, b) kept in LDS once a scan of all masks finds no more than this many that can still matter; while it finds
// more, every step scans all masks again
constexpr int NB_CAND_LIST = 256;

constexpr int NB_THREADS = wreg::THREADS, NB_WAVES = wreg::WAVES;
constexpr long long NB_INF = 0x7fffffffffffffffLL;
constexpr int NB_IDX_BITS = 24;                      // a candidate's key is gap << 24 | b: gap < 2^34, M <= 2^24

// the border stage's parameters (maskborder.h) and what the pairing adds
template <class S>
struct NeighP : mborder::BorderP<S> {
    const int* group;            // [M] or NULL
    long long r2;
    long long* table;            // [M, 6]
};

using mborder::box_gap;

// (d, i) < (best, idx): a candidate that can still take the place of the nearest so far (idx < 0: none yet)
__device__ __forceinline__ bool beats(long long d, long i, long long best, long idx) { return idx < 0 || d < best || (d == best && i < idx); }

template <class S>
__global__ __launch_bounds__(NB_THREADS) void mask_neighbour_kernel(const NeighP<S> p) {
    __shared__ uint32_t s_pts[NB_LDS_POINTS];
    __shared__ long long s_list[NB_CAND_LIST];
    __shared__ long long s_red[NB_WAVES];
    __shared__ int s_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long a = blockIdx.x;
    long long* row = p.table + a * 6;
    const long long within0 = p.r2 < 0 ? -1 : 0;
    const long long na_pix = p.sums[a * 3];
    if (na_pix <= 0) {
        if (tid == 0) { row[0] = -1; row[1] = -1; row[2] = -1; row[3] = -1; row[4] = 0; row[5] = within0; }
        return;
    }
    const int4 ba = reinterpret_cast<const int4*>(p.bbox)[a];
    const View va = p.src.view(a);
    const int ga = p.group ? p.group[a] : 0;
    const long offa = p.point_off[a];
    const int na = (int)min((long)p.nborder[a], p.point_off[a + 1] - offa);
    const uint32_t* pa = p.points + offa;
    for (int i = tid; i < min(na, NB_LDS_POINTS); i += NB_THREADS) s_pts[i] = pa[i];

    const long long fixed = max(p.r2, 2LL);                 // a pair at most this far apart is counted, whatever the nearest is
    long long best_any = NB_INF, best_grp = NB_INF;
    long idx_any = -1, idx_grp = -1;
    long long touching = 0, within = within0;
    long long last = -1;                                     // key of the candidate evaluated last: keys ascend strictly
    bool listed = false;
    int nlist = 0;
    const long long idx_mask = (1LL << NB_IDX_BITS) - 1;

    for (;;) {
        // the smallest key above `last` among the masks that can still matter
        long long kmin = NB_INF;
        if (!listed) {
            if (tid == 0) s_n = 0;
            __syncthreads();                                 // (first trip: s_pts is written too)
            for (long b = tid; b < p.M; b += NB_THREADS) {
                if (b == a || p.sums[b * 3] <= 0) continue;
                const int4 bb = reinterpret_cast<const int4*>(p.bbox)[b];
                if (bb.x < 0) continue;
                const long long gap = box_gap(ba, bb), key = (gap << NB_IDX_BITS) | b;
                if (key <= last) continue;
                const bool same = !p.group || p.group[b] == ga;
                if (!(gap <= fixed || beats(gap, b, best_any, idx_any) || (same && beats(gap, b, best_grp, idx_grp)))) continue;
                kmin = min(kmin, key);
                const int slot = atomicAdd(&s_n, 1);         // LDS
                if (slot < NB_CAND_LIST) s_list[slot] = key;
            }
            __syncthreads();
            nlist = s_n;
            listed = nlist <= NB_CAND_LIST;                  // the list holds every mask that can matter from here on
        } else {
            for (int i = tid; i < nlist; i += NB_THREADS) {
                const long long key = s_list[i];
                if (key <= last) continue;
                const long b = key & idx_mask;
                const long long gap = key >> NB_IDX_BITS;
                const bool same = !p.group || p.group[b] == ga;
                if (gap <= fixed || beats(gap, b, best_any, idx_any) || (same && beats(gap, b, best_grp, idx_grp))) kmin = min(kmin, key);
            }
        }
        kmin = wreg::block_min(kmin, s_red);
        if (kmin == NB_INF) break;
        last = kmin;
        const long b = kmin & idx_mask;
        const bool same = !p.group || p.group[b] == ga;
        const int4 bb = reinterpret_cast<const int4*>(p.bbox)[b];

        // d2(a, b), exact where it is at most `lim`; a value above `lim` changes nothing below
        const long long lim = max(fixed, max(idx_any < 0 ? NB_INF : best_any, same ? (idx_grp < 0 ? NB_INF : best_grp) : 0LL));
        long long d2 = NB_INF;
        bool shared = false;
        if ((kmin >> NB_IDX_BITS) == 0) {                    // the boxes meet: a shared pixel?
            const View vb = p.src.view(b);
            const long long c = mwords::pair_count<1>(va, ba, vb, bb, tid, NB_THREADS);
            shared = -wreg::block_min(-c, s_red) > 0;
        }
        if (shared) d2 = 0;
        else {
            const long offb = p.point_off[b];
            const int nb = (int)min((long)p.nborder[b], p.point_off[b + 1] - offb);
            const uint32_t* pb = p.points + offb;
            unsigned long long dmin = ~0ULL;
            // a wave takes 64 of b's points at a time, one per lane, and hands them round; its lanes share a's points
            for (int q0 = wave * 64; q0 < nb; q0 += NB_THREADS) {
                const int cnt = min(64, nb - q0);
                const uint32_t qv = lane < cnt ? pb[q0 + lane] : 0u;
                for (int j = 0; j < cnt; ++j) {
                    const uint32_t q = __shfl(qv, j, 64);
                    const int qy = q >> 16, qx = q & 0xffff;
                    // q is at least this far from every pixel of a
                    const long long ey = max(0, max(ba.x - qy, qy - ba.z)), ex = max(0, max(ba.y - qx, qx - ba.w));
                    if (ex * ex + ey * ey > lim) continue;
                    for (int i = lane; i < na; i += 64) {
                        const uint32_t t = i < NB_LDS_POINTS ? s_pts[i] : pa[i];
                        // |dx|, |dy| <= 65535: each square fits 32 unsigned bits, their sum does not
                        const unsigned dy = (unsigned)abs((int)(t >> 16) - qy), dx = (unsigned)abs((int)(t & 0xffff) - qx);
                        const unsigned long long d = (unsigned long long)(dx * dx) + (unsigned long long)(dy * dy);
                        dmin = min(dmin, d);
                    }
                }
            }
            d2 = wreg::block_min(dmin > (unsigned long long)NB_INF ? NB_INF : (long long)dmin, s_red);
        }
        if (d2 <= 2) ++touching;
        if (p.r2 >= 0 && d2 <= p.r2) ++within;
        if (d2 != NB_INF && beats(d2, b, best_any, idx_any)) { best_any = d2; idx_any = b; }
        if (same && d2 != NB_INF && beats(d2, b, best_grp, idx_grp)) { best_grp = d2; idx_grp = b; }
    }
    if (tid == 0) {
        row[0] = idx_any < 0 ? -1 : best_any; row[1] = idx_any;
        row[2] = idx_grp < 0 ? -1 : best_grp; row[3] = idx_grp;
        row[4] = touching; row[5] = within;
    }
}

template <class S>
int launch_neighbours(const NeighP<S>& p, hipStream_t st, const char* name) {
    const int e = mborder::launch_border<S>(p, st, name);
    return e != DEMIA_OK ? e : wreg::launch<mask_neighbour_kernel<S>>(p, (unsigned)p.M, 0, st, name);
}

}  // namespace

#define NB_REQUIRE_COMMON()                                                                                                   \
    DEMIA_REQUIRE(M >= 0 && M < (1LL << NB_IDX_BITS) && H > 0 && W > 0 && H <= 65535 && W <= 65535, "shapes");            \
    if (M == 0) return DEMIA_OK;                                                                                              \
    DEMIA_REQUIRE(bbox && point_off && points && nborder && sums && table, "args")

extern "C" int demia_mask_neighbours(const uint32_t* masks, const int32_t* bbox, const int32_t* group, int64_t M, int H, int W, int64_t r2,
                                     const int64_t* point_off, uint32_t* points, int32_t* nborder, int64_t* sums, int64_t* table,
                                     void* stream) {
    NB_REQUIRE_COMMON();
    DEMIA_REQUIRE(masks != nullptr, "args");
    NeighP<PlaneWords> p{{PlaneWords{masks, H, (W + 31) >> 5, nullptr}, bbox, (long)M, H, W, reinterpret_cast<const long*>(point_off),
                          points, nborder, reinterpret_cast<long long*>(sums)},
                         group, (long long)r2, reinterpret_cast<long long*>(table)};
    return launch_neighbours(p, (hipStream_t)stream, "mask_neighbour_kernel");
}

extern "C" int demia_crop_neighbours(const uint32_t* payload, const int32_t* room, const int64_t* offsets, const int32_t* bbox,
                                     const int32_t* group, int64_t M, int H, int W, int64_t r2, const int64_t* point_off, uint32_t* points,
                                     int32_t* nborder, int64_t* sums, int64_t* table, void* stream) {
    NB_REQUIRE_COMMON();
    DEMIA_REQUIRE(payload && room && offsets, "args");
    NeighP<CropWords> p{{CropWords{payload, room, reinterpret_cast<const long*>(offsets)}, bbox, (long)M, H, W,
                         reinterpret_cast<const long*>(point_off), points, nborder, reinterpret_cast<long long*>(sums)},
                        group, (long long)r2, reinterpret_cast<long long*>(table)};
    return launch_neighbours(p, (hipStream_t)stream, "mask_neighbour_kernel<crop>");
}

// Agglomerate statistics (demia_mask_agglomerates / demia_crop_agglomerates; definitions: include/deepemia_hip.h): which masks of
// one frame together form one body -- the LINK graph between masks, its connected components, and moments that count a pixel
// shared by linked masks once -- on the mask WORDS, three kernels over a word source (maskwords.h) behind the border stage of
// maskborder.h, which the neighbour stage shares; the block reductions and the launch are those of wordregion.h.
//
// mask_link_kernel       row a of the link matrix, one workgroup per a.  The candidates are the b != a with a pixel, a's group and box
//                        gap <= L2 (the gap never exceeds d2), found 256 at a time by ballot.  A pair whose boxes meet is first asked
//                        for a shared pixel (mwords::pair_count); otherwise "some border point of a lies within L2 of some border
//                        point of b", over a's points near b's box and b's points near a's box, left at the first pair found.  Every pair is decided from
//                        BOTH sides by the same symmetric predicate, so a workgroup writes its own row and nothing else: one launch,
//                        no word with two writers.  The row is assembled in LDS 8 words (256 masks) at a time.
// mask_component_kernel  minimum-label propagation over the rows with pointer jumping, to its fixed point, on ONE workgroup: the
//                        labels live in LDS up to `lds_cap` masks and in `label` itself beyond.  The fixed point -- every label
//                        the smallest index of its component -- is unique, so the order of the updates does not matter.
// mask_own_kernel        the six moments of the pixels of m that no linked b < m holds, one workgroup per m: a & ~b word by word.
//
// Integers only, order-free sums, no f32 / f64, no global atomics, plain vector stores.
#include "maskborder.h"

namespace {

using mborder::box_gap;
using mwords::CropWords;
using mwords::PlaneWords;
using mwords::View;

constexpr int AG_THREADS = wreg::THREADS, AG_WAVES = wreg::WAVES;
constexpr int AG_LDS_POINTS = 8192;                 // a's border points staged in LDS (32 KiB, as in the neighbour kernel); beyond: global
constexpr int AG_NEAR = 256;                         // a's points within L2 of b's box kept in LDS; a pair with more takes all of a's
constexpr int AG_LABEL_LDS = 8192;                   // labels held in LDS by the component kernel (32 KiB)
constexpr int AG_ROW_LDS = 1024;                     // words of row m staged by the own kernel: M <= 32768
constexpr int AG_OWN_LIST = 64;                      // linked lower masks whose view and clipped box the own kernel keeps in LDS
constexpr long AG_MAX_M = 32768;
constexpr int AG_MAX_HW = 32767;

template <class S>
struct AggP : mborder::BorderP<S> {
    const int* group;            // [M] or NULL
    long long L2;
    uint32_t* links;             // [M, wpl]
    int wpl;                     // ceil(M / 32)
    int* degree;                 // [M]
    int* label;                  // [M]
    long long* own;              // [M, 6]
    int lds_cap;                 // labels in LDS while M <= lds_cap
};

template <class S>
__global__ __launch_bounds__(AG_THREADS) void mask_link_kernel(const AggP<S> p) {
    __shared__ uint32_t s_pts[AG_LDS_POINTS];
    __shared__ uint32_t s_near[AG_NEAR];
    __shared__ int s_nnear;
    __shared__ unsigned long long s_cand[AG_WAVES];
    __shared__ uint32_t s_bits[AG_THREADS / 32];
    __shared__ long long s_red[AG_WAVES];
    __shared__ long s_found;                                 // b + 1 of the candidate a pair was found for: never reset, b ascends
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long a = blockIdx.x;
    const int4 ba = reinterpret_cast<const int4*>(p.bbox)[a];
    const bool alive = p.sums[a * 3] > 0 && ba.x >= 0;
    const View va = p.src.view(a);
    const int ga = p.group ? p.group[a] : 0;
    const long offa = p.point_off[a];
    const int na = alive ? (int)min((long)p.nborder[a], p.point_off[a + 1] - offa) : 0;
    const uint32_t* pa = p.points + offa;
    for (int i = tid; i < min(na, AG_LDS_POINTS); i += AG_THREADS) s_pts[i] = pa[i];
    if (tid == 0) s_found = 0;
    int deg = 0;

    for (long c0 = 0; c0 < (long)p.wpl * 32; c0 += AG_THREADS) {
        bool cand = false;
        const long bt = c0 + tid;
        if (alive && bt < p.M && bt != a && p.sums[bt * 3] > 0) {
            const int4 bb = reinterpret_cast<const int4*>(p.bbox)[bt];
            cand = bb.x >= 0 && (!p.group || p.group[bt] == ga) && box_gap(ba, bb) <= p.L2;
        }
        const unsigned long long bal = __ballot(cand);
        if (lane == 0) s_cand[wave] = bal;
        if (tid < AG_THREADS / 32) s_bits[tid] = 0u;
        __syncthreads();                                     // (first trip: s_pts and s_found are written too)
        for (int wv = 0; wv < AG_WAVES; ++wv) {
            unsigned long long todo = s_cand[wv];
            while (todo) {
                const int j = __ffsll(todo) - 1;
                todo &= todo - 1;
                const int rel = wv * 64 + j;
                const long b = c0 + rel;
                const int4 bb = reinterpret_cast<const int4*>(p.bbox)[b];
                bool linked = false;
                if (box_gap(ba, bb) == 0) {                  // the boxes meet: a shared pixel?
                    const View vb = p.src.view(b);
                    const long long c = mwords::pair_count<1>(va, ba, vb, bb, tid, AG_THREADS);
                    linked = -wreg::block_min(-c, s_red) > 0;
                }
                if (!linked) {
                    const long offb = p.point_off[b];
                    const int nb = (int)min((long)p.nborder[b], p.point_off[b + 1] - offb);
                    const uint32_t* pb = p.points + offb;
                    const volatile long* found = &s_found;
                    // a's points within L2 of b's box: no other point of a can be within L2 of a pixel of b.  Mostly a few, or none
                    // (a small b inside a large a's box, away from its border)
                    if (tid == 0) s_nnear = 0;
                    __syncthreads();
                    for (int i = tid; i < na; i += AG_THREADS) {
                        const uint32_t t = i < AG_LDS_POINTS ? s_pts[i] : pa[i];
                        const int ty = t >> 16, tx = t & 0xffff;
                        const long long ey = max(0, max(bb.x - ty, ty - bb.z)), ex = max(0, max(bb.y - tx, tx - bb.w));
                        if (ex * ex + ey * ey > p.L2) continue;
                        const int k = atomicAdd(&s_nnear, 1);    // LDS; the order is unspecified and nothing depends on it
                        if (k < AG_NEAR) s_near[k] = t;
                    }
                    __syncthreads();
                    const int nnear = s_nnear;
                    if (nnear <= AG_NEAR) {
                        // one of b's points per thread, pruned against a's box, against the list; left at the first pair found
                        for (int q0 = tid; q0 < nb && nnear > 0 && *found != b + 1; q0 += AG_THREADS) {
                            const uint32_t q = pb[q0];
                            const int qy = q >> 16, qx = q & 0xffff;
                            const long long ey = max(0, max(ba.x - qy, qy - ba.z)), ex = max(0, max(ba.y - qx, qx - ba.w));
                            if (ex * ex + ey * ey > p.L2) continue;
                            bool mine = false;
                            for (int k = 0; k < nnear && !mine; ++k) {
                                const uint32_t t = s_near[k];
                                const long long dy = (int)(t >> 16) - qy, dx = (int)(t & 0xffff) - qx;
                                mine = dx * dx + dy * dy <= p.L2;
                            }
                            if (mine) {
                                s_found = b + 1;
                                break;
                            }
                        }
                    } else {
                        // a wave takes 64 of b's points at a time, one per lane, and hands them round; its lanes share a's points
                        for (int q0 = wave * 64; q0 < nb && *found != b + 1; q0 += AG_THREADS) {
                            const int cnt = min(64, nb - q0);
                            const uint32_t qv = lane < cnt ? pb[q0 + lane] : 0u;
                            bool hit = false;
                            for (int jq = 0; jq < cnt && !hit; ++jq) {
                                const uint32_t q = __shfl(qv, jq, 64);
                                const int qy = q >> 16, qx = q & 0xffff;
                                // q is at least this far from every pixel of a
                                const long long ey = max(0, max(ba.x - qy, qy - ba.z)), ex = max(0, max(ba.y - qx, qx - ba.w));
                                if (ex * ex + ey * ey > p.L2) continue;
                                bool mine = false;
                                for (int i = lane; i < na; i += 64) {
                                    const uint32_t t = i < AG_LDS_POINTS ? s_pts[i] : pa[i];
                                    // |dx|, |dy| <= 32767: the sum of the squares fits 31 bits
                                    const long long dy = (int)(t >> 16) - qy, dx = (int)(t & 0xffff) - qx;
                                    mine = mine || dx * dx + dy * dy <= p.L2;
                                }
                                hit = __any(mine);               // wave-uniform: q is
                            }
                            if (hit) {
                                if (lane == 0) s_found = b + 1;
                                break;
                            }
                        }
                    }
                    __syncthreads();
                    linked = s_found == b + 1;
                    __syncthreads();                         // nobody still reads s_found when the next candidate writes it
                }
                if (linked) {
                    ++deg;
                    if (tid == 0) s_bits[rel >> 5] |= 1u << (rel & 31);
                }
            }
        }
        __syncthreads();
        const long w = (c0 >> 5) + tid;
        if (tid < AG_THREADS / 32 && w < p.wpl) p.links[a * p.wpl + w] = s_bits[tid];
        __syncthreads();                                     // s_bits and s_cand are free for the next 256
    }
    if (tid == 0) p.degree[a] = deg;
}

// One workgroup.  L[m] is always the index of a member of m's component, at most m; both steps only lower it:
//   sweep   L[m] <- min(L[m], L[b] over the b linked to m), one WAVE per row;
//   jump    L[m] <- L[L[m]], repeated until nothing moves.
// A sweep that changes nothing is the fixed point: L is constant on every component and L[min] = min.  The minimum reaches a
// member at graph distance d after at most d sweeps, so there are at most (largest component's diameter + 1) sweeps and never more
// than M; the jumps make it about log2 of that on chains.  A label read while another thread lowers it is an older, larger, still
// valid value: the fixed point does not depend on it.
template <class S>
__global__ __launch_bounds__(AG_THREADS) void mask_component_kernel(const AggP<S> p) {
    __shared__ int s_label[AG_LABEL_LDS];
    __shared__ int s_changed;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = (int)p.M;
    const bool in_lds = M <= p.lds_cap;
    volatile int* L = in_lds ? s_label : p.label;
    for (int m = tid; m < M; m += AG_THREADS) L[m] = p.sums[(long)m * 3] > 0 ? m : -1;
    for (;;) {
        __syncthreads();
        if (tid == 0) s_changed = 0;
        __syncthreads();
        for (int m = wave; m < M; m += AG_WAVES) {
            const int cur = L[m];
            if (cur < 0 || p.degree[m] == 0) continue;
            int mn = cur;
            const uint32_t* row = p.links + (long)m * p.wpl;
            for (int w = lane; w < p.wpl; w += 64) {
                uint32_t bits = row[w];
                while (bits) {
                    const int b = 32 * w + __ffs(bits) - 1;
                    bits &= bits - 1;
                    mn = min(mn, (int)L[b]);
                }
            }
            for (int d = 32; d > 0; d >>= 1) mn = min(mn, __shfl_xor(mn, d, 64));
            if (lane == 0 && mn < cur) { L[m] = mn; s_changed = 1; }
        }
        __syncthreads();
        if (!s_changed) break;
        for (;;) {
            __syncthreads();
            if (tid == 0) s_changed = 0;
            __syncthreads();
            for (int m = tid; m < M; m += AG_THREADS) {
                const int l = L[m];
                if (l < 0) continue;
                const int ll = L[l];
                if (ll < l) { L[m] = ll; s_changed = 1; }
            }
            __syncthreads();
            if (!s_changed) break;
        }
    }
    if (in_lds)
        for (int m = tid; m < M; m += AG_THREADS) p.label[m] = s_label[m];
}

// a linked lower mask as the own kernel reads it: its view and its clipped box
struct OwnB {
    View v;
    int y0, y1, c0, c1;
};

template <class S>
__global__ __launch_bounds__(AG_THREADS) void mask_own_kernel(const AggP<S> p) {
    __shared__ uint32_t s_row[AG_ROW_LDS];
    __shared__ OwnB s_b[AG_OWN_LIST];
    __shared__ int s_nb;
    __shared__ long long s_red[AG_WAVES * 6];
    const int tid = threadIdx.x;
    const long m = blockIdx.x;
    const View v = p.src.view(m);
    const int4 bm = reinterpret_cast<const int4*>(p.bbox)[m];
    // the links of m to lower indices: words 0 .. m >> 5 of its row, the last one cut below bit m
    const int nrow = (int)(m >> 5) + 1;
    for (int w = tid; w < nrow; w += AG_THREADS) {
        uint32_t bits = p.links[m * p.wpl + w];
        if (w == nrow - 1) bits &= (1u << (m & 31)) - 1u;
        s_row[w] = bits;
    }
    if (tid == 0) s_nb = 0;
    __syncthreads();
    long long acc[6] = {0, 0, 0, 0, 0, 0};
    int y0, y1, c0, c1;
    const bool has = mwords::clipped_box(v, bm, p.H, p.W, y0, y1, c0, c1);
    // the linked lower masks whose clipped box meets m's, listed once (in no stated order: and-not commutes), so that a word
    // of m does not fetch their rooms and boxes again; with more than the list holds every word scans the row instead
    if (has)
        for (int w = tid; w < nrow; w += AG_THREADS) {
            uint32_t bits = s_row[w];
            while (bits) {
                const long b = 32 * w + __ffs(bits) - 1;
                bits &= bits - 1;
                OwnB e;
                e.v = p.src.view(b);
                if (!mwords::clipped_box(e.v, reinterpret_cast<const int4*>(p.bbox)[b], p.H, p.W, e.y0, e.y1, e.c0, e.c1)) continue;
                if (e.y1 < y0 || e.y0 > y1 || e.c1 < c0 || e.c0 > c1) continue;
                const int k = atomicAdd(&s_nb, 1);           // LDS
                if (k < AG_OWN_LIST) s_b[k] = e;
            }
        }
    __syncthreads();
    const int nlist = s_nb;
    if (has) {
        const int rw = c1 - c0 + 1, n = (y1 - y0 + 1) * rw;
        const int wlast = (p.W - 1) >> 5;
        const uint32_t tail = (p.W & 31) ? (1u << (p.W & 31)) - 1u : 0xffffffffu;      // columns beyond W - 1 are nobody's pixels
        for (int i = tid; i < n; i += AG_THREADS) {
            const int ly = i / rw, y = y0 + ly, wx = c0 + (i - ly * rw);
            uint32_t a = mwords::word_at(v, y, wx);
            if (wx == wlast) a &= tail;
            for (int k = 0; k < nlist && nlist <= AG_OWN_LIST && a; ++k) {
                if (y < s_b[k].y0 || y > s_b[k].y1 || wx < s_b[k].c0 || wx > s_b[k].c1) continue;
                a &= ~mwords::word_at(s_b[k].v, y, wx);
            }
            for (int w = 0; w < nrow && nlist > AG_OWN_LIST && a; ++w) {
                uint32_t bits = s_row[w];
                while (bits && a) {
                    const long b = 32 * w + __ffs(bits) - 1;
                    bits &= bits - 1;
                    const View vb = p.src.view(b);
                    int by0, by1, bc0, bc1;
                    if (!mwords::clipped_box(vb, reinterpret_cast<const int4*>(p.bbox)[b], p.H, p.W, by0, by1, bc0, bc1)) continue;
                    if (y < by0 || y > by1 || wx < bc0 || wx > bc1) continue;
                    a &= ~mwords::word_at(vb, y, wx);
                }
            }
            if (!a) continue;
            const long long na = __popc(a), x0 = 32 * wx;
            long long sk = 0, sk2 = 0;                       // the sums of the bit positions and of their squares
            while (a) {
                const int k = __ffs(a) - 1;
                a &= a - 1;
                sk += k;
                sk2 += k * k;
            }
            const long long sx = na * x0 + sk;
            acc[0] += na;
            acc[1] += sx;
            acc[2] += na * y;
            acc[3] += na * x0 * x0 + 2 * x0 * sk + sk2;
            acc[4] += na * y * y;
            acc[5] += sx * y;
        }
    }
    wreg::block_sum(acc, s_red);
    if (tid == 0)
        for (int j = 0; j < 6; ++j) p.own[m * 6 + j] = acc[j];
}

template <class S>
int launch_agglomerates(const AggP<S>& p, int have_border, hipStream_t st, const char* name) {
    int e = DEMIA_OK;
    if (!have_border) e = mborder::launch_border<S>(p, st, name);
    if (e == DEMIA_OK) e = wreg::launch<mask_link_kernel<S>>(p, (unsigned)p.M, 0, st, name);
    if (e == DEMIA_OK) e = wreg::launch<mask_component_kernel<S>>(p, 1u, 0, st, name);
    if (e == DEMIA_OK) e = wreg::launch<mask_own_kernel<S>>(p, (unsigned)p.M, 0, st, name);
    return e;
}

}  // namespace

#define AG_REQUIRE_COMMON()                                                                                                   \
    DEMIA_REQUIRE(M >= 0 && M <= AG_MAX_M, "M <= 32768: the link matrix is at most 128 MiB");                                 \
    DEMIA_REQUIRE(H > 0 && W > 0 && H <= AG_MAX_HW && W <= AG_MAX_HW, "H, W <= 32767: N * x^2 stays below 2^60");             \
    DEMIA_REQUIRE(L2 >= 2, "L2 >= 2");                                                                                        \
    if (M == 0) return DEMIA_OK;                                                                                              \
    DEMIA_REQUIRE(bbox && point_off && points && nborder && sums && links && degree && label && own, "args");                 \
    const int wpl = (int)((M + 31) >> 5);                                                                                     \
    const int cap = label_lds_cap <= 0 ? AG_LABEL_LDS : (label_lds_cap < AG_LABEL_LDS ? label_lds_cap : AG_LABEL_LDS)

extern "C" int demia_mask_agglomerates(const uint32_t* masks, const int32_t* bbox, const int32_t* group, int64_t M, int H, int W, int64_t L2,
                                       const int64_t* point_off, uint32_t* points, int32_t* nborder, int64_t* sums, int have_border,
                                       uint32_t* links, int32_t* degree, int32_t* label, int64_t* own, int label_lds_cap, void* stream) {
    AG_REQUIRE_COMMON();
    DEMIA_REQUIRE(masks != nullptr, "args");
    AggP<PlaneWords> p{{PlaneWords{masks, H, (W + 31) >> 5, nullptr}, bbox, (long)M, H, W, reinterpret_cast<const long*>(point_off), points,
                        nborder, reinterpret_cast<long long*>(sums)},
                       group, (long long)L2, links, wpl, degree, label, reinterpret_cast<long long*>(own), cap};
    return launch_agglomerates(p, have_border, (hipStream_t)stream, "mask_agglomerates");
}

extern "C" int demia_crop_agglomerates(const uint32_t* payload, const int32_t* room, const int64_t* offsets, const int32_t* bbox,
                                       const int32_t* group, int64_t M, int H, int W, int64_t L2, const int64_t* point_off, uint32_t* points,
                                       int32_t* nborder, int64_t* sums, int have_border, uint32_t* links, int32_t* degree, int32_t* label,
                                       int64_t* own, int label_lds_cap, void* stream) {
    AG_REQUIRE_COMMON();
    DEMIA_REQUIRE(payload && room && offsets, "args");
    AggP<CropWords> p{{CropWords{payload, room, reinterpret_cast<const long*>(offsets)}, bbox, (long)M, H, W,
                       reinterpret_cast<const long*>(point_off), points, nborder, reinterpret_cast<long long*>(sums)},
                      group, (long long)L2, links, wpl, degree, label, reinterpret_cast<long long*>(own), cap};
    return launch_agglomerates(p, have_border, (hipStream_t)stream, "mask_agglomerates<crop>");
}

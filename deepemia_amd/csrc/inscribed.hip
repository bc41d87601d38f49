// Largest inscribed circle and distance-based thickness per external contour (demia_mask_inscribed / demia_crop_inscribed;
// definition: include/deepemia_hip.h).  The first measurement that works on the mask WORDS, not on the contour points: one
// kernel over a word source (maskwords.h), one workgroup per mask, on the region stage of wordregion.h with ONE work buffer.
//
// The stage hands over the region of the mask (tight box + 1 ring, clipped to the frame) as A and, per contour, its component
// in B.  Everything outside the region is background: where the region ends on its ring the nearest background is never
// farther than the ring, and where it ends on the frame the definition says so.  What is this file's: per component, row by row
//   G[x]   the vertical distance of pixel (x, y) to the nearest zero of its column (0 for a background pixel), by search
//          in the bits a word at a time, into a row buffer in LDS (u16: G <= ceil(rh / 2));
//   D2(x)  = min over x' of (x - x')^2 + G[x']^2, started at G[x]^2 and walked outwards while d^2 < best,
// and an integer reduction over the bits of B: count, int64 sum, and the maximum of the key (D2, -y, -x).  Integer sums and
// an ordered maximum do not depend on which thread saw which pixel.  No per-pixel table, no f32, plain vector stores.
#include "wordregion.h"

namespace {

using mwords::CropWords;
using mwords::PlaneWords;

constexpr int INSC_WAVE_ROW = 1024;     // a region up to this many pixels wide: every wave has a row buffer and takes rows of its own
constexpr int INSC_LDS_MAX = 160 * 1024 - 1024;      // LDS of a CU less the kernel's static words

template <bool BLOCK>
__device__ __forceinline__ void team_sync() {
    if (BLOCK) __syncthreads();
    else {                                                   // one wave: its LDS accesses retire in order
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
}

// The reduction of one component (bits of B) over the rows y = team, team + nteams, ...; BLOCK: the whole block is one team.
template <bool BLOCK>
__device__ __forceinline__ void reduce_rows(const uint32_t* A, const uint32_t* B, int stride, int rh, int rw, int ry0, int wx0,
                                            uint16_t* g, long long& sd, int& cnt, unsigned long long& key) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int team_n = BLOCK ? 256 : 64, tl = BLOCK ? (int)threadIdx.x : lane;
    const int rpx = 32 * rw;
    for (int y = BLOCK ? 0 : wave; y < rh; y += BLOCK ? 1 : 4) {
        if (!BLOCK) {                                        // a row without a pixel of the component
            bool any = false;
            for (int lx = lane; lx < rw; lx += 64) any |= B[y * stride + lx] != 0u;
            if (!__any(any)) continue;
        }
        const int kmax = min(y + 1, rh - y);                // rows -1 and rh are background
        // G of the row, lane = WORD: acc holds the pixels whose column is set in all of the rows y - k + 1 .. y + k - 1; a bit
        // that drops at step k has G = k (two loads per step serve 32 pixels; A may be global memory)
        for (int lx = tl; lx < rw; lx += team_n) {
            uint32_t acc = A[y * stride + lx];
            uint16_t* gw = g + 32 * lx;
            for (uint32_t z = ~acc; z; z &= z - 1u) gw[__ffs((int)z) - 1] = 0;
            for (int k = 1; acc; ++k) {
                const uint32_t nxt = k < kmax ? acc & A[(y - k) * stride + lx] & A[(y + k) * stride + lx] : 0u;
                for (uint32_t drop = acc & ~nxt; drop; drop &= drop - 1u) gw[__ffs((int)drop) - 1] = (uint16_t)k;
                acc = nxt;
            }
        }
        if (tl == 0) { g[-1] = 0; g[rpx] = 0; }             // columns -1 and 32 * rw are background
        team_sync<BLOCK>();
        for (int x = tl; x < rpx; x += team_n) {
            if (!((B[y * stride + (x >> 5)] >> (x & 31)) & 1u)) continue;
            const uint32_t g0 = g[x];
            uint32_t best = g0 * g0;
            // four steps per test of the bound, their loads in flight together.  Every candidate is the squared distance to a real
            // background pixel (a step past the bound included), so the minimum is exact; an index past an end of the buffer is
            // clamped to that end, whose zero then stands for a step at least as far as the one that met it
            for (uint32_t d = 1; d * d < best; d += 4) {
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    const int dd = (int)(d + j);
                    const uint32_t gm = min((uint32_t)g[max(x - dd, -1)], (uint32_t)g[min(x + dd, rpx)]);
                    best = min(best, (uint32_t)(dd * dd) + gm * gm);
                }
            }
            sd += best;
            ++cnt;
            const unsigned long long kk = ((unsigned long long)best << 32) | ((unsigned long long)(0xFFFF - (ry0 + y)) << 16) |
                                          (unsigned long long)(0xFFFF - (32 * wx0 + x));
            key = kk > key ? kk : key;
        }
        team_sync<BLOCK>();                                  // the next row overwrites g
    }
}

template <class S>
__global__ __launch_bounds__(256) void mask_inscribed_kernel(const wreg::Params<S> p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    __shared__ int s_changed;
    __shared__ long long s_red[wreg::WAVES * 2];
    wreg::Stage<1> r;
    if (!wreg::stage(p, blockIdx.x, false, smem, r)) return;
    uint16_t* G = reinterpret_cast<uint16_t*>(smem + wreg::lds_words(1));
    const bool wave_rows = 32 * r.rw <= INSC_WAVE_ROW;
    uint16_t* g = G + (wave_rows ? (threadIdx.x >> 6) * (INSC_WAVE_ROW + 2) : 0) + 1;
    for (int c = 0; c < r.nc; ++c) {
        if (!wreg::component(r, c, &s_changed)) continue;
        long long sd = 0;
        int cnt = 0;
        unsigned long long key = 0;
        if (wave_rows) reduce_rows<false>(r.A, r.B[0], r.stride, r.rh, r.rw, r.ry0, r.wx0, g, sd, cnt, key);
        else reduce_rows<true>(r.A, r.B[0], r.stride, r.rh, r.rw, r.ry0, r.wx0, g, sd, cnt, key);
        long long a[2] = {sd, cnt};
        wreg::block_sum(a, s_red);
        key = wreg::block_max(key, s_red);
        if (threadIdx.x == 0) {
            double* o = r.out + c * wreg::COLS;
            const double r2 = (double)(key >> 32), nn = (double)a[1], sd2 = (double)a[0];
            o[0] = r2;
            o[1] = (double)(0xFFFF - (int)(key & 0xFFFFu));
            o[2] = (double)(0xFFFF - (int)((key >> 16) & 0xFFFFu));
            o[3] = nn;
            o[4] = sd2;
            o[5] = 2.0 * sqrt(r2) * p.um;
            o[6] = sqrt(sd2 / nn) * p.um;
            o[7] = sqrt(M_PI * r2 / nn);
        }
    }
}

// dynamic LDS: the stage's two region buffers and the row buffer(s) of G
int inscribed_lds_bytes(int W) {
    const int wpr = (W + 31) >> 5;
    const int wide = 32 * wpr + 2, gcap = wide > 4 * (INSC_WAVE_ROW + 2) ? wide : 4 * (INSC_WAVE_ROW + 2);
    return wreg::lds_words(1) * 4 + ((gcap * 2 + 15) & ~15);
}

}  // namespace

// what both entries require, around the arguments that are the entry's own
#define INSC_REQUIRE(own_args)                                                                                        \
    DEMIA_REQUIRE(M >= 0 && H > 0 && W > 0 && C > 0 && out_c > 0, "shapes");                                          \
    if (M == 0) return DEMIA_OK;                                                                                      \
    DEMIA_REQUIRE((own_args) && scratch && bbox && count && info && out, "args");                                     \
    DEMIA_REQUIRE(H <= 0xFFFF && W <= 0xFFFF && inscribed_lds_bytes(W) <= INSC_LDS_MAX, "sizes")

extern "C" int demia_mask_inscribed(const int32_t* select, const uint32_t* masks, uint32_t* scratch, const int32_t* bbox,
                                    const int32_t* count, const int32_t* info, int M, int H, int W, int C, double um_pix,
                                    double* out, int out_c, void* stream) {
    INSC_REQUIRE(masks && masks != scratch);
    wreg::Params<PlaneWords> p{PlaneWords{masks, H, (W + 31) >> 5, nullptr}, select, scratch, nullptr, nullptr, nullptr, bbox, count, info,
                               H, W, C, um_pix, out, out_c};
    return wreg::launch<mask_inscribed_kernel<PlaneWords>>(p, M, inscribed_lds_bytes(W), (hipStream_t)stream, "mask_inscribed_kernel");
}

extern "C" int demia_crop_inscribed(const int32_t* select, const uint32_t* payload, const int32_t* room, const int64_t* offsets,
                                    const int32_t* bbox, const int32_t* count, const int32_t* info, int M, int H, int W, int C,
                                    double um_pix, double* out, int out_c, uint32_t* scratch, const int64_t* scratch_off, void* stream) {
    INSC_REQUIRE(payload && room && offsets && scratch_off);
    wreg::Params<CropWords> p{CropWords{payload, room, reinterpret_cast<const long*>(offsets)}, select, scratch,
                              reinterpret_cast<const long*>(scratch_off), nullptr, nullptr, bbox, count, info, H, W, C, um_pix, out, out_c};
    return wreg::launch<mask_inscribed_kernel<CropWords>>(p, M, inscribed_lds_bytes(W), (hipStream_t)stream, "mask_inscribed_kernel<crop>");
}


// Largest inscribed circle and distance-based thickness per external contour (demia_mask_inscribed / demia_crop_inscribed;
// definition: include/deepemia_hip.h).  The first measurement that works on the mask WORDS, not on the contour points: one
// kernel over a word source (maskwords.h), one workgroup per mask, the region machinery of maskregion.h as it is.
//
// Per mask the region (tight box + 1 ring, clipped to the frame; mreg::region_of) is staged as the tracer stages it: in LDS
// up to the tracer's large buffer, beyond that in the caller's scratch under the tracer's contract.  Everything outside the
// region is background: where the region ends on its ring the nearest background is never farther than the ring, and where
// it ends on the frame the definition says so.  Per contour: seed (sx, sy), mreg::flood<true> of its component into B, then
// row by row
//   G[x]   the vertical distance of pixel (x, y) to the nearest zero of its column (0 for a background pixel), by search
//          in the bits a word at a time, into a row buffer in LDS (u16: G <= ceil(rh / 2));
//   D2(x)  = min over x' of (x - x')^2 + G[x']^2, started at G[x]^2 and walked outwards while d^2 < best,
// and an integer reduction over the bits of B: count, int64 sum, and the maximum of the key (D2, -y, -x).  Integer sums and
// an ordered maximum do not depend on which thread saw which pixel.  No per-pixel table, no f32, plain vector stores.
#include <type_traits>
#include "common.h"
#include "maskregion.h"
#include "maskwords.h"

namespace {

using mwords::CropWords;
using mwords::PlaneWords;

constexpr int INSC_COLS = 8;
constexpr int INSC_WORDS = 8192;        // LDS words per region buffer: the tracer's TRACE_WORDS (contours.hip) -- its scratch contract
constexpr int INSC_WAVE_ROW = 1024;     // a region up to this many pixels wide: every wave has a row buffer and takes rows of its own
constexpr int INSC_LDS_MAX = 160 * 1024 - 1024;      // LDS of a CU less the kernel's static words

template <class S>
struct InscP {
    S src;
    const int* select;           // [M] or NULL: position t reads the words of mask select[t]
    uint32_t* scratch;
    const long* scratch_off;     // crops: [set] words into scratch (demia_crop_contour_scratch)
    const int* bbox;             // [M, 4]
    const int* count;            // [M]
    const int* info;             // [M, C, 4]
    int H, W, C;
    double um;
    double* out;                 // [M, out_c, 8]
    int out_c;
};

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
__global__ __launch_bounds__(256) void mask_inscribed_kernel(const InscP<S> p) {
    constexpr bool PLANE = std::is_same<S, PlaneWords>::value;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    __shared__ int s_changed;
    __shared__ long long s_sd[4];
    __shared__ unsigned long long s_key[4];
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const long t = blockIdx.x;
    const long mw = p.select ? p.select[t] : t;
    const int wpr = (p.W + 31) >> 5;
    double* out = p.out + t * p.out_c * INSC_COLS;
    const mwords::View v = p.src.view(mw);
    const int4 b4 = reinterpret_cast<const int4*>(p.bbox)[t];
    int y0 = max(b4.x, 0), x0 = max(b4.y, 0), y1 = min(b4.z, p.H - 1), x1 = min(b4.w, p.W - 1);
    if constexpr (!PLANE) {
        // the box is inside the room by contract; clipped to it, the region lies inside the ROOM's region, which is what the
        // host sized the scratch from (as the tracer does)
        const int4 r = reinterpret_cast<const int4*>(p.src.room)[mw];
        y0 = max(y0, r.x); x0 = max(x0, r.y); y1 = min(y1, r.z); x1 = min(x1, r.w);
    }
    const bool empty = b4.x < 0 || v.rows == 0 || y0 > y1 || x0 > x1;
    const int nc = empty ? 0 : min(max(p.count[t], 0), min(p.out_c, p.C));
    for (int i = nc * INSC_COLS + tid; i < p.out_c * INSC_COLS; i += nt) out[i] = 0.0;
    if (nc == 0) return;
    int ry0, wx0, rh, rw;
    mreg::region_of(y0, x0, y1, x1, 1, p.H, p.W, ry0, wx0, rh, rw);
    const int pn = (rh + 2) * (rw + 2), n = rh * rw;        // pn: the tracer's padded image, the unit of its LDS / scratch rule
    const uint32_t* A = nullptr;
    uint32_t* B;
    int stride = rw;
    uint32_t* stage = nullptr;
    if (pn <= INSC_WORDS) { stage = smem; B = smem + INSC_WORDS; }
    else if constexpr (PLANE) {                             // the plane itself and the scratch plane, region in place
        A = v.p + (long)ry0 * wpr + wx0;
        B = p.scratch + mw * p.H * wpr + (long)ry0 * wpr + wx0;
        stride = wpr;
    } else { stage = p.scratch + p.scratch_off[mw]; B = stage + pn; }
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
    uint16_t* G = reinterpret_cast<uint16_t*>(smem + 2 * INSC_WORDS);
    const int rpx = 32 * rw;
    const bool wave_rows = rpx <= INSC_WAVE_ROW;
    uint16_t* g = G + (wave_rows ? wave * (INSC_WAVE_ROW + 2) : 0) + 1;
    for (int c = 0; c < nc; ++c) {
        const int4 inf = reinterpret_cast<const int4*>(p.info)[t * p.C + c];      // sx, sy, npts, offset
        const int ly = inf.y - ry0, px = inf.x - 32 * wx0;
        for (int i = tid; i < n; i += nt) B[(i / rw) * stride + i % rw] = 0u;
        __syncthreads();
        const bool ok = (unsigned)ly < (unsigned)rh && (unsigned)px < (unsigned)rpx && ((A[ly * stride + (px >> 5)] >> (px & 31)) & 1u);
        double* o = out + c * INSC_COLS;
        if (!ok) {                                           // not a trace of these words: no component to measure
            if (tid < INSC_COLS) o[tid] = 0.0;
            continue;
        }
        if (tid == 0) B[ly * stride + (px >> 5)] = 1u << (px & 31);
        __syncthreads();
        mreg::flood<true>(A, 0u, B, stride, rh, rw, &s_changed);
        __syncthreads();
        long long sd = 0;
        int cnt = 0;
        unsigned long long key = 0;
        if (wave_rows) reduce_rows<false>(A, B, stride, rh, rw, ry0, wx0, g, sd, cnt, key);
        else reduce_rows<true>(A, B, stride, rh, rw, ry0, wx0, g, sd, cnt, key);
        for (int s = 32; s > 0; s >>= 1) {
            sd += __shfl_xor(sd, s, 64);
            cnt += __shfl_xor(cnt, s, 64);
            const unsigned long long k2 = __shfl_xor(key, s, 64);
            key = k2 > key ? k2 : key;
        }
        if (lane == 0) { s_sd[wave] = sd; s_cnt[wave] = cnt; s_key[wave] = key; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w) {
                sd += s_sd[w];
                cnt += s_cnt[w];
                key = s_key[w] > key ? s_key[w] : key;
            }
            const double r2 = (double)(key >> 32), nn = (double)cnt, sd2 = (double)sd;
            o[0] = r2;
            o[1] = (double)(0xFFFF - (int)(key & 0xFFFFu));
            o[2] = (double)(0xFFFF - (int)((key >> 16) & 0xFFFFu));
            o[3] = nn;
            o[4] = sd2;
            o[5] = 2.0 * sqrt(r2) * p.um;
            o[6] = sqrt(sd2 / nn) * p.um;
            o[7] = sqrt(M_PI * r2 / nn);
        }
        __syncthreads();                                     // the next contour reuses B and the s_ words
    }
}

// dynamic LDS: the two region buffers and the row buffer(s) of G
int inscribed_lds_bytes(int W) {
    const int wpr = (W + 31) >> 5;
    const int wide = 32 * wpr + 2, gcap = wide > 4 * (INSC_WAVE_ROW + 2) ? wide : 4 * (INSC_WAVE_ROW + 2);
    return 2 * INSC_WORDS * 4 + ((gcap * 2 + 15) & ~15);
}

template <class S>
int launch_inscribed(const InscP<S>& p, int M, hipStream_t st, const char* name) {
    const int lds = inscribed_lds_bytes(p.W);
    auto k = mask_inscribed_kernel<S>;
    static int lds_set = 0;                                 // per instantiation
    if (lds > lds_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        lds_set = lds;
    }
    hipLaunchKernelGGL(k, dim3(M), dim3(256), lds, st, p);
    DEMIA_CHECK_LAUNCH(name);
    return DEMIA_OK;
}

}  // namespace

extern "C" int demia_mask_inscribed(const int32_t* select, const uint32_t* masks, uint32_t* scratch, const int32_t* bbox,
                                    const int32_t* count, const int32_t* info, int M, int H, int W, int C, double um_pix,
                                    double* out, int out_c, void* stream) {
    DEMIA_REQUIRE(M >= 0 && H > 0 && W > 0 && C > 0 && out_c > 0, "shapes");
    if (M == 0) return DEMIA_OK;
    DEMIA_REQUIRE(masks && scratch && masks != scratch && bbox && count && info && out, "args");
    DEMIA_REQUIRE(H <= 0xFFFF && W <= 0xFFFF && inscribed_lds_bytes(W) <= INSC_LDS_MAX, "sizes");
    InscP<PlaneWords> p{PlaneWords{masks, H, (W + 31) >> 5, nullptr}, select, scratch, nullptr, bbox, count, info, H, W, C, um_pix, out, out_c};
    return launch_inscribed(p, M, (hipStream_t)stream, "mask_inscribed_kernel");
}

extern "C" int demia_crop_inscribed(const int32_t* select, const uint32_t* payload, const int32_t* room, const int64_t* offsets,
                                    const int32_t* bbox, const int32_t* count, const int32_t* info, int M, int H, int W, int C,
                                    double um_pix, double* out, int out_c, uint32_t* scratch, const int64_t* scratch_off, void* stream) {
    DEMIA_REQUIRE(M >= 0 && H > 0 && W > 0 && C > 0 && out_c > 0, "shapes");
    if (M == 0) return DEMIA_OK;
    DEMIA_REQUIRE(payload && room && offsets && bbox && count && info && out && scratch && scratch_off, "args");
    DEMIA_REQUIRE(H <= 0xFFFF && W <= 0xFFFF && inscribed_lds_bytes(W) <= INSC_LDS_MAX, "sizes");
    InscP<CropWords> p{CropWords{payload, room, reinterpret_cast<const long*>(offsets)}, select, scratch,
                       reinterpret_cast<const long*>(scratch_off), bbox, count, info, H, W, C, um_pix, out, out_c};
    return launch_inscribed(p, M, (hipStream_t)stream, "mask_inscribed_kernel<crop>");
}

// Error maps of the evaluate task (demia_mask_error_map / demia_crop_error_map; definitions: include/deepemia_hip.h): one picture per
// image that puts the detections over the ground truth -- where they agree, where a detection has pixels no annotation has, where
// an annotation has pixels no detection has -- with the outlines of both on top, painted from the packed words of the two mask
// sets.  One kernel over a word source (maskwords.h), planes or crop-framed sets, one source type per entry.
//
// error_map_kernel         one workgroup per TILE of EM_ROWS rows x EM_WORDS word columns of the frame, one thread per word of it.
//                          The masks of both sets whose boxes meet the tile are found 256 at a time by ballot (as mask_link_kernel
//                          finds its candidates); every one of them takes a ROUND: its words over the tile and a halo of t rows and
//                          one word column are staged in LDS (mwords::word_at: 0 outside the view and never fetched there; the box
//                          prunes the fetches), eroded along the rows into a second buffer, and each thread ANDs 2t + 1 of those
//                          down its column.  The thread ORs the mask's word into the fill union of its state and the word's outline
//                          m & ~eroded into the line class of its state: eight 32-pixel accumulators in registers.  Rounds follow
//                          each other without a list, so no capacity limits how many masks may meet one tile.  Then the four counts
//                          of the tile (popcounts, wreg::block_sum, one row of partials) and the painting: the accumulators pass
//                          through LDS so that a thread paints four neighbouring pixels and a wave a contiguous run of the row.
// error_map_counts_kernel  one workgroup: the sum of the partial rows.
//
// Both buffers of a round exist twice: the stage of round k + 1 writes the halves round k does not read, so a round has two barriers.
// Integers only, boolean word operations and popcounts, no global atomics, plain vector stores.
#include "wordregion.h"

namespace {

using mwords::CropWords;
using mwords::PlaneWords;
using mwords::View;

constexpr int EM_THREADS = wreg::THREADS, EM_WAVES = wreg::WAVES;
constexpr int EM_ROWS = 32;                          // rows of a tile
constexpr int EM_WORDS = 8;                          // word columns of a tile: 256 pixels
constexpr int EM_MAX_LINE = 4;                       // the widest line
constexpr int EM_HROWS = EM_ROWS + 2 * EM_MAX_LINE;  // staged rows: the tile and t rows on either side
constexpr int EM_HCOLS = EM_WORDS + 2;               // staged word columns: the tile and one on either side (t <= 32)
constexpr int EM_ACC = 8;                            // accumulators per thread
constexpr int EM_QUAD = 4;                           // pixels a thread paints at a time
constexpr int EM_MAX_HW = 65535;

static_assert(EM_ROWS * EM_WORDS == EM_THREADS, "one thread per word of the tile");
static_assert((EM_WORDS * 32 / EM_QUAD) == 64 && EM_ROWS % (EM_THREADS / 64) == 0, "a wave paints one row of the tile at a time");

// the accumulators: three fill unions, then the five line classes in the order of their priority (and of the palette, from 3 on)
enum { A_DALL = 0, A_GALL, A_GC, A_LINE_UNMATCHED, A_LINE_MISSED, A_LINE_MATCHED_D, A_LINE_MATCHED_G, A_LINE_CROWD };

template <class S>
struct ErrorMapP {
    S det, gt;
    const int* d_bbox;           // [D, 4]
    const int* g_bbox;           // [G, 4]
    const int* d_state;          // [D]
    const int* g_state;          // [G]
    long D, G;
    int H, W, C, alpha, line;
    uint8_t palette[24];
    const uint8_t* src;          // [H, W, C]
    uint8_t* dst;                // [H, W, 3]
    long long* partial;          // [tiles, 4]
};

__host__ __device__ __forceinline__ long em_tiles_x(int W) { return (((W + 31) >> 5) + EM_WORDS - 1) / EM_WORDS; }
__host__ __device__ __forceinline__ long em_tiles(int H, int W) { return em_tiles_x(W) * ((H + EM_ROWS - 1) / EM_ROWS); }

template <class S>
__global__ __launch_bounds__(EM_THREADS) void error_map_kernel(const ErrorMapP<S> p) {
    __shared__ uint32_t s_raw[2][EM_HROWS * EM_HCOLS];
    __shared__ uint32_t s_row[2][EM_HROWS * EM_WORDS];
    __shared__ uint32_t s_acc[EM_ACC][EM_THREADS];
    __shared__ unsigned long long s_cand[2][EM_WAVES];
    __shared__ long long s_red[EM_WAVES * 4];
    __shared__ int s_pal[24];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = p.H, W = p.W, t = p.line, wpr = (W + 31) >> 5;
    const long tiles_x = em_tiles_x(W), tile = blockIdx.x;
    const int y0 = (int)(tile / tiles_x) * EM_ROWS, w0 = (int)(tile % tiles_x) * EM_WORDS;
    const int y1 = min(y0 + EM_ROWS, H) - 1, x0 = w0 * 32, x1 = min(x0 + EM_WORDS * 32, W) - 1;      // the tile's pixels, inclusive
    const int hrows = EM_ROWS + 2 * t;
    const int r = tid / EM_WORDS, c = tid % EM_WORDS;                                                // this thread's word of the tile
    // bits of the last word column beyond column W - 1 are nobody's pixels
    const uint32_t last_mask = (W & 31) ? ((1u << (W & 31)) - 1u) : ~0u;
    if (tid < 24) s_pal[tid] = p.palette[tid];

    uint32_t acc[EM_ACC];
#pragma unroll
    for (int k = 0; k < EM_ACC; ++k) acc[k] = 0u;

    const long N = p.D + p.G;
    int round = 0, batch = 0;
    for (long c0 = 0; c0 < N; c0 += EM_THREADS, ++batch) {
        bool cand = false;
        const long i = c0 + tid;
        if (i < N) {
            const bool isg = i >= p.D;
            const long m = isg ? i - p.D : i;
            const int st = isg ? p.g_state[m] : p.d_state[m];
            const int4 b = reinterpret_cast<const int4*>(isg ? p.g_bbox : p.d_bbox)[m];
            cand = st >= 1 && st <= (isg ? 3 : 2) && b.x >= 0 && b.x <= y1 && b.z >= y0 && b.y <= x1 && b.w >= x0;
        }
        const unsigned long long bal = __ballot(cand);
        if (lane == 0) s_cand[batch & 1][wave] = bal;
        __syncthreads();                                     // (batch k + 2 writes these slots behind the barrier of batch k + 1)
        for (int wv = 0; wv < EM_WAVES; ++wv) {
            unsigned long long todo = s_cand[batch & 1][wv];
            while (todo) {                                   // block-uniform
                const int j = __ffsll(todo) - 1;
                todo &= todo - 1;
                const long ii = c0 + wv * 64 + j;
                const bool isg = ii >= p.D;
                const long m = isg ? ii - p.D : ii;
                const int st = isg ? p.g_state[m] : p.d_state[m];
                const int4 b = reinterpret_cast<const int4*>(isg ? p.g_bbox : p.d_bbox)[m];
                const View v = isg ? p.gt.view(m) : p.det.view(m);
                const int buf = round & 1;
                ++round;
                // rows y0 - t .. y0 + EM_ROWS + t - 1 x word columns w0 - 1 .. w0 + EM_WORDS; a word outside the mask's box or the
                // frame is a zero operand and is not fetched
                const int by0 = max(b.x, 0), by1 = min(b.z, H - 1), bw0 = max(b.y, 0) >> 5, bw1 = min(min(b.w, W - 1) >> 5, wpr - 1);
                for (int k = tid; k < hrows * EM_HCOLS; k += EM_THREADS) {
                    const int ly = k / EM_HCOLS, lx = k - ly * EM_HCOLS;
                    const int y = y0 - t + ly, wx = w0 - 1 + lx;
                    uint32_t w = 0u;
                    if (y >= by0 && y <= by1 && wx >= bw0 && wx <= bw1) {
                        w = mwords::word_at(v, y, wx);
                        if (wx == wpr - 1) w &= last_mask;
                    }
                    s_raw[buf][k] = w;
                }
                __syncthreads();
                // along the rows: the AND of the 2t + 1 shifts of a row, through the words on either side
                for (int k = tid; k < hrows * EM_WORDS; k += EM_THREADS) {
                    const int ly = k / EM_WORDS, lx = k - ly * EM_WORDS;
                    const uint32_t* q = &s_raw[buf][ly * EM_HCOLS + lx];
                    const uint32_t L = q[0], M = q[1], R = q[2];
                    uint32_t h = M;
                    for (int s = 1; s <= t; ++s) h &= ((M >> s) | (R << (32 - s))) & ((M << s) | (L >> (32 - s)));
                    s_row[buf][k] = h;
                }
                __syncthreads();
                // down the column; then the word's share of the fill union and of the line class of the mask's state
                const uint32_t mine = s_raw[buf][(r + t) * EM_HCOLS + c + 1];
                uint32_t e = mine;
                for (int s = 0; s <= 2 * t && e; ++s) e &= s_row[buf][(r + s) * EM_WORDS + c];
                const uint32_t edge = mine & ~e;
                const int fill = isg ? (st == 3 ? A_GC : A_GALL) : A_DALL;
                const int cls = isg ? (st == 3 ? A_LINE_CROWD : st == 2 ? A_LINE_MISSED : A_LINE_MATCHED_G)
                                    : (st == 2 ? A_LINE_UNMATCHED : A_LINE_MATCHED_D);
#pragma unroll
                for (int k = 0; k < EM_ACC; ++k) acc[k] |= (k == fill ? mine : 0u) | (k == cls ? edge : 0u);
            }
        }
    }

    // ---- the counts, on the fill classes
    const uint32_t Dw = acc[A_DALL], Gw = acc[A_GALL], Cw = acc[A_GC];
    long long cnt[4] = {__popc(Dw & Gw), __popc(Dw & ~Gw & ~Cw), __popc(Gw & ~Dw), __popc(Dw & Cw & ~Gw)};      // agree, excess, missing, ignored
#pragma unroll
    for (int k = 0; k < EM_ACC; ++k) s_acc[k][tid] = acc[k];
    wreg::block_sum(cnt, s_red);                             // (its barriers publish s_acc and s_pal)
    if (tid == 0)
        for (int k = 0; k < 4; ++k) p.partial[tile * 4 + k] = cnt[k];

    // ---- the painting: EM_QUAD pixels per thread, a wave per row of the tile.  Where every row of both images starts on a 4-byte
    // boundary (block-uniform) a quad moves as whole dwords, else byte by byte
    const int C = p.C, alpha = p.alpha;
    const bool dwords = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(p.src) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.dst) & 3) == 0;
    const int qx = tid & 63, wc = qx >> 3, sh = (qx & 7) * EM_QUAD;
    const int x = x0 + qx * EM_QUAD;
    for (int rr = tid >> 6; rr < EM_ROWS; rr += EM_THREADS / 64) {
        const int y = y0 + rr;
        if (y >= H || x >= W) continue;
        uint32_t nib[EM_ACC];
#pragma unroll
        for (int k = 0; k < EM_ACC; ++k) nib[k] = (s_acc[k][rr * EM_WORDS + wc] >> sh) & 15u;
        const long px0 = (long)y * W + x;
        const int npx = min(EM_QUAD, W - x);
        uint32_t base[3] = {0u, 0u, 0u};                    // the quad's base pixels: 12 bytes, BGR BGR BGR BGR
        if (C == 3) {
            if (dwords) {
                const uint32_t* s4 = reinterpret_cast<const uint32_t*>(p.src + px0 * 3);
                base[0] = s4[0]; base[1] = s4[1]; base[2] = s4[2];
            } else {
#pragma unroll
                for (int k = 0; k < EM_QUAD * 3; ++k)
                    if (k < npx * 3) base[k >> 2] |= (uint32_t)p.src[px0 * 3 + k] << ((k & 3) * 8);
            }
        } else {
            uint32_t g4 = 0u;
            if (dwords) g4 = *reinterpret_cast<const uint32_t*>(p.src + px0);
            else {
#pragma unroll
                for (int k = 0; k < EM_QUAD; ++k)
                    if (k < npx) g4 |= (uint32_t)p.src[px0 + k] << (k * 8);
            }
#pragma unroll
            for (int k = 0; k < EM_QUAD * 3; ++k) base[k >> 2] |= ((g4 >> ((k / 3) * 8)) & 255u) << ((k & 3) * 8);
        }
        uint32_t out[3] = {0u, 0u, 0u};
#pragma unroll
        for (int q = 0; q < EM_QUAD; ++q) {
            const bool d = (nib[A_DALL] >> q) & 1u, g = (nib[A_GALL] >> q) & 1u, cr = (nib[A_GC] >> q) & 1u;
            const int fill = (d && g) ? 0 : (d && !cr) ? 1 : (g && !d) ? 2 : -1;             // (d && !g && cr: ignored, not filled)
            int cls = -1;
#pragma unroll
            for (int k = EM_ACC - 1; k >= A_LINE_UNMATCHED; --k)
                if ((nib[k] >> q) & 1u) cls = k;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int k = q * 3 + ch;
                int val = (int)((base[k >> 2] >> ((k & 3) * 8)) & 255u);
                if (cls >= 0) val = s_pal[cls * 3 + ch];
                else if (fill >= 0) val = (val * (256 - alpha) + s_pal[fill * 3 + ch] * alpha + 128) >> 8;
                out[k >> 2] |= (uint32_t)val << ((k & 3) * 8);
            }
        }
        if (dwords) {
            uint32_t* d4 = reinterpret_cast<uint32_t*>(p.dst + px0 * 3);
            d4[0] = out[0]; d4[1] = out[1]; d4[2] = out[2];
        } else {
#pragma unroll
            for (int k = 0; k < EM_QUAD * 3; ++k)
                if (k < npx * 3) p.dst[px0 * 3 + k] = (uint8_t)(out[k >> 2] >> ((k & 3) * 8));
        }
    }
}

__global__ __launch_bounds__(EM_THREADS) void error_map_counts_kernel(const long long* __restrict__ partial, long tiles, long long* __restrict__ counts) {
    __shared__ long long s_red[EM_WAVES * 4];
    long long a[4] = {0, 0, 0, 0};
    for (long i = threadIdx.x; i < tiles; i += EM_THREADS)
        for (int k = 0; k < 4; ++k) a[k] += partial[i * 4 + k];
    wreg::block_sum(a, s_red);
    if (threadIdx.x == 0)
        for (int k = 0; k < 4; ++k) counts[k] = a[k];
}

template <class S>
int launch_error_map(ErrorMapP<S> p, const uint8_t* palette_host, long long* counts, hipStream_t st, const char* name) {
    for (int k = 0; k < 24; ++k) p.palette[k] = palette_host[k];
    const long tiles = em_tiles(p.H, p.W);
    const int e = wreg::launch<error_map_kernel<S>>(p, (unsigned)tiles, 0, st, name);
    if (e != DEMIA_OK) return e;
    hipLaunchKernelGGL(error_map_counts_kernel, dim3(1), dim3(EM_THREADS), 0, st, p.partial, tiles, counts);
    DEMIA_CHECK_LAUNCH("error_map_counts_kernel");
    return DEMIA_OK;
}

}  // namespace

extern "C" int64_t demia_error_map_tiles(int H, int W) { return (H > 0 && W > 0) ? em_tiles(H, W) : 0; }

// what both entries require, around the arguments that are the entry's own
#define EM_REQUIRE(own_det, own_gt)                                                                                           \
    DEMIA_REQUIRE(D >= 0 && G >= 0 && D + G < (1L << 31), "counts");                                                          \
    DEMIA_REQUIRE(H > 0 && W > 0 && H <= EM_MAX_HW && W <= EM_MAX_HW, "shapes");                                              \
    DEMIA_REQUIRE(C == 1 || C == 3, "channels");                                                                              \
    DEMIA_REQUIRE(alpha >= 0 && alpha <= 256, "alpha");                                                                       \
    DEMIA_REQUIRE(line >= 1 && line <= EM_MAX_LINE, "line");                                                                  \
    DEMIA_REQUIRE(src && dst && (const void*)src != (const void*)dst && palette && partial && counts, "args");               \
    DEMIA_REQUIRE(D == 0 || ((own_det) && det_bbox && d_state), "detections");                                               \
    DEMIA_REQUIRE(G == 0 || ((own_gt) && gt_bbox && g_state), "annotations")

extern "C" int demia_mask_error_map(const uint32_t* det, const int32_t* det_bbox, const int32_t* d_state, int64_t D, const uint32_t* gt,
                                    const int32_t* gt_bbox, const int32_t* g_state, int64_t G, int H, int W, const uint8_t* src, int C,
                                    uint8_t* dst, int alpha, int line, const uint8_t* palette, int64_t* partial, int64_t* counts,
                                    void* stream) {
    EM_REQUIRE(det, gt);
    const int wpr = (W + 31) >> 5;
    ErrorMapP<PlaneWords> p{PlaneWords{det, H, wpr, nullptr}, PlaneWords{gt, H, wpr, nullptr}, det_bbox, gt_bbox, d_state, g_state,
                            (long)D, (long)G, H, W, C, alpha, line, {}, src, dst, reinterpret_cast<long long*>(partial)};
    return launch_error_map(p, palette, reinterpret_cast<long long*>(counts), (hipStream_t)stream, "error_map_kernel");
}

extern "C" int demia_crop_error_map(const uint32_t* det_payload, const int32_t* det_room, const int64_t* det_offsets, const int32_t* det_bbox,
                                    const int32_t* d_state, int64_t D, const uint32_t* gt_payload, const int32_t* gt_room,
                                    const int64_t* gt_offsets, const int32_t* gt_bbox, const int32_t* g_state, int64_t G, int H, int W,
                                    const uint8_t* src, int C, uint8_t* dst, int alpha, int line, const uint8_t* palette, int64_t* partial,
                                    int64_t* counts, void* stream) {
    EM_REQUIRE(det_payload && det_room && det_offsets, gt_payload && gt_room && gt_offsets);
    ErrorMapP<CropWords> p{CropWords{det_payload, det_room, reinterpret_cast<const long*>(det_offsets)},
                           CropWords{gt_payload, gt_room, reinterpret_cast<const long*>(gt_offsets)}, det_bbox, gt_bbox, d_state, g_state,
                           (long)D, (long)G, H, W, C, alpha, line, {}, src, dst, reinterpret_cast<long long*>(partial)};
    return launch_error_map(p, palette, reinterpret_cast<long long*>(counts), (hipStream_t)stream, "error_map_kernel<crop>");
}

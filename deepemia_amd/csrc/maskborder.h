// The border STAGE of the kernels that relate the masks of one frame to each other (neighbours.hip, agglomerates.hip), stated
// ONCE: what the border kernel is given (BorderP), the kernel, and the squared distance of two boxes.  Definition of the points,
// the sums and point_off: include/deepemia_hip.h (demia_mask_neighbours).
//
// mask_border_kernel    the border pixels of every mask as points (y << 16 | x), compacted into points[point_off[m] ..), with the
//                       border count, the pixel count and the coordinate sums.  A border word is A & ~(up & down & left & right), 32
//                       pixels per lane-operation; the neighbour words of a word outside the view read 0 and are never fetched.
#pragma once
#include "wordregion.h"

namespace mborder {
namespace {

using mwords::View;

constexpr int THREADS = wreg::THREADS, WAVES = wreg::WAVES;

template <class S>
struct BorderP {
    S src;
    const int* bbox;             // [M, 4]
    long M;
    int H, W;
    const long* point_off;       // [M + 1]
    uint32_t* points;
    int* nborder;                // [M]
    long long* sums;             // [M, 3] N, Sx, Sy
};

template <class S>
__global__ __launch_bounds__(THREADS) void mask_border_kernel(const BorderP<S> p) {
    __shared__ int s_count;
    __shared__ long long s_red[WAVES * 3];
    const int tid = threadIdx.x;
    const long m = blockIdx.x;
    const View v = p.src.view(m);
    const int4 b = reinterpret_cast<const int4*>(p.bbox)[m];
    const long off = p.point_off[m];
    const long cap = p.point_off[m + 1] - off;               // border <= pixels: the host sized it from the pixel counts
    uint32_t* out = p.points + off;
    if (tid == 0) s_count = 0;
    __syncthreads();
    long long acc[3] = {0, 0, 0};
    int y0, y1, c0, c1;
    if (mwords::clipped_box(v, b, p.H, p.W, y0, y1, c0, c1)) {
        const int rw = c1 - c0 + 1, n = (y1 - y0 + 1) * rw;
        const int wlast = (p.W - 1) >> 5;
        const uint32_t tail = (p.W & 31) ? (1u << (p.W & 31)) - 1u : 0xffffffffu;      // columns beyond W - 1 are nobody's pixels
        for (int i = tid; i < n; i += THREADS) {
            const int ly = i / rw, y = y0 + ly, wx = c0 + (i - ly * rw);
            uint32_t a = mwords::word_at(v, y, wx);
            if (wx == wlast) a &= tail;
            if (!a) continue;
            const uint32_t up = y > 0 ? mwords::word_at(v, y - 1, wx) : 0u, dn = y < p.H - 1 ? mwords::word_at(v, y + 1, wx) : 0u;
            const uint32_t wl = mwords::word_at(v, y, wx - 1);
            uint32_t wr = wx < wlast ? mwords::word_at(v, y, wx + 1) : 0u;
            if (wx + 1 == wlast) wr &= tail;
            const uint32_t lf = (a << 1) | (wl >> 31), rt = (a >> 1) | (wr << 31);
            uint32_t bd = a & ~(up & dn & lf & rt);
            const int na = __popc(a);
            // sum of the bit positions of a word, by bit of the position
            const int sx = __popc(a & 0xaaaaaaaau) + 2 * __popc(a & 0xccccccccu) + 4 * __popc(a & 0xf0f0f0f0u) + 8 * __popc(a & 0xff00ff00u) +
                           16 * __popc(a & 0xffff0000u);
            acc[0] += na;
            acc[1] += (long long)na * (32 * wx) + sx;
            acc[2] += (long long)na * y;
            if (bd) {
                int k = atomicAdd(&s_count, __popc(bd));      // LDS; the order inside a mask is unspecified
                while (bd) {
                    const int bit = __ffs(bd) - 1;
                    bd &= bd - 1;
                    if (k < cap) out[k] = ((uint32_t)y << 16) | (uint32_t)(32 * wx + bit);
                    ++k;
                }
            }
        }
    }
    wreg::block_sum(acc, s_red);                             // (its barrier: s_count is final)
    if (tid == 0) {
        for (int j = 0; j < 3; ++j) p.sums[m * 3 + j] = acc[j];
        p.nborder[m] = s_count;
    }
}

// the squared distance of two boxes: never more than d2 of the masks inside them
__device__ __forceinline__ long long box_gap(const int4 a, const int4 b) {
    const long long gy = max(0, max(b.x - a.z, a.x - b.z)), gx = max(0, max(b.y - a.w, a.y - b.w));
    return gx * gx + gy * gy;
}

template <class S>
int launch_border(const BorderP<S>& p, hipStream_t st, const char* name) {
    return wreg::launch<mask_border_kernel<S>>(p, (unsigned)p.M, 0, st, name);
}

}  // namespace
}  // namespace mborder

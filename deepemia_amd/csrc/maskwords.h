// Where the packed words of a mask live, as a type: the kernels that only READ masks (maskops.hip: pair counts, gray
// histogram, pooled gather; evaluate.hip: cross matrix, run lengths; wordregion.h and its kernels; neighbours.hip) are written
// once over a word SOURCE and instantiated for both layouts,
//
//   PlaneWords   full-frame planes [M, H, wpr]
//   CropWords    crop-framed sets (cropops.hip: room, offsets, payload)
//
// A source hands out a View: the rectangle of the GLOBAL word grid (rows y0 .. y0 + rows - 1 x word columns c0 .. c0 + cols - 1)
// that mask m owns, row-major at p.  Bit (x & 31) of word (x >> 5) in both layouts, so two views over one frame share the
// word alignment and |a & b| needs no shifts.  A plane is the view that covers the whole frame.
#pragma once
#include "common.h"

namespace mwords {

struct View {
    const uint32_t* p;
    int y0, c0, rows, cols;          // first row, first word column, extent (rows == 0: empty)
};

struct PlaneWords {
    const uint32_t* masks;
    int H, wpr;
    const long* index;               // optional: mask m is plane index[m] (the pooled gather)
    __device__ __forceinline__ View view(long m) const { return View{masks + (index ? index[m] : m) * H * wpr, 0, 0, H, wpr}; }
};

struct CropWords {
    const uint32_t* payload;
    const int* room;                 // [M, 4] y0, x0, y1, x1 (inclusive), -1: empty
    const long* offsets;
    __device__ __forceinline__ View view(long m) const {
        const int4 r = reinterpret_cast<const int4*>(room)[m];
        const int c0 = r.y >> 5;
        return View{payload + offsets[m], r.x, c0, r.x < 0 ? 0 : r.z - r.x + 1, r.x < 0 ? 0 : (r.w >> 5) - c0 + 1};
    }
};

// Pixel (y, x) of the frame as view v stores it: 0 for every pixel outside the view, so a kernel that looks one pixel past
// a mask's box (the run-length encoder reads the last row of the column before it) never reads another mask's words.
__device__ __forceinline__ uint32_t pixel(const View v, int y, int x) {
    const int ly = y - v.y0, lx = (x >> 5) - v.c0;
    if (ly < 0 || ly >= v.rows || lx < 0 || lx >= v.cols) return 0u;
    return (v.p[(long)ly * v.cols + lx] >> (x & 31)) & 1u;
}

// The word-granular sibling of pixel(): word column wx of row y of the frame as view v stores it, 0 outside the view and never
// fetched there.
__device__ __forceinline__ uint32_t word_at(const View v, int y, int wx) {
    const int ly = y - v.y0, lx = wx - v.c0;
    if ((unsigned)ly >= (unsigned)v.rows || (unsigned)lx >= (unsigned)v.cols) return 0u;
    return v.p[(long)ly * v.cols + lx];
}

// The box b of a mask clipped to the frame and to its view v: rows y0 .. y1, word columns c0 .. c1 (empty: returns false) -- for
// one mask what pair_count's window is for two.
__device__ __forceinline__ bool clipped_box(const View v, const int4 b, int H, int W, int& y0, int& y1, int& c0, int& c1) {
    if (b.x < 0 || v.rows == 0) return false;
    y0 = max(max(b.x, 0), v.y0);
    y1 = min(min(b.z, H - 1), v.y0 + v.rows - 1);
    c0 = max(max(b.y, 0) >> 5, v.c0);
    c1 = min(min(b.w, W - 1) >> 5, v.c0 + v.cols - 1);
    return y0 <= y1 && c0 <= c1;
}

// popcount(a & b) over the intersection of two tight boxes (y0, x0, y1, x1), each operand addressed with its own view's
// stride; the lanes of the caller share the words (it reduces the result over them).  The window is clipped to both
// views, so a box that is not inside its view cannot make a thread read outside its mask's words.
// UNROLL trips of the window loop are issued together: the pair matrix, one WAVE per pair, asks for 8 (32 loads in flight per
// lane on a long window, what its plane form has always had); 1 leaves the loop rolled.
template <int UNROLL>
__device__ __forceinline__ int pair_count(const View a, const int4 ba, const View b, const int4 bb, int lane, int nlanes) {
    if (ba.x < 0 || bb.x < 0 || a.rows == 0 || b.rows == 0) return 0;
    const int y0 = max(max(ba.x, bb.x), max(a.y0, b.y0));
    const int y1 = min(min(ba.z, bb.z), min(a.y0 + a.rows, b.y0 + b.rows) - 1);
    const int x0 = max(ba.y, bb.y), x1 = min(ba.w, bb.w);
    if (y0 > y1 || x0 > x1) return 0;
    const int wx0 = max(x0 >> 5, max(a.c0, b.c0));
    const int wx1 = min(x1 >> 5, min(a.c0 + a.cols, b.c0 + b.cols) - 1);
    if (wx0 > wx1) return 0;
    const int rw = wx1 - wx0 + 1, rh = y1 - y0 + 1;
    const uint32_t* qa = a.p + (long)(y0 - a.y0) * a.cols + (wx0 - a.c0);
    const uint32_t* qb = b.p + (long)(y0 - b.y0) * b.cols + (wx0 - b.c0);
    int c = 0;
#pragma unroll UNROLL
    for (int t = lane; t < rh * rw; t += nlanes) {
        const int ly = t / rw, lx = t - ly * rw;
        c += __popc(qa[(long)ly * a.cols + lx] & qb[(long)ly * b.cols + lx]);
    }
    return c;
}

// Word column wx of row y of the frame [H, W] after tile mask `src` ([sh, ceil(sw / 32)] words) is resized to
// (tile_h, tile_w) with cv2's INTER_NEAREST rule (float64 index, floor, clamp) and pasted at (xo, yo).  Bits outside the
// tile and the frame are 0, the padding bits beyond column W - 1 included.
__device__ __forceinline__ uint32_t placed_word(const uint32_t* __restrict__ src, int sh, int sw, int tile_h, int tile_w, int xo, int yo,
                                                int H, int W, int y, int wx) {
    const int ty = y - yo;
    if (y < 0 || y >= H || ty < 0 || ty >= tile_h) return 0u;
    const double fy = 1.0 / ((double)tile_h / (double)sh), fx = 1.0 / ((double)tile_w / (double)sw);
    const int sy = min((int)floor((double)ty * fy), sh - 1);
    const uint32_t* srow = src + (long)sy * ((sw + 31) >> 5);
    uint32_t bits = 0u;
    for (int bb = 0; bb < 32; ++bb) {
        const int x = wx * 32 + bb;
        if (x >= W) break;
        const int tx = x - xo;
        if (x < 0 || tx < 0 || tx >= tile_w) continue;
        const int sx = min((int)floor((double)tx * fx), sw - 1);
        bits |= ((srow[sx >> 5] >> (sx & 31)) & 1u) << bb;
    }
    return bits;
}

}  // namespace mwords

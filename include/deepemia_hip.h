/*
 * deepemia_hip.h -- C ABI of libdeepemia_hip.so (gfx950 / MI355X only).
 *
 * This is the drop-in boundary for ONE path of Deam0on/deepEMIA: the
 * Detectron2 `DefaultPredictor.__call__` that the reference invokes at
 *   src/functions/inference.py:1395, 1398, 1507, 1669   (predictor(image))
 * built by src/data/models.py:103-107 (load_model -> DefaultPredictor(cfg)),
 * plus the per-mask post-processing / dedup / measurement reductions that the
 * reference runs on the host afterwards.
 *
 * Conventions
 *   - every entry point is `extern "C"`, takes raw DEVICE pointers + sizes +
 *     a `hipStream_t` (passed as void*), and returns 0 on success or a negative
 *     DEMIA_E* code; no exceptions cross the ABI, nothing is allocated or freed
 *     behind the caller's back, no ownership is transferred;
 *   - all launches are asynchronous on the given stream and graph-capturable
 *     (no hipMalloc / hipFree / sync inside);
 *   - tensors are NHWC ("pixel-major, channel-minor"); `dtype` is 0 = f32,
 *     1 = bf16;
 *   - re-entrant per stream; one host thread per GPU.
 */
#ifndef DEEPEMIA_HIP_H
#define DEEPEMIA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEMIA_OK 0
#define DEMIA_EINVAL (-1)   /* bad shape / unsupported combination            */
#define DEMIA_ELAUNCH (-2)  /* hipLaunch / runtime error (see demia_last_error) */

#define DEMIA_F32 0
#define DEMIA_BF16 1
#define DEMIA_F32X3 2   /* conv only: f32 activations, weights pre-split into 3 bf16 planes, tiled (see demia_conv2d_nhwc) */
#define DEMIA_BF16X2 3  /* conv only: f32 activations, weights as 2 bf16 planes (same tiling): 16-bit operands */
#define DEMIA_F16X2 4   /* conv only: f32 activations, weights as 2 fp16 planes (same tiling), power-of-two operand scales */
#define DEMIA_P32 5     /* activations as two pre-scaled fp16 planes, [pixels][C / 32][2][32] behind a 128-byte zero header
                           (demia_conv2d_p32 below); taken by demia_roi_align and demia_maxpool3x3s2_p32 */

#define DEMIA_ACT_NONE 0
#define DEMIA_ACT_RELU 1
#define DEMIA_ACT_SIGMOID 2

#define DEMIA_RES_NONE 0
#define DEMIA_RES_SAME 1      /* residual has the output's shape                      */
#define DEMIA_RES_UP2 2       /* residual is (Ho/2 rounded up, Wo/2 rounded up): nearest x2  */

/* library / device info ------------------------------------------------------------*/
int demia_abi_version(void);
const char* demia_last_error(void);
const char* demia_build_arch(void);   /* "gfx950" */
/* "product": what the default path runs -- the P32 conv kernel (f16x2 / f16), the exact-f32 conv kernel (the parity suite's control
 * arithmetic), every non-conv kernel.  "dev" (`make DEV=1` -> libdeepemia_hip_dev.so, loaded with DEEPEMIA_DEV_LIB=1): also the
 * kernels of the non-default precisions behind demia_conv2d_nhwc (f32x3, bf16x2, f16x2r, bf16) and the experimental tiles /
 * schedules of the P32 kernel reachable through tile hints.  Same symbols in both. */
const char* demia_build_flavor(void);
/* A HIP stream restricted to the compute units whose bit is set in mask (bit i of word i / 32; words = 8 for the 256 CUs of an
 * MI355X) -- hipExtStreamCreateWithCUMask behind the C ABI, so that the host side (which holds streams as torch objects) can give
 * the network's stream a mask that leaves a few CUs per XCD to the latency-bound post-processing kernels of the images in flight.
 * The caller owns the stream: demia_stream_destroy.  Replaces nothing in the reference (its loop is sequential,
 * inference.py:713-942). */
int demia_stream_create_cu_mask(const uint32_t* mask, int words, void** stream);
int demia_stream_destroy(void* stream);
/* Single-plane arithmetic is chosen PER LAUNCH (`single` of demia_conv_p32_desc / demia_roialign_desc, the `single` argument of
 * the stem / pool entry points), never process-wide: engines of different precisions may share the library.
 * (demia_conv2d_p32_single is the conv entry point demia_conv2d_p32 forwards to when d->single != 0: the same source compiled
 * with one MFMA per product; same descriptor.) */
struct demia_conv_p32_desc;
int demia_conv2d_p32_single(const struct demia_conv_p32_desc* d, void* stream);

/* a3: convolution as implicit GEMM on MFMA -------------------------------------------
 * Replaces every Conv2d(+FrozenBatchNorm)(+ReLU)(+residual add) / Linear /
 * ConvTranspose2d(k2,s2) that Detectron2's GeneralizedRCNN runs inside
 * predictor(image) (inference.py:1395).
 *   in        [N, H, W, Cin]        dtype `dtype`
 *   w         [CoutPad, KH, KW, Cin] dtype `dtype`, CoutPad = multiple of 32 >= Cout
 *   scale/bias [Cout] f32 or NULL    y = acc * scale + bias   (FrozenBN folded / conv bias)
 *   residual  NULL or out-shaped (RES_SAME) / half-res (RES_UP2), dtype `out_dtype`
 *   out       [N, Ho, Wo, Cout]      dtype `out_dtype`
 * Cin must be a multiple of 64 (bf16) / 32 (f32, f32x3, f16x2, bf16x2).  dtype DEMIA_F32X3 computes the f32 product on the bf16
 * matrix pipe from three-way split operands (six bf16 MFMAs per f32 FMA tile, error ~ one f32 rounding): `in` is
 * f32, `w` holds the three bf16 planes of the f32 weights, CoutPad % 64 == 0, output f32.  DEMIA_BF16X2 is the same
 * with two planes and three MFMAs (16 significand bits per operand, error <= 3 * 2^-16 per product).
 * Layout of `w` for these two dtypes (NP = 3 / 2 planes, x = x1 + x2 + x3 with x1 = bf16(x), x2 = bf16(x - x1), ...):
 *   [CoutPad / 64][KH*KW*Cin / 32][NP][64][32] bf16,  K = (kh, kw, cin) walked in steps of 32
 * i.e. the 64-channel x 32-k piece of one plane that a K-step reads is 4 KiB contiguous (whole 128-byte lines per
 * wave load).  ABI version 3 (version 2 took row-major [NP][CoutPad][K] planes).
 * DEMIA_F16X2: two fp16 planes per operand (x1 = half(x), x2 = half(x - x1): 22 significand bits, error <= 3 * 2^-22
 * per product -- an f32-sized error from three MFMAs).  fp16 has five exponent bits, so the caller brings the weights
 * into range with an exact power of two per output channel BEFORE splitting them (and divides `scale` by it), and
 * the kernel scales the activations by 2^(13 - ilogb(*amax_in)); `amax_in` is a device scalar holding an upper bound
 * of |in| (NULL: no scaling, |in| must stay below 6e4).  `amax_out` (any dtype, may be NULL): device scalar into
 * which the kernel accumulates max |out| with an atomic max -- zero it before the launch; it is the next layer's
 * `amax_in`.  DEMIA_F16X2 takes its planes in the same tiling, [CoutPad / 64][K / 32][2][64][32] fp16.  */
typedef struct demia_conv_desc {
    const void* in;
    const void* w;
    const float* scale;
    const float* bias;
    const void* residual;
    void* out;
    int32_t N, H, W, Cin;
    int32_t Ho, Wo, Cout, CoutPad;
    int32_t KH, KW, stride, pad;
    int32_t dtype, out_dtype;
    int32_t act, res_mode;
    int32_t out_ld;          /* elements between consecutive output pixels (>= Cout); 0 -> Cout */
    int32_t tile_hint;       /* 0 = auto; else BN in {128, 64, 32} */
    const float* amax_in;    /* DEMIA_F16X2: device scalar, upper bound of |in| (see above); else ignored */
    float* amax_out;         /* NULL or device scalar: max |out| is accumulated (atomic max) */
} demia_conv_desc;
int demia_conv2d_nhwc(const demia_conv_desc* d, void* stream);
/* K-step of this build's DEMIA_F16X2 kernel = innermost extent of its weight-plane tiling (32 unless built otherwise) */
int demia_conv_f16x2_kstep(void);

/* a3: the same convolution with BOTH operands pre-split into fp16 planes ("P32" activations) -------------------
 * The default arithmetic of the product path (precision "f16x2"): f32-sized error from three fp16 MFMAs per
 * product, operands moved global -> LDS by LDS-DMA.  Replaces the same Detectron2 layers as demia_conv2d_nhwc.
 *   P32 activation buffer: 128 zero bytes, then [pixels][C / 32][2][32] fp16 -- per pixel and 32-channel group one
 *       128-byte line of 32 high halves + 32 low halves of x * s (s = meta[1], an exact power of two; x = (h + l) / s).
 *       The caller zeroes the 128-byte header once; padding taps read it.
 *   meta: 2 device floats per tensor: [0] = max |x| (atomic max, accumulated by the producing kernel; the caller zeroes
 *       it before every forward), [1] = s (written by the producing kernel).
 *   w: [CoutPad / 64][ksteps][64][2][32] fp16, ksteps = (Cin / 32) * KH * KW walked channel-group OUTER, tap inner;
 *       planes of w * 2^e(co) (max |.| in [2^14, 2^15) per output channel, the caller divides `scale` by 2^e(co)).
 *   wbound = max_co(|scale_co| * sum_k |w_co,k|) (true weights), bbound = max |bias|: the kernel scales its P32 output
 *       with s = 2^(14 - ilogb(in_meta[0] * wbound + bbound + res_meta[0])), so that |out * s| < 2^15.
 *   out: P32 (out_f32 = 0; Cout % 32 == 0; out_meta required) or plain f32 [M, out_ld] (out_f32 = 1).
 *   residual: P32 of the output's shape (RES_SAME) or half resolution (RES_UP2), with its meta.               */
typedef struct demia_conv_p32_desc {
    const void* in;
    const float* in_meta;
    const void* w;
    const float* scale;
    const float* bias;
    const void* residual;
    const float* res_meta;
    void* out;
    float* out_meta;
    float wbound, bbound;
    int32_t N, H, W, Cin;
    int32_t Ho, Wo, Cout, CoutPad;
    int32_t KH, KW, stride, pad;
    int32_t act, res_mode;
    int32_t out_f32;
    int32_t out_ld;          /* f32 output: elements between consecutive output pixels (>= Cout); 0 -> Cout */
    int32_t tile_hint;       /* 0 = auto (a cost model fitted on MI355X picks the tile); else the id of an instantiated tile (tuning) */
    /* Optional fused 1x1 head (head_n in 1..4, Cout % 256 == 0): instead of writing the P32 output, every 256-channel block
     * b of an activated output row m is multiplied by head_w [head_n][256] (+ head_b, then head_act) and stored as f32 at
     * head_out[(m * (Cout / 256) + b) * head_ld + j].  Used for the mask head: ConvTranspose2d(k2, s2) as a GEMM onto
     * (dy, dx, co) + ReLU, then the class predictor + sigmoid -- the 4 x 256-channel deconv output never reaches HBM.   */
    const float* head_w;
    const float* head_b;
    float* head_out;
    int32_t head_n, head_ld, head_act;
    /* Scale groups.  groups <= 1: one {max |x|, s} pair per tensor (in_meta, res_meta, out_meta point at 2 floats).
     * groups > 1: the metas are [groups][2] and output row m of this call belongs to group (m + row0) / group_rows -- one
     * group per IMAGE of the batch, so that the planes (and therefore the results) of an image do not depend on what
     * else is in the batch.  group_rows >= 128; row0 is the global index of this call's first output row when a tensor
     * goes through in several calls.                                                                                   */
    int32_t groups, group_rows, row0;
    /* 0: f16x2 -- three MFMAs per product (the default, f32-sized error).  1: ONE MFMA per product on the high planes of both
     * operands (fp16 operands, f32 accumulation: the arithmetic of the reference's autocast predictor, inference.py:1390-1395),
     * output still split into both planes -- the per-stage precision map of DESIGN.md section 7 runs single stages this way.
     * 2: as 1, and the output's low plane is written as zeros (`--precision f16`, flagged NON-parity, every layer).          */
    int32_t single;
    /* Optional fused 1x1 LAYER (head_planes != NULL; head_n must be 0): the P32 output of this layer (Cout == CoutPad == 256, no
     * residual, single == 0) is consumed in the epilogue by a 1x1 stride-1 layer of head_cout <= 16 output channels with f32
     * output, and never written -- `out` and `out_meta` are not touched and may be NULL.  head_planes: that layer's weights in
     * the `w` tiling above ([CoutPad / 64][8][64][2][32] fp16, Cin = 256; the first 16 output channels are read), head_scale /
     * head_bias: its `scale` / `bias` ([head_cout] f32 or NULL).  Row m of the result goes to head_out[m * head_ld + j], j <
     * head_cout (head_ld >= head_cout; the other columns are not written).  The result is BIT-IDENTICAL to running the two
     * layers as two calls (planes out, then out_f32 = 1): same planes of v * s, same product order.  Used for the RPN head
     * (3x3 conv + ReLU, then objectness + anchor deltas).                                                                  */
    const void* head_planes;
    const float* head_scale;
    const float* head_bias;
    int32_t head_cout;
} demia_conv_p32_desc;
int demia_conv2d_p32(const demia_conv_p32_desc* d, void* stream);

/* a3: Pillow-exact ResizeShortestEdge + (x - mean) + zero pad -------------------------
 * Replaces T.ResizeShortestEdge.get_transform(img).apply_image(img) +
 * normalisation + ImageList.from_tensors inside DefaultPredictor.__call__ /
 * GeneralizedRCNN.preprocess_image (Detectron2 0.6), called from inference.py:1395.
 * Two separable 8-bit fixed-point passes (22-bit coefficients) identical to
 * Pillow's ImagingResample.  Coefficient tables are computed by the host.
 *   src     [N, H, W, 3] u8 (BGR)         tmp [N, H, newW, 3] u8
 *   xmin/xsize [newW] i32, xk [newW, ksx] i32; same for y
 *   dst     [N, PH + 6, PW + 8, 4] `dtype`: interior at (+3, +3) holds the
 *           normalised image, channel 3 and every border / pad element = 0.   */
int demia_resize_h_u8(const uint8_t* src, uint8_t* tmp, int N, int H, int W, int newW,
                      const int32_t* xmin, const int32_t* xsize, const int32_t* xk, int ksx, void* stream);
int demia_resize_v_norm(const uint8_t* tmp, void* dst, int N, int H, int newW, int newH, int PH, int PW,
                        const int32_t* ymin, const int32_t* ysize, const int32_t* yk, int ksy,
                        const float* mean3, int dtype, void* stream);

/* a2: tile upscale, cv2.resize(tile, (w*f, h*f), INTER_LINEAR) on u8 BGR (inference.py:2379-2382) ------
 * OpenCV's fixed-point bilinear: xofs/yofs [out, 2] i32 source indices, ialpha/ibeta [out, 2] i16
 * 11-bit coefficients (host tables, deepemia_amd.engine.cv_linear_tables). src [N,H,W,3] -> dst [N,oh,ow,3] */
int demia_resize_linear_u8(const uint8_t* src, uint8_t* dst, int N, int H, int W, int out_h, int out_w,
                           const int32_t* xofs, const int16_t* ialpha, const int32_t* yofs, const int16_t* ibeta,
                           void* stream);

/* a3: ResNet stem: conv 7x7 s2 p3 (3->64) + FrozenBN + ReLU, then maxpool 3x3 s2 p1 ----
 *   in   [N, PH + 6, PW + 8, 4] f32 (see above)    w [7, 8, 4, 64] f32 (kh, kw, c, co; kw 7 and c 3 zero)
 *   mid  [N, PH/2, PW/2, 64]   out [N, PH/4, PW/4, 64]                              */
int demia_stem_conv(const void* in, const void* w, const float* scale, const float* bias, void* mid,
                    int N, int PH, int PW, int dtype, void* stream);
/* The same stem (7x7 s2 p3 + FrozenBN + ReLU, f32 NHWC out) on the matrix pipe in the f16x2 arithmetic: the input is split
 * into two fp16 planes of x * s_in (s_in an exact power of two with |x| s_in < 2^15) while it is staged, w_planes
 * [2][7][64][32] fp16 hold w * 2^e(co) with K ordered (kh, kw padded to 8, c padded to 4), and `scale` carries the FrozenBN
 * scale divided by s_in * 2^e(co).  Replaces the same Detectron2 BasicStem.conv1 as demia_stem_conv. */
int demia_stem_conv_mfma(const float* in, const void* w_planes, const float* scale, const float* bias, float* mid, int N,
                         int PH, int PW, float s_in, void* stream);
/* ... and stem + max pool (3x3 s2 p1) in ONE kernel, P32 planes out: the f32 stem output is never written.  out / out_meta /
 * s_out / groups as demia_maxpool3x3s2_p32 (s_out = the planes' power-of-two scale from the a-priori bound of the stem output). */
int demia_stem_pool_mfma(const float* in, const void* w_planes, const float* scale, const float* bias, void* out, float* out_meta,
                         int N, int PH, int PW, float s_in, float s_out, int groups, int single, void* stream);
/* The fused front end: both Pillow passes in ONE launch, and the stem + pool reading its bytes.
 *   dst  [N, PH + 6, PW + 8] pixels of four BYTES (c0, c1, c2, flag) in the geometry of the f32 stem input above.
 *        Decoding rule: x[c] = flag ? (float)c_c - mean[c] : 0 for c < 3, x[3] = 0 -- bit for bit the f32 buffer that
 *        demia_resize_h_u8 + demia_resize_v_norm write.  The kernel stores (c0, c1, c2, 1) for the newH x newW image pixels
 *        at (+3, +3) and NOTHING else: border and padding are recognised by flag = 0 in a buffer the caller zeroed once.
 *        dst is 16-byte aligned.  `tmp` does not exist: the horizontally resized rows (rounded and clipped to u8, as Pillow's)
 *        live in an LDS ring of ksy rows.  W == newW: no horizontal pass (x tables may be NULL).  The tables are monotone.
 *   strip  output rows per workgroup; <= 0: chosen from the grid size.
 * demia_resize_hv_fits: the kernel's LDS bytes, or 0 when a source row of W pixels and ksy ring rows of newW pixels do not
 * fit its 60 KiB window -- then demia_resize_hv_u8x4 fails and the two launches above are the path. */
int64_t demia_resize_hv_fits(int W, int newW, int ksy);
int demia_resize_hv_u8x4(const uint8_t* src, void* dst, int N, int H, int W, int newH, int newW, int PH, int PW,
                         const int32_t* xmin, const int32_t* xsize, const int32_t* xk, int ksx,
                         const int32_t* ymin, const int32_t* ysize, const int32_t* yk, int ksy, int strip, void* stream);
/* demia_stem_pool_mfma on that buffer (8-byte aligned): staging decodes by the rule above with the host array mean3, then
 * the same multiply by s_in and plane split; planes and meta are bit-identical to demia_stem_pool_mfma on the f32 buffer. */
int demia_stem_pool_mfma_u8(const uint8_t* in, const float* mean3, const void* w_planes, const float* scale, const float* bias,
                            void* out, float* out_meta, int N, int PH, int PW, float s_in, float s_out, int groups, int single,
                            void* stream);
int demia_maxpool3x3s2(const void* in, void* out, int N, int H, int W, int C, int dtype, void* stream);
/* the same pool from an f32 input into a P32 buffer scaled with the power of two `s` (the caller derives it from the
 * stem's a-priori bound); out_meta receives {max |out| (atomic max; zero it first), s} -- one pair (groups <= 1) or one
 * per image (groups == N, see demia_conv_p32_desc).  C % 32 == 0.  single != 0: the low plane is written as zeros
 * (`--precision f16`, as in demia_conv_p32_desc.single = 2). */
int demia_maxpool3x3s2_p32(const float* in, void* out, float* out_meta, float s, int N, int H, int W, int C, int groups, int single,
                           void* stream);
/* LastLevelMaxPool (kernel 1, stride 2): p6 = p5[:, ::2, ::2, :] */
int demia_subsample2(const void* in, void* out, int N, int H, int W, int C, int dtype, void* stream);

/* a3: RPN proposal selection --------------------------------------------------------
 * Replaces RPN.predict_proposals / find_top_rpn_proposals (Detectron2 0.6):
 * per image and level the top `pre_topk` objectness logits in STABLE descending
 * order (ties: lower flattened (h, w, a) index first), anchor generation + delta
 * decode (weights 1,1,1,1, clamp log(1000/16)), clip to the image, drop non-finite /
 * empty boxes, per-level hard NMS (IoU > thresh suppresses), then the `post_topk`
 * best survivors over all levels in stable descending score order.
 *   head[l]   [N, H_l, W_l, head_ld] f32: channels 0..2 = logits (a), 3..14 = deltas (a*4 + c)
 *   out_boxes [N, post_topk, 4] f32, out_scores [N, post_topk] f32, out_count [N] i32
 *   workspace: demia_rpn_workspace_bytes(N) bytes                                      */
typedef struct demia_rpn_desc {
    const float* head[5];
    int32_t H[5], W[5], stride[5];
    const float* cell_anchors;   /* HOST pointer, [5][3][4] f32: (x1,y1,x2,y2) of anchor a at the origin */
    int32_t head_ld;
    int32_t N;
    int32_t img_h, img_w;        /* unpadded network-input size boxes are clipped to */
    int32_t pre_topk, post_topk; /* 1 <= pre_topk <= 1000, 1 <= post_topk <= 1024; head_ld >= 15 (else DEMIA_EINVAL) */
    float nms_thresh;
    float* out_boxes;
    float* out_scores;
    int32_t* out_count;
    void* workspace;
} demia_rpn_desc;
int64_t demia_rpn_workspace_bytes(int N);
int demia_rpn_proposals(const demia_rpn_desc* d, void* stream);

/* a3: ROIAlignV2 (aligned, sampling_ratio 0 = adaptive) over p2..p5 -------------------
 * Replaces ROIPooler.forward -> torchvision.ops.roi_align(aligned=True) incl. the
 * FPN level assignment floor(4 + log2(sqrt(area)/224 + 1e-8)) clamped to [2, 5].
 *   feat[l] [N, H_l, W_l, C] `dtype`; boxes [N, R, 4] f32 (network-input coords);
 *   count [N] i32 (rows >= count[n] are written as zeros); out [N, R, P, P, C] `dtype`
 * dtype DEMIA_P32: feat[l] / out are P32 buffers (pointers to their 128-byte headers); taps and averages are convex
 * combinations, so the output takes the coarsest of the levels' scales and the largest of their max |x|. */
typedef struct demia_roialign_desc {
    const void* feat[4];
    int32_t H[4], W[4];
    int32_t N, R, C, P, dtype;
    const float* boxes;
    const int32_t* count;
    void* out;
    const float* meta[4];    /* dtype DEMIA_P32: {max |x|, s} of each level (device floats); else ignored */
    float* out_meta;         /* dtype DEMIA_P32: receives {max over the levels' max |x|, min over the levels' s} */
    int32_t groups;          /* dtype DEMIA_P32: <= 1 = one meta pair per tensor; N = metas are [N][2], one scale group per image */
    int32_t single;          /* dtype DEMIA_P32: != 0 writes a zero low plane (`--precision f16`) */
    const int32_t* order;    /* NULL, or [N * R] from demia_roi_order: workgroup b pools ROI order[b] (the output row of a ROI stays
                              * where it is: same results, neighbouring workgroups share feature lines in one XCD's L2) */
} demia_roialign_desc;
int demia_roi_align(const demia_roialign_desc* d, void* stream);
/* The launch order for demia_roi_align: per image its R (<= 1024) ROIs sorted by (FPN level, row band, column) of the box centre,
 * dealt to the eight XCDs in runs of R / 8.  boxes [N, R, 4] f32 (network-input coords), count [N]; order [N * R] i32 out. */
int demia_roi_order(const float* boxes, const int32_t* count, int N, int R, int32_t* order, void* stream);

/* a3: Fast R-CNN inference ---------------------------------------------------------
 * Replaces FastRCNNOutputLayers.inference / fast_rcnn_inference_single_image:
 * softmax over K+1 logits, class-specific delta decode (weights 10,10,5,5), clip,
 * score > thresh (strict), candidates in row-major (proposal, class) order, stable
 * descending sort, per-class hard NMS (IoU > 0.5), first `topk` survivors.
 *   logits [N, R, ld] f32: channels 0..K = class logits, K+1 .. K+4K = deltas
 *   props  [N, R, 4] f32, prop_count [N] i32
 *   det_boxes [N, topk, 4] f32 (network-input coords), det_scores [N, topk] f32,
 *   det_classes [N, topk] i32, det_count [N] i32;  0 < topk <= 1024 (Detectron2's TEST.DETECTIONS_PER_IMAGE; the kept list lives in LDS, 24 bytes per slot;
 *   the rows of a smaller topk are the first rows of a larger one's); rows past det_count are zero; any number of classes K as long as
 *   R * min(K, floor(1 / score_thresh)) <= 4096 (a softmax row has at most floor(1 / thresh) scores above thresh;
 *   R = 1000: every K for thresholds above 0.2, K <= 4 below)                                            */
typedef struct demia_dets_desc {
    const float* logits;
    int32_t ld;
    const float* props;
    const int32_t* prop_count;
    int32_t N, R, K;
    int32_t img_h, img_w;
    float score_thresh, nms_thresh;
    int32_t topk;
    float* det_boxes;
    float* det_scores;
    int32_t* det_classes;
    int32_t* det_count;
} demia_dets_desc;
int demia_box_detections(const demia_dets_desc* d, void* stream);

/* a3: mask paste (paste_masks_in_image / _do_paste_mask, Detectron2 0.6) --------------
 * Boxes are rescaled to the original image (scale_x = out_w / img_w ...), clipped,
 * empty boxes flagged; each 28x28 probability map is resampled with bilinear
 * grid_sample(align_corners=False, zero padding) and thresholded (>= 0.5).
 *   mask_logit_or_prob [N*D, 196, 4, ld] f32 -- deconv-blocked layout: pixel (2y+dy, 2x+dx)
 *        of instance i lives at [(i*196 + y*14 + x), dy*2+dx, class]; already sigmoid-ed
 *   det_boxes [N, D, 4] f32 network-input coords, det_classes, det_count as above
 *   out_boxes [N, D, 4] f32 output-image coords (clipped); valid [N, D] u8 (nonempty)
 *   packed    [N, D, out_h, ceil(out_w/32)] u32 : bit (x & 31) of word x>>5 = mask[y][x]; the padding bits of
 *             a partial last word are always 0.  Every packed-mask entry point takes the TRUE width W.   */
typedef struct demia_paste_desc {
    const float* mask_prob;
    int32_t ld;
    const float* det_boxes;
    const int32_t* det_classes;
    const int32_t* det_count;
    int32_t N, D;             /* any N * D that an int32 holds */
    int32_t img_h, img_w;     /* network-input size */
    int32_t out_h, out_w;     /* original image size */
    float* out_boxes;
    uint8_t* valid;
    uint32_t* packed;
    int32_t* out_bbox;        /* optional [N, D, 4] i32: y0, x0, y1, x1 (inclusive) of the pixels the paste can set,
                                 -1 for invalid instances -- the bbox hint of the packed-mask entry points */
    const int32_t* prev_bbox; /* optional [N, D, 4] i32 (incremental paste): `packed` is known to be ZERO outside these boxes
                                 (the out_bbox of the previous paste into the same buffer; all -1 after a memset) -- only the
                                 union of each instance's old and new box is written instead of whole 512-KiB planes.
                                 Must not alias out_bbox; needs out_bbox. */
} demia_paste_desc;
int demia_paste_masks(const demia_paste_desc* d, void* stream);
/* packed bits -> Detectron2's (M, H, W) bool bytes (pred_masks drop-in layout) */
int demia_unpack_masks(const uint32_t* packed, uint8_t* out_bool, int64_t M, int H, int W, void* stream);
/* per-mask popcount ("np.sum(mask)", inference.py:1688, 2599) and tight bbox [M,4] = y0,x0,y1,x1 (inclusive; -1 if empty).
 * hint (optional, [M,4]): a box known to contain every set pixel of the mask; only that region is read. */
int demia_mask_area_bbox(const uint32_t* packed, const int32_t* hint, int32_t* area, int32_t* bbox, int64_t M, int H, int W,
                         void* stream);

/* a9-a15: packed-mask morphology (all masks [M, H, ceil(W/32)] u32, W = true pixel width) ---------------
 * Replace, on bit-packed device masks, what the reference does with scipy / scikit-image / numpy on
 * dense host arrays.  demia_mask_program runs a sequence of per-mask stages IN PLACE on the bbox region
 * of every mask (one workgroup per mask, region staged in LDS; the frame outside the box is not touched):
 *   DEMIA_MOP_FILL        scipy.ndimage.binary_fill_holes        (mask_utils.py:75; inference.py:193, 1780)
 *   DEMIA_MOP_DILATE /    skimage dilation / erosion, 3x3 cross, 'reflect' border
 *   DEMIA_MOP_ERODE                                              (mask_utils.py:76; inference.py:196-198, 1786-1796)
 *   DEMIA_MOP_DROP_MULTI  if skimage.measure.label(mask).max() > 1 (8-connected): mask[:] = 0
 *                                                                (mask_utils.py:79-81)
 *   DEMIA_MOP_FLAG_MULTI  the same test without changing the mask
 *   DEMIA_MOP_GATE        masks with active[m] == 0 (or active == NULL) stop here (inference.py:1443: the
 *                         fill -> erosion -> dilation of process_masks_parallel only runs for calls with > 2 masks)
 * program = up to 8 stage codes, 4 bits each, low nibble first, 0 ends it.
 *   bbox     [M, 4] i32 y0, x0, y1, x1 inclusive, -1 for empty masks; a SUPERSET of the tight box is fine
 *            (demia_mask_area_bbox, demia_paste_desc.out_bbox, or bbox_out of an earlier program)
 *   scratch  same shape as masks; only regions larger than 64 KiB of LDS use it
 *   area / bbox_out / flag (each optional): popcount and tight bbox of the result; flag = a *_MULTI stage fired.
 * Other entry points:
 *   overlap_prefix  overlap += mask; mask[overlap > 1] = 0 over the masks of one call, in order
 *                                                             (mask_utils.py:77-78); bbox optional (supersets ok)
 *   column_counts   np.sum(masks, axis=(0, 1)) (per-column pixel counts; `counts` pre-zeroed)
 *                                                             (mask_utils.py:62)
 *   pair_intersections  np.count_nonzero(a[pi[p]] & b[pj[p]]) (inference.py:431, 2710;
 *                                                              spatial_constraints.py:143, 186)
 *   place_tiles     cv2.resize(mask, (tile_w, tile_h), INTER_NEAREST) + paste into a zero (H, W)
 *                   frame at (x_off, y_off)                   (inference.py:2399-2420)
 * seg (overlap_prefix, column_counts): NULL, or a non-decreasing segment id per mask so that the masks of
 * many (tile, class) calls share ONE launch; column_counts then fills counts[S, W] (pre-zeroed).   */
enum { DEMIA_MOP_END = 0, DEMIA_MOP_FILL = 1, DEMIA_MOP_DILATE = 2, DEMIA_MOP_ERODE = 3, DEMIA_MOP_DROP_MULTI = 4,
       DEMIA_MOP_FLAG_MULTI = 5, DEMIA_MOP_GATE = 6 };
int demia_mask_program(uint32_t* masks, uint32_t* scratch, const int32_t* bbox, const uint8_t* active, uint32_t program,
                       int64_t M, int H, int W, int32_t* area, int32_t* bbox_out, int32_t* flag, void* stream);
/* The same with a WORKLIST [M + 2] i32 (device, contents ignored on entry): the launch over all masks handles the small
 * regions and lists the masks that need the 64-KiB-LDS variant, which then runs as a fixed grid over that list instead of
 * one workgroup per mask (three of four masks of a real batch are small).  worklist == NULL: demia_mask_program. */
int demia_mask_program_wl(uint32_t* masks, uint32_t* scratch, const int32_t* bbox, const uint8_t* active, uint32_t program,
                          int64_t M, int H, int W, int32_t* area, int32_t* bbox_out, int32_t* flag, int32_t* worklist, void* stream);
int demia_mask_overlap_prefix(uint32_t* masks, const int32_t* seg, const int32_t* bbox, int64_t M, int H, int W, void* stream);
int demia_mask_column_counts(const uint32_t* masks, const int32_t* seg, const int32_t* bbox, int64_t M, int H, int W,
                             int32_t* counts, void* stream);
int demia_mask_pair_intersections(const uint32_t* a, const uint32_t* b, const int32_t* pi, const int32_t* pj,
                                  const int32_t* bbox_a, const int32_t* bbox_b, int32_t* out, int64_t P,
                                  int H, int W, void* stream);
/* pair_matrix: the intersection counts of EVERY pair inside a segment (the masks of one tile or one class pass) in one
 * launch, with the pair list made on the device from the boxes -- what the greedy IoU loops (inference.py:1451-1459) and
 * step 2 of deduplicate_masks_smart (inference.py:2640-2671) ask for, without a host round trip to build the list.
 * first[i] / count[i]: first mask and length of mask i's segment; label (optional): only equal-label pairs are counted;
 * out [M, ld] pre-zeroed, out[i][j - first[i]] = np.count_nonzero(mask_i & mask_j) for j > i (upper triangle). */
int demia_mask_pair_matrix(const uint32_t* masks, const int32_t* bbox, const int32_t* first, const int32_t* count,
                           const int32_t* label, int32_t* out, int64_t M, int ld, int H, int W, void* stream);
/* Host-side decision loops (no GPU work): the reference's sequential greedy filters for a whole batch of tiles in one
 * native call over the integer tables the device reduced.  inter [n, ld] / row_first: the matrix of demia_mask_pair_matrix
 * (host copy).  greedy_keep: inference.py:1451-1459 per segment (keep[p] = 0 / 1).  dedup_smart: step 2 of
 * deduplicate_masks_smart, inference.py:2640-2671, bug for bug; items / scores / classes per tile entry,
 * bbox [n][4] = y0, x0, y1, x1 and area [n] per global mask; keep_out = kept LOCAL positions per tile in keeping order. */
int demia_host_greedy_keep(const int32_t* inter, int ld, const int32_t* row_first, const int64_t* area, const int32_t* seg_first,
                           const int32_t* seg_len, int S, double thr, uint8_t* keep);
int demia_host_dedup_smart(const int32_t* inter, int ld, const int32_t* row_first, const int64_t* area, const int64_t* bbox,
                           const int32_t* items, const double* scores, const int32_t* classes, const int32_t* tile_off, int T,
                           double thr, int32_t* keep_out, int32_t* keep_cnt);
/* The float columns of measurements_results.csv as text (inference.py:1209-1230 writes them with csv.writer, i.e. repr()):
 * vals [rows][cols] f64 -> per row the Python repr() of its floats joined by ',', rows separated by '\n'.  Returns the
 * bytes written, -1 if cap < rows * cols * 26 + rows. */
int64_t demia_host_repr_rows(const double* vals, int64_t rows, int cols, char* out, int64_t cap);
/* a16: the EncodedPixels column of R50_flip_results.csv (inference.py:917-925: `" ".join(map(str, rle_encoding(mask)))`,
 * mask_utils.py:17-35) for M masks in one host call, from the bbox-cropped packed words of demia_mask_crop_pack: 1-based
 * (start, length) pairs over the column-major flattening of an H-row frame, as decimal text separated by single blanks.
 * text_off [M + 1]: mask m's text is out[text_off[m] .. text_off[m + 1]).  Returns the bytes written, or -(bytes needed)
 * when cap is too small.  Host code: nothing here touches the GPU. */
int64_t demia_host_rle_text(const uint32_t* payload, const int32_t* bbox, const int64_t* offsets, int64_t M, int H,
                            char* out, int64_t cap, int64_t* text_off);
int demia_mask_place_tiles(const uint32_t* src, uint32_t* dst, const int32_t* x_off, const int32_t* y_off, int64_t T,
                           int src_h, int src_w, int tile_h, int tile_w, int H, int W, void* stream);
/* Instance tables (what the ranks exchange before the global duplicate / containment filters,
 * inference.py:2452-2460): the payload of mask m is its bbox rows x word columns, row-major, at payload[offsets[m]];
 * offsets [M] i64 = exclusive prefix sums of rows * word columns (0 for empty masks, bbox -1).  crop_unpack writes
 * the regions into `masks`, which the caller has zeroed.                                                           */
int demia_mask_crop_pack(const uint32_t* masks, const int32_t* bbox, const int64_t* offsets, int64_t M, int H, int W,
                         uint32_t* payload, void* stream);
/* dst[i] = src[index[i]] for masks that are ZERO OUTSIDE their bbox (every mask of this path is: paste hint, program
 * output): replaces the plane-to-plane gathers between the stages of the class loop (`masks[sel]` copies of the dense
 * reference, inference.py:1405-1440, 2452-2472).  Only the box is read; the destination plane is written once (zeros
 * outside the box).  index [M] i64 into src [*, H, W/32]; bbox [M, 4] (-1: empty -> a zero plane); dst [M, H, W/32]. */
int demia_mask_gather_regions(const uint32_t* src, const int64_t* index, const int32_t* bbox, int64_t M, int H, int W,
                              uint32_t* dst, void* stream);
/* The same gather into a POOL of planes that stay zero outside per-slot boxes: pool [>= M, H, W/32] zeroed once, prev [>= M, 4]
 * i32 initialised to -1.  Slot m receives src[index[m]] (zero outside bbox[m]); only the union of prev[m] and bbox[m] is
 * written, and prev[m] becomes bbox[m] grown by `grow` pixels -- the reach of the in-place stages that follow (a dilation:
 * 1).  For callers that consume a batch's planes before the pool comes round again (the tile-batch loop). */
int demia_mask_gather_regions_pooled(const uint32_t* src, const int64_t* index, const int32_t* bbox, int64_t M, int H, int W,
                                     uint32_t* pool, int32_t* prev, int grow, void* stream);
int demia_mask_crop_unpack(const uint32_t* payload, const int32_t* bbox, const int64_t* offsets, int64_t M, int H, int W,
                           uint32_t* masks, void* stream);

/* Crop-framed mask sets (csrc/cropops.hip): the stages after the tile -> global mapping on masks kept in the global frame as
 * (room, cropped words) instead of planes [M, H, W/32].  room [M, 4] i32 = (y0, x0, y1, x1) inclusive, -1 = empty: the rectangle
 * mask m's words are stored for, laid out exactly as demia_mask_crop_pack lays out a bbox -- rows y0 .. y1 x the word columns
 * (x0 >> 5) .. (x1 >> 5) of the GLOBAL word grid, row-major at payload[offsets[m]]; bbox [M, 4] the TIGHT boxes (inside the
 * rooms; bits outside them and beyond column W - 1 are zero).  Nothing allocates; every entry is graph-capturable.
 * place_tiles: demia_mask_place_tiles (same nearest resize of the src_h x src_w tile-frame masks to tile_h x tile_w, same paste
 *   at (x_off, y_off), same clip at the frame edge) into each mask's room -- the caller's upper bound of its tight box --
 *   with area / tight bbox reduced on the way out; one workgroup per mask, which writes its own room only.
 * gather: dst[i] = src[index[i]] (dst_room[i] is the room of src mask index[i]).
 * reroom: dst[i] = src mask index[i] (i when index is NULL) stored for dst_room[i], in the same layout at dst[dst_offsets[i]]: a
 *   destination word inside the source room is a copy of the source word, any other destination word is zero (both rooms lie
 *   on the global word grid: no bit shifts); an empty destination room (-1) writes nothing.  max_dst_words >= the words of the
 *   largest destination room (the caller knows it from its own room tables): the grid is masks x slabs of it.  src and dst must
 *   not alias.  How a set is tightened to its boxes for the instance tables, and rebuilt from a gathered table's rows.
 * pair_matrix / pair_intersections: contract and output layout of demia_mask_pair_matrix / demia_mask_pair_intersections.
 * unpack_pooled: masks [first, first + n) into slots 0 .. n - 1 of a plane pool that stays zero outside prev (the rule of
 *   demia_mask_gather_regions_pooled): how the plane kernels (contours, measurements, histograms, programs) reach a set.
 * gray_histogram: contract, bins and BGR -> gray arithmetic of demia_mask_gray_histogram, read from the rooms' words in place. */
int demia_crop_place_tiles(const uint32_t* src, const int32_t* x_off, const int32_t* y_off, int64_t M, int src_h, int src_w,
                           int tile_h, int tile_w, int H, int W, const int32_t* room, const int64_t* offsets, uint32_t* payload,
                           int32_t* area, int32_t* bbox, void* stream);
int demia_crop_gather(const uint32_t* src, const int64_t* src_offsets, const int64_t* index, const int32_t* dst_room,
                      const int64_t* dst_offsets, int64_t M, uint32_t* dst, void* stream);
int demia_crop_reroom(const uint32_t* src, const int32_t* src_room, const int64_t* src_offsets, const int64_t* index,
                      const int32_t* dst_room, const int64_t* dst_offsets, int64_t M, int64_t max_dst_words, uint32_t* dst, void* stream);
int demia_crop_pair_matrix(const uint32_t* payload, const int32_t* room, const int64_t* offsets, const int32_t* bbox,
                           const int32_t* first, const int32_t* count, const int32_t* label, int32_t* out, int64_t M, int ld,
                           void* stream);
int demia_crop_pair_intersections(const uint32_t* payload_a, const int32_t* room_a, const int64_t* offsets_a, const int32_t* bbox_a,
                                  const uint32_t* payload_b, const int32_t* room_b, const int64_t* offsets_b, const int32_t* bbox_b,
                                  const int32_t* pi, const int32_t* pj, int32_t* out, int64_t P, void* stream);
int demia_crop_unpack_pooled(const uint32_t* payload, const int32_t* room, const int64_t* offsets, const int32_t* bbox,
                             int64_t first, int64_t n, int H, int W, uint32_t* pool, int32_t* prev, int grow, void* stream);
int demia_crop_gray_histogram(const uint32_t* payload, const int32_t* room, const int64_t* offsets, const int32_t* bbox,
                              const uint8_t* image, int channels, int64_t M, int H, int W, int32_t* hist, void* stream);

/* a18: contrast distribution (measurements.py:195-215, switched by `measure_contrast_distribution`, inference.py:58,1198):
 * per mask the 256-bin histogram of gray = cv2.cvtColor(image, COLOR_BGR2GRAY) over the mask's pixels -- what
 * np.histogram(gray[mask > 0], bins=256, range=(0, 255)) counts (integer data: bin i = pixels of value i).  The CDF and the
 * three np.interp calls on 256 numbers stay on the host.
 *   image [H, W, channels] u8 (channels 3 = BGR, 1 = already gray); bbox [M, 4] a superset of each mask's tight box (-1: empty);
 *   hist [M, 256] i32 (written, not accumulated).                                                                        */
int demia_mask_gray_histogram(const uint32_t* masks, const int32_t* bbox, const uint8_t* image, int channels,
                              int64_t M, int H, int W, int32_t* hist, void* stream);

/* a17/a18: contours and morphometrics ---------------------------------------------------------
 * demia_mask_contours = cv2.findContours(mask, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) per mask
 * (inference.py:1164, 2605) + cv2.contourArea + cv2.arcLength(closed) (inference.py:1175, 2607;
 * measurements.py:134-135).  Components nested in holes are skipped as RETR_EXTERNAL does (the
 * kernel floods the outside background of the bbox region itself).  bbox may be a superset of the tight box;
 * scratch (same shape as masks) is only used by regions larger than the LDS buffers.
 *   count [M]; info [M, C, 4] = start x, start y, n points, offset into `points`;
 *   red [M, C, 2] f64 = area, perimeter; points [max_points, 2] i32 (x, y);
 *   counters [4] i32: [0] points used, [1] error bits (1 candidates, 2 contours > C, 4 points),
 *            [2] / [3] statistics: masks whose parallel border walk fell back to the sequential one / used it.
 * Contours of one mask come out unordered: OpenCV's order is descending (start y, start x).
 * demia_contour_measure = calculate_measurements (measurements.py:114-233) per contour:
 *   out [M, out_c, 12] f64 = major_axis_length, minor_axis_length, eccentricity, Length, Width,
 *   CircularED, Aspect_Ratio, Circularity, Chords, Feret_diam, Roundness, Sphericity; out_c <= C is the number
 *   of contour slots per mask the caller wants back (contours c >= out_c are skipped): with one contour per mask
 *   the table that crosses PCIe is M x 12 doubles instead of M x C x 12.                         */
int64_t demia_contour_work_ints(int M, int C, int max_points);
int64_t demia_contour_work_floats(int M, int C, int max_points);
int64_t demia_contour_work_doubles(int M, int C, int max_points);
int demia_mask_contours(const uint32_t* masks, uint32_t* scratch, const int32_t* bbox, int M, int H, int W, int C,
                        int max_points, int32_t* count, int32_t* info, double* red, int32_t* points,
                        int32_t* counters, void* stream);
/* The same with a WORKLIST [M + 2] i32 (device, contents ignored on entry), as demia_mask_program_wl: the large-region variant
 * runs over the masks the small one listed instead of over all M.  worklist == NULL: demia_mask_contours. */
int demia_mask_contours_wl(const uint32_t* masks, uint32_t* scratch, const int32_t* bbox, int M, int H, int W, int C,
                           int max_points, int32_t* count, int32_t* info, double* red, int32_t* points,
                           int32_t* counters, int32_t* worklist, void* stream);
/* demia_mask_contours_wl for a crop-framed set (payload, room, offsets, bbox as the demia_crop_* entries take them): the same
 * tracer reads each mask's words in place, with the contract and the output layouts above, so its tables feed
 * demia_contour_measure unchanged.  A word of a traced region (tight box + 1 ring, clipped to the frame) that lies outside the
 * mask's room is zero and is never fetched.  No full-frame plane exists anywhere: a region larger than the LDS buffers works in
 * scratch[scratch_off[m] ..) (u32 words: the region with its zero ring, then the flood buffer), which
 * demia_crop_contour_scratch sizes from the HOST copy of the rooms alone (nothing there touches the GPU): it fills scratch_off
 * [M] i64 and returns the total words -- 2 x the padded region of the ROOM (an upper bound of the box's) for a mask whose room
 * region exceeds the large LDS buffer, 0 for every other mask.  With a total of 0, scratch and scratch_off may be any non-NULL
 * device pointers: they are not read. */
int64_t demia_crop_contour_scratch(const int32_t* room_host, int64_t M, int H, int W, int64_t* scratch_off);
int demia_crop_contours_wl(const uint32_t* payload, const int32_t* room, const int64_t* offsets, const int32_t* bbox, int M, int H,
                           int W, int C, int max_points, int32_t* count, int32_t* info, double* red, int32_t* points,
                           int32_t* counters, int32_t* worklist, uint32_t* scratch, const int64_t* scratch_off, void* stream);
int demia_contour_measure(const int32_t* select /* [M] or NULL */, const int32_t* count, const int32_t* info,
                          const double* red, const int32_t* points, int M,
                          int C, int max_points, int32_t* work_i, float* work_f, double* work_d, double um_pix,
                          double* out, int out_c, void* stream);

/* demia_contour_shape = convex-hull shape descriptors per contour (not in the reference program; opt-in:
 * inference_settings.shape_descriptors).  It reads the tables of a trace exactly as demia_contour_measure does (select, count,
 * info, red, points, out_c) and writes nothing but `out` and its scratch.  For a contour with integer points P (n >= 1, repeats
 * allowed), A = red[.., 0], L = red[.., 1], um = um_pix:
 *   H   the strict convex hull of the distinct points (collinear points are no vertices); k = |H|: 1 for one distinct point,
 *       2 for collinear points, else >= 3;
 *   S2  twice the hull area, an exact integer (0 for k < 3);
 *   PH  the hull perimeter in px (k = 2: twice the distance of the two points; k = 1: 0);
 *   F2  the largest squared distance between two points of P, an exact integer; MaxFeret = sqrt(F2);
 *   MinFeret  over the hull edges, the minimum of the largest distance of a hull vertex from the edge's line (0 for k < 3);
 *   FeretAngle  direction of the max-Feret chord in degrees in [0, 180), y upwards: atan2(-(yb - ya), xb - xa), 180 folds to 0;
 *       among the pairs at squared distance F2, ordered so that a < b by (x, y), the smallest a, then the smallest b; k = 1: 0.
 *   out [M, out_c, 10] f64 = S2, F2, k, S2/2 * um^2, PH * um, A / (S2/2) (0 if S2 == 0), PH / L (0 if L == 0), MaxFeret * um,
 *       MinFeret * um, FeretAngle.  Values 0-2 are integers held exactly; the two ratios carry no um.
 * Hull, pair search and tie rule decide in 64-bit integers (exact for coordinates below 2^30); no f32 anywhere.
 *   work_i [demia_contour_shape_work_ints(M, C, max_points)] i32: scratch of contours above 256 points, carved by point offset
 *       (contour t owns [off, off + n + 4) of the point pool, as the tracer leaves it).
 * One launch, no allocation, capturable. */
int64_t demia_contour_shape_work_ints(int M, int C, int max_points);
int demia_contour_shape(const int32_t* select /* [M] or NULL */, const int32_t* count, const int32_t* info, const double* red,
                        const int32_t* points, int M, int C, int max_points, int32_t* work_i, double um_pix,
                        double* out /* [M, out_c, 10] */, int out_c, void* stream);

/* demia_mask_inscribed / demia_crop_inscribed = largest inscribed circle and distance-based thickness per external contour (not
 * in the reference program; opt-in: inference_settings.inscribed_descriptors).  The first measurement on the mask WORDS: for a
 * mask (frame H x W, bit set = foreground) and its contour c as the trace reports it, info[m, c] = (sx, sy, npts, offset):
 *   background  every unset pixel of the mask, holes included, and every position outside the frame (a mask that touches the
 *               frame edge is bounded by it);
 *   D2(p)  for a foreground pixel p, the smallest squared Euclidean distance between the centres of p and of a background
 *          pixel: an integer >= 1;
 *   K(c)   the 8-connected component of the mask that contains (sx, sy).  (A component nested in a hole has no external contour
 *          and no row; its pixels are in nobody's K but are foreground, not background, for D2.)
 *   R2 = max D2 over K;  (cx, cy) = the raster-first pixel of K with D2 = R2 (smallest y, then smallest x; frame coordinates);
 *   N = |K|;  SD2 = sum of D2 over K, summed in int64.  A square filling the frame maximises it at about side^4 / 24: 3.1e15
 *   for the widest frame this project meets (16500 px), below 2^53 = 9.0e15, so the f64 holds it exactly.
 *   out [M, out_c, 8] f64 = R2, cx, cy, N, SD2, 2 sqrt(R2) um (inscribed diameter), sqrt(SD2 / N) um (RMS distance to the
 *       boundary), sqrt(pi R2 / N) (inscribed diameter over the diameter of the circle of area N; no um).  Values 0-4 are integers
 *       held exactly.  Slots c >= min(count[m], out_c), masks with an empty box, and a start pixel that is not set hold zeros.
 * The tables (bbox, count, info, out) are indexed by position t < M; the WORDS -- planes and scratch planes, or payload, room,
 * offsets and scratch_off -- by select[t] (select == NULL: t), so a chunk of a larger set is served from the set's own words.
 * bbox may be any superset of the tight box that is zero outside it (crops: inside the room).  The kernel reads the words and
 * count / info and writes nothing but `out` and its scratch, under exactly the tracer's contract: a region (tight box + 1 ring,
 * clipped to the frame) beyond the tracer's large LDS buffer works in the scratch plane of its mask (demia_mask_contours) or in
 * scratch[scratch_off[.] ..) (demia_crop_contour_scratch); a region word outside the room is zero and is never fetched.
 * Integer decisions only, no f32; the result does not depend on alignment, position or launch layout.  H, W <= 65535, W <= ~49000
 * (the row buffer lives in LDS).  One launch, no allocation, capturable. */
int demia_mask_inscribed(const int32_t* select /* [M] or NULL */, const uint32_t* masks, uint32_t* scratch, const int32_t* bbox,
                         const int32_t* count, const int32_t* info, int M, int H, int W, int C, double um_pix,
                         double* out /* [M, out_c, 8] */, int out_c, void* stream);
int demia_crop_inscribed(const int32_t* select /* [M] or NULL */, const uint32_t* payload, const int32_t* room, const int64_t* offsets,
                         const int32_t* bbox, const int32_t* count, const int32_t* info, int M, int H, int W, int C, double um_pix,
                         double* out /* [M, out_c, 8] */, int out_c, uint32_t* scratch, const int64_t* scratch_off, void* stream);

/* demia_mask_skeleton / demia_crop_skeleton = the morphological skeleton of a mask and, per external contour, its length, end and
 * branch points (not in the reference program; opt-in: inference_settings.skeleton_descriptors).  The second measurement on the
 * mask WORDS.  Background is every unset pixel of the mask and every position outside the frame, as for demia_mask_inscribed.
 * For a pixel P, with y downwards, p2 = N, p3 = NE, p4 = E, p5 = SE, p6 = S, p7 = SW, p8 = W, p9 = NW.
 *   S   the skeleton of the mask: Guo-Hall thinning (1989, algorithm A1), fully parallel.  With
 *         C  = (!p2 & (p3|p4)) + (!p4 & (p5|p6)) + (!p6 & (p7|p8)) + (!p8 & (p9|p2)),
 *         N1 = (p9|p2) + (p3|p4) + (p5|p6) + (p7|p8),  N2 = (p2|p3) + (p4|p5) + (p6|p7) + (p8|p9),  N = min(N1, N2),
 *       a sub-iteration deletes, simultaneously, every set pixel with C == 1, 2 <= N <= 3 and m == 0, all pixels evaluated on the
 *       state before it; sub-iteration 0 uses m = (p6 | p7 | !p9) & p8, sub-iteration 1 uses m = (p2 | p3 | !p5) & p4.  The pair
 *       (0, 1) is repeated until a whole pair deletes nothing.  S is a function of the mask alone.  Distinct 8-connected
 *       components are never 8-adjacent, so thinning the mask once equals the union of thinning each component.
 * Per contour c as the trace reports it, info[m, c] = (sx, sy, npts, offset):
 *   K(c)   the 8-connected component of the mask that contains (sx, sy);  Sk = S & K;  Npix = |K|;
 *   n      |Sk|;
 *   n4     pairs of horizontally or vertically adjacent pixels of Sk;
 *   nd     diagonal links: pairs (x, y), (x+1, y+1) both in Sk with neither (x+1, y) nor (x, y+1) in Sk, and pairs (x, y),
 *          (x-1, y+1) both in Sk with neither (x-1, y) nor (x, y+1) in Sk;
 *   ends   pixels of Sk with exactly one 8-neighbour in Sk;
 *   branches  pixels of Sk whose cyclic sequence p2, p3, ..., p9, p2 (taken in Sk) has three or more 0 -> 1 transitions.
 *   out [M, out_c, 8] f64 = n, n4, nd, ends, branches, Npix, (n4 + sqrt(2) nd) um (skeleton length), (Npix / n) um (mean width).
 *       Values 0-5 are integers held exactly.  Slots c >= min(count[m], out_c), masks with an empty box, and a start pixel that is
 *       not set hold zeros.  A component nested in a hole has no row.
 * Tables and words are indexed as for demia_mask_inscribed (tables by position t, words and scratches by select[t]); bbox may be
 * any superset of the tight box that is zero outside it (crops: inside the room).
 *   skel_out  NULL, or a buffer laid out like the source words ([., H, wpr] planes, or a payload with the same room and offsets):
 *       the kernel writes S into every word of the mask's region (tight box + 1 ring, clipped to the frame; crops: the words of it
 *       that lie in the room) and nothing outside it; a mask with an empty box writes nothing.
 *   count == NULL, info == NULL and out == NULL: the entry only thins into skel_out (C and out_c are ignored).
 * Scratch: a region up to the tracer's large LDS buffer (8192 words, padded) works in LDS, three buffers.  A larger one reads
 * the mask in place and works
 *   planes: in the scratch plane of its mask (`scratch`, as demia_mask_contours) and in the plane of its mask in `scratch2`, both
 *           [., H, wpr] and indexed like the planes; only the region's words of either are written;
 *   crops:  in scratch[scratch_off[.] ..) under the tracer's contract (demia_crop_contour_scratch: two padded room regions) and in
 *           scratch2[scratch2_off[.] ..), which demia_crop_skeleton_scratch sizes from the HOST copy of the rooms alone: it fills
 *           scratch2_off [M] i64 and returns the total words, ONE padded region of the room for a mask whose room region exceeds
 *           the large LDS buffer, 0 for every other mask.  With a total of 0 the pointers are not read (any non-NULL will do).
 * A region word outside the room is zero and is never fetched.  The kernel reads the words and count / info and writes nothing but
 * out, skel_out and its scratches.  Boolean word operations and popcounts only: no per-pixel loop, no f32; the result does not
 * depend on alignment, position or launch layout.  H x ceil(W / 32) < 2^26.  One launch, no allocation, capturable. */
int demia_mask_skeleton(const int32_t* select /* [M] or NULL */, const uint32_t* masks, uint32_t* scratch, const int32_t* bbox,
                        const int32_t* count, const int32_t* info, int M, int H, int W, int C, double um_pix,
                        double* out /* [M, out_c, 8] */, int out_c, uint32_t* scratch2, uint32_t* skel_out, void* stream);
int64_t demia_crop_skeleton_scratch(const int32_t* room_host, int64_t M, int H, int W, int64_t* scratch2_off);
int demia_crop_skeleton(const int32_t* select /* [M] or NULL */, const uint32_t* payload, const int32_t* room, const int64_t* offsets,
                        const int32_t* bbox, const int32_t* count, const int32_t* info, int M, int H, int W, int C, double um_pix,
                        double* out /* [M, out_c, 8] */, int out_c, uint32_t* scratch, const int64_t* scratch_off, uint32_t* scratch2,
                        const int64_t* scratch2_off, uint32_t* skel_out, void* stream);

/* demia_mask_neighbours / demia_crop_neighbours = nearest edge-to-edge gaps and contact counts BETWEEN the masks of one frame (not
 * in the reference program; opt-in: inference_settings.neighbour_statistics).  Not a value per contour of one mask but a relation
 * between masks, one row per mask.  Frame H x W, H, W <= 65535; M < 2^24 masks.
 *   P(m)   the set pixels of mask m;  N(m) = |P(m)|;  Sx, Sy = the sums of x and of y over P(m), int64.
 *   d2(a, b) = min over p in P(a), q in P(b) of (px - qx)^2 + (py - qy)^2, int64, between pixel centres: 0 when the masks share a
 *          pixel (a mask contained in another shares), 1 for 4-adjacent pixels, 2 for diagonal ones; a mask nested in another's
 *          HOLE is disjoint from it and has a positive distance.
 *   nearest neighbour of a   the b != a with N(b) > 0 that minimises (d2(a, b), b) lexicographically: the lower index wins a tie;
 *   nearest in the same group   the same over the b with group[b] == group[a] (group == NULL: every mask is in one group);
 *   touching   the number of b != a, N(b) > 0, with d2(a, b) <= 2 (overlapping or 8-adjacent);
 *   within     the number of b != a, N(b) > 0, with d2(a, b) <= r2;  r2 < 0: not asked for, the value is -1.
 *   table [M, 6] i64 = d2_any, idx_any, d2_group, idx_group, touching, within; d2 and idx are -1 where no such b exists.  A mask with
 *       N = 0 has no distances and is nobody's neighbour: -1, -1, -1, -1, 0, within (0, or -1 for r2 < 0).
 *   sums [M, 3] i64 = N, Sx, Sy;  nborder [M] i32 = the number of border pixels of m.
 *   points   the border pixels of mask m as (y << 16) | x in points[point_off[m] .. point_off[m] + nborder[m]), in no stated order.  A
 *       border pixel is a set pixel with an unset 4-neighbour, positions outside the frame counting as unset (a harmless
 *       superset of the pixels that face another mask): for disjoint masks the minimum over border pixels is the minimum over all.
 *   point_off [M + 1] i64, made by the host: the exclusive prefix sum of upper bounds of the border counts (the pixel counts
 *       serve: border <= pixels), so nothing is counted first and nothing overflows; a mask whose border exceeds its share is cut
 *       to it.  Nothing outside points[0 .. point_off[M]), nborder, sums and table is written.
 * bbox may be any superset of the tight box that is zero outside it (crops: inside the room); a word outside a mask's view is zero
 * and is never fetched; bits beyond column W - 1 are masked off.  Two kernels, one workgroup per mask each: the borders, then per
 * mask a the masks b in ascending (box gap, b) while the gap -- a lower bound of d2 -- is at most max(nearest so far, r2, 2); a pair
 * whose boxes meet is first asked for a shared pixel over the box intersection.  a's border points are staged in LDS up to 8192
 * and read from `points` beyond; the candidates are listed in LDS once at most 256 remain.  Integer comparisons only, no f32 or
 * f64 on the device, plain vector stores; the result does not depend on alignment, position, launch layout or the frame form.
 * M == 0: DEMIA_OK without a launch.  No allocation, one stream, capturable. */
int demia_mask_neighbours(const uint32_t* masks, const int32_t* bbox, const int32_t* group /* [M] or NULL */, int64_t M, int H, int W,
                          int64_t r2, const int64_t* point_off /* [M + 1] */, uint32_t* points, int32_t* nborder /* [M] */,
                          int64_t* sums /* [M, 3] */, int64_t* table /* [M, 6] */, void* stream);
int demia_crop_neighbours(const uint32_t* payload, const int32_t* room, const int64_t* offsets, const int32_t* bbox,
                          const int32_t* group /* [M] or NULL */, int64_t M, int H, int W, int64_t r2,
                          const int64_t* point_off /* [M + 1] */, uint32_t* points, int32_t* nborder /* [M] */,
                          int64_t* sums /* [M, 3] */, int64_t* table /* [M, 6] */, void* stream);

/* demia_mask_agglomerates / demia_crop_agglomerates = which masks of one frame together form one body: the link graph between the
 * masks, its connected components, and moments that count a pixel shared by linked masks once (not in the reference program;
 * opt-in: inference_settings.agglomerate_statistics).  One row per mask on the device; the host sums the rows of a component.
 * P, N, d2, bbox, points, point_off, nborder and sums [M, 3] are those of demia_mask_neighbours above.
 *   L2   the link threshold in squared pixels, L2 >= 2; 2 is the neighbour stage's "touching": 8-connected contact.
 *   link(a, b)   a != b, N(a) > 0, N(b) > 0, d2(a, b) <= L2 and, with a group array, group[a] == group[b].  Symmetric.
 *   links [M, ceil(M / 32)] u32: bit (b & 31) of word (b >> 5) of row a is link(a, b); symmetric, the diagonal and the pad bits
 *       beyond M - 1 are zero.  It stays on the device.
 *   degree [M] i32 = the popcount of row m.
 *   label [M] i32 = the smallest index in m's connected component of the link graph; -1 for a mask with N = 0.  It does not
 *       depend on the order of evaluation.
 *   own [M, 6] i64 = N, Sx, Sy, Sxx, Syy, Sxy over the pixels of m in columns < W that belong to no mask b < m with link(b, m), in
 *       absolute pixel coordinates.  Two overlapping masks of one component are linked directly (d2 = 0, same group), so the sum
 *       of own over a component is exactly the moments of the OR of its members; with group == NULL the sum of own[:, 0] over all
 *       masks is the pixel count of the OR of every mask.
 * Limits (DEMIA_EINVAL with a message): M <= 32768 (links is at most 128 MiB); H, W <= 32767 (N * x^2 stays below 2^60); L2 >= 2.
 * have_border   1: points, nborder and sums were filled on this stream already (the caller's neighbour stage on the same masks,
 *       bbox and point_off) and the border kernel is not launched again; 0: it is launched here.
 * label_lds_cap   the component kernel holds the labels in LDS while M <= the cap and in `label` itself beyond; <= 0: the
 *       default, 8192 (also the most).  Both paths give the same labels; a small cap lets a test take the second.
 * Three kernels behind the border kernel: link (one workgroup per a; candidates by group and box gap <= L2 -- the gap never
 * exceeds d2 --, boxes that meet are first asked for a shared pixel, otherwise "some border point of a within L2 of some border
 * point of b", left at the first pair; each pair is decided from both sides, so a workgroup writes its own row only), component
 * (ONE workgroup: minimum-label propagation with pointer jumping to the fixed point), own (one workgroup per m: a & ~b word by
 * word over m's clipped box).  A word outside a view reads 0 and is never fetched.  All sums are int64 and order-free; no f32 or
 * f64 on the device, no global atomics, plain vector stores.  Nothing outside points[0 .. point_off[M]), nborder, sums, links,
 * degree, label and own is written.  M == 0: DEMIA_OK, nothing is touched.  No allocation, one stream, capturable. */
int demia_mask_agglomerates(const uint32_t* masks, const int32_t* bbox, const int32_t* group /* [M] or NULL */, int64_t M, int H, int W,
                            int64_t L2, const int64_t* point_off /* [M + 1] */, uint32_t* points, int32_t* nborder /* [M] */,
                            int64_t* sums /* [M, 3] */, int have_border, uint32_t* links /* [M, ceil(M / 32)] */,
                            int32_t* degree /* [M] */, int32_t* label /* [M] */, int64_t* own /* [M, 6] */, int label_lds_cap,
                            void* stream);
int demia_crop_agglomerates(const uint32_t* payload, const int32_t* room, const int64_t* offsets, const int32_t* bbox,
                            const int32_t* group /* [M] or NULL */, int64_t M, int H, int W, int64_t L2,
                            const int64_t* point_off /* [M + 1] */, uint32_t* points, int32_t* nborder /* [M] */,
                            int64_t* sums /* [M, 3] */, int have_border, uint32_t* links /* [M, ceil(M / 32)] */,
                            int32_t* degree /* [M] */, int32_t* label /* [M] */, int64_t* own /* [M, 6] */, int label_lds_cap,
                            void* stream);

/* Evaluate task (COCO box / mask AP on a test split) ---------------------------------------------------------------------
 * poly_rasterize: pycocotools' frPyObjects + merge of polygons into packed masks [M, H, ceil(W/32)] (rleFrPoly's rule:
 *   x5 lattice, (int)(5c + .5), the y-boundary points of the edge walk, a pixel set iff an odd number of points lie at
 *   column-major positions <= x * H + y).  xy [V][2] f64 (x, y); polygon p = vertices vert_off[p] .. vert_off[p + 1] (ring
 *   closed implicitly); edges: edge_poly [E] / edge_idx [E] = polygon and vertex index of each edge; bnd_off [P + 1] i64:
 *   room for polygon p's boundary points in bnd ([*, 2] i32, at most one point per walk point of its edges); bnd_cnt [P] and
 *   err [1] zeroed by the caller (err bit 1: a list overflowed); mask m = polygons mask_poly[m] .. mask_poly[m + 1].  area /
 *   bbox (optional, together): demia_mask_area_bbox of the result.
 * mask_cross_matrix: out [D, ld] i32: row i, column c = |det_i & gt_(gt_first[i] + c)| for c < min(gt_count[i], ld); 0 for
 *   pairs with disjoint boxes (no mask read) or, with labels, different labels.  det and gt share H and W.
 * mask_rle_colmajor: column-major run lengths, the background run first (pycocotools' encode).  offsets == NULL: count
 *   pass, n_counts [M] = number of runs; else write pass into counts[offsets[m] .. offsets[m + 1]) (offsets [M + 1] i64 on
 *   the device, from the count pass).  H * W < 2^32.  A slot whose size (offsets[m + 1] - offsets[m]) disagrees with the mask's
 *   run count is left alone, so offsets cut at the end of a sized buffer never make the kernel write past it.
 * The same three for a crop-framed set (payload, room, offsets, bbox as the demia_crop_* entries take them): the evaluate
 * task scores rooms, never planes.
 *   crop_poly_rasterize: the rasteriser's words go to the rooms instead of planes: word t of mask m's room is row
 *     room.y0 + t / cols, word column (room.x0 >> 5) + t % cols, written to payload[offsets[m] + t] by exactly one thread, and no
 *     other word of payload is written; max_room_words >= the words of the largest room (the grid is masks x slabs of it).
 *     The boundary points stay in frame coordinates, so the bits are those of poly_rasterize's plane inside the room.  area
 *     [M] / bbox [M, 4] (required): pixel count and tight box of the room's words, reduced on the device.  The rooms come from
 *     the caller, from the vertices alone; err bit 2 is set when a mask's kept boundary points could set a pixel outside its
 *     room (their rectangle, columns min px .. max px x rows min py .. max py - 1, is not inside it) -- the pixels of such
 *     a mask are NOT all stored and the caller must not use the result.  An empty room (-1) stores nothing.
 *   crop_cross_matrix: mask_cross_matrix with both sides crop-framed sets over one frame (same kernel, same counts).
 *   crop_rle_colmajor: mask_rle_colmajor of a set, same two-pass protocol (room_offsets: the set's word offsets; offsets: the
 *     run offsets of the write pass).  A pixel outside a mask's room reads as 0.
 * host_coco_match / host_rle_string: host code (nothing touches the GPU), see hostloops.hip. */
int demia_poly_rasterize(const double* xy, const int32_t* vert_off, const int32_t* edge_poly, const int32_t* edge_idx,
                         const int64_t* bnd_off, int32_t* bnd, int32_t* bnd_cnt, int32_t* err, int64_t E,
                         const int32_t* mask_poly, int64_t M, int H, int W, uint32_t* out, int32_t* area, int32_t* bbox,
                         void* stream);
int demia_mask_cross_matrix(const uint32_t* det, const int32_t* det_bbox, const int32_t* det_label, const uint32_t* gt,
                            const int32_t* gt_bbox, const int32_t* gt_label, const int32_t* gt_first, const int32_t* gt_count,
                            int32_t* out, int64_t D, int ld, int H, int W, void* stream);
int demia_mask_rle_colmajor(const uint32_t* masks, const int32_t* bbox, int32_t* n_counts, const int64_t* offsets,
                            uint32_t* counts, int64_t M, int H, int W, void* stream);
int demia_crop_poly_rasterize(const double* xy, const int32_t* vert_off, const int32_t* edge_poly, const int32_t* edge_idx,
                              const int64_t* bnd_off, int32_t* bnd, int32_t* bnd_cnt, int32_t* err, int64_t E,
                              const int32_t* mask_poly, int64_t M, int H, int W, const int32_t* room, const int64_t* offsets,
                              int64_t max_room_words, uint32_t* payload, int32_t* area, int32_t* bbox, void* stream);
int demia_crop_cross_matrix(const uint32_t* det_payload, const int32_t* det_room, const int64_t* det_offsets,
                            const int32_t* det_bbox, const int32_t* det_label, const uint32_t* gt_payload, const int32_t* gt_room,
                            const int64_t* gt_offsets, const int32_t* gt_bbox, const int32_t* gt_label, const int32_t* gt_first,
                            const int32_t* gt_count, int32_t* out, int64_t D, int ld, void* stream);
int demia_crop_rle_colmajor(const uint32_t* payload, const int32_t* room, const int64_t* room_offsets, const int32_t* bbox,
                            int32_t* n_counts, const int64_t* offsets, uint32_t* counts, int64_t M, int H, int W, void* stream);
int demia_host_coco_match(int64_t G, const int64_t* dt_off, const int64_t* gt_off, const double* dt_score,
                          const double* dt_area, const int64_t* dt_row, const double* gt_area, const uint8_t* gt_crowd,
                          const int64_t* gt_col, const double* iou, const double* area_rng, int A, const double* thr, int T,
                          int max_det, int32_t* dt_rank, uint8_t* dt_matched, uint8_t* dt_ignore, uint8_t* gt_ignore);
int64_t demia_host_rle_string(const uint32_t* counts, const int64_t* offsets, int64_t M, char* out, int64_t cap,
                              int64_t* text_off);

/* demia_mask_boundary_band / demia_crop_boundary_band = the boundary band of a mask, for Boundary IoU (Cheng et al., "Boundary
 * IoU", CVPR 2021; not in the reference program; opt-in: evaluation.boundary_ap).  The definitions, stated here once:
 *   width   the erosion width of an H x W frame is d = max(1, int(round(ratio * sqrt(H*H + W*W)))), round = Python's round (half to
 *           even), ratio = evaluation.boundary_dilation_ratio (default 0.02); evaluation.boundary_width, an integer >= 1, gives d
 *           directly in pixels.  (cocoeval.boundary_width computes it; the kernel takes d.)
 *   eroded(m, d)[y, x] = 1 iff every pixel (y + j, x + i), |i| <= d, |j| <= d, is 1; pixels outside the frame count as 0.
 *   band(m, d) = m & ~eroded(m, d).  A subset of the mask, so it fits the mask's room; it has the mask's tight box; a mask thinner
 *           than 2d + 1 in either direction is its own band.
 *   The published construction -- pad a 1-px zero ring, then d iterations of a 3 x 3 erosion whose own border counts as set -- gives
 *           the same eroded mask.
 *   bIoU(a, g) = |band(a) & band(g)| / (|band(a)| + |band(g)| - |band(a) & band(g)|), the denominator |band(a)| for a crowd g, 0
 *           where the intersection is 0: cocoeval.mask_iou on band counts (cocoeval.boundary_iou).
 *   The IoU of the evaluate task `boundary` is min(mask IoU, bIoU) element by element, crowd columns included; a detection's area
 *           and the area ranges are those of `segm`: mask pixels, not band pixels.
 * The entries:
 *   band       laid out like the source words ([M, H, wpr] planes, or a payload with the SAME room and offsets).  The CALLER zeroes
 *              it; the kernel writes the words of each mask's box (clipped to the frame; crops: to the room) and nothing else, so
 *              planes stay zero outside each box and a room outside its box.  A mask with an empty box writes nothing.  The padding
 *              bits beyond column W - 1 stay zero.
 *   band_area  [M] i32 = |band(m, d)|, 0 for an empty box.
 *   bbox       any superset of the tight box that is zero outside it (crops: inside the room).
 *   d          1 <= d < 2^24.  If 2d + 1 exceeds the box's width or height the band is the mask: it is copied and counted.
 * One workgroup per mask on the words of its box, 32 pixels per lane operation: the AND over 2d + 1 pixels of a row by doubling
 * shifts (funnel shifts of two words), then the same over rows -- about 2 log2(2d + 1) passes, two buffers.  A region of at most
 * 8192 words works in LDS.  A larger one works in the output's own words of the region and in scratch:
 *   planes: `scratch` is [M, H, wpr], indexed like the planes; only the box's words of a large region are written;
 *   crops:  scratch[scratch_off[m] ..), which demia_crop_boundary_scratch sizes from the HOST copy of the rooms alone: it fills
 *           scratch_off [M] i64 and returns the total words, the room's words for a room of more than 8192 words, 0 for every other
 *           mask.  With a total of 0 the scratch is not touched (any non-NULL pointer will do).
 * A word outside the box, the room or the frame is a zero operand and is never fetched: a crop kernel never reads outside its mask's
 * room.  The source words are only read; nothing but band, band_area and scratch is written; no buffer of a call may be another
 * one.  Boolean word operations and popcounts, plain vector stores; the result does not depend on alignment, position, launch
 * layout or the frame form.  H x ceil(W / 32) < 2^26.  M == 0: DEMIA_OK without a launch.  One launch, no allocation, capturable. */
int demia_mask_boundary_band(const uint32_t* masks, const int32_t* bbox, int64_t M, int H, int W, int d, uint32_t* band,
                             int32_t* band_area /* [M] */, uint32_t* scratch, void* stream);
int64_t demia_crop_boundary_scratch(const int32_t* room_host, int64_t M, int H, int W, int64_t* scratch_off);
int demia_crop_boundary_band(const uint32_t* payload, const int32_t* room, const int64_t* offsets, const int32_t* bbox, int64_t M,
                             int H, int W, int d, uint32_t* band, int32_t* band_area /* [M] */, uint32_t* scratch,
                             const int64_t* scratch_off, void* stream);

/* demia_mask_outline_agreement / demia_crop_outline_agreement = surface distances between the outlines of matched pairs of masks of
 * one frame, a detection and its annotation (not in the reference program; opt-in: evaluation.outline_agreement).  The device
 * returns integers only; the report (ASSD, RMS, Hausdorff, HD95, NSD; cocoeval.outline_values) is f64 on the host from them.
 * The definitions, stated here once:
 *   border pixel   a set pixel in columns < W with an unset 4-neighbour, positions outside the frame counting as unset: what the
 *           border stage of demia_mask_neighbours writes, by the same kernel.  B(m) = the border pixels of mask m; every mask with
 *           a pixel has one.
 *   d2(p, T) = min over t in B(T) of (px - tx)^2 + (py - ty)^2, int64, between pixel centres, exact (coordinates go up to 65535,
 *           so d2 can exceed 2^32).
 *   q(d2)  = isqrt(d2 << 16) = floor(256 * sqrt(d2)): the distance in 1/256 px, rounded down, an exact integer function.
 *   bin(d2) = min(127, the smallest integer c with c * c >= d2) = min(127, ceil(sqrt(d2))): bin 0 holds d2 = 0, bin c <= 126 the
 *           distances in (c - 1, c] px, bin 127 SATURATES: it holds everything beyond 126 px.  The cumulative count up to c <= 126
 *           is therefore the number of points at most c px away.
 *   pairs [P, 2] i32 = (detection index, annotation index); a mask may be named by several pairs or by none.  Every pair is
 *           measured in both directions: direction 0 has the detection as the SOURCE S and the annotation as the TARGET T,
 *           direction 1 the reverse.
 *   out [P, 2, 136] i32, one record per pair and direction, 8-byte aligned: four little-endian i64
 *           n = |B(S)|,  max_d2 = max over p in B(S) of d2(p, T),  sum_d2 = their sum,  sum_q = the sum of q(d2(p, T)),
 *           then hist [128] i32, hist[c] = the number of p in B(S) with bin(d2(p, T)) = c.  The CALLER zeroes out.  Where S or T has
 *           no border point the record is n and zeros; a pair with an index outside its set leaves its records zero.
 * Both sets' border stages write what demia_mask_neighbours' does, per set: points behind point_off ([count + 1] i64, the host's
 * exclusive prefix sum of the pixel counts), nborder [count] i32, sums [count, 3] i64.  bbox: any superset of the tight box that is
 * zero outside it (crops: inside the room).  H, W <= 65535.
 * The distance kernel splits the source points of a pair-direction into shares of demia_outline_source_share() points, one
 * workgroup per share, each thread holding 4 source points and their minima in registers; the target points pass through LDS in
 * tiles of demia_outline_target_tile().  demia_outline_chunks fills chunk_off [2 P + 1] i64 from the HOST copies of the pixel
 * counts and the pair list -- pair-direction 2 p + dir gets ceil(pixels of its source / share) workgroups, at least 1 and at most
 * 256, the shares beyond are strided over -- and returns the grid, n_chunks = chunk_off[2 P]; the entries take its device copy.
 * Workgroups reduce in LDS first and combine on the record with integer vector atomics (add, unsigned max), so the result does
 * not depend on scheduling, on the number of workgroups, on alignment, position or the frame form.  No f32 or f64 on the device.
 * Nothing but the two border stages' outputs and out is written.  P == 0, D == 0 or G == 0: DEMIA_OK without a launch.  Three
 * launches (two border stages, one distance kernel), no allocation, one stream, capturable. */
int demia_outline_source_share(void);
int demia_outline_target_tile(void);
int64_t demia_outline_chunks(const int64_t* det_area_host /* [D] */, int64_t D, const int64_t* gt_area_host /* [G] */, int64_t G,
                             const int32_t* pairs_host /* [P, 2] */, int64_t P, int64_t* chunk_off /* [2 P + 1] */);
int demia_mask_outline_agreement(const uint32_t* det, const int32_t* det_bbox, int64_t D, const uint32_t* gt, const int32_t* gt_bbox,
                                 int64_t G, int H, int W, const int64_t* det_point_off /* [D + 1] */, uint32_t* det_points,
                                 int32_t* det_nborder /* [D] */, int64_t* det_sums /* [D, 3] */,
                                 const int64_t* gt_point_off /* [G + 1] */, uint32_t* gt_points, int32_t* gt_nborder /* [G] */,
                                 int64_t* gt_sums /* [G, 3] */, const int32_t* pairs /* [P, 2] */, int64_t P,
                                 const int64_t* chunk_off /* [2 P + 1] */, int64_t n_chunks, int32_t* out /* [P, 2, 136] */,
                                 void* stream);
int demia_crop_outline_agreement(const uint32_t* det_payload, const int32_t* det_room, const int64_t* det_offsets,
                                 const int32_t* det_bbox, int64_t D, const uint32_t* gt_payload, const int32_t* gt_room,
                                 const int64_t* gt_offsets, const int32_t* gt_bbox, int64_t G, int H, int W,
                                 const int64_t* det_point_off /* [D + 1] */, uint32_t* det_points, int32_t* det_nborder /* [D] */,
                                 int64_t* det_sums /* [D, 3] */, const int64_t* gt_point_off /* [G + 1] */, uint32_t* gt_points,
                                 int32_t* gt_nborder /* [G] */, int64_t* gt_sums /* [G, 3] */, const int32_t* pairs /* [P, 2] */,
                                 int64_t P, const int64_t* chunk_off /* [2 P + 1] */, int64_t n_chunks,
                                 int32_t* out /* [P, 2, 136] */, void* stream);

/* demia_mask_error_map / demia_crop_error_map = the error map of one image of the evaluate task (`--task evaluate --visualize`; not
 * the reference's Detectron2 Visualizer picture, whose look is not reproduced): the detections over the ground truth, painted from
 * the packed words of both sets.  The definitions, stated here once:
 *   inputs   a frame of H x W pixels; src u8 [H, W, C], C = 1 (gray) or 3 (BGR); dst u8 [H, W, 3] BGR, a buffer distinct from src;
 *           D detections and G annotations over the frame, from the same word source, with boxes (any superset of the tight boxes
 *           that is zero outside it, -1 = empty) and states
 *             d_state [D] i32   0 = not drawn and not counted, 1 = matched, 2 = unmatched (spurious)
 *             g_state [G] i32   0 = skip, 1 = matched, 2 = missed, 3 = crowd region        (any other value: as 0)
 *           alpha in 0 .. 256; the line width t in 1 .. 4; a palette of 8 BGR triples.
 *   sets     Dall = the union of the detections of state 1 or 2, Gall = the union of the annotations of state 1 or 2, Gc = the union
 *           of the annotations of state 3.  Bits of mask words beyond column W - 1 are nobody's pixels.
 *   fill class of a pixel, the first that applies:  agree  in Dall & Gall;  ignored  in (Dall & Gc) \ Gall, counted and NOT filled;
 *           excess  in Dall \ Gall \ Gc;  missing  in Gall \ Dall;  else none.
 *   base     b = src for C = 3, the gray byte in all three channels for C = 1.
 *   fill     a pixel of class agree, excess or missing is (b_c * (256 - alpha) + colour_c * alpha + 128) >> 8 per channel; every
 *           other pixel is b.
 *   outline  outline_t(m) = m \ erode_t(m), erode_t the erosion by the (2t + 1) x (2t + 1) square, pixels outside the frame counting
 *           as not set: a mask thinner than 2t + 1 is all outline, and a mask on the frame's edge has outline there.
 *   lines    an outline pixel is painted SOLID over the fill, in the colour of the highest class it belongs to:  1 unmatched
 *           detection,  2 missed annotation,  3 matched detection,  4 matched annotation,  5 crowd region.
 *   palette  [8, 3] u8 BGR: agree, excess, missing, unmatched-detection line, missed-annotation line, matched-detection line,
 *           matched-annotation line, crowd line.  (The defaults are cocoeval.ERROR_MAP_PALETTE, and nowhere else.)
 *   counts   [4] i64 = the pixels of class agree, excess, missing, ignored -- of the FILL classes, whatever the lines cover.
 * Nothing depends on the order of the masks within a state, so dst and counts are unique: integers, exact.
 * The entries: palette is a HOST pointer to the 24 bytes (they and the scalars travel by value with the launch); partial is the
 * caller's [demia_error_map_tiles(H, W), 4] i64, one row of counts per tile, every row written; counts is written, not added to.
 * One workgroup of 256 threads per tile of 32 rows x 8 word columns: the masks of both sets whose boxes meet the tile are found 256
 * at a time by ballot and taken one after the other (no list, no limit on how many meet a tile), each through LDS -- its words over
 * the tile and a halo of t rows and one word column, the erosion along the rows, then down the columns -- into eight 32-pixel
 * accumulators per thread (three unions, five line classes); a second kernel of one workgroup sums the partial rows.  A word outside
 * a mask's box, its view (crops: its room) or the frame is a zero operand and is never fetched; the tile is never clipped to a view.
 * The mask words and src are only read; nothing but dst, partial and counts is written.  Boolean word operations, popcounts and the
 * integer blend; no global atomics, plain vector stores.  D == 0 and G == 0 are valid: dst is b and the counts are 0 when both are.
 * H, W <= 65535.  Two launches, no allocation, one stream, capturable. */
int64_t demia_error_map_tiles(int H, int W);
int demia_mask_error_map(const uint32_t* det, const int32_t* det_bbox, const int32_t* d_state /* [D] */, int64_t D, const uint32_t* gt,
                         const int32_t* gt_bbox, const int32_t* g_state /* [G] */, int64_t G, int H, int W, const uint8_t* src, int C,
                         uint8_t* dst, int alpha, int line, const uint8_t* palette /* host, [8, 3] */, int64_t* partial /* [tiles, 4] */,
                         int64_t* counts /* [4] */, void* stream);
int demia_crop_error_map(const uint32_t* det_payload, const int32_t* det_room, const int64_t* det_offsets, const int32_t* det_bbox,
                         const int32_t* d_state /* [D] */, int64_t D, const uint32_t* gt_payload, const int32_t* gt_room,
                         const int64_t* gt_offsets, const int32_t* gt_bbox, const int32_t* g_state /* [G] */, int64_t G, int H, int W,
                         const uint8_t* src, int C, uint8_t* dst, int alpha, int line, const uint8_t* palette /* host, [8, 3] */,
                         int64_t* partial /* [tiles, 4] */, int64_t* counts /* [4] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPEMIA_HIP_H */

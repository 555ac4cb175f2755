/*
 * dcap.h -- C-ABI of libdcap_hip.so: the MI355X (gfx950) kernels of the dense-captioning hot path.
 *
 * The reference (frosinastojanovska/image-captioning) has no FFI of its own: every arithmetic op on
 * the path is a Keras-2.1 / TF-1.x call.  Each entry point below replaces one family of those call
 * sites (cited as file:line relative to the reference root); the Python host side
 * (the modules under image-captioning_amd/) binds them with ctypes and keeps the reference's module/function names.
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions (all entry points):
 *   - return 0 on success, a negative DC_E* code otherwise; dc_last_error() gives a thread-local text;
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller;
 *   - enqueue-only on `stream` (a hipStream_t passed as void*): no allocation, no synchronisation,
 *     safe under hipGraph stream capture; stateless and re-entrant on distinct streams;
 *   - scratch memory is a caller-provided workspace; dc_*_workspace_bytes() gives the size; a workspace that receives split-K
 *     slabs (the GEMMs and convolutions) sits on a 16-byte boundary unless the output width N is not a multiple of 4 (DC_EALIGN);
 *   - tensors are row-major, activations NHWC, float32 unless stated.
 */
#ifndef DCAP_H
#define DCAP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DC_OK            0
#define DC_EINVAL       -1   /* bad shape / null pointer / unsupported combination */
#define DC_EALIGN       -2   /* pointer or leading dimension not 16-byte aligned where required */
#define DC_EWORKSPACE   -3   /* workspace too small */
#define DC_ELAUNCH      -4   /* HIP launch error (text in dc_last_error) */

/* ABI version = 100*major + minor.  The major number changes whenever a descriptor struct's layout changes (fields removed or
 * reordered: round 5 removed dc_conv_desc.w_split / w_wino4 and grew dc_amsgrad_desc => major 6); a caller compiled against this
 * header checks dc_version() / 100 == DC_ABI_VERSION / 100 before the first call (image-captioning_amd/_lib.py does at load). */
#define DC_ABI_VERSION 600
int         dc_version(void);
const char* dc_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * GEMM  C[M,N] = epilogue(A[M,K] * B[K,N])            (fp32 in, fp32 MFMA accumulate)
 * Replaces KL.Dense / the LSTM kernels' x.W products / the 7x7-valid + 1x1 RoI-head convs:
 *   dense_img_cap_separate_models/text_generation_model.py:143-144,153-154,251-259
 *   dense_img_cap_separate_models/text_generation_model_v2.py:141-150,157,163-164
 * and their gradients (dgrad = dY*W^T: b_trans=1; wgrad = A^T*dY: a_trans=1).
 *   a_trans=0: A is [M][lda] (K contiguous);   a_trans=1: A is [K][lda] (M contiguous)
 *   b_trans=0: B is [K][ldb] (N contiguous, the Keras [in,out] kernel);  b_trans=1: B is [N][ldb]
 *   a_gather (optional, a_trans=0): row m of A is A[a_gather[m]] -- the fused KL.Embedding lookup
 *     (text_generation_model.py:135-140, _v2.py:155-156); with a_trans=1 it indexes the K rows
 *     (A^T of a gathered matrix: the embedding-side wgrad)
 * epilogue: v = acc*scale[n] + shift[n] (each optional), += residual[m][n] (optional),
 *           relu (optional), then C = v  or  C += v (accumulate).
 * split_k > 1 partitions K over blockIdx.z through fp32 slabs in the workspace (deterministic
 * reduction order); 0 lets the library choose.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int M, N, K;
    const float*   A;  int lda;  int a_trans;
    const int32_t* a_gather;
    const float*   B;  int ldb;  int b_trans;
    float*         C;  int ldc;
    const float*   scale;
    const float*   shift;
    const float*   residual;  int ldr;
    int res_rows;             /* >0: residual row = m % res_rows (per-RoI term broadcast over timesteps) */
    int relu;
    int accumulate;
    int split_k;
} dc_gemm_desc;

size_t dc_gemm_workspace_bytes(const dc_gemm_desc* d);
int    dc_gemm_f32(const dc_gemm_desc* d, void* workspace, size_t workspace_bytes, void* stream);
/* Test / profiling aid (host only, launches nothing): the block tile (bm x bn: 128 x 128, 128 x 64 or 64 x 64) and the split-K factor
 * dc_gemm_f32 picks for `d`, from the rule the launch itself applies.  For a K that is not a multiple of 32 and is run as a bulk launch
 * plus a range-checked tail launch, the answer is the bulk launch's (the tail accumulates onto it on 64 x 64 tiles, unsplit).
 * *split_k is the factor the rule hands to the launch, which then cuts K into slices of whole 32-deep K-tiles: 28 asked of 256 K-tiles
 * run as 26 slices (25 of 10 K-tiles, one of 6).  dc_conv2d_tile_config and dc_conv2d_wgrad_tile_config report it the same way.
 * dc_gemm_workspace_bytes, dc_conv2d_workspace_bytes and dc_conv2d_wgrad_workspace_bytes count the slices that run (26 slabs there):
 * the size a query gives is the size the launch checks, and one byte less is refused with DC_EWORKSPACE. */
int    dc_gemm_tile_config(const dc_gemm_desc* d, int* bm, int* bn, int* split_k);

/* ------------------------------------------------------------------------------------------------
 * GEMM with bf16 operands (bit patterns in uint16_t), fp32 accumulate on the bf16 matrix pipe -- the arithmetic BASELINE
 * configs[4] asks for (joint model in bf16: dense_img_cap/dense_model.py:738-817 RoI head + Model-3 decoder, :936-946
 * vocabulary softmax).  Same operand conventions and epilogue as dc_gemm_f32; the result is written as fp32 (C), as bf16
 * (Cb: the next bf16 GEMM's operand), or both.  K, lda, ldb multiples of 8; a K-major operand (a_trans = 1 / b_trans = 0)
 * needs its row length (M / N) to be a multiple of 8.  a_gather (optional) indexes rows of a table of a_gather_rows rows:
 * with a_trans = 0 tile row m is table row a_gather[m] (embedding lookup), with a_trans = 1 K row k is a_gather[k].
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int M, N, K;
    const uint16_t* A;  int lda;  int a_trans;
    const int32_t*  a_gather;  int a_gather_rows;
    const uint16_t* B;  int ldb;  int b_trans;
    float*          C;  int ldc;
    uint16_t*       Cb; int ldcb;
    const float*    scale;
    const float*    shift;
    const float*    residual;  int ldr;
    int res_rows;
    int relu;
    int accumulate;
    int split_k;
} dc_gemm_bf16_desc;

size_t dc_gemm_bf16_workspace_bytes(const dc_gemm_bf16_desc* d);
int    dc_gemm_bf16(const dc_gemm_bf16_desc* d, void* workspace, size_t workspace_bytes, void* stream);
/* Profiling / test aid: the block tile dc_gemm_bf16 runs `d` on -- 256 (bgemm256_kernel: 256 x 256 x 64, 8 waves, one block per CU,
 * v_mfma_f32_16x16x32_bf16) or 128 (bgemm_kernel: 128 x 128 x 64, 4 waves, two blocks per CU); *split_k (may be NULL) receives the
 * number of split-K slices.  Returns 0 for an invalid descriptor. */
int    dc_gemm_bf16_tile(const dc_gemm_bf16_desc* d, int* split_k);

/* conv2d weight gradient on the bf16 matrix pipe (configs[4]: the joint model's trainable FPN / RPN convolutions,
 * dense_img_cap/dense_model.py:1829-1831): dw[cout][(ky,kx,ci)] (+)= sum over output pixels of dy[p][cout] * x[p*stride + tap - pad][ci],
 * packed like the forward weights, fp32 accumulation and output.  x [N,H,W,Cin] and dy [N,Ho,Wo,Cout] are bf16 (dc_cast_f32_bf16 of the
 * fp32 activations / gradients).  Cin % 128 == 0, Cout % 8 == 0.  Same sums as dc_conv2d_wgrad_f32 on operands rounded to bf16. */
typedef struct {
    int N, H, W, Cin;
    int Cout, kh, kw, stride, pad_t, pad_l;
    int Ho, Wo;
    const uint16_t* x;
    const uint16_t* dy;
    float* dw;
    int accumulate;
    int split_k;
} dc_conv_wgrad_bf16_desc;
size_t dc_conv2d_wgrad_bf16_workspace_bytes(const dc_conv_wgrad_bf16_desc* d);
int    dc_conv2d_wgrad_bf16(const dc_conv_wgrad_bf16_desc* d, void* workspace, size_t workspace_bytes, void* stream);
/* Test / profiling aid: the block tile (256 | 128) and split-K slices dc_conv2d_wgrad_bf16 runs `d` with. */
int    dc_conv2d_wgrad_bf16_tile(const dc_conv_wgrad_bf16_desc* d, int* split_k);

/* conv2d forward with bf16 STORAGE (configs[4]: "bf16"): bf16 NHWC activations and bf16 packed weights in HBM, fp32 accumulation,
 * the same fused epilogue as dc_conv2d_nhwc_f32 (frozen-BN scale / shift, residual (fp32), ReLU), output in fp32 (y), bf16 (y_bf16: the
 * next convolution's input) or both.  Replaces the same Keras layers as dc_conv2d_nhwc_f32 (feature_generation/dense_model.py:85-100,
 * :120-139, :1406-1421) for the joint model's bf16 mode; on weights rotated by dc_conv_weight_dgrad_pack it is the data gradient.
 *   x [N,H,W,Cin] bf16, Cin % 64 == 0;  w PACKED [Cout][kh*kw*Cin] bf16;  y / y_bf16 [N,Ho,Wo,Cout];
 *   res_mode: 0 none, 1 residual of the output's shape, 2 residual on the 2x coarser map (nearest-upsampled), as for the fp32
 *   convolution.  Taps in the padding read zeros. */
typedef struct {
    int N, H, W, Cin;
    int Cout, kh, kw, stride, pad_t, pad_l;
    int Ho, Wo;
    const uint16_t* x;
    const uint16_t* w;
    float*          y;        /* may be NULL when y_bf16 is given */
    uint16_t*       y_bf16;   /* may be NULL when y is given */
    const float* scale;
    const float* shift;
    const float* residual;  int res_mode;
    int relu;
    int split_k;
    int tile;                 /* 0 = the library's cost model picks the block tile; 64 | 128 | 256 = run on that tile where the shape allows it
                               * (tests and benchmarks; dc_conv2d_bf16_tile reports what will run) */
} dc_conv_bf16_desc;
size_t dc_conv2d_bf16_workspace_bytes(const dc_conv_bf16_desc* d);
int    dc_conv2d_bf16(const dc_conv_bf16_desc* d, void* workspace, size_t workspace_bytes, void* stream);
/* Test / profiling aid: the block tile `d` runs on -- 256 (bconv256_kernel, 256 x 256 x 64), 128 (bconv_kernel) or 64 (bconv64_kernel: whole K
 * loop per block, no split-K); *split_k (may be NULL) = slices. */
int    dc_conv2d_bf16_tile(const dc_conv_bf16_desc* d, int* split_k);

/* fp32 -> bf16 (round to nearest even): the bf16 shadow of weights / activations that feed dc_gemm_bf16.
 * _2d: rows x cols with row strides, output columns cols..cols_out-1 zero-filled (pads K to a multiple of 8). */
int dc_cast_f32_bf16(const float* x, uint16_t* out, size_t n, void* stream);
/* bf16 -> fp32 (exact).  Data-parallel joint model with a bf16 gradient exchange (configs[4]'s buckets travel as bf16,
 * half the bytes on xGMI): the all-reduced bf16 bucket goes back into the fp32 gradient bucket the clip norm and AMSGrad read. */
int dc_cast_bf16_f32(const uint16_t* x, float* out, size_t n, void* stream);
int dc_cast_f32_bf16_2d(const float* x, int ld_in, uint16_t* out, int ld_out, int rows, int cols, int cols_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * conv2d NHWC forward as an implicit GEMM (LDS im2col tiles), fused frozen-BN / bias / residual /
 * ReLU epilogue.  Replaces KL.Conv2D + BatchNorm(training=False) + Add + Activation('relu'):
 *   feature_generation/dense_model.py:85-100 (identity_block), :120-139 (conv_block),
 *   :146-149 (stem), :1406-1421 (FPN laterals / 3x3), UpSampling2D+Add :1407-1415 (res_mode 2).
 *   x [N,H,W,Cin]; w PACKED [Cout][kh*kw*Cin] (cin fastest; dc_pack helper on the host side);
 *   y [N,Ho,Wo,Cout];  y = relu?( scale[c]*conv + shift[c] + residual )
 *   res_mode: 0 none, 1 residual [N,Ho,Wo,Cout], 2 residual [N,Ho/2,Wo/2,Cout] nearest-upsampled x2.
 * Cin must be a multiple of 32, except the stem: Cin==4 (RGBX), kh==kw==7, stride 2, with w packed
 * as [Cout][7][8][4] (kx==7 and c==3 entries zero).
 * ------------------------------------------------------------------------------------------------ */
#define DC_MATH_F32 0
#define DC_MATH_BF16X3 1
#define DC_MATH_BF16X2 2
#define DC_MATH_BF16 3
typedef struct {
    int N, H, W, Cin;
    int Cout, kh, kw, stride, pad_t, pad_l;
    int Ho, Wo;
    const float* x;
    const float* w;
    float*       y;
    const float* scale;
    const float* shift;
    const float* residual;  int res_mode;
    int relu;
    int split_k;
    int accumulate;           /* wgrad only: dw += (a weight shared by several inputs, e.g. the RPN over P2..P6) */
    int math;                 /* forward only: DC_MATH_F32 = fp32 MFMA (exact fp32 products), DC_MATH_BF16X3 = every operand
                                 element split into three bf16 pieces, six bf16 MFMA products, fp32 accumulate (fp32-grade
                                 accuracy on the bf16 matrix pipe; csrc/igemm_bf16s.h); DC_MATH_BF16X2 = two pieces, three
                                 products: a 16-bit-mantissa product (2^-16 relative; TF32 is 2^-11) at half the MFMAs;
                                 DC_MATH_BF16 = operands rounded once to bf16, one product, fp32 accumulate -- plain bf16 compute,
                                 the arithmetic BASELINE configs[4] names (2^-9 relative per operand) */
    const float* w_wino;      /* optional with DC_MATH_F32, forward only: the weights of a 3x3 / stride 1 / pad 1 layer transformed by
                                 dc_conv2d_winograd_pack_f32 (16 * Cin * Cout floats).  Non-NULL = run the layer in the Winograd
                                 F(2x2, 3x3) form: fp32 throughout, 16 products per 2x2 output tile instead of 36 (the minimal-filtering
                                 algorithm cuDNN picks for these layers under the reference's TF); needs Cin, Cout multiples of 32, no
                                 residual.  Layers that do not qualify ignore the field */
    const uint16_t* w_wino_b3; /* optional, like w_wino (and preferred when both are given): the same transformed weights split into three bf16
                                 pieces per element by dc_conv2d_winograd_pack_b3 (16 * Cin * Cout * 3 bf16).  The 16 products per tile then
                                 run on the BF16 matrix pipe in split arithmetic -- six bf16 MFMA products per fp32 product, fp32
                                 accumulation: DC_MATH_BF16X3's fp32-grade arithmetic -- transforms in fp32 as before */
} dc_conv_desc;

/* x = p0 + p1 + p2 with bf16 pieces rounded to nearest even: out[0..n) = p0, out[n..2n) = p1, out[2n..3n) = p2. */
int dc_split_bf16x3_f32(const float* x, uint16_t* out, size_t n, void* stream);
size_t dc_conv2d_workspace_bytes(const dc_conv_desc* d);
int    dc_conv2d_nhwc_f32(const dc_conv_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* Profiling aid: the block tile (bm x bn) and split-K factor dc_conv2d_nhwc_f32 picks for `d`, i.e.
 * which igemm_kernel<bm,bn,...> instantiation runs (bench.py maps layers to rocprof kernel names). */
int    dc_conv2d_tile_config(const dc_conv_desc* d, int* bm, int* bn, int* split_k);
/* Profiling aid: rocprof's spelling (without the "void dcap::" prefix and the parameter list) of the kernel template
 * instantiation that dc_conv2d_nhwc_f32 launches for `d`.  buf_bytes >= 96. */
int    dc_conv2d_kernel_name(const dc_conv_desc* d, char* buf, size_t buf_bytes);
/* 1 when `d` runs on the dense (pointwise: 1x1, stride 1, unpadded) A-operand loader instead of the im2col one. */
int    dc_conv2d_is_pointwise(const dc_conv_desc* d);
/* Winograd F(2x2, 3x3) weight transform U = G g G^T of a packed 3x3 kernel w [Cout][9*Cin] into the fragment order the kernel
 * reads (dc_conv_desc.w_wino); done once per frozen weight.  Replaces nothing in the reference: it is how the KL.Conv2D(3x3) layers of
 * feature_generation/dense_model.py:85-100, :1417-1421 are evaluated. */
size_t dc_conv2d_winograd_weight_bytes(int Cin, int Cout);
int    dc_conv2d_winograd_pack_f32(const float* w, float* u, int Cin, int Cout, void* stream);
size_t dc_conv2d_winograd_b3_weight_bytes(int Cin, int Cout);
int    dc_conv2d_winograd_pack_b3(const float* w, uint16_t* u, int Cin, int Cout, void* stream);
/* Two chained pointwise (1x1, stride 1) convolutions in one launch (csrc/conv_chain.hip, round 5): y = act1((x W1^T) * scale1 + shift1
 * [+ residual]) is written out AND contracted on the spot with the second kernel, z = act2((y W2^T) * scale2 + shift2) -- the last
 * convolution of a ResNet bottleneck (branch2c + shortcut + ReLU) and the first of the next block (branch2a + ReLU):
 * feature_generation/dense_model.py:85-100, :120-139, frozen BatchNorm folded into scale / shift like dc_conv2d_nhwc_f32.  fp32 operands,
 * exact fp32 MFMA products.  x [M][K1], y / residual [M][N1], z [M][N2] row-major (NHWC pixels = rows); w1 / w2: the packed kernels
 * [N][K] re-ordered ONCE by dc_pw_chain_pack_f32 (same size).  Shapes: dc_pw_chain_supported (K1 % 32 == 0; N1 -> N2 = 1024 -> 256 or
 * 512 -> 128: a block owns 32 pixels, the intermediate rows stay in LDS; or K1 -> N1 -> N2 = 64 -> 256 -> 64, the stage-2 seam: a
 * streaming kernel whose layer-1 accumulators are layer 2's MFMA operands, fp32 products only).  No workspace. */
typedef struct {
    int M, K1, N1, N2;
    const float* x;
    const float* w1;
    const float* scale1;      /* NULL = 1 */
    const float* shift1;
    const float* residual;    /* NULL = none */
    int relu1;
    float* y;
    const float* w2;
    const float* scale2;
    const float* shift2;
    int relu2;
    float* z;
    const uint16_t* w1_b3;    /* optional, BOTH or neither (then w1 / w2 may be NULL): the kernels split into three bf16 pieces per element by */
    const uint16_t* w2_b3;    /* dc_pw_chain_pack_b3 (3 * N * K bf16): both layers' products on the BF16 matrix pipe in split arithmetic (six
                                 bf16 MFMA products per fp32 product, fp32 accumulation: fp32-grade, DC_MATH_BF16X3's arithmetic) */
} dc_pw_chain_desc;
int dc_pw_chain_supported(int K1, int N1, int N2);
int dc_pw_chain_pack_f32(const float* w, float* out, int N, int K, void* stream);
int dc_pw_chain_pack_b3(const float* w, uint16_t* out, int N, int K, void* stream);
int dc_pw_chain_f32(const dc_pw_chain_desc* d, void* stream);
/* Profiling aid: rocprof's spelling of the kernel instantiation dc_pw_chain_f32 launches for `d` (buf_bytes >= 40). */
int dc_pw_chain_kernel_name(const dc_pw_chain_desc* d, char* buf, size_t buf_bytes);

/* CUs the persistent Winograd grids may occupy (process-wide; a multiple of 8 -- one share per XCD; 0 restores the default:
 * DCAP_WINO_CUS or all 256).  A persistent block holds its CU for the whole launch: in a data-parallel run (parallel_model.py:58-102
 * -> one rank per GPU here) the RCCL all-reduce of another queue needs CUs of its own to overlap the encoder pass, so
 * ParallelModel / bench.py set 248 when world > 1.  Applies to launches of at least eight rounds of work items per block (the
 * long-running ones: fpn_p2 at the benchmark's size); shorter launches keep the full grid, where a smaller one would add a whole
 * round.  Takes effect at the next launch; a captured hipGraph keeps the grid it was captured with. */
int    dc_set_persistent_cus(int n);
int    dc_get_persistent_cus(void);

/* ------------------------------------------------------------------------------------------------
 * conv2d weight gradient (for the layers the joint model trains: fpn_*, rpn_*, dense_img_cap/dense_model.py
 * train(layers="no_backbone") :1829-1831):  dw[cout][(ky,kx,ci)] = sum over output pixels of
 * dy[p][cout] * x[p*stride + (ky,kx) - pad][ci]   -- packed like the forward weights, so the optimizer
 * updates the packed tensor directly.  Uses the fields N,H,W,Cin,Cout,kh,kw,stride,pad_*,Ho,Wo and
 * x (activations), y (= dy, [N,Ho,Wo,Cout]), w (= dw OUT).  Cin % 64 == 0, Cout % 4 == 0, N*Ho*Wo % 32 == 0.
 * The data gradient needs no entry point of its own: for stride-1 convs it is dc_conv2d_nhwc_f32 on dy with
 * the kernel rotated by 180 degrees and cin/cout swapped (packing.pack_conv_kernel_dgrad).
 * ------------------------------------------------------------------------------------------------ */
size_t dc_conv2d_wgrad_workspace_bytes(const dc_conv_desc* d);
int    dc_conv2d_wgrad_f32(const dc_conv_desc* d, void* workspace, size_t workspace_bytes, void* stream);
/* Test / profiling aid (host only, launches nothing): the block tile (bm x bn over Cout x kh*kw*Cin) and the split-K factor (over the
 * N*Ho*Wo pixels) dc_conv2d_wgrad_f32 picks for `d`, from the rule the launch itself applies. */
int    dc_conv2d_wgrad_tile_config(const dc_conv_desc* d, int* bm, int* bn, int* split_k);

/* KL.MaxPooling2D((3,3), strides 2, 'same') (dense_model.py:150); C % 4 == 0. */
int dc_maxpool3x3s2_same_f32(const float* x, float* y, int N, int H, int W, int C, void* stream);

/* KL.MaxPooling2D((2,2), strides 2) of keras.applications VGG16 (image captioning/vgg16.py:9-18 loads that model; the
 * alternative-backbone benchmark config); C % 4 == 0, H and W even. */
int dc_maxpool2x2s2_f32(const float* x, float* y, int N, int H, int W, int C, void* stream);

/* mold_image (dense_model.py:2050-2055) fused with the RGBX repack the stem kernel wants:
 * out[n,h,w,0..2] = float(img_u8) - mean[c], out[...,3] = 0. */
int dc_mold_image_rgbx_f32(const uint8_t* img, float* out, int N, int H, int W,
                           float mean_r, float mean_g, float mean_b, void* stream);
/* The same with the pixel zero-padded to `channels` floats (channels % 4 == 0): the first convolution of the VGG16 alternative
 * backbone reads 32-channel pixels (the implicit-GEMM loader wants Cin % 32 == 0). */
int dc_mold_image_padded_f32(const uint8_t* img, float* out, int N, int H, int W, int channels,
                             float mean_r, float mean_g, float mean_b, void* stream);

/* ------------------------------------------------------------------------------------------------
 * utils.resize_image (dense_img_cap_separate_models/utils.py:290-340) for a batch of raw uint8 RGB images of ANY sizes in one call:
 * image b [h][w][3] is resampled to [new_h][new_w][3] exactly as PIL.Image.resize((new_w, new_h), resample=BILINEAR) does it
 * (ImagingResample, 8 bits per channel: horizontal pass into a uint8 intermediate, then the vertical pass; per axis the window
 * and triangle-filter weights in float64, normalised, rounded to 22 fractional bits; pixel = clamp(((1 << 21) + sum k * p) >> 22))
 * and written into out[b] of the uint8 canvas [B][H][W][3] at (top, left); every other byte of the canvas is written as 0, so the
 * canvas may be a reused buffer.  The device's bytes are PIL's, bit for bit.
 *   packed: ONE device buffer (4-byte aligned: its head is int32), B records of DC_RESIZE_RECORD_INTS int32
 *     { byte offset of the image in `packed`, h, w, new_h, new_w, top, left, byte offset of the intermediate in the workspace }
 *     followed by the images' bytes end to end, each at any byte offset: one host-to-device copy per batch.
 *   records: the HOST's copy of those B records (the one host pointer of this interface): it sizes the grids and the workspace and
 *     is checked before anything is launched -- a null pointer, a zero size, a window that leaves the canvas, an image that leaves
 *     `packed`, an intermediate offset other than the sum of h * new_w * 3 over the images before, or any byte count (packed,
 *     canvas, workspace) of 2^31 or more is DC_EINVAL.  The device never reads it and nothing is read back.
 *   workspace (16-byte aligned): the intermediates (sum of h * new_w * 3 bytes), then the coefficient tables, which a first
 *     kernel fills from the records' sizes alone.
 * Neither the images nor the canvas have an alignment rule (every access to them is one byte).  Three launches on `stream`
 * whatever B is; no allocation, no synchronisation, capturable.
 * ------------------------------------------------------------------------------------------------ */
#define DC_RESIZE_RECORD_INTS 8

typedef struct {
    int B;
    const uint8_t* packed;
    size_t         packed_bytes;
    const int32_t* records;
    uint8_t*       out;
    int H, W;
} dc_resize_pad_desc;

size_t dc_resize_pad_u8_workspace_bytes(const dc_resize_pad_desc* d);
int    dc_resize_pad_u8(const dc_resize_pad_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* The same with load_image_gt's augmentation (dense_model.py:953-984: image[:, ::-1] on the resized AND padded square), per image:
 * with flag 1, out[b][y][x][c] is byte [y][W - 1 - x][c] of what dc_resize_pad_u8 writes for image b -- the window moves to columns
 * [W - left - new_w, W - left), and when W - new_w is odd the padding's odd column changes sides.  No mirrored source is resampled:
 * the vertical kernel (shared with dc_resize_pad_u8) computes the unflipped canvas' byte with the unflipped pass's coefficients and
 * stores it at the mirrored column, so the bytes are PIL's by construction.  With every flag 0 the canvas is dc_resize_pad_u8's.
 *   The flags travel in the one packed upload: B int32 at byte `flips_offset` of d->packed (e.g. between the records and the first
 *   image; such a buffer is still valid for dc_resize_pad_u8, which only wants image offsets >= B * DC_RESIZE_RECORD_INTS * 4).
 *   flips: the HOST's copy of the B flags, checked with the records before anything is launched: a null pointer, a value other than
 *   0 or 1, a block off a 4-byte boundary, one that overlaps the records or an image or leaves `packed` is DC_EINVAL and the canvas
 *   stays untouched.  The device never reads the host copy.
 * Workspace, launches (three, whatever B is) and every other rule are dc_resize_pad_u8's; size the workspace with
 * dc_resize_pad_u8_workspace_bytes (the layout is the same). */
int    dc_resize_pad_flip_u8(const dc_resize_pad_desc* d, const int32_t* flips, size_t flips_offset, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PyramidROIAlign forward (feature_generation/dense_model.py:317-418): level routing
 * k = clamp(4 + round_half_even(log2(sqrt(h*w) / (224/sqrt(image_area)))), 2, 5) and
 * tf.image.crop_and_resize(bilinear, 1 sample per bin, extrapolation 0) in one gather kernel.
 *   maps[l] = P(2+l) [B,Hl,Wl,C] (C % 4 == 0, C <= 256*4); boxes [B*R,4] normalised (y1,x1,y2,x2), batch-major;
 *   out [B*R,pool,pool,C] in box order (the reference's final reorder, :397-411, is the identity
 *   here because nothing is regrouped by level).  levels_out (optional) [B*R] int32.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int B, R, C, pool;
    const float* maps[4];
    int Hs[4], Ws[4];
    const float* boxes;
    float image_area;
    float* out;
    int32_t* levels_out;
} dc_roialign_desc;

int dc_roi_align_pyramid_f32(const dc_roialign_desc* d, void* stream);

/* The FPN output convolutions computed only where PyramidROIAlign reads.  When the boxes are known before the encoder pass (ground-truth
 * boxes: the caption-training flows), the pyramid maps P2..P5 have one consumer, the gather above, which reads at most pool * pool * 4
 * pixels per box.  The split-bf16 Winograd kernel works on tile groups of 8 x 16 output pixels (ragged at the bottom / right edges);
 * group index = (image * groups_y + group row) * groups_x + group column, groups_y * groups_x = dc_conv2d_winograd_group_count(H, W).
 *
 * dc_roi_tile_groups: for every box and bin the routing and the sample of dc_roi_align_pyramid_f32 (the same device functions), a mark
 * on the group of each of the four corner pixels at the routed level (a sample outside the map marks nothing), then per level the
 * marked groups in ascending index into lists[l] and their number into counts[l].  One small launch; the host never reads either.
 *   boxes [B*R,4] as in dc_roialign_desc; Hs / Ws: the extents of P2..P5; marks: scratch, B * (sum of the four levels' group counts)
 *   int32; lists[l]: B * dc_conv2d_winograd_group_count(Hs[l], Ws[l]) int32; counts: 4 int32.
 * dc_conv2d_winograd_groups_f32: the layer `d` on the listed groups only -- every output element inside a listed group gets the value
 * dc_conv2d_nhwc_f32 gives it, bit for bit; nothing else of d->y is written; count[0] == 0 is a no-op.  `groups` / `count` are device
 * pointers (a level's list and its count).  The layer must be one the split-bf16 Winograd kernel takes (3x3, stride 1, pad 1, Cin and
 * Cout multiples of 32, no residual, DC_MATH_F32, w_wino_b3 given): anything else is DC_EINVAL, there is no other path. */
typedef struct {
    int B, R, pool;
    int Hs[4], Ws[4];
    const float* boxes;
    float image_area;
    int32_t* marks;
    int32_t* lists[4];
    int32_t* counts;
} dc_roi_groups_desc;

int dc_roi_tile_groups(const dc_roi_groups_desc* d, void* stream);
int dc_conv2d_winograd_group_count(int H, int W);
int dc_conv2d_winograd_groups_f32(const dc_conv_desc* d, const int32_t* groups, const int32_t* count, void* stream);

/* The lateral 1x1 in front of fpn_p2 computed only where the list-driven fpn_p2 reads it (the other laterals stay dense: their maps
 * are listed almost whole).
 *
 * dc_roi_tile_groups_lateral: dc_roi_tile_groups, and in the same launch the tiles of the level-2 map that hold a pixel of a listed
 * level-2 group or of its one-pixel ring (the halo the 3x3 convolution reads): every listed group and its up to eight neighbours in the
 * group grid of the same image, in ascending group index into lat_list (B * dc_conv2d_winograd_group_count of level 2, int32), their
 * number into lat_count[0].  The descriptor is dc_roi_tile_groups' own, unchanged.
 * dc_conv2d_nhwc_tiles_f32: the pointwise layer `d` on the listed 8 x 16-pixel tile groups only (`tiles` / `count`: device pointers) --
 * every output element inside a listed tile gets the value dc_conv2d_nhwc_f32 gives it, bit for bit (the upsample-add operand of
 * res_mode 2 included); nothing else of d->y is written; count[0] == 0 is a no-op.  The layer must be a 1x1 / stride 1 / unpadded
 * convolution in DC_MATH_BF16X3 that dc_conv2d_nhwc_f32 runs on 128 x 128 tiles without split-K (dc_conv2d_tile_config; split_k = 1
 * pins that where the dense rule would split), res_mode 0 or 2, Cout % 4 == 0: anything else is DC_EINVAL, there is no other path. */
/* dc_conv2d_winograd_levels_f32: dc_conv2d_winograd_groups_f32 for `nlevels` (1..4) layers in ONE launch -- d: an array of nlevels
 * descriptors, lists: a host array of nlevels device pointers (level l's group list), counts: device pointer to nlevels int32 (level
 * l's count at counts[l]).  The work items of all levels cost the same, so the layers must agree in N, Cin, Cout and relu (DC_EINVAL
 * otherwise); each must be a layer dc_conv2d_winograd_groups_f32 takes.  Every listed group of every level gets the dense values bit
 * for bit, nothing else is written, an empty level contributes nothing. */
int dc_conv2d_winograd_levels_f32(const dc_conv_desc* d, int nlevels, const int32_t* const* lists, const int32_t* counts, void* stream);
int dc_roi_tile_groups_lateral(const dc_roi_groups_desc* d, int32_t* lat_list, int32_t* lat_count, void* stream);
int dc_conv2d_nhwc_tiles_f32(const dc_conv_desc* d, const int32_t* tiles, const int32_t* count, void* stream);

/* KL.MaxPooling2D(pool_size=(1,1), strides=2): P6 = every other pixel of P5 (dense_model.py:1423). */
int dc_subsample2_f32(const float* x, float* y, int N, int H, int W, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RPN scores + ProposalLayer (feature_generation/dense_model.py:684-725, :221-305): per image
 *   fg score = softmax(class logits)[1] per anchor, deltas *= RPN_BBOX_STD_DEV,
 *   tf.nn.top_k(scores, pre_nms_limit) (stable: lower anchor index first among ties),
 *   apply_box_deltas -> clip to the image -> normalise by [h,w,h,w] (float32, TF's operation order),
 *   tf.image.non_max_suppression(threshold) -> first `proposal_count` survivors, zero padded.
 * heads[l] = the fused RPN head output of pyramid level l, NHWC [B,Hl,Wl,A*6]: channels a*2+{bg,fg}
 * (rpn_class_raw) followed by A*2 + a*4 + {dy,dx,dh,dw} (rpn_bbox_pred); anchors [A_total,4] pixels in
 * generate_pyramid_anchors order (level, y, x, ratio).
 * Optional outputs for tests: scores_out [B,A_total], order_out [B,pre_nms_limit] (anchor index of each
 * sorted candidate), keep_out [B,proposal_count] (candidate rank of each kept box, -1 padded).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int B, levels, anchors_per_loc;
    const float* heads[5];
    int Hs[5], Ws[5];
    int head_stride;          /* floats per cell in heads[] (0 = anchors_per_loc*6; > that when the head is padded) */
    const float* anchors;
    int A_total;
    float std_dev[4];
    float image_h, image_w;
    int pre_nms_limit, proposal_count;
    float nms_threshold;
    float* proposals;
    float* scores_out;
    int32_t* order_out;
    int32_t* keep_out;
} dc_proposal_desc;

size_t dc_proposals_workspace_bytes(const dc_proposal_desc* d);
int    dc_proposals_f32(const dc_proposal_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GenerationMatchLayer + unmold_generations (dense_img_cap/dense_model.py:593-630, :1925-1962) for B images with N RoIs each, in
 * float64 by the operations of the NumPy host path, in its order: the results are that path's bit for bit.
 *   rois [B][N][4] float32, normalised (y1,x1,y2,x2).  Scores, exactly one of: word_scores [B*N][T] float32 (the greedy decoder's
 *   word probabilities; caption score = sum over t = 0..T-1, in index order, of log((double) p)) or caption_scores float32, RoI i of
 *   image b at element (b*N + i) * caption_stride (column 0 of the beam decoder's [B*N][k] scores: caption_stride = k).
 *   image_consts [B][DC_REFINE_CONSTS] float64 in DEVICE memory, per image: the window y1, x1, y2, x2; IMAGE_SHAPE h, w;
 *   unmold_generations' shift y, x and scale (computed by the host as that function computes it); one unused word.
 *   Order: np.argsort(scores, kind="stable")[::-1] -- score descending, the HIGHER RoI index first among equal scores (-0 equals +0),
 *   NaN before everything, -inf (a word probability of 0) an ordinary value.  Boxes: (double) roi * (h,w,h,w), y clipped to the
 *   window's [y1,y2], x to [x1,x2].  NMS: greedy in that order, box j is suppressed by a kept box i when
 *   ih*iw / (area_i + area_j - ih*iw) > threshold with ih = max(min(y2_i,y2_j) - max(y1_i,y1_j), 0), iw alike -- the corners as they
 *   are, and a 0/0 NaN suppresses nothing (all-zero padding RoIs all survive); the first max_instances survivors go on.  Each is
 *   rounded half to even, (box - shift) * scale is truncated toward zero to int32, and boxes with (y2-y1)*(x2-x1) <= 0 are dropped,
 *   the others keeping their order.
 * Outputs (fixed size): boxes_out int32 [B][max_instances][4] (16-byte aligned; zeros after the last survivor), keep_out int32
 * [B][max_instances] (each survivor's index into the image's N RoIs, in score order; -1 after the last), count_out int32 [B],
 * scores_out float64 [B][N] (the caption scores in RoI order).
 * Limit: N <= DC_REFINE_MAX_ROIS (the one-workgroup NMS scan holds 128 mask words per row); larger N is DC_EINVAL.  Five launches on
 * `stream`, workspace 32-byte aligned; no allocation, no synchronisation, capturable.
 * ------------------------------------------------------------------------------------------------ */
#define DC_REFINE_CONSTS 10
#define DC_REFINE_MAX_ROIS 8192

typedef struct {
    int B, N, T;
    const float* rois;
    const float* word_scores;
    const float* caption_scores;
    int caption_stride;
    const double* image_consts;
    double threshold;
    int max_instances;
    int32_t* boxes_out;
    int32_t* keep_out;
    int32_t* count_out;
    double* scores_out;
} dc_refine_desc;

size_t dc_refine_generations_workspace_bytes(const dc_refine_desc* d);
int    dc_refine_generations_f64(const dc_refine_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * refine_detections from the line after the class selection + the box part of unmold_detections (mask_rcnn/mask_rcnn_model.py :689-738,
 * :2281-2301) for B images with N RoIs each, by the operations of the NumPy host path (mask_rcnn_model.refine_detections /
 * unmold_boxes) in its order and its number formats, one rounding per NumPy operation.
 *   rois [B][N][4] float32, normalised (y1,x1,y2,x2); class_ids int32 [B][N], scores float32 [B][N] and deltas float32 [B][N][4]: what
 *   dc_class_select_f32 leaves.  std_dev: BBOX_STD_DEV as four doubles; image_h, image_w: IMAGE_SHAPE's, as doubles.
 *   image_consts [B][DC_REFINE_CONSTS] float64 in DEVICE memory, a row as dc_refine_generations_f64 takes it: words 0-3 the window
 *   y1, x1, y2, x2 (read as the float32 values the DetectionLayer sees), words 6-8 unmold_detections' shift y, x and scale; words 4, 5
 *   and 9 are not read.
 *   Boxes: d_k = (double) delta_k * std_k; height = r2 - r0, width = r3 - r1, cy = r0 + 0.5f height, cx alike, in float32;
 *   cy = (float)((double) cy + d0 (double) height), cx alike; height = (float)((double) height * exp(d2)), width alike, exp in float64;
 *   y1 = cy - 0.5f height, x1 alike, y2 = y1 + height, x2 = x1 + width in float32; each coordinate (float)((double) v * image_h or
 *   image_w); clipped to the window in float32 as max(min(v, hi), lo); rounded half to even to int32.
 *   Candidates: class_id > 0 and (min_confidence == 0 or score >= (float) min_confidence -- NumPy compares the float32 scores with the
 *   Python float in float32).  Every other RoI neither suppresses nor survives.
 *   Order: np.argsort(scores, kind="stable")[::-1] -- score descending, the HIGHER RoI index first among equal scores (-0 equals +0,
 *   NaN before everything), the rule of dc_refine_generations_f64.  (The reference's default sort promises no order among ties.)
 *   NMS: greedy in that order; box j is suppressed by a kept box i OF THE SAME CLASS when, on the int32 boxes taken as float32,
 *   ih*iw / (area_i + area_j - ih*iw) > (float) threshold in float32, ih = max(min(y2_i,y2_j) - max(y1_i,y1_j), 0), iw alike; a 0/0 NaN
 *   suppresses nothing.  This one global scan with suppression inside a class only keeps what the reference's per-class NMS, the union
 *   of its results and the final sort by score keep, in the same order: a box's fate depends on the kept boxes of its own class ahead
 *   of it alone, and the global order restricted to a class is that class's order.
 *   The first max_instances survivors go on; each gives (int32) trunc(((double) box - shift) * scale); boxes with
 *   (y2-y1)*(x2-x1) <= 0 there are dropped, the others keep their order.
 * Outputs, each [B][max_instances] rows; rows behind the last survivor hold a zero box, class id -1, score 0 and keep -1:
 *   count_out int32 [B]; boxes_out int32 [..][4] in the molded image; rois_out int32 [..][4] in the original image; norm_out float32
 *   [..][4] = (float)((double) box / (double)(h,w,h,w)), what the mask head's RoIAlign takes; class_ids_out int32; scores_out float32
 *   (the words copied); keep_out int32, the RoI's index.  Every access is of one element: no alignment rule beyond the element's own.
 * Not bit equality without condition: np.exp and the device library's float64 exp are each within 1 ulp of the true value and are not
 * the same function.  A difference in that last bit reaches the output only where it flips the float32 rounding of a height or width
 * and that flip in turn moves an rint or an NMS decision; everything else is the host path's result bit for bit.  Deltas are
 * expected finite.
 * Limit: N <= DC_REFINE_DET_MAX_ROIS (one workgroup per image holds the image's boxes, classes, indices and keys in 56 KB of static
 * LDS); larger N, B < 1, N < 1, max_instances < 1, a null pointer or one off its element's boundary is DC_EINVAL.  ONE launch on `stream` (B workgroups of up to 1024
 * threads), no workspace, no allocation, no synchronisation, capturable; identical bits from call to call.
 * ------------------------------------------------------------------------------------------------ */
#define DC_REFINE_DET_MAX_ROIS 2048

typedef struct {
    int B, N;
    const float* rois;
    const int32_t* class_ids;
    const float* scores;
    const float* deltas;
    const double* image_consts;
    double std_dev[4];
    double image_h, image_w;
    double min_confidence;
    double threshold;
    int max_instances;
    int32_t* count_out;
    int32_t* boxes_out;
    int32_t* rois_out;
    float* norm_out;
    int32_t* class_ids_out;
    float* scores_out;
    int32_t* keep_out;
} dc_refine_det_desc;

int dc_refine_detections_f32(const dc_refine_det_desc* d, void* stream);

/* PyramidROIAlign backward: d(maps) += bilinear scatter of d(out) (gradients to the boxes are stopped in the
 * reference, dense_model.py:378-379).  dmaps[l] must be zero-initialised by the caller; accumulation uses
 * float atomics (order-dependent in the last bits).  Same descriptor as the forward; `out` holds d(out) and
 * `maps` the gradient maps (written). */
int dc_roi_align_pyramid_bwd_f32(const dc_roialign_desc* d, void* stream);

/* FPN top-down backward: out[n,y,x,c] (+)= sum of the 2x2 block of fine[n,2y..2y+1,2x..2x+1,c]
 * (the gradient of UpSampling2D(2) + Add, dense_model.py:1407-1415). */
int dc_downsample2x_sum_f32(const float* fine, float* out, int N, int Ho, int Wo, int C, int accumulate, void* stream);
/* ... and, in the same pass, the bf16 copy of `out` that the bf16 weight-gradient GEMM of the lateral convolution reads (NULL: none). */
int dc_downsample2x_sum_dual_f32(const float* fine, float* out, uint16_t* out_bf16, int N, int Ho, int Wo, int C, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Keras-2.1 LSTM over a whole sequence (gate blocks i,f,c,o; hard-sigmoid gates; tanh; mask carry).
 * Replaces KL.LSTM: text_generation_model.py:141-142,150-151; _v2.py:157,163.
 * Time-major: row (t*B + b).  The caller first computes zx = x*kernel + bias with dc_gemm_f32
 * (optionally with the fused embedding gather); this call runs the recurrence:
 *   z_t = zx_t + h_{t-1}*U ; i,f,o = hs(z) ; g = tanh(z_c) ; c' = f*c + i*g ; h' = o*tanh(c')
 *   masked rows (mask[t*B+b]==0) carry h,c from t-1 (zeros before the first unmasked step).
 * zx is updated IN PLACE to the full pre-activation z (saved for backward).
 *   z [T*B][4U] in/out, U_rec [U][4U], mask [T*B] uint8 or NULL, h_seq/c_seq [T*B][U] out.
 *   Forward: U_rec, h_seq, rec_masks and the workspace are 16-byte aligned; backward: U_rec, h_seq, dz and the workspace; the single
 *   step: h_prev.  A fused step reads them 16 bytes at a time or a later step hands them to dc_gemm_f32 as A / B: DC_EALIGN before
 *   the first launch otherwise.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int B, T, U;
    float* z;
    const float* U_rec;
    const uint8_t* mask;
    float* h_seq;
    float* c_seq;
    const float* rec_masks;   /* optional [4][B][U]: Keras recurrent_dropout masks (values 0 or 1/(1-rate)), one per gate i,f,c,o,
                                 fixed over the timesteps: z_g = x W_g + (h_{t-1} * m_g) U_g + b_g  (training phase of
                                 LSTM(recurrent_dropout=0.2), text_generation_model.py:141-142).  NULL = no dropout. */
} dc_lstm_fwd_desc;

size_t dc_lstm_seq_workspace_bytes(int B, int T, int U);
int    dc_lstm_seq_fwd_f32(const dc_lstm_fwd_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the recurrence.  dh_seq [T*B][U] (may be NULL) is the gradient w.r.t. every step's
 * output, dh_last [B][U] (may be NULL) an extra gradient on the last step's output.
 * Outputs: dz [T*B][4U] (caller derives dkernel = x^T dz, dbias = colsum dz, dx = dz kernel^T with
 * dc_gemm_f32 / dc_colsum_f32) and dU_rec [U][4U] (written, or accumulated if accumulate_dU).  dU_rec may be NULL: the
 * caller then forms it itself, dU_rec = h_seq[0 .. (T-1)B)^T dz[B .. TB) (with rec_masks: per gate g from h_seq * m_g) -- the
 * bf16 joint model does, on the bf16 matrix pipe from the bf16 copies it already holds. */
typedef struct {
    int B, T, U;
    const float* z;
    const float* U_rec;
    const uint8_t* mask;
    const float* h_seq;
    const float* c_seq;
    const float* dh_seq;
    const float* dh_last;
    float* dz;
    float* dU_rec;
    int accumulate_dU;
    const float* rec_masks;   /* the masks of the forward call (or NULL) */
} dc_lstm_bwd_desc;

int dc_lstm_seq_bwd_f32(const dc_lstm_bwd_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* Host-only (nothing is launched): which instance of the fused step kernels runs a (B, U) problem -- direction 0: the forward step of
 * dc_lstm_seq_fwd_f32 / dc_lstm_step_f32 (rec_masks != 0: the recurrent-dropout step), 1: the backward step of dc_lstm_seq_bwd_f32 (one
 * rule with and without masks).  rows = batch rows per block, waves = waves per block, from the helpers the launches themselves call;
 * rows = waves = 0 where the step is not fused (U % 32 != 0 forward, U % 16 != 0 backward).  DC_EINVAL: B <= 0, U <= 0, U % 4 != 0, a
 * direction other than 0 / 1, a null rows / waves. */
int dc_lstm_step_tile_config(int B, int U, int direction, int rec_masks, int* rows, int* waves);

/* ------------------------------------------------------------------------------------------------
 * ONE timestep of the recurrence above with carried state: incremental greedy decoding feeds one token per call instead of
 * re-running the whole zero-padded prefix (ROICaptionInferenceLayer, text_generation_model.py:192-232; dense_img_cap/dense_model.py:820).
 *   z [B][4U] in/out (x*kernel + bias in, the full pre-activation out), U_rec [U][4U], h_prev / c_prev [B][U] (both NULL: zeros,
 *   the sequence's first step), mask [B] uint8 or NULL (all live): rows with mask 0 copy h_prev / c_prev (Keras' mask carry),
 *   h / c [B][U] out (must not alias h_prev / c_prev).  The same kernels as dc_lstm_seq_fwd_f32 at the same B: T calls that feed
 *   h, c forward give its h_seq / c_seq bit for bit.
 *   U_packed: U % 32 == 0 runs the fused step on a line-contiguous copy of U_rec (4U^2 floats) made by dc_lstm_pack_urec_f32 --
 *   once per decode instead of once per step; NULL repacks into the workspace on every call.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int B, U;
    float* z;
    const float* U_rec;
    const float* U_packed;
    const float* h_prev;
    const float* c_prev;
    const uint8_t* mask;
    float* h;
    float* c;
} dc_lstm_step_desc;

int    dc_lstm_pack_urec_f32(const float* U_rec, int U, float* U_packed, void* stream);   /* U % 32 == 0; U_packed: 4*U*U floats */
size_t dc_lstm_step_workspace_bytes(int B, int U);
int    dc_lstm_step_f32(const dc_lstm_step_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * softmax + K.categorical_crossentropy (clip 1e-7) forward and d/dlogits in one pass per row.
 * Replaces Dense(..., activation='softmax') + keras.losses.categorical_crossentropy /
 * roi_caption_loss: text_generation_model.py:154,286-294; _v2.py:164,267.
 *   logits [M][ld] (V valid columns); targets [M] int32 (the argmax of the reference's one-hot rows);
 *   probs (optional) [M][ld]; loss_rows (optional) [M]; dlogits (optional, may alias logits) [M][ld]:
 *   dlogits = grad_scale * (p - onehot) for rows whose target probability is inside [1e-7, 1-1e-7], else 0.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int M, V, ld;
    const float* logits;
    const int32_t* targets;
    float* probs;
    float* loss_rows;
    float* dlogits;
    float grad_scale;
    const float* row_weights; /* optional [M]: loss_rows and dlogits rows are multiplied by it (0 drops a row) */
    int keras_sparse;         /* 1: K.sparse_categorical_crossentropy on probabilities (dense_img_cap/dense_model.py:943-945):
                                 q = clip(p,1e-7,1-1e-7); loss = -log q_t + log sum(q), gradient through clip and sum */
} dc_softmax_ce_desc;

int dc_softmax_ce_f32(const dc_softmax_ce_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Vocabulary projection FUSED with softmax + cross-entropy: logits = X[M,K] * W[K,V] + bias are reduced tile by tile inside
 * the GEMM and never written.  Replaces Dense(V, activation='softmax') + the losses above in training:
 *   text_generation_model.py:153-154,286-294; text_generation_model_v2.py:164,267; dense_img_cap/dense_model.py:787-817,936-946.
 *   bf16 = 0: X, W float32 (fp32 MFMA), K % 32 == 0, V % 4 == 0;  bf16 = 1: X, W bf16 bit patterns, K % 8 == 0, V % 8 == 0.
 *   loss_rows [M] (optional), dlogits [M][lddl] (optional; float32, or bf16 when dl_bf16 -- then columns V..lddl-1 are written
 *   as zeros so the matrix can feed dc_gemm_bf16 as an operand), dbias [V] (optional, needs dlogits): column sums of dlogits,
 *   combined in a fixed order.  Semantics of loss / gradient / row_weights / keras_sparse exactly as dc_softmax_ce_f32.
 * Cost model: one GEMM pass for the loss plus one for the gradient, against one pass plus four sweeps over a [M,V] float32 matrix
 * unfused; keras_sparse adds a pass that sums the clipped probabilities -- only on the row tiles that hold a probability outside
 * [1e-7, 1 - 1e-7] (the first pass keeps every row's smallest logit; elsewhere nothing is clipped and the sums are 1).
 * materialize_bf16 (round 6, configs[4]'s bf16 arithmetic): one GEMM pass + one in-place elementwise pass over the bf16 [M,V] buffer.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int M, V, K;
    int bf16;
    const void* X;  int ldx;
    const void* W;  int ldw;
    const float* bias;
    const int32_t* targets;
    const float* row_weights;
    float grad_scale;
    int keras_sparse;
    float* loss_rows;
    void* dlogits;  int lddl;  int dl_bf16;
    float* dbias;
    int materialize_bf16;     /* bf16 = dl_bf16 = 1 with dlogits, large problems (the 256-square tile): the first GEMM pass ROUNDS the logits to
                                 bf16 and parks them in the dlogits buffer; statistics, loss and gradient are those of the rounded logits
                                 (what a bf16 framework that materialises its logits computes); the clip sums and the gradient are then
                                 elementwise passes over that buffer, in place -- ONE GEMM pass instead of two or three.  0 (default) and
                                 every other shape: fp32 logits recomputed per pass, never stored. */
} dc_vocab_ce_desc;

size_t dc_vocab_ce_workspace_bytes(const dc_vocab_ce_desc* d);
int    dc_vocab_ce(const dc_vocab_ce_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Vocabulary projection FUSED with the row top-1 (greedy decoding): logits = X[M,K] * W[K,V] + bias are reduced tile by tile inside
 * the GEMM and never written.  Replaces, per decoded token, Dense(V, activation='softmax') + tf.argmax + the chosen word's probability
 * of ROICaptionInferenceLayer (text_generation_model.py:192-232, :222-225; dense_img_cap/dense_model.py:820).
 *   X, W float32 (fp32 MFMA products, as dc_gemm_f32), K % 32 == 0, ldx % 4 == 0, ldw % 4 == 0, ldw >= V rounded up to 4 (the
 *   columns up to that are read, never used: any V >= 1); X, W, bias 16-byte aligned; bias [V] or NULL.
 *   tokens [M] int32 (out): id = argmax_v z_v, the LOWEST index on ties (dc_argmax_rows_f32, tf.argmax) -- the next decode step's
 *   embedding-gather rows;  ids (optional): ids[m * ld_ids] = id (e.g. column j of a row-major [B,T] matrix);  probs (optional):
 *   probs[m * ld_probs] = softmax(z)_id = 1 / sum_v exp(z_v - max z);  mask (optional) [M] uint8: id != 0 (the Keras mask of the token).
 * Runs the kernels of dc_vocab_topk_f32 at k = 1: per (row, 128-column tile) the epilogue keeps max, argmax and sum exp; a second
 * launch combines the tiles of a row in a fixed order, so the result is deterministic and the same at every M.  A row without an
 * orderable logit (NaNs only) gets id 0 and probability 1 / s.  Workspace: dc_vocab_top1_workspace_bytes(M, V) =
 * dc_vocab_topk_workspace_bytes(M, V, 1) (16 bytes per row and tile).
 * Cost model: one GEMM pass (2 M K V flops; W streamed about once: the row tiles of a column panel run side by side) + M ceil(V/128)
 * x 16 bytes of partials, against the unfused [M,V] logits store + a softmax pass + an argmax pass + a gather (4 sweeps of 4 M V
 * bytes).  Greedy decoding with it runs the vocabulary layer over the B live rows once per token instead of T*B rows per token.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int M, V, K;
    const float* X;  int ldx;
    const float* W;  int ldw;
    const float* bias;
    int32_t* tokens;
    int32_t* ids;    int ld_ids;
    float* probs;    int ld_probs;
    uint8_t* mask;
} dc_vocab_top1_desc;

size_t dc_vocab_top1_workspace_bytes(int M, int V);
int    dc_vocab_top1_f32(const dc_vocab_top1_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Vocabulary projection FUSED with the row top-k (beam search, 1 <= k <= 8, V >= k): the k best words of each row and their softmax
 * probabilities, from logits = X[M,K] * W[K,V] + bias that are never written.  Replaces, per beam and token, model.predict's softmax
 * row + np.argsort(...)[-k:] of the reference's beam loop (image captioning/test.py:33-44) for the v2 decoders.
 *   X, W, bias: as dc_vocab_top1_f32 (any V >= k).  ids [M][k] int32, probs [M][k] float32 (out, contiguous): the k best words in the
 *   order value descending, then column ascending; probs[m][r] = exp(z_r - max z) / sum_v exp(z_v - max z); ranks past the
 *   row's orderable (non-NaN) logits get id 0 and probability 0.  k = 1 gives dc_vocab_top1_f32's id and probability (the same kernels).
 * Per (row, 128-column tile) the epilogue keeps max, sum exp and the tile's k best (value, column) pairs (k threshold rounds of the
 * 32-lane shuffle reduction); a second launch, one wave per row, combines the tiles_n * k candidates in an order fixed by V alone, so
 * the result is deterministic and the same at every M.  Workspace: dc_vocab_topk_workspace_bytes(M, V, k) (8 (k + 1) bytes per row
 * and tile).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int M, V, K, k;
    const float* X;  int ldx;
    const float* W;  int ldw;
    const float* bias;
    int32_t* ids;
    float* probs;
} dc_vocab_topk_desc;

size_t dc_vocab_topk_workspace_bytes(int M, int V, int k);
int    dc_vocab_topk_f32(const dc_vocab_topk_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The two fused vocabulary reductions above on bf16 operands and the bf16 matrix pipe (fp32 accumulate): the arithmetic a bf16 model
 * trains its vocabulary layer in (dc_vocab_ce, bf16 = 1), for decoding that model.  Outputs, tie rule, NaN rule, k range: as the
 * fp32 entry points (the epilogue's rounds and the row kernel are the same code).
 *   X [M][ldx], W [K][ldw]: bf16 bit patterns; bias fp32 [V] or NULL.  Operand rules of dc_vocab_ce's bf16 branch: K, ldx, ldw
 *   multiples of 8, X, W, bias 16-byte aligned, operands < 2 GiB; any V >= k provided ldw >= V rounded up to 8 (the columns up to that
 *   are read, never used).
 *   tile: 0 = automatic, 128 or 256.  128: bgemm_core.h's 128 x 128 loop and the fp32 kernel's LDS epilogue, one cell per row and
 *   128-column tile.  256: bgemm256_core.h's 256 x 256 loop; every wave reduces its 64-column slice of the tile in registers and
 *   writes its own cell (ceil(V / 64) cells per row).  Automatic picks the tile dc_vocab_ce's bf16 branch picks for the same M, V, K
 *   (dc_vocab_topk_bf16_tile tells which, without launching).
 * Deterministic; with `tile` fixed the result of a row is the same at every M (automatic may pick another tile at another M).  The
 * two tiles sum the K products of a logit in different orders: between them, and against a float64 reference, ids agree on every
 * row whose adjacent top-(k+1) logit gaps exceed the fp32 dot-product bound 2 K 2^-24 max_v sum_k |x_k w_kv|.
 * Workspace: dc_vocab_topk_bf16_workspace_bytes(M, V, K, k, tile) (8 (k + 1) bytes per row and cell); 0 for a tile that is none of the three.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int M, V, K;
    const void* X;   int ldx;
    const void* W;   int ldw;
    const float* bias;
    int32_t* tokens;
    int32_t* ids;    int ld_ids;
    float* probs;    int ld_probs;
    uint8_t* mask;
    int tile;
} dc_vocab_top1_bf16_desc;

typedef struct {
    int M, V, K, k;
    const void* X;   int ldx;
    const void* W;   int ldw;
    const float* bias;
    int32_t* ids;
    float* probs;
    int tile;
} dc_vocab_topk_bf16_desc;

int    dc_vocab_topk_bf16_tile(int M, int V, int K);
size_t dc_vocab_top1_bf16_workspace_bytes(int M, int V, int K, int tile);
size_t dc_vocab_topk_bf16_workspace_bytes(int M, int V, int K, int k, int tile);
int    dc_vocab_top1_bf16(const dc_vocab_top1_bf16_desc* d, void* workspace, size_t workspace_bytes, void* stream);
int    dc_vocab_topk_bf16(const dc_vocab_topk_bf16_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Vocabulary projection FUSED with a draw from the model's own word distribution (stochastic decoding), by the Gumbel-max
 * identity: argmax_v (z_v / t + g_v) with g_v i.i.d. standard Gumbel is an exact draw from softmax(z / t).  The [M,V] logits
 * z = X W + bias are never written; the draw is one more reduction of the tile epilogue.  The reference never samples: this
 * contract is defined here and restated in float64 by the tests.
 *   What is drawn: for row i the word argmax_v fma(z_v, inv_t, g(i, v)) (one fused multiply-add in fp32), the LOWER column on
 *   equal values.  inv_t = 1 / temperature (finite, > 0).  A NaN logit never wins; a row with no orderable logit yields id 0,
 *   as the top-1 entry points do.
 *   The noise is counter-based: (r0, r1) = Philox-2x32-10 with counter (v >> 1, offset + i (32-bit wrapping)) and key seed, both
 *   output words kept; r = (v & 1) ? r1 : r0;  u = ((r >> 9) + 0.5) * 2^-23 (exact in fp32, in [2^-24, 1 - 2^-24]);
 *   g = -logf(-logf(u)) with the accurate logf.  g is a pure function of (seed, offset + i, v): it does not depend on M, the
 *   tile shape, the grid, the precision of the operands or the call, so rows [a, b) of a call equal a call on those rows
 *   with offset + a, and a caller that decodes step j over n rows passes offset0 + j * n.
 *   probs: the probability the model gives the chosen word at temperature 1 over the whole vocabulary,
 *   exp(z_w - m) / s with m, s the row's maximum and sum of exp(z - m) over the UNPERTURBED logits (the tile epilogue's
 *   arithmetic of the top-k kernels): the quantity the greedy and beam entry points report.
 *   top_k: 0 = the whole vocabulary; 1..8 (V >= top_k) = the draw is restricted to the row's top_k best words, in the order the
 *   top-k entry points return them: the same g(i, v) is added to those candidates' z * inv_t and the best taken.  probs keeps
 *   its meaning.  top_k = 1 is greedy: the top-1 entry point's ids and probabilities bit for bit.
 *   Outputs, operand rules, strides: as the top-1 entry points (tokens [M], optional ids / probs with a row stride, optional
 *   mask [M] = id != 0).
 * Kernels: top_k = 0 runs the 128 x 128 tile loop of the top-1 kernels (fp32 MFMA, or bf16 on bgemm_core.h's loop) into an
 * epilogue that writes, per (row, 128-column tile), a cell of three float2: (max, sum exp) of the unperturbed logits, the tile's
 * best perturbed pair (y, column (int bits); INT_MAX = none) and that column's unperturbed logit.  A row kernel (one wave per
 * row) reduces the cells in an order fixed by the tile count alone.  The bf16 256 x 256 tile has no sampling epilogue: tile = 256
 * with top_k = 0 is refused, 0 means 128.  top_k >= 1 runs the top-k tile kernel unchanged (bf16: tile as there) and a row
 * kernel that perturbs the k row winners.  Ordinary launches on the caller's stream, capturable.
 * Workspace: dc_vocab_sample_workspace_bytes(M, V, top_k): 24 bytes per row and tile at top_k = 0, else the top-k workspace.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int M, V, K;
    const float* X;  int ldx;
    const float* W;  int ldw;
    const float* bias;
    int32_t* tokens;
    int32_t* ids;    int ld_ids;
    float* probs;    int ld_probs;
    uint8_t* mask;
    float inv_t;
    uint32_t seed, offset;
    int top_k;
} dc_vocab_sample_desc;

typedef struct {
    int M, V, K;
    const void* X;   int ldx;
    const void* W;   int ldw;
    const float* bias;
    int32_t* tokens;
    int32_t* ids;    int ld_ids;
    float* probs;    int ld_probs;
    uint8_t* mask;
    int tile;
    float inv_t;
    uint32_t seed, offset;
    int top_k;
} dc_vocab_sample_bf16_desc;

size_t dc_vocab_sample_workspace_bytes(int M, int V, int top_k);
size_t dc_vocab_sample_bf16_workspace_bytes(int M, int V, int K, int top_k, int tile);
int    dc_vocab_sample_f32(const dc_vocab_sample_desc* d, void* workspace, size_t workspace_bytes, void* stream);
int    dc_vocab_sample_bf16(const dc_vocab_sample_bf16_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * One beam-search step for R RoIs with k beams each (image captioning/test.py:33-56).  Rows of the per-beam
 * tensors are BEAM-MAJOR: beam b of RoI r is row b * R + r.
 *   cand_ids / cand_probs [k*R][k]: dc_vocab_topk_f32's output for every beam row;  nb: live beams (1 at the first step, then k);
 *   scores_in [R][k] (NULL: zeros).  Candidate (b, i) scores scores_in[r][b] + p (log_score 0, the reference's rule) or + log p.
 *   The k best of the nb * k candidates, in the order score descending, parent beam ascending, word id ascending, become beams 0..k-1:
 *   scores_out [R][k], parents / tokens_hist [steps][R][k] at step j, tokens [k*R] (optional: the next embedding-gather rows),
 *   mask [k*R] (optional: token != 0).  h_in / c_in -> h_out / c_out [k*R][U] (optional, U % 4 == 0, 16-byte aligned): row q * R + r
 *   receives row parent * R + r (the word LSTM's state follows its beam).
 * dc_beam_step_f32: the same step (same rows, order and fallback; dc_beam_select_f32 runs its kernel) with two additions.
 *   Row sets: n_sets <= DC_BEAM_MAX_SETS entries (src, dst, U), each [k*R][U] with U % 4 == 0 and 16-byte aligned bases; widths may
 *   differ.  Row q * R + r of dst receives row parent * R + r of src.  No dst may overlap a src or another dst.  n_sets = 0: no copy.
 *   End token: end_id (-1: none), finished_in uint8 [k*R] (NULL: nobody is finished), finished_out uint8 [k*R] (required when
 *   end_id >= 0; must not alias finished_in).  A finished beam proposes exactly ONE candidate: token 0 at its scores_in entry, nothing
 *   added under either score rule, its parent itself; its cand_ids / cand_probs rows are not read.  A live beam proposes its k words.
 *   New beam q is finished when its parent was or its token is end_id.  A finished beam's token 0 writes mask 0, so the next LSTM
 *   steps carry its state (the carry a generated 0 gets anyway).  After the first step there are always at least k candidates: a live
 *   beam brings k, and at worst k finished beams bring one each.
 *   One block of four waves per RoI: every wave repeats the k selection rounds, the row copies are spread over the block.
 * dc_beam_backtrace: parents / tokens_hist [steps][R][k] -> seq [R][k][steps], the beams' token sequences.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int R, k, nb, steps, j, log_score;
    const int32_t* cand_ids;
    const float* cand_probs;
    const float* scores_in;
    float* scores_out;
    int32_t* parents;
    int32_t* tokens_hist;
    int32_t* tokens;
    uint8_t* mask;
    int U;
    const float* h_in;
    const float* c_in;
    float* h_out;
    float* c_out;
} dc_beam_select_desc;

#define DC_BEAM_MAX_SETS 4

typedef struct {
    int R, k, nb, steps, j, log_score;
    const int32_t* cand_ids;
    const float* cand_probs;
    const float* scores_in;
    float* scores_out;
    int32_t* parents;
    int32_t* tokens_hist;
    int32_t* tokens;
    uint8_t* mask;
    int end_id;
    const uint8_t* finished_in;
    uint8_t* finished_out;
    int n_sets;
    int U[DC_BEAM_MAX_SETS];
    const float* src[DC_BEAM_MAX_SETS];
    float* dst[DC_BEAM_MAX_SETS];
} dc_beam_step_desc;

int    dc_beam_select_f32(const dc_beam_select_desc* d, void* stream);
int    dc_beam_step_f32(const dc_beam_step_desc* d, void* stream);
int    dc_beam_backtrace(const int32_t* parents, const int32_t* tokens_hist, int steps, int R, int k, int32_t* seq, void* stream);

/* tf.argmax over the last axis, lowest index wins ties (text_generation_model.py:222-225). */
int dc_argmax_rows_f32(const float* x, int M, int V, int ld, int32_t* out, void* stream);

/* Row gather (data movement only): out[n][0:width] = idx[n] >= 0 ? src[idx[n]][0:width] : 0.
 * Builds the Concatenate() operands of the decoders (text_generation_model.py:147-152; _v2.py:161)
 * from per-RoI / per-timestep rows, and routes their gradients back (inverse index). width % 4 == 0. */
int dc_gather_rows_f32(const float* src, int ld_src, const int32_t* idx, float* out, int ld_out,
                       int n_rows, int width, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Trainable RoI head (v1 / joint model: TimeDistributed Conv2D + BatchNorm(training=False) + ReLU with
 * trainable kernel, bias, gamma, beta; text_generation_model.py:251-262).  The conv itself is a
 * dc_gemm_f32 without epilogue (acc = x*kernel); these two kernels apply / differentiate
 *   n = (acc + bias - mean) / sqrt(var + eps),  y = relu(gamma*n + beta)        (eps = 1e-3)
 * fwd: y [M][ld] from acc [M][ld].
 * bwd: given dy (gradient w.r.t. y) and the saved acc: dacc [M][ld] (gradient w.r.t. acc, also the
 *      conv-bias gradient's summand) and the column reductions dgamma, dbeta, dbias [N].
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int M, N, ld;
    const float* acc;
    const float* bias; const float* gamma; const float* beta; const float* mean; const float* var;
    float eps;
    float* y;              /* fwd out */
    const float* dy;       /* bwd in  */
    float* dacc;           /* bwd out */
    float* dgamma; float* dbeta; float* dbias;   /* bwd out [N] */
} dc_bn_relu_desc;

int dc_bn_relu_fwd_f32(const dc_bn_relu_desc* d, void* stream);
int dc_bn_relu_bwd_f32(const dc_bn_relu_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Joint-model helpers (dense_img_cap/dense_model.py).
 * dc_conv_weight_dgrad_pack: packed forward weights [Cout][kh*kw*Cin] -> packed data-gradient weights
 *   [Cin][kh*kw*Cout] (taps rotated 180 degrees), re-derived on the device after every optimizer step.
 * dc_rpn_loss_grad: rpn_class_loss_graph + rpn_bbox_loss_graph (:877-933) for ONE image: `sel` lists the n_sel
 *   non-neutral anchors as (level, cell*A + a) pairs with their match (+1/-1) in anchor order; target_deltas
 *   [n_pos][4] in the order of the positive ones.  Writes d(loss)/d(head) into the (pre-zeroed) padded head
 *   gradients dheads[l] [H,W,head_stride] of this image and losses[0..1] = (class, bbox).
 * dc_scatter2_add: fine[n,2y,2x,c] += coarse[n,y,x,c]  (backward of P6 = MaxPooling2D(1, strides 2)(P5)).
 * dc_axpy: y += a*x  (L2 regulariser gradient, compile() :1715-1718).
 * ------------------------------------------------------------------------------------------------ */
int dc_conv_weight_dgrad_pack_f32(const float* w, float* out, int Cout, int kh, int kw, int Cin, void* stream);
typedef struct {
    int levels, anchors_per_loc, head_stride;
    const float* heads[5];
    float*       dheads[5];
    int Hs[5], Ws[5];
    int n_sel, n_pos;
    const int32_t* sel_level;     /* [n_sel] */
    const int32_t* sel_index;     /* [n_sel] cell*A + a within the level */
    const int32_t* sel_match;     /* [n_sel] +1 / -1 */
    const float*   target_deltas; /* [n_pos][4] */
    float* losses;                /* [2] */
    const int32_t* counts_dev;    /* optional: device words {n_sel, n_pos} that override the two fields above (which then give the
                                     CAPACITY of sel_* / target_deltas): the launch is the same whatever the image's counts are, so a
                                     captured hipGraph can replay it */
} dc_rpn_loss_desc;
int dc_rpn_loss_grad_f32(const dc_rpn_loss_desc* d, void* stream);
int dc_scatter2_add_f32(const float* coarse, float* fine, int N, int Hc, int Wc, int C, void* stream);
/* DetectionTargetLayer for one image on the device (dense_img_cap/dense_model.py:450-572 detection_targets_graph; :421-447
 * overlaps_graph in float32).  proposals [n_proposals][4] / gt_boxes [n_gt][4]: (y1,x1,y2,x2) normalised, all-zero rows are padding;
 * gt_captions [n_gt][T] token ids.  Positives: best IoU >= 0.5 (at most max_positive = int(TRAIN_ROIS_PER_IMAGE * ROI_POSITIVE_RATIO)),
 * negatives: best IoU < 0.5, int32(inv_ratio * float32(n_pos)) - n_pos of them (inv_ratio = float32(1 / ROI_POSITIVE_RATIO)).
 * tf.random_shuffle of the two index lists = ascending order of Philox-2x32-10(counter = (position of the proposal among the non-zero
 * ones, offset + *offset_dev), key = seed) with the position breaking ties (shuffle = 0: proposal order); the reference's shuffle is
 * non-deterministic, this one is reproducible from (seed, offset).  offset_dev (optional): a device word added to `offset`, so that a
 * captured hipGraph draws a fresh sample every replay.
 * Writes rois [n_rois][4] (positives, then negatives, zero padded), captions [n_rois][T] (the best GT box's caption for positives,
 * zeros otherwise) and counts = {n_pos, n_neg}.  Limits: n_proposals <= 4096, n_gt <= 512.  ceil(n_proposals / 256) workgroups, each
 * building the same class / key table in its LDS and ranking its own 256 proposals (outputs are disjoint rows); one image per call (a batch:
 * one call per image, dense_img_cap/utils.py batch_slice); no workspace. */
typedef struct {
    int n_proposals, n_gt, n_rois, T;
    const float*   proposals;
    const float*   gt_boxes;
    const int32_t* gt_captions;
    int   max_positive;
    float inv_ratio;
    int   shuffle;
    uint32_t seed, offset;
    const uint32_t* offset_dev;
    float*   rois;
    int32_t* captions;
    int32_t* counts;          /* [2] */
} dc_detection_targets_desc;
int dc_detection_targets_f32(const dc_detection_targets_desc* d, void* stream);
/* build_rpn_targets (dense_img_cap/dense_model.py:1095-1183) for B images on the device, written in the packed form dc_rpn_loss_grad_f32
 * reads with batched heads.  anchors [A][4] float64 (utils.generate_pyramid_anchors' own array), gt_boxes [B][gt_capacity][4] float64,
 * gt_counts [B]: the images' box counts as DEVICE words (clamped to 0..gt_capacity; no launch shape depends on them).  Per image: the
 * float64 IoU matrix with utils.compute_overlaps' operations in its order, best box = first argmax; negative (-1) below 0.3, positive
 * (1) where an anchor attains a box's column maximum (a column maximum of 0 claims every anchor with IoU 0, as on the host) or reaches
 * 0.7; without boxes every anchor is a negative.  np.random.choice is replaced by counter-based keys: key(a) = word 0 of
 * Philox-2x32-10(counter = (a, offset + *offset_dev), key = seed + b * 0x85EBCA6B) for anchor a of image b; the budget / 2 positives
 * with the smallest (key, a) pairs stay, then the budget - (positives kept) negatives with the smallest pairs; the rest is neutral.
 * Output, images in order and anchors ascending: sel_level / sel_index (a - start of its level + b * level_sizes[level]: the index
 * inside the level's [B,h,w,anchors] head tensor) / sel_match, each [B * budget]; deltas [B * budget][4] float32: the kept positives'
 * ((gcy - acy) / ah, (gcx - acx) / aw, log(gh / ah), log(gw / aw)) / std_dev against their best box, computed in float64, rows packed in
 * the same order; counts = {n_sel, n_pos} over the batch; the unused tail of every output is zeroed.  Limits: budget 2..1024,
 * gt_capacity 1..512, B <= 64, at most 5 levels whose sizes sum to A; anchors / gt_boxes 8-byte, the workspace 16-byte aligned
 * (DC_EALIGN).  Eight launches, integer atomics only: two calls give identical bits.  Boxes are expected finite. */
typedef struct {
    int B, A, n_levels;
    int level_sizes[5];           /* anchors per image of each pyramid level (h * w * anchors per location) */
    int gt_capacity, budget;
    const double*   anchors;
    const double*   gt_boxes;
    const int32_t*  gt_counts;
    double   std_dev[4];
    uint32_t seed, offset;
    const uint32_t* offset_dev;   /* optional device word added to offset (a captured hipGraph draws fresh keys every replay) */
    int32_t* counts;              /* [2] */
    int32_t* sel_level;
    int32_t* sel_index;
    int32_t* sel_match;
    float*   deltas;
} dc_rpn_targets_desc;
size_t dc_rpn_targets_workspace(const dc_rpn_targets_desc* d);
int dc_rpn_targets_f64(const dc_rpn_targets_desc* d, void* workspace, size_t workspace_bytes, void* stream);
/* Index tables of the Model-3 decoder from device-resident captions [B][T] (dense_img_cap/dense_model.py:1572-1580: target = caption
 * shifted left by one; imgcap_caption_loss_graph :936-946: mean over positions with target > 0): ids_tm / targets_tm [T*B] time-major
 * (row t*B + b), mask = ids != 0, row_weights = [target > 0] / max(count, 1), live_count[0] = count (may be NULL). */
int dc_caption_tables_i32(const int32_t* captions, int B, int T, int32_t* ids_tm, uint8_t* mask, int32_t* targets_tm, float* row_weights,
                          int32_t* live_count, void* stream);
/* keras.regularizers.l2(WEIGHT_DECAY)(w) / size(w) summed over the trainable non-BN weights
 * (dense_img_cap/dense_model.py:1712-1718) over one flat bucket: coef[i] = WEIGHT_DECAY/size of i's tensor (0 where not
 * regularised).  grad[i] = grad[i]*mask[i] + 2*coef[i]*w[i] (grad may be NULL; mask = the 0/1 subset set_trainable() left
 * trainable, :1732-1774, NULL = all of it); loss[0] = sum coef[i]*w[i]^2 (loss may be NULL), summed in a fixed order through
 * `workspace` (dc_l2_reg_workspace_bytes; only needed with a loss): bit-reproducible. */
size_t dc_l2_reg_workspace_bytes(size_t n);
int dc_l2_reg_f32(const float* w, const float* coef, const float* mask, float* grad, size_t n, float* loss, void* workspace,
                  size_t workspace_bytes, void* stream);

int dc_axpy_f32(float a, const float* x, float* y, size_t n, void* stream);

/* out = (y > 0) ? dy : 0 over [M][N] (row strides ld): backward of Activation('relu') given its output. */
int dc_relu_bwd_f32(const float* dy, const float* y, float* out, int M, int N, int ld, void* stream);
/* The same over n contiguous elements (n % 4 == 0) with 16-byte accesses, writing the fp32 result and / or its bf16 copy (either may be
 * NULL): the RPN branch's d(shared) feeds bf16 convolutions, and a separate cast pass would read the fp32 result once more. */
int dc_relu_bwd_dual_f32(const float* dy, const float* y, float* out, uint16_t* out_bf16, size_t n, void* stream);

/* out[b][n] = sum_t x[t*B + b][n]  (time-major fold: the per-RoI gradient of a term that was broadcast
 * over timesteps -- RepeatVector(feature), text_generation_model.py:146). */
int dc_fold_time_f32(const float* x, int T, int B, int N, int ld, float* out, int ld_out, void* stream);

/* demb[v][w] = sum over the rows m (ascending) with ids[m] == v of dx[m][w]: the gradient of a trainable KL.Embedding(V, W)
 * (image captioning/model.py:36-39) from d(embedded tokens) dx [n][W] (rows ld apart) and the n token ids.  EVERY row of demb [V][W]
 * (rows ld_e apart) is written -- zeros for a word the batch does not hold -- in one fixed order without atomics: bit-reproducible.
 * An id outside [0, V) contributes nothing.  DC_EINVAL: a null pointer, n / V / W < 1, ld or ld_e below W. */
int dc_embedding_grad_f32(const float* dx, int ld, const int32_t* ids, int n, float* demb, int ld_e, int V, int W, void* stream);

/* out[b][c] = (((x[b][0][c] + x[b][1][c]) + x[b][2][c]) + ... + x[b][K-1][c]) / K in float32: the additions sequential over k, then one
 * correctly rounded division -- what np.mean(float32[K, ...], axis=0) computes, bit for bit (the image-level feature vector of
 * feature_generation/generate_roi_features.py:60-75: the mean of the [1000,7,7,256] RoIAlign block over its RoIs).  A tree or split-K
 * sum (dc_colsum_f32) or a multiplication by 1 / K gives other bits from K = 3 on.
 * x: B blocks of K rows of C floats, rows ld floats apart (ld >= C), blocks batch_stride floats apart; out: B rows, ld_out floats
 * apart.  One launch, grid over (columns, B).  Any pointer alignment and any C: rows are read 16 bytes at a time where x, ld and
 * batch_stride keep them on 16-byte boundaries, element by element otherwise -- the same values either way.
 * DC_EINVAL before anything is launched: a null pointer, B outside 1..65535, K outside 1..2^24 - 1, C < 1, ld or ld_out below C. */
int dc_row_mean_f32(const float* x, int B, int K, int C, long ld, long batch_stride, float* out, long ld_out, void* stream);

/* out[n] (+)= sum_m x[m][n]  -- bias gradients (K.sum over batch/time inside the Dense/Conv backward of Keras).
 * Tall matrices are summed in row chunks through `workspace` (dc_colsum_workspace_bytes) and combined in a fixed
 * order: bit-reproducible.  Without workspace the kernel falls back to one chunk. */
size_t dc_colsum_workspace_bytes(int M, int N, int ld);
int dc_colsum_f32(const float* x, int M, int N, int ld, float* out, int accumulate, void* workspace, size_t workspace_bytes,
                  void* stream);

/* out[0] (+)= sum(x^2) -- global-norm clipping (Adam(clipnorm=0.5), dense_img_cap/dense_model.py:1699).  Block partials go
 * through `workspace` (dc_sumsq_workspace_bytes) and are combined in a fixed order: every data-parallel rank derives the
 * same clip scale from the same all-reduced gradient, and a run is bit-reproducible. */
size_t dc_sumsq_workspace_bytes(size_t n);
int dc_sumsq_f32(const float* x, size_t n, float* out, int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* Inverted-dropout mask of ones: out[i] = 1/(1-rate) with probability 1-rate, else 0 -- K.dropout(K.ones_like(h), rate), the
 * per-gate recurrent_dropout masks Keras' LSTMCell draws in the training phase (recurrent.py _generate_recurrent_dropout_mask;
 * used by text_generation_model.py:141-142 and dense_img_cap/dense_model.py:769-770 with rate 0.2).  Counter-based
 * (Philox-2x32-10): element i of stream (seed, offset) is a pure function of (i, seed, offset).  offset_dev (optional): a device
 * word added to `offset` (a captured hipGraph then draws fresh masks every replay: the host bumps the word between replays). */
int dc_dropout_mask_f32(float* out, size_t n, float rate, uint32_t seed, uint32_t offset, const uint32_t* offset_dev, void* stream);

/* Training ResNet stages (dense_img_cap/dense_model.py:1829-1845: layers "3+" | "4+" | "5+" | "all"; BatchNorm with frozen
 * statistics :51-61, trainable gamma / beta and convolution).
 *   dc_bn_fold_f32: scale[c] = gamma[c] / sqrt(var[c] + eps), shift[c] = beta[c] + (bias[c] - mean[c]) * scale[c] -- the fused
 *     epilogue operands of the forward convolution, refreshed from the trained parameters before every pass.
 *   dc_bn_bwd_f32: given dz [rows][channels] = d(loss)/d(BN output) and the BN output itself as a - b (b may be NULL):
 *     dacc = dz * scale (gradient w.r.t. the convolution output, also the summand of the conv-bias gradient) and
 *     dzn = dz * (a - b - beta) / gamma (0 where dz == 0); column sums of dzn / dz are dgamma / dbeta, dbias = scale * dbeta.
 *   dc_mul_f32: out = a * b elementwise. */
int dc_bn_fold_f32(const float* gamma, const float* beta, const float* bias, const float* mean, const float* var, float eps,
                   float* scale, float* shift, int n, void* stream);
int dc_bn_bwd_f32(const float* dz, const float* a, const float* b, const float* gamma, const float* beta, const float* scale,
                  float* dacc, float* dzn, long rows, int channels, void* stream);
int dc_mul_f32(const float* a, const float* b, float* out, size_t n, void* stream);
/* Backward of dc_maxpool3x3s2_same_f32 (the stem's pool, trained with layers = "all"): dx[pixel] = sum of dy over the windows whose
 * first maximum (row-major, as TF's MaxPoolGrad) is this pixel.  x [N,H,W,C], y / dy [N,ceil(H/2),ceil(W/2),C]. */
int dc_maxpool3x3s2_same_bwd_f32(const float* x, const float* y, const float* dy, float* dx, int N, int H, int W, int C, void* stream);

/* bytes of zeros at p (pointer and size multiples of 4): a kernel, not a memset node -- a captured hipMemsetAsync node faulted on its
 * second replay on this runtime (round 4), so the library and its callers zero buffers with this. */
int dc_zero_fill(void* p, size_t bytes, void* stream);

/* mean of loss rows: out[0] = sum(x)/n. */
int dc_mean_f32(const float* x, size_t n, float* out, void* stream);

/* Piecewise-constant per-element coefficients over a flat parameter bucket: segment s covers elements [start[s], start[s+1]) and
 * carries coef[s] (WEIGHT_DECAY / size(tensor), 0 for BatchNorm gamma / beta and padding) and mask[s] (1 = trainable, 0 = frozen;
 * mask NULL = everything trains).  The arrays live in DEVICE memory; start has nseg + 1 ascending entries, start[0] = 0, start[nseg] = n.
 * Replaces the two n-element float vectors dc_l2_reg_f32 reads (2 x 300 MB per step for the joint model's 77 M parameters). */
typedef struct {
    const int32_t* start;
    const float* coef;
    const float* mask;
    int nseg;
} dc_reg_segments;

/* ------------------------------------------------------------------------------------------------
 * keras.optimizers.Adam(amsgrad=True) fused over one flat parameter bucket
 * (text_generation_model.py:425; _v2.py:266): with g' = g * grad_scale * clip,
 *   m = b1*m + (1-b1)*g' ; v = b2*v + (1-b2)*g'^2 ; vhat = max(vhat, v) ; p -= lr_t*m/(sqrt(vhat)+eps)
 * lr_t = lr*sqrt(1-b2^t)/(1-b1^t) is computed by the caller.  If gnorm_sq (device scalar: sum of
 * squares of the UNSCALED gradients) is non-NULL and clipnorm > 0, clip = clipnorm/norm when
 * norm >= clipnorm (norm taken after grad_scale), else 1.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    size_t n;
    float* p;
    const float* g;
    float* m;
    float* v;
    float* vhat;
    float lr_t, beta1, beta2, eps;
    float grad_scale;
    const float* gnorm_sq;
    float clipnorm;
    uint16_t* p_bf16;         /* optional: bf16 shadow of p (the operand copy the bf16 GEMMs read), refreshed in the same pass */
    size_t n_bf16;            /* the shadow covers p[0 .. n_bf16) (a multiple of 4) */
    const float* lr_t_dev;    /* optional: a device word that overrides lr_t (Keras' lr_t depends on the iteration count; a captured
                                 hipGraph reads this step's value from memory the host refreshed before the replay) */
    const dc_reg_segments* reg; /* optional (HOST pointer, read during the call): the joint model's regulariser and trainable mask applied
                                 INSIDE this pass -- the gradient the update sees is g * mask + 2 * coef * p with per-segment constants --
                                 instead of by a dc_l2_reg_f32 pass that rewrites the gradient bucket first; gnorm_sq must then come from
                                 dc_reg_sumsq_f32 (the norm of that same regularised gradient).  The gradient bucket is left as it was */
} dc_amsgrad_desc;

int dc_amsgrad_step_f32(const dc_amsgrad_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * keras.optimizers.Adam (amsgrad=False) and keras.optimizers.SGD (momentum, nesterov) fused over one flat parameter bucket: the
 * siblings of the launch above that read and write only the streams their update needs (Adam: p, g, m, v -- no vhat; SGD with
 * momentum: p, g, velocity; plain SGD: p, g).  fp32, per element, in this order:
 *   g' = g * mask + 2 * coef * p (reg given, else g) ; gg = g' * grad_scale * clip (clip as dc_amsgrad_step_f32 takes it from
 *   gnorm_sq / clipnorm) ; clipvalue > 0: gg = min(max(gg, -clipvalue), clipvalue)   (Keras' get_gradients: by norm, then by value)
 *   DC_OPT_ADAM: m = beta1*m + (1-beta1)*gg ; v = beta2*v + (1-beta2)*gg*gg ; p -= step * m / (sqrt(v) + eps)
 *                (step = lr*sqrt(1-beta2^t)/(1-beta1^t), computed by the caller)
 *   DC_OPT_SGD:  u = step*gg ; vel = beta1*vel - u ; p += nesterov ? beta1*vel - u : vel      (beta1 = the momentum, step = lr)
 *                beta1 == 0 and state0 == NULL: p -= u, no state is read or written
 * ------------------------------------------------------------------------------------------------ */
#define DC_OPT_ADAM 0
#define DC_OPT_SGD 1
typedef struct {
    int kind;                 /* DC_OPT_ADAM | DC_OPT_SGD */
    int nesterov;             /* DC_OPT_SGD only */
    size_t n;
    float* p;
    const float* g;
    float* state0;            /* Adam: m; SGD: the velocity (NULL with beta1 == 0) */
    float* state1;            /* Adam: v; SGD: NULL */
    float step;               /* the word the update multiplies with */
    const float* step_dev;    /* optional: a device word that overrides step (as lr_t_dev above: a captured hipGraph replays with this
                                 step's value) */
    float beta1, beta2, eps;
    float grad_scale;
    const float* gnorm_sq;    /* as above */
    float clipnorm;
    float clipvalue;          /* 0 = off */
    uint16_t* p_bf16;         /* as above: the bf16 shadow of p[0 .. n_bf16), refreshed in the same pass */
    size_t n_bf16;
    const dc_reg_segments* reg; /* as above: HOST pointer, read during the call; gnorm_sq then comes from dc_reg_sumsq_f32 */
} dc_optimizer_desc;

int dc_optimizer_step_f32(const dc_optimizer_desc* d, void* stream);

/* One READ-ONLY pass over (w, g) in front of the fused update above (round 5: replaces dc_l2_reg_f32 + dc_sumsq_f32 = three reads and
 * one write of the bucket + one more read, by two reads): loss[0] = sum coef * w^2 (the L2 term of dense_img_cap/dense_model.py:1715-1718),
 * gnorm_sq[0] = sum (g * mask + 2 * coef * w)^2 (what Adam(clipnorm=0.5), :1699, clips by), both as block partials in block order
 * through `workspace`, added by one block in a fixed tree (bit-reproducible).  Either output may be NULL. */
size_t dc_reg_sumsq_workspace_bytes(size_t n);
int dc_reg_sumsq_f32(const float* w, const float* g, const dc_reg_segments* reg, size_t n, float* loss, float* gnorm_sq, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RoI tag head: sigmoid + focal loss + d/dlogits in one launch (roi_tag_classification/model.py:48-66 focal_loss, :877-887
 * roi_tag_classes_loss_graph, on Keras 2.1's K.binary_crossentropy over probabilities).
 *   z [M][ldz] float32 logits (C valid columns; the projection GEMM's output, bias added); t [M][ldt] int32 multi-hot targets.
 *   per element:  p = sigmoid(z) ; q = clip(p, lo, hi), lo = (float)1e-7, hi = (float)(1 - 1e-7) ; x = log(q / (1 - q)) ;
 *                 bce = max(x, 0) - x t + log(1 + exp(-|x|)) ; fw = t == 1 ? 1 - p : p (the UNCLIPPED p) ;
 *                 a = t == 1 ? alpha : 1 - alpha ; L = a * fw^gamma * bce
 *   A row is live when one of its targets is 1.  loss_rows[m] = sum_c L (live) or 0 (dead); the model's loss is the SUM of loss_rows.
 *   dz [M][lddz] = grad_scale * dL/dz as TensorFlow differentiates the above: through fw's unclipped p, and through the clip only
 *   where lo <= p <= hi.  Dead rows are exact zeros in both outputs whatever their logits hold (the reference gathers them away
 *   before any arithmetic).  dz may alias z.
 *   Evaluated from the logit (exp(-|z|), log1p; p and 1 - p both without cancellation): any finite z gives finite results.
 *   alpha in [0, 1]; gamma 0, 1 or 2 (exact products), anything else DC_EINVAL.  Strides are free: 16-byte accesses when every base and
 *   stride allows them, 4-byte accesses otherwise -- no alignment refusal.  loss_rows and dz are each optional.
 *   One 256-thread block per row: the liveness reduction, then the element pass, then a fixed-order wave / LDS reduction of the row
 *   loss -- no atomics, a row's result does not depend on M or on scheduling.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int M, C;
    const float* z;
    int ldz;
    const int32_t* t;
    int ldt;
    float alpha, gamma, grad_scale;
    float* loss_rows;         /* optional [M] */
    float* dz;                /* optional [M][lddz] */
    int lddz;
} dc_tag_focal_desc;

int dc_tag_focal_f32(const dc_tag_focal_desc* d, void* stream);

/* Inference side of the same head: probs [M][ldp] = sigmoid(z) in float32 and scores [M] = the reference's classes_scores
 * (model.py:644-646): the sum over the classes with p > min_confidence of log p -- decided on the float32 p that is written,
 * log((double)p) accumulated in float64 in a fixed order and rounded once -- or (float)-3.4e38 when no class qualifies.
 * One block per row; either output may be NULL; no alignment rule. */
int dc_tag_scores_f32(const float* z, int ldz, int M, int C, float min_confidence, float* probs, int ldp, float* scores, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Caption metrics on token ids (eval/bleu, eval/rouge, eval/cider of the reference; caption_metrics.py states the formulas).
 * A sentence is a row of int32 ids >= 0 and a length; what lies past the length is never read as a token.  One 64-lane wave per
 * record with the candidate's positions on the lanes: a sentence holds at most DC_CAPTION_MAX_TOKENS tokens (a longer length is
 * read as that many; the Python side refuses it by name).  Any number of references per record, any base alignment.
 *   cand [N][ld_cand] of Tc valid columns, cand_len [N]; refs [M][ld_refs] of Tr valid columns, ref_len [M] (lengths are clamped
 *   into 0..min(width, DC_CAPTION_MAX_TOKENS)); ref_start [N+1] the CSR index of a record's references (clamped into 0..M).
 *   stats [N][12] int32, exact: correct_1..4 (sum over the candidate's distinct k-grams of min(count, max over references of count)),
 *     guess_1..4 = max(0, len - k + 1), testlen, reflen (the reference length closest to testlen, the shorter on a tie), lcs_max, 0.
 *   bleu [4][N] float64: (prod_{j<=k} (correct_j + 1e-15) / (guess_j + 1e-9))^(1/k), times exp(1 - 1/ratio) when
 *     ratio = (testlen + 1e-15) / (reflen + 1e-9) < 1.
 *   rouge [N] float64: (1 + b^2) P R / (R + b^2 P), b = 1.2, P = max_r l / max(1, len cand), R = max_r l / max(1, len ref), 0 when
 *     either is 0.  lcs = 0: l = the positions of the shorter sentence (the candidate on equal lengths) whose token occurs in the
 *     longer one -- what the reference fork's my_lcs returns; lcs = 1: l = the longest common subsequence.
 * N-gram equality compares the ids (up to four int32), nothing is hashed; float64 in a fixed order, no atomics: identical bits from
 * call to call.  DC_EINVAL: a null pointer, N < 1, M < 1, a width below 1 or above its row stride, lcs not 0 / 1.
 * ------------------------------------------------------------------------------------------------ */
#define DC_CAPTION_MAX_TOKENS 64
typedef struct {
    int N, M, Tc, Tr;
    const int32_t* cand;
    int ld_cand;
    const int32_t* cand_len;
    const int32_t* refs;
    int ld_refs;
    const int32_t* ref_len;
    const int32_t* ref_start;
    int lcs;
    int32_t* stats;
    double* bleu;
    double* rouge;
} dc_caption_metrics_desc;

int dc_caption_metrics_f64(const dc_caption_metrics_desc* d, void* stream);

/* CIDEr (n = 4, sigma = 6) per record from dense n-gram ids.  Sentences 0..N-1 are the candidates, N..S-1 the references in
 * ref_start's order.  grams [4][S][T] int32: grams[k-1][s][i] = the id of the k-gram that starts at position i of sentence s, ids of
 * order k in 0..G_k-1 with equal ids exactly for equal n-grams OF ONE GROUP (the caller numbers them; a value outside 0..G_k-1 is
 * "no n-gram").  df [df_len] int32: the document frequency of id g of order k at df[df_off[k-1] + g] (G_k = the next offset, or
 * df_len, minus this one).  group_n [N]: the size of the record's group.  sent_len [S] (clamped to min(T, DC_CAPTION_MAX_TOKENS)).
 *   weight of g = tf * (log group_n - log max(1, df)); per order and reference sum over the candidate's distinct grams of
 *   min(w_c, w_r) w_r / (|c| |r|) (no division when a norm is 0), times exp(-delta^2 / 72), delta the difference of max(len - 1, 0);
 *   cider [N] float64 = mean over the orders of the sum over the references, / references, * 10.
 * One wave per record, float64 in a fixed order, no atomics.  DC_EINVAL: a null pointer, N < 1, S <= N, T < 1, bad df_off. */
typedef struct {
    int N, S, T;
    const int32_t* grams;
    const int32_t* sent_len;
    const int32_t* ref_start;
    const int32_t* df;
    int df_off[4];
    int df_len;
    const int32_t* group_n;
    double* cider;
} dc_caption_cider_desc;

int dc_caption_cider_f64(const dc_caption_cider_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mask R-CNN inference behind the shared RoI head (mask_rcnn/mask_rcnn_model.py; detect.hip).  None of the three allocates,
 * synchronises or reads back; all are capturable and give identical bits from call to call.
 *
 * dc_class_select_f32: per RoI r of logits [R][ld_logits] (C valid columns) and deltas [R][ld_deltas] (4 C valid columns):
 *   class_ids[r] = the LOWEST index of the maximal logit (the argmax of the logits, not of rounded probabilities);
 *   scores[r]    = 1 / sum_j exp(z_j - z_max) in float32: accurate expf, the terms of a lane added in index order (j = lane, lane + 64,
 *                  ...), the 64 lane sums by an xor butterfly -- an order C alone fixes;
 *   deltas_out[r][0..3] = deltas[r][4 class .. 4 class + 3], the words copied.
 *   This is mrcnn_class (softmax) + the first three lines of refine_detections (:684-688).  Logits are expected finite.  One wave per
 *   row.  C is any value from 2 up; strides are free (every access is 4 bytes).  DC_EINVAL: a null pointer, R < 1, C < 2, a stride
 *   below its row length, a pointer off a 4-byte boundary.
 * ------------------------------------------------------------------------------------------------ */
int dc_class_select_f32(const float* logits, int ld_logits, const float* deltas, int ld_deltas, int R, int C, int32_t* class_ids,
                        float* scores, float* deltas_out, void* stream);

/* dc_mask_head_tail_f32: mrcnn_mask_deconv (Conv2DTranspose 2x2, stride 2, ReLU) fused with mrcnn_mask (1x1, sigmoid) for each RoI's
 * own class k = class_ids[n] only:
 *   out[n][2y+dy][2x+dx] = sigmoid(bm[k] + sum_c' relu(bd[c'] + sum_c x[n][y][x][c] * wd[dy][dx][c'][c]) * wm_t[k][c'])
 *   x [N][P][P][Cin] (the fourth mask convolution's output); wd [2][2][Cmid][Cin], the Keras kernel as it is stored; bd [Cmid];
 *   wm_t [C][Cmid], the mrcnn_mask kernel [Cmid][C] TRANSPOSED (a class column becomes one contiguous row: packing.pack_mask_tail);
 *   bm [C]; class_ids int32 [N] in device memory; out [N][2P][2P].
 * The [N P P, Cin] x [Cin, 4 Cmid] product runs on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation in k order, as
 * DC_MATH_F32); ReLU, the dot with the class row and the sigmoid are the tile's epilogue, so neither the [N][2P][2P][Cmid] map nor an
 * all-class map is ever written.  A 128-row tile may hold rows of several RoIs: the class is looked up per row.  The dot over c' is
 * summed in a fixed order (per lane in channel order, then the two lane halves).  A class id outside [0, C) writes zeros for that
 * RoI and reads nothing with it.  The sigmoid is evaluated from exp(-|z|): finite and monotone for any finite z.
 * x, wd and wm_t are read 16 bytes at a time when all three bases sit on 16-byte boundaries and 4 bytes at a time otherwise (the same
 * products in the same order, so the same bits): no alignment refusal.
 * DC_EINVAL: a null pointer, N < 1, P outside 1..16, C < 1, Cin not a multiple of 32 in 32..256 (a lane keeps half a pixel's inputs
 * in registers), Cmid not a multiple of 32 in 32..4096, a pointer off a 4-byte boundary. */
typedef struct {
    int N, P, Cin, Cmid, C;
    const float* x;
    const float* wd;
    const float* bd;
    const float* wm_t;
    const float* bm;
    const int32_t* class_ids;
    float* out;
} dc_mask_head_tail_desc;

int dc_mask_head_tail_f32(const dc_mask_head_tail_desc* d, void* stream);

/* dc_mask_paste_u8: utils.unmold_mask for the M detections of one image.  masks [M][h][w] float32 (h, w in 1..64), boxes int32 [M][4]
 * (y1, x1, y2, x2) in the original image, in DEVICE memory (the host need not know them), out uint8 [M][H][W].  Per detection:
 *   1. scipy 1.0's bytescale with the mask's own minimum and maximum, in float32: scale = (float)(255.0 / (double)(cmax - cmin)) with
 *      a zero range read as 1; byte = (uint8) trunc(clip((m - cmin) * scale, 0, 255) + 0.5f), one rounding per operation;
 *   2. PIL.Image.resize((x2 - x1, y2 - y1), BILINEAR) of that 8-bit image: the horizontal-then-vertical integer arithmetic of
 *      dc_resize_pad_u8, with the same coefficient code;
 *   3. out[m][y1 + y][x1 + x] = byte >= 128; every byte outside the box is written as 0, so the buffer may be reused.
 * A box with non-positive area, or one that leaves the image (y1 < 0, x1 < 0, y2 > H, x2 > W), gives a plane of zeros; nothing is
 * written outside out[m].  Workspace (16-byte aligned): the byte images, the horizontal intermediates (h x W each) and per
 * detection a coefficient table sized for the largest box the image allows.  Four launches whatever M is; M = 0 launches nothing.
 * DC_EINVAL: a null pointer (with M > 0), M outside 0..65535, a mask side outside 1..64, H or W outside 1..2^24 or H W >= 2^31. */
typedef struct {
    int M, h, w, H, W;
    const float* masks;
    const int32_t* boxes;
    uint8_t* out;
} dc_mask_paste_desc;

size_t dc_mask_paste_u8_workspace_bytes(const dc_mask_paste_desc* d);
int    dc_mask_paste_u8(const dc_mask_paste_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* dc_mask_rle_u32: the planes dc_mask_paste_u8 would write for the M detections of one image, as COCO's uncompressed run-length
 * encoding, built on the device without the planes: no [M][H][W] buffer is allocated, written or read.  masks, boxes, h, w, H, W and
 * M are dc_mask_paste_u8's, with its limits.
 * The encoding of one [H][W] plane.  Pixels are read column-major, pixel (y, x) at index i = x * H + y; bit[-1] = 0.  With
 * t_0 < t_1 < ... < t_{T-1} the indices at which bit[i] != bit[i-1], the counts are the T + 1 differences of
 * [0, t_0, ..., t_{T-1}, H * W]: runs of zeros and ones in turn, starting with zeros, so counts[0] = 0 exactly when pixel (0, 0) is
 * set.  The last entry is the final run, whatever its value: a plane whose last pixel is set ends on its run of ones, and NO
 * zero-length run of zeros is appended.  A plane of zeros is [H * W]; sum(counts) = H * W always.  (mask_rle.py encodes by the same
 * rule on the host.)
 * Outputs: offsets int32 [M + 1] and counts uint32 [capacity], both in device memory.  counts[offsets[m] .. offsets[m+1] - 1] is
 * detection m's encoding.  offsets is exact whatever capacity is, and offsets[M] is the number of words the encodings need: entries at
 * flat indices below min(offsets[M], capacity) are written, nothing at or beyond capacity is touched, and a caller that finds
 * offsets[M] > capacity calls again with that capacity.  A box with non-positive area, or one that leaves the image, encodes as
 * [H * W].  M = 0 writes offsets[0] = 0 and nothing else.
 * The work: dc_mask_paste_u8's bytescale, coefficient and horizontal launches as they are; then one wave per (detection, box column)
 * walks 64 rows a step, takes the transitions from a ballot of the thresholded bits and counts them; a prefix sum over the columns
 * of each detection and one over the detections give every transition its slot; the walk runs again and stores the positions; a
 * last launch differences them.  Integer work without atomics: the same bytes on every run.  Seven launches whatever M is.
 * The scratch memory travels in the descriptor: workspace (16-byte aligned) of at least dc_mask_rle_workspace_bytes(d) bytes, which
 * depends on M, h, w, H, W and capacity -- dc_mask_paste_u8's three regions, one int per (detection, column 0..W), one per
 * detection and capacity words of positions.  DC_EWORKSPACE when it is null (with M > 0), too small or misaligned.
 * DC_EINVAL: dc_mask_paste_u8's cases, a null offsets, a null counts with capacity > 0, a negative capacity, offsets or counts off
 * a 4-byte boundary, and M * (H * W + 1) >= 2^31 (the int32 offsets could not hold the worst case). */
typedef struct {
    int M, h, w, H, W, capacity;
    const float* masks;
    const int32_t* boxes;
    int32_t* offsets;
    uint32_t* counts;
    void* workspace;
    size_t workspace_bytes;
} dc_mask_rle_desc;

size_t dc_mask_rle_workspace_bytes(const dc_mask_rle_desc* d);
int    dc_mask_rle_u32(const dc_mask_rle_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Scoring detections against ground truth (csrc/detect_eval.hip): the evaluation side of mask_rcnn/utils.py (compute_overlaps,
 * compute_ap :568-633) and pycocotools' rleIou.  Integer and float64 work in a fixed order without atomics: the same bytes on every
 * run.  The host statements they are held to, bit for bit: mask_rle.iou, utils.compute_overlaps, detection_eval.ap_from_overlaps.
 * ------------------------------------------------------------------------------------------------ */

/* dc_rle_iou_f64: mask IoU of D detections with G ground truths, both as packed run-length encodings in DEVICE memory, in the form
 * dc_mask_rle_u32 writes: offsets_d int32 [D + 1] with counts_d uint32 [capacity_d], offsets_g int32 [G + 1] with counts_g uint32
 * [capacity_g], every mask of the one size H x W.  n_det (optional, device): rows at or beyond n_det[0] are written as 0 without a
 * walk (the rows behind an image's last detection under refine="device").  iscrowd (optional, device uint8 [G]): a non-zero flag
 * makes column g the crowd IoU.
 * Outputs: iou float64 [D][ld]; where non-null, inter int32 [D][ld], the intersections, and area int32 [D + G], the detections' areas
 * then the ground truths'; status int32 [4].  With I the pixels set in both masks and a_d, a_g the areas, exact integers,
 * iou = I / (a_d + a_g - I) as ONE float64 division, for a crowd column I / a_d, and 0 where the denominator is 0.
 * status[0] / status[1]: where offsets_d[D] > capacity_d (offsets_g[G] > capacity_g) the words that set needs, else 0.  With either
 * non-zero nothing at or beyond a capacity is read, every iou is NaN and every inter and area -1: the caller reruns dc_mask_rle_u32
 * with that capacity.  status[2]: the masks whose counts do not sum to H W (or whose offsets are not increasing inside 0..capacity):
 * such a mask's row or column is NaN (inter, area: -1).  status[3] = min(max(n_det[0], 0), D), the rows computed.
 * The work: pass 1, one wave per mask of either set, scans the counts into run ends and the set pixels below each end, and takes the
 * area and the first and last set index; pass 2, one wave per pair, is 0 at once where the two set-index ranges do not meet;
 * otherwise the lanes take the shorter encoding's runs of ones 64 at a time and count the other mask's set pixels inside each by two
 * binary searches in its run ends; a wave sum gives I.  Three launches; D = 0 or G = 0 launches the status write alone (area is not
 * written then) and needs no workspace.
 * The scratch memory travels in the descriptor: workspace (16-byte aligned) of at least dc_rle_iou_workspace_bytes bytes -- two words
 * per count word of capacity_d + capacity_g and four per mask.  DC_EWORKSPACE when it is null, too small or misaligned.
 * DC_EINVAL: a null descriptor, offsets_d, offsets_g or status; a null iou with D, G > 0; a null counts with its capacity above 0; D
 * or G outside 0..1024; H or W below 1 or H W >= 2^31; a negative capacity; ld < G; a pointer off its element's boundary. */
typedef struct {
    int D, G, H, W, capacity_d, capacity_g, ld;
    const int32_t* offsets_d;
    const uint32_t* counts_d;
    const int32_t* offsets_g;
    const uint32_t* counts_g;
    const int32_t* n_det;
    const uint8_t* iscrowd;
    double* iou;
    int32_t* inter;
    int32_t* area;
    int32_t* status;
    void* workspace;
    size_t workspace_bytes;
} dc_rle_iou_desc;

size_t dc_rle_iou_workspace_bytes(const dc_rle_iou_desc* d);
int    dc_rle_iou_f64(const dc_rle_iou_desc* d, void* stream);

/* dc_box_iou_f64: utils.compute_overlaps for B images: boxes int32 [B][Dmax][4] and gt_boxes int32 [B][Gmax][4] as (y1, x1, y2, x2)
 * -> out float64 [B][Dmax][ld], every entry of the Dmax x Gmax block written.  compute_iou's formula on integers -- areas, clipped
 * intersection sides, inter = iw * ih, union = area + area - inter, in int64 (NumPy's int32 results wherever those do not wrap) --
 * and ONE float64 division; a zero union gives the NaN NumPy's 0 / 0 gives.  One launch; B Dmax Gmax = 0 launches nothing.
 * DC_EINVAL: B outside 0..65535, Dmax or Gmax outside 0..1024, ld < Gmax, and with something to compute a null pointer, a box array
 * off a 16-byte boundary or out off an 8-byte boundary. */
int dc_box_iou_f64(const int32_t* boxes, const int32_t* gt_boxes, int B, int Dmax, int Gmax, int ld, double* out, void* stream);

/* dc_detection_ap_f64: utils.compute_ap's matching and average precision on a GIVEN IoU matrix, for B images and T thresholds at
 * once (detection_eval.ap_from_overlaps on the host).  overlaps float64 [B][Dmax][ld], row = prediction in the caller's order; n_det,
 * n_gt int32 [B] in DEVICE memory (under refine="device" the host does not know n_det), clipped to 0..Dmax and 0..Gmax: only the
 * leading n_det x n_gt block of an image is read; pred_class int32 [B][Dmax], pred_score float32 [B][Dmax], gt_class int32
 * [B][Gmax]; thresholds float64 [T].
 * Outputs: ap float64 [B][T]; where non-null, pred_match int32 [B][T][Dmax] -- per prediction IN RANK ORDER the ground truth matched
 * to it or -1 --, gt_match int32 [B][T][Gmax] -- the rank of the prediction matched to it or -1 -- and order int32 [B][Dmax], the
 * prediction at each rank; entries behind n_det / n_gt are -1.
 * The rule.  Predictions are ranked by score, descending, equal scores the HIGHER index first (np.argsort(kind="stable")[::-1]; a
 * NaN score ranks first).  In rank order each takes, among the still unmatched ground truths of its class with IoU >= threshold, the
 * one of the highest IoU, on equal IoU the higher index; a NaN IoU is never eligible.  Then, as the reference: precisions
 * hits / (rank + 1) in float64; recalls hits / n_gt as a FLOAT32 quotient widened to float64; [0] and [0] / [0] and [1] around them;
 * the right-to-left maximum of the precisions; the sum of (recall step) * precision over the indices where the recall changes, in
 * NumPy's order for fewer than 128 terms at any length: a plain loop below 8 terms, otherwise eight accumulators over the whole
 * groups of 8 combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and the remainder in sequence.  n_gt = 0 gives NaN.
 * One launch of T x B workgroups: a rank sort by all threads, the matching by one wave that keeps the matched set in registers (no
 * barrier inside the loop), the sums by one thread.  No workspace.  B = 0 launches nothing.
 * DC_EINVAL: a null descriptor; B outside 0..65535; Dmax or Gmax outside 0..1024; T outside 1..16; ld < Gmax; with B > 0 a null
 * n_det, n_gt, thresholds or ap, a null overlaps with Dmax, Gmax > 0, a null pred_class or pred_score with Dmax > 0, a null gt_class
 * with Gmax > 0, or a pointer off its element's boundary. */
typedef struct {
    int B, Dmax, Gmax, ld, T;
    const double* overlaps;
    const int32_t* n_det;
    const int32_t* n_gt;
    const int32_t* pred_class;
    const float* pred_score;
    const int32_t* gt_class;
    const double* thresholds;
    double* ap;
    int32_t* pred_match;
    int32_t* gt_match;
    int32_t* order;
} dc_detection_ap_desc;

int dc_detection_ap_f64(const dc_detection_ap_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DCAP_H */

// gemm_bf16.hip -- dc_gemm_bf16: dense GEMM with bf16 operands in memory and fp32 accumulation on
// v_mfma_f32_32x32x16_bf16 (bgemm_core.h), all three layouts of a training step (NN / NT / TN), the fused epilogue of
// dc_gemm_f32 plus an optional bf16 copy of the output; and the fp32 -> bf16 cast that feeds it.
#include "bgemm256_core.h"
#include <algorithm>
#include <cstdlib>

namespace dcap {

// dW tile [128 cout][128 (tap, ci)] over the pixel range of this split-K slice
__global__ __launch_bounds__(256, 2) void bgemm_wgrad_kernel(BOperand dy, BIm2col xc, Epilogue ep, int M, int N, int K, int klen,
                                                          float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    char* smem = reinterpret_cast<char*>(smem_f);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int m0, n0;
    BGeo128::origin(M, N, m0, n0);
    const int kbeg = blockIdx.z * klen, kend = min(K, kbeg + klen);
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    BLoadDense<BGeo128, false, true> la;
    BLoadIm2col<BGeo128> lb;
    la.init(dy, m0, lane, wave, kbeg);
    lb.init(xc, n0, lane, wave, kbeg);
    f32x16 acc[2][2];
    bgemm_mainloop_t(la, lb, smem, kbeg, kend, acc, wm, wn);
    store_tile<BT, BT>(acc, smem_f, ep, partial, M, N, m0, n0, wm, wn);
}

// The same weight gradient on the 256 x 256 tile (bgemm256_core.h): the K-major im2col operand as two 128-column sub-images.
__global__ __launch_bounds__(b256::NTHREADS, 2) void bgemm256_wgrad_kernel(BOperand dy, BIm2col xc, Epilogue ep, int M, int N, int K, int klen, float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int m0, n0;
    b256::Geo::origin(M, N, m0, n0);
    const int kbeg = blockIdx.z * klen, kend = min(K, kbeg + klen);
    BLoadDense<b256::Geo, false, true> la;
    BLoadIm2col<b256::Geo> lb;
    la.init(dy, m0, lane, wave, kbeg);
    lb.init(xc, n0, lane, wave, kbeg);
    b256::f32x4 acc[8][4];
    b256::mainloop(la, lb, reinterpret_cast<char*>(smem_f), kbeg, kend, acc);
    b256::store_tile(acc, ep, partial, M, N, m0, n0);
}

static int bgemm_validate(const dc_gemm_bf16_desc* d) {
    DC_REQUIRE(d != nullptr, DC_EINVAL, "dc_gemm_bf16: null descriptor");
    DC_REQUIRE(d->M > 0 && d->N > 0 && d->K > 0, DC_EINVAL, "dc_gemm_bf16: M,N,K must be positive (got %d,%d,%d)", d->M, d->N, d->K);
    DC_REQUIRE(d->A && d->B && (d->C || d->Cb), DC_EINVAL, "dc_gemm_bf16: A, B and one of C / Cb must be non-null");
    DC_REQUIRE(d->lda >= (d->a_trans ? d->M : d->K) && d->ldb >= (d->b_trans ? d->K : d->N), DC_EINVAL,
               "dc_gemm_bf16: leading dimension smaller than the row length");
    DC_REQUIRE((!d->C || d->ldc >= d->N) && (!d->Cb || d->ldcb >= d->N), DC_EINVAL, "dc_gemm_bf16: ldc / ldcb smaller than N");
    DC_REQUIRE((d->K & 7) == 0 && (d->lda & 7) == 0 && (d->ldb & 7) == 0 && aligned16(d->A) && aligned16(d->B), DC_EALIGN,
               "dc_gemm_bf16: K, lda, ldb must be multiples of 8 (16-byte chunks) and A, B 16-byte aligned");
    DC_REQUIRE((!d->a_trans || ((d->M & 7) == 0)) && (d->b_trans || ((d->N & 7) == 0)), DC_EALIGN,
               "dc_gemm_bf16: a K-major operand needs its row length (M for A^T, N for B) to be a multiple of 8");
    DC_REQUIRE(!d->accumulate || d->C, DC_EINVAL, "dc_gemm_bf16: accumulate needs the fp32 output C");
    DC_REQUIRE(!d->residual || d->ldr >= d->N, DC_EINVAL, "dc_gemm_bf16: ldr smaller than N");
    const size_t lim = (size_t)0x7FFFFFF0u;              // 32-bit buffer offsets, with the out-of-range marker above every operand
    const size_t a_span = (size_t)(d->a_trans ? d->K : d->M) * d->lda * 2, b_span = (size_t)(d->b_trans ? d->N : d->K) * d->ldb * 2;
    DC_REQUIRE((d->a_gather || a_span < lim) && b_span < lim, DC_EINVAL, "dc_gemm_bf16: operands must span < 2 GiB");
    DC_REQUIRE(!d->a_gather || d->a_gather_rows > 0, DC_EINVAL, "dc_gemm_bf16: a_gather needs a_gather_rows (rows of the gathered table)");
    DC_REQUIRE(!d->a_gather || (size_t)d->a_gather_rows * d->lda * 2 < lim, DC_EINVAL, "dc_gemm_bf16: gathered table must span < 2 GiB");
    return DC_OK;
}

static Epilogue bgemm_epilogue(const dc_gemm_bf16_desc* d) {
    Epilogue ep{d->C, d->ldc, d->scale, d->shift, d->residual, d->ldr, d->residual ? (d->res_rows > 0 ? 3 : 1) : 0, d->res_rows, 0, d->relu,
                d->accumulate, 0};
    ep.Cb = d->Cb;
    ep.ldcb = d->ldcb;
    ep.vec4 = (d->N & 3) == 0 && (!d->C || ((d->ldc & 3) == 0 && aligned16(d->C))) && (!d->Cb || ((d->ldcb & 3) == 0 && (reinterpret_cast<uintptr_t>(d->Cb) & 7u) == 0)) &&
              (!d->residual || ((d->ldr & 3) == 0 && aligned16(d->residual))) && (!d->scale || aligned16(d->scale)) && (!d->shift || aligned16(d->shift));
    return ep;
}

static void bgemm_operands(const dc_gemm_bf16_desc* d, BOperand& a, BOperand& b) {
    const size_t a_rows = d->a_gather ? (size_t)d->a_gather_rows : (size_t)(d->a_trans ? d->K : d->M);
    a = BOperand{d->A, d->lda, d->M, d->a_gather, (unsigned)(a_rows * d->lda * 2)};
    b = BOperand{d->B, d->ldb, d->N, nullptr, (unsigned)((size_t)(d->b_trans ? d->N : d->K) * d->ldb * 2)};
}

__global__ __launch_bounds__(256) void cast_bf16_kernel(const float* __restrict__ x, unsigned short* __restrict__ out, size_t n) {
    typedef unsigned short us4 __attribute__((ext_vector_type(4)));
    const size_t n4 = n >> 2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        reinterpret_cast<us4*>(out)[i] = us4{Epilogue::bf16_bits(v.x), Epilogue::bf16_bits(v.y), Epilogue::bf16_bits(v.z), Epilogue::bf16_bits(v.w)};
    }
    for (size_t i = (n4 << 2) + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = Epilogue::bf16_bits(x[i]);
}

// bf16 -> fp32 (exact): the gradient bucket after a bf16 all-reduce, back where the clip norm and the optimizer read it
__global__ __launch_bounds__(256) void uncast_bf16_kernel(const unsigned short* __restrict__ x, float* __restrict__ out, size_t n) {
    typedef unsigned short us4 __attribute__((ext_vector_type(4)));
    auto f = [](unsigned short b) { return __builtin_bit_cast(float, (unsigned)b << 16); };
    const size_t n4 = n >> 2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const us4 v = reinterpret_cast<const us4*>(x)[i];
        reinterpret_cast<float4*>(out)[i] = make_float4(f(v[0]), f(v[1]), f(v[2]), f(v[3]));
    }
    for (size_t i = (n4 << 2) + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = f(x[i]);
}

// rows x cols fp32 (row stride ld_in) -> bf16 (row stride ld_out), columns cols..cols_out-1 zero-filled (K padding)
__global__ __launch_bounds__(256) void cast_bf16_2d_kernel(const float* __restrict__ x, long ld_in, unsigned short* __restrict__ out, long ld_out,
                                                           int rows, int cols, int cols_out) {
    const long total = (long)rows * cols_out;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int r = (int)(idx / cols_out), c = (int)(idx - (long)r * cols_out);
        out[(long)r * ld_out + c] = c < cols ? Epilogue::bf16_bits(x[(long)r * ld_in + c]) : (unsigned short)0;
    }
}

}  // namespace dcap

using namespace dcap;

// the 256-square kernel (bgemm256_core.h) where its grid fills the chip; the K-major gather (embedding-side weight gradient) stays
// on the 128-square loop
static BPlan bgemm_plan(const dc_gemm_bf16_desc* d) {
    const bool big = !(d->a_gather && d->a_trans) && b256::prefer(d->M, d->N, d->K, d->split_k, bgemm_epilogue(d).vec4 != 0);
    return b256::plan(big, d->M, d->N, d->K, d->split_k);
}

extern "C" size_t dc_gemm_bf16_workspace_bytes(const dc_gemm_bf16_desc* d) {
    if (!d || d->M <= 0 || d->N <= 0 || d->K <= 0) return 0;
    return bgemm_plan(d).workspace_bytes(d->M, d->N);
}

extern "C" int dc_gemm_bf16_tile(const dc_gemm_bf16_desc* d, int* split_k) {
    if (!d || d->M <= 0 || d->N <= 0 || d->K <= 0) return 0;
    const BPlan p = bgemm_plan(d);
    if (split_k) *split_k = p.sp.split;
    return p.tile;
}

template <bool AKC, bool BKC>
static int bgemm_launch(const dc_gemm_bf16_desc* d, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const BPlan p = bgemm_plan(d);
    const Epilogue ep = bgemm_epilogue(d);
    BOperand a, b;
    bgemm_operands(d, a, b);
    if (p.tile == 256)
        return bgemm_run<b256::Geo, &b256::bgemm256_kernel<AKC, BKC>>("bgemm256 split-K", "bgemm256_kernel", a, b, ep, d->M, d->N, d->K, p.sp, workspace,
                                                                      workspace_bytes, s);
    return bgemm_run<BGeo128, &bgemm_kernel<AKC, BKC>>("bgemm split-K", "bgemm_kernel", a, b, ep, d->M, d->N, d->K, p.sp, workspace, workspace_bytes, s);
}

extern "C" int dc_gemm_bf16(const dc_gemm_bf16_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = bgemm_validate(d);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!d->a_trans && !d->b_trans) return bgemm_launch<true, false>(d, workspace, workspace_bytes, s);
    if (!d->a_trans && d->b_trans) return bgemm_launch<true, true>(d, workspace, workspace_bytes, s);
    if (d->a_trans && !d->b_trans) return bgemm_launch<false, false>(d, workspace, workspace_bytes, s);
    return bgemm_launch<false, true>(d, workspace, workspace_bytes, s);
}

static int wgrad_bf16_validate(const dc_conv_wgrad_bf16_desc* d) {
    DC_REQUIRE(d && d->x && d->dy && d->dw, DC_EINVAL, "dc_conv2d_wgrad_bf16: x, dy and dw must be non-null");
    DC_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Ho > 0 && d->Wo > 0 && d->kh >= 1 && d->kw >= 1 && d->stride >= 1, DC_EINVAL,
               "dc_conv2d_wgrad_bf16: bad shape");
    DC_REQUIRE(d->Cin % 128 == 0 && d->Cout % 8 == 0, DC_EINVAL,
               "dc_conv2d_wgrad_bf16: needs Cin %% 128 == 0 (a 128-column tile inside one tap) and Cout %% 8 == 0");
    DC_REQUIRE(aligned16(d->x) && aligned16(d->dy) && aligned16(d->dw), DC_EALIGN, "dc_conv2d_wgrad_bf16: pointers must be 16-byte aligned");
    DC_REQUIRE((size_t)d->N * d->H * d->W * d->Cin * 2 < (size_t)0x7FFFFFF0u && (size_t)d->N * d->Ho * d->Wo * d->Cout * 2 < (size_t)0x7FFFFFF0u,
               DC_EINVAL, "dc_conv2d_wgrad_bf16: x and dy must span < 2 GiB");
    return DC_OK;
}

static BPlan wgrad_plan(const dc_conv_wgrad_bf16_desc* d) {
    const int M = d->Cout, N = d->kh * d->kw * d->Cin, K = d->N * d->Ho * d->Wo;
    const bool big = (d->Cout & 7) == 0 && b256::prefer(M, N, K, d->split_k, true);
    return b256::plan(big, M, N, K, d->split_k);
}

extern "C" size_t dc_conv2d_wgrad_bf16_workspace_bytes(const dc_conv_wgrad_bf16_desc* d) {
    if (!d || wgrad_bf16_validate(d)) return 0;
    return wgrad_plan(d).workspace_bytes(d->Cout, d->kh * d->kw * d->Cin);
}

extern "C" int dc_conv2d_wgrad_bf16_tile(const dc_conv_wgrad_bf16_desc* d, int* split_k) {
    if (!d || wgrad_bf16_validate(d)) return 0;
    const BPlan p = wgrad_plan(d);
    if (split_k) *split_k = p.sp.split;
    return p.tile;
}

extern "C" int dc_conv2d_wgrad_bf16(const dc_conv_wgrad_bf16_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = wgrad_bf16_validate(d);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int M = d->Cout, N = d->kh * d->kw * d->Cin, K = d->N * d->Ho * d->Wo;
    const BPlan p = wgrad_plan(d);
    const Epilogue ep{d->dw, N, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, d->accumulate, 1};   // vec4: dw rows are k*k*Cin floats (Cin % 128 == 0), 16-byte aligned base
    const BOperand dy{d->dy, d->Cout, M, nullptr, (unsigned)((size_t)K * d->Cout * 2)};
    const BIm2col xc{d->x, d->H, d->W, d->Cin, d->Ho, d->Wo, d->stride, d->pad_t, d->pad_l, d->kw, K, (unsigned)((size_t)d->N * d->H * d->W * d->Cin * 2), N};
    const char* who = "dc_conv2d_wgrad_bf16 split-K";
    if (p.tile == 256) return bgemm_run<b256::Geo, &bgemm256_wgrad_kernel>(who, "bgemm256_wgrad_kernel", dy, xc, ep, M, N, K, p.sp, workspace, workspace_bytes, s);
    return bgemm_run<BGeo128, &bgemm_wgrad_kernel>(who, "bgemm_wgrad_kernel", dy, xc, ep, M, N, K, p.sp, workspace, workspace_bytes, s);
}

extern "C" int dc_cast_f32_bf16(const float* x, uint16_t* out, size_t n, void* stream) {
    DC_REQUIRE(x && out && n > 0, DC_EINVAL, "dc_cast_f32_bf16: bad arguments");
    DC_REQUIRE(aligned16(x) && (reinterpret_cast<uintptr_t>(out) & 7u) == 0, DC_EALIGN, "dc_cast_f32_bf16: x 16-byte, out 8-byte aligned");
    const int blocks = (int)std::min<size_t>((n / 4 + 255) / 256 + 1, (size_t)kNumCU * 8);
    hipLaunchKernelGGL(cast_bf16_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), x, out, n);
    return check_launch("cast_bf16_kernel");
}

extern "C" int dc_cast_bf16_f32(const uint16_t* x, float* out, size_t n, void* stream) {
    DC_REQUIRE(x && out && n > 0, DC_EINVAL, "dc_cast_bf16_f32: bad arguments");
    DC_REQUIRE(aligned16(out) && (reinterpret_cast<uintptr_t>(x) & 7u) == 0, DC_EALIGN, "dc_cast_bf16_f32: out 16-byte, x 8-byte aligned");
    const int blocks = (int)std::min<size_t>((n / 4 + 255) / 256 + 1, (size_t)kNumCU * 8);
    hipLaunchKernelGGL(uncast_bf16_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), x, out, n);
    return check_launch("uncast_bf16_kernel");
}

extern "C" int dc_cast_f32_bf16_2d(const float* x, int ld_in, uint16_t* out, int ld_out, int rows, int cols, int cols_out, void* stream) {
    DC_REQUIRE(x && out && rows > 0 && cols > 0 && cols_out >= cols && ld_in >= cols && ld_out >= cols_out, DC_EINVAL, "dc_cast_f32_bf16_2d: bad arguments");
    const long total = (long)rows * cols_out;
    const int blocks = (int)std::min<long>((total + 255) / 256, (long)kNumCU * 8);
    hipLaunchKernelGGL(cast_bf16_2d_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), x, (long)ld_in, out, (long)ld_out, rows, cols, cols_out);
    return check_launch("cast_bf16_2d_kernel");
}

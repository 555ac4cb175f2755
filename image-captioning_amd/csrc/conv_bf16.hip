// conv_bf16.hip -- conv2d forward (and, on rotated weights, the data gradient) with bf16 STORAGE: bf16 NHWC activations and bf16
// packed weights in HBM, fp32 accumulation, fp32 and / or bf16 output.  BASELINE configs[4] ("bf16").
//
// The implicit GEMM  y[pixel][cout] = sum_k im2col(x)[pixel][k] * w[cout][k],  k = (tap, ci),  runs on the bf16 GEMM main loop
// (bgemm_core.h: 128 x 128 x 64 tiles, LDS-DMA staging, v_mfma_f32_32x32x16_bf16).  A K-tile is 64 channels of ONE tap
// (Cin % 64 == 0), so the A-operand tile is, for each of the 128 output pixels of the block, a contiguous 128-byte run of the
// shifted input pixel: each lane's 16-byte LDS-DMA piece is addressed as  pixel base + tap offset  and taps that fall into the
// padding load hardware zeros (the lane's offset is replaced by an out-of-range one).  No im2col buffer, no staging
// registers, no conversion: the split-bf16 loop this replaces (igemm_bf16s.h with one product) loaded fp32, rounded on the
// way to LDS and synchronised every 32 k -- 250 TFLOP/s on the joint model's layers.
#include "bgemm64_core.h"
#include <algorithm>
#include <cstdlib>

namespace dcap {

struct BConvA {
    const unsigned short* x;       // bf16 [N, H, W, Cin]
    int H, W, Cin, Ho, Wo, stride, pad_t, pad_l, kw, M;      // M = N*Ho*Wo output pixels
    unsigned bytes;
};

// The A operand on any of the three tiles (geometry G: bgemm_core.h).  (ky, kx, c0) is the (tap, channel chunk) of the NEXT K-tile:
// derived once from kbeg, then advanced by an add and two compares after the last half of each K-tile -- the main loops issue every
// (K-tile, half) exactly once and in order, 64 channels at a time, so k0 serves only the k0 < kend test.  The empty K-tiles that
// b64::mainloop and b256::mainloop issue past the end advance the walk too; nothing live is loaded after them.
template <class G>
struct BLoadConvA {
    static constexpr bool KC = true;
    __amdgpu_buffer_rsrc_t rsrc;
    BConvA c;
    unsigned base[G::HALVES][G::NP];               // [half][piece]: byte offset of (image n, row 0, col 0, this lane's channel chunk)
    int iy0[G::HALVES][G::NP], ix0[G::HALVES][G::NP];   // input row / column of tap (0, 0) for this lane's output pixel
    int ky, kx, c0;
    __device__ __forceinline__ void init(const BConvA& cc, int m0, int lane, int wave, int kbeg) {
        c = cc;
        const int tap = kbeg / c.Cin;                                      // block-uniform; k = tap * Cin + channel
        ky = tap / c.kw;
        kx = tap - ky * c.kw;
        c0 = kbeg - tap * c.Cin;
        rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(c.x), 0, (int)c.bytes, 0x00020000);
#pragma unroll
        for (int u = 0; u < G::HALVES; ++u)
#pragma unroll
            for (int j = 0; j < G::NP; ++j) {
                const int r = 8 * (wave * G::NP + j) + (lane >> 3);        // sub-image row (output pixel) of this lane's chunk
                const int ch = (lane & 7) ^ ((r >> 1) & 7);                // source chunk that lands in LDS chunk (lane & 7)
                const int p = min(m0 + G::template tile_index<true>(u, r), c.M - 1);   // pixels past the end feed rows that are never stored
                const int n = p / (c.Ho * c.Wo), rem = p - n * (c.Ho * c.Wo);
                const int oy = rem / c.Wo, ox = rem - oy * c.Wo;
                iy0[u][j] = oy * c.stride - c.pad_t;
                ix0[u][j] = ox * c.stride - c.pad_l;
                base[u][j] = (unsigned)(((long)n * c.H * c.W * c.Cin + 8 * ch) * 2);
            }
    }
    __device__ __forceinline__ void issue(int u, char* img, int k0, int kend, int wave) {
        const bool live = k0 < kend;
        const int tapoff = ((ky * c.W + kx) * c.Cin + c0) * 2;             // block-uniform
#pragma unroll
        for (int j = 0; j < G::NP; ++j) {
            const int iy = iy0[u][j] + ky, ix = ix0[u][j] + kx;
            const bool in = live && (unsigned)iy < (unsigned)c.H && (unsigned)ix < (unsigned)c.W;
            const unsigned off = base[u][j] + (unsigned)((iy0[u][j] * c.W + ix0[u][j]) * c.Cin * 2);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (DC_LDS void*)(img + (wave * G::NP + j) * 1024), 16, (int)(in ? off + (unsigned)tapoff : kOobOffset), 0, 0, 0);
        }
        if (u == G::HALVES - 1) {
            c0 += G::BK;
            if (c0 >= c.Cin) {
                c0 = 0;
                if (++kx >= c.kw) { kx = 0; ++ky; }
            }
        }
    }
};

__global__ __launch_bounds__(256, 2) void bconv_kernel(BConvA a, BOperand b, Epilogue ep, int M, int N, int K, int klen,
                                                       float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    char* smem = reinterpret_cast<char*>(smem_f);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int m0, n0;
    BGeo128::origin(M, N, m0, n0);
    const int kbeg = blockIdx.z * klen, kend = min(K, kbeg + klen);
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    BLoadConvA<BGeo128> la;
    BLoadDense<BGeo128, true, false> lb;
    la.init(a, m0, lane, wave, kbeg);
    lb.init(b, n0, lane, wave, kbeg);
    f32x16 acc[2][2];
    bgemm_mainloop_t(la, lb, smem, kbeg, kend, acc, wm, wn);
    store_tile<BT, BT>(acc, smem_f, ep, partial, M, N, m0, n0, wm, wn);
}

// The 256 x 256 tile (bgemm256_core.h)
__global__ __launch_bounds__(b256::NTHREADS, 2) void bconv256_kernel(BConvA a, BOperand b, Epilogue ep, int M, int N, int K, int klen, float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int m0, n0;
    b256::Geo::origin(M, N, m0, n0);
    const int kbeg = blockIdx.z * klen, kend = min(K, kbeg + klen);
    BLoadConvA<b256::Geo> la;
    BLoadDense<b256::Geo, true, false> lb;
    la.init(a, m0, lane, wave, kbeg);
    lb.init(b, n0, lane, wave, kbeg);
    b256::f32x4 acc[8][4];
    b256::mainloop(la, lb, reinterpret_cast<char*>(smem_f), kbeg, kend, acc);
    b256::store_tile(acc, ep, partial, M, N, m0, n0);
}

// ... and the 64 x 64 tile (bgemm64_core.h): the whole K loop in one block
__global__ __launch_bounds__(b64::NTHREADS, 2) void bconv64_kernel(BConvA a, BOperand b, Epilogue ep, int M, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int m0, n0;
    b64::Geo::origin(M, N, m0, n0);
    BLoadConvA<b64::Geo> la;
    BLoadDense<b64::Geo, true, false> lb;
    la.init(a, m0, lane, wave, 0);
    lb.init(b, n0, lane, wave, 0);
    b64::f32x4 acc[2][2];
    b64::mainloop(la, lb, reinterpret_cast<char*>(smem_f), 0, K, acc);
    b64::store_tile(acc, ep, M, N, m0, n0);
}

static int conv_bf16_validate(const dc_conv_bf16_desc* d) {
    DC_REQUIRE(d && d->x && d->w && (d->y || d->y_bf16), DC_EINVAL, "dc_conv2d_bf16: x, w and at least one of y / y_bf16 must be non-null");
    DC_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Ho > 0 && d->Wo > 0 && d->kh >= 1 && d->kw >= 1 && d->stride >= 1 && d->Cout > 0, DC_EINVAL,
               "dc_conv2d_bf16: bad shape");
    DC_REQUIRE(d->Cin % BKB == 0, DC_EINVAL, "dc_conv2d_bf16: Cin %% 64 == 0 required (a K-tile is 64 channels of one tap), got %d", d->Cin);
    DC_REQUIRE(d->res_mode >= 0 && d->res_mode <= 2 && (d->res_mode == 0) == (d->residual == nullptr), DC_EINVAL, "dc_conv2d_bf16: residual / res_mode mismatch");
    DC_REQUIRE(d->res_mode != 2 || ((d->Ho & 1) == 0 && (d->Wo & 1) == 0), DC_EINVAL, "dc_conv2d_bf16: res_mode 2 needs even Ho, Wo");
    DC_REQUIRE(aligned16(d->x) && aligned16(d->w) && (!d->y || aligned16(d->y)) && (!d->y_bf16 || aligned16(d->y_bf16)), DC_EALIGN,
               "dc_conv2d_bf16: x, w, y, y_bf16 must be 16-byte aligned");
    DC_REQUIRE((size_t)d->N * d->H * d->W * d->Cin * 2 < (size_t)0x7FFFFFF0u && (size_t)d->Cout * d->kh * d->kw * d->Cin * 2 < (size_t)0x7FFFFFF0u, DC_EINVAL,
               "dc_conv2d_bf16: x and w must span < 2 GiB");
    return DC_OK;
}

// split-K for the convolution: two blocks per CU on the chip, >= 4 K-tiles per slice
static BSplit bconv_split(int M, int N, int K, int user_split) {
    constexpr int target = 2 * kNumCU;
    if (user_split > 0) return bgemm_split(M, N, K, user_split);
    const int tiles = ((M + BT - 1) / BT) * ((N + BT - 1) / BT);
    const int ktiles = (K + BKB - 1) / BKB;
    int s = 1;
    if (tiles < target && ktiles >= 8) {
        s = (target + tiles - 1) / tiles;
        s = std::min(s, std::min(ktiles / 4, 32));
        s = std::max(s, 1);
    }
    const int klen = ((ktiles + s - 1) / s) * BKB;
    return BSplit{(K + klen - 1) / klen, klen};
}

}  // namespace dcap

using namespace dcap;

// Which tile runs this layer: 256 (the P2 / P3-level FPN and RPN layers and their data gradients), 64 (the one-image trunk layers:
// whole K loop in one block, no split-K slabs) or 128, by the cost model of bgemm256_core.h / bgemm64_core.h.
// dc_conv_bf16_desc.tile = 64 | 128 | 256 forces a choice where the shape allows it (tests, benches).
static int bconv_tile(const dc_conv_bf16_desc* d, bool vec4, int M, int N, int K) {
    const int forced = d->tile;
    if (!vec4 || M < 4 || N < 4) return 128;
    if (forced == 128) return 128;
    if (forced == 64 && d->split_k <= 1) return 64;
    if (forced == 256) return ((long)((M + 255) / 256) * ((N + 255) / 256) * 65536 <= 4L * M * N) ? 256 : 128;     // (not for slivers of a tile)
    const bool can256 = (double)((M + 255) / 256) * ((N + 255) / 256) * 65536.0 <= 1.25 * (double)M * N;
    const double c256 = can256 ? b256::tile_cost_us(M, N, K, 256, b256::split(M, N, K, d->split_k)) : 1e30;
    const double c128 = b256::tile_cost_us(M, N, K, 128, bconv_split(M, N, K, d->split_k));
    const double c64 = d->split_k > 1 ? 1e30 : b64::cost_us(M, N, K);           // (a caller that asks for slabs gets a split-K tile)
    return (c256 <= c128 && c256 <= c64) ? 256 : (c64 < c128 ? 64 : 128);
}

struct BConvPlan : BPlan {
    int M, N, K;                   // the implicit GEMM
    bool vec4;                     // 16-byte epilogue accesses are possible (Epilogue::vec4)
};
static BConvPlan bconv_plan(const dc_conv_bf16_desc* d) {
    const int M = d->N * d->Ho * d->Wo, N = d->Cout, K = d->kh * d->kw * d->Cin;
    const bool vec4 = (d->Cout & 3) == 0 && (!d->residual || aligned16(d->residual)) && (!d->scale || aligned16(d->scale)) && (!d->shift || aligned16(d->shift));
    const int tile = bconv_tile(d, vec4, M, N, K);
    const BSplit sp = tile == 256 ? b256::split(M, N, K, d->split_k) : tile == 64 ? BSplit{1, ((K + BKB - 1) / BKB) * BKB} : bconv_split(M, N, K, d->split_k);
    return BConvPlan{{tile, sp}, M, N, K, vec4};
}

extern "C" size_t dc_conv2d_bf16_workspace_bytes(const dc_conv_bf16_desc* d) {
    if (!d || conv_bf16_validate(d)) return 0;
    const BConvPlan p = bconv_plan(d);
    return p.workspace_bytes(p.M, p.N);
}

extern "C" int dc_conv2d_bf16_tile(const dc_conv_bf16_desc* d, int* split_k) {
    if (!d || conv_bf16_validate(d)) return 0;
    const BConvPlan p = bconv_plan(d);
    if (split_k) *split_k = p.sp.split;
    return p.tile;
}

extern "C" int dc_conv2d_bf16(const dc_conv_bf16_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = conv_bf16_validate(d);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const BConvPlan p = bconv_plan(d);
    const int M = p.M, N = p.N, K = p.K;
    Epilogue ep{d->y, d->Cout, d->scale, d->shift, d->residual, d->Cout, d->res_mode, d->Ho, d->Wo, d->relu, 0, p.vec4};
    ep.Cb = d->y_bf16;
    ep.ldcb = d->Cout;
    const BConvA a{d->x, d->H, d->W, d->Cin, d->Ho, d->Wo, d->stride, d->pad_t, d->pad_l, d->kw, M, (unsigned)((size_t)d->N * d->H * d->W * d->Cin * 2)};
    const BOperand b{d->w, K, N, nullptr, (unsigned)((size_t)N * K * 2)};
    const char* who = "dc_conv2d_bf16 split-K";
    if (p.tile == 256) return bgemm_run<b256::Geo, &bconv256_kernel>(who, "bconv256_kernel", a, b, ep, M, N, K, p.sp, workspace, workspace_bytes, s);
    if (p.tile == 128) return bgemm_run<BGeo128, &bconv_kernel>(who, "bconv_kernel", a, b, ep, M, N, K, p.sp, workspace, workspace_bytes, s);
    DC_ENSURE_DYN_LDS(&bconv64_kernel, 160 * 1024);
    const int tiles = ((M + b64::BM - 1) / b64::BM) * ((N + b64::BN - 1) / b64::BN);
    hipLaunchKernelGGL(bconv64_kernel, dim3(tiles), dim3(b64::NTHREADS), b64::LDS_BYTES, s, a, b, ep, M, N, K);
    return check_launch("bconv64_kernel");
}

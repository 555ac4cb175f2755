// vocab_top1.hip -- dc_vocab_top1_f32: the vocabulary projection FUSED with the row top-1 (greedy decoding).
//
// Replaces, per decoded token, Dense(V, activation='softmax') + tf.argmax + the chosen word's probability of the reference's
// ROICaptionInferenceLayer (dense_img_cap_separate_models/text_generation_model.py:192-232; dense_img_cap/dense_model.py:820):
// the [M, V] logits are never written.  The fp32 MFMA main loop of dc_vocab_ce (igemm_core.h, 128 x 128 tiles) runs ONCE over
// the output tiles and each tile ends in a reduction epilogue while it sits in LDS: per (row, column tile) the largest logit, its
// column (lowest index on ties) and the sum of exp(z - max) over the tile -- wavefront shuffles over the 32 lanes that share a
// row.  A second launch, one wave per row, combines the tiles in a fixed order (tile j's partials always meet in the same lane and
// the same shuffle tree, whatever M is): id = the argmax, p = 1 / sum_v exp(z_v - max z) = the softmax probability of that word.
// No persistent grid, no cross-block spin: an ordinary grid plus one combine launch.
#include "igemm_core.h"
#include <algorithm>
#include <climits>

namespace dcap {

constexpr int T1_ST = 4;                 // floats of per-(row, column tile) partials: max, sum exp, argmax (int bits), -

struct Top1Args {
    int M, V, tiles_m, tiles_n;
    const float* bias;                   // [V] or null
    float* stats;                        // [M][tiles_n][T1_ST]
};

// (value, column) pair order of the row maximum: the larger value wins, the lower column on equal values.  -inf / NaN columns
// never win against a finite logit (NaN compares false both ways).
__device__ __forceinline__ void top1_take(float& m, int& i, float om, int oi) {
    if (om > m || (om == m && oi < i)) { m = om; i = oi; }
}

__device__ __forceinline__ void top1_epilogue(f32x16 (&acc)[2][2], float* Cs, const Top1Args& ta, int m0, int n0, int wm, int wn, int tile_n) {
    constexpr int LDC = 128 + 4;
    const int tid = threadIdx.x, lane = tid & 63;
    {
        const int i = lane & 31, h = lane >> 5;
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int r = 0; r < 16; ++r) Cs[(wm + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * LDC + wn + tn * 32 + i] = acc[tm][tn][r];
    }
    __syncthreads();
    const int c4 = tid & 31, rp = tid >> 5;                    // 32 lanes x 4 columns per row, 8 rows per pass
    const int col = n0 + 4 * c4;
    float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ta.bias && col + 3 < ta.V) b4 = *reinterpret_cast<const float4*>(ta.bias + col);
    else if (ta.bias) {
        if (col < ta.V) b4.x = ta.bias[col];
        if (col + 1 < ta.V) b4.y = ta.bias[col + 1];
        if (col + 2 < ta.V) b4.z = ta.bias[col + 2];
    }
    const bool v0 = col < ta.V, v1 = col + 1 < ta.V, v2 = col + 2 < ta.V, v3 = col + 3 < ta.V;
#pragma unroll 2
    for (int p = 0; p < 16; ++p) {
        const int lr = p * 8 + rp, row = m0 + lr;
        float4 z = *reinterpret_cast<const float4*>(&Cs[lr * LDC + 4 * c4]);
        z.x += b4.x; z.y += b4.y; z.z += b4.z; z.w += b4.w;
        float mx = -INFINITY;
        int ix = INT_MAX;
        if (v0) top1_take(mx, ix, z.x, col);
        if (v1) top1_take(mx, ix, z.y, col + 1);
        if (v2) top1_take(mx, ix, z.z, col + 2);
        if (v3) top1_take(mx, ix, z.w, col + 3);
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            const float om = __shfl_xor(mx, o, 64);
            const int oi = __shfl_xor(ix, o, 64);
            top1_take(mx, ix, om, oi);
        }
        float s = (v0 ? expf(z.x - mx) : 0.f) + (v1 ? expf(z.y - mx) : 0.f) + (v2 ? expf(z.z - mx) : 0.f) + (v3 ? expf(z.w - mx) : 0.f);
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (row < ta.M && c4 == 0)
            *reinterpret_cast<float4*>(ta.stats + ((long)row * ta.tiles_n + tile_n) * T1_ST) = make_float4(mx, s, __int_as_float(ix), 0.f);
    }
}

using T1A = DenseKCT<true>;
using T1B = DenseMCT<true>;

// Row tiles fastest: the tiles_m blocks that share a column panel of W run side by side, so W streams from HBM about once.
__global__ __launch_bounds__(256, 2) void vocab_top1_f32_kernel(T1A al, T1B bl, Top1Args ta, int K) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_m = lid % ta.tiles_m, tile_n = lid / ta.tiles_m;
    const int m0 = tile_m * 128, n0 = tile_n * 128;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    f32x16 acc[2][2];
    igemm_mainloop<128, 128, T1A, T1B>(al, bl, smem, m0, n0, 0, K, acc, wm, wn);
    top1_epilogue(acc, smem, ta, m0, n0, wm, wn, tile_n);
}

// One wave per row: m = max_j m_j; id = the lowest column among the tiles that reach m (tile j holds columns 128 j ..: the lowest
// such tile's own argmax); s = sum_j s_j exp(m_j - m) (lane-strided over j, then a fixed xor tree); p = 1 / s.
__global__ __launch_bounds__(256) void vocab_top1_rows_kernel(int M, int tiles_n, const float* __restrict__ stats, int32_t* __restrict__ tokens,
                                                              int32_t* __restrict__ ids, long ld_ids, float* __restrict__ probs, long ld_probs,
                                                              uint8_t* __restrict__ mask) {
    const int row = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (row >= M) return;
    const float4* st = reinterpret_cast<const float4*>(stats) + (long)row * tiles_n;
    float m = -INFINITY;
    for (int j = lane; j < tiles_n; j += 64) m = fmaxf(m, st[j].x);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float s = 0.f;
    int id = INT_MAX;
    for (int j = lane; j < tiles_n; j += 64) {
        const float4 q = st[j];
        s += q.y * expf(q.x - m);
        if (q.x == m) id = min(id, __float_as_int(q.z));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); id = min(id, __shfl_xor(id, o, 64)); }
    if (lane != 0) return;
    if (id == INT_MAX) id = 0;                                 // (a row without a finite logit: tf.argmax's first column)
    tokens[row] = id;
    if (ids) ids[row * ld_ids] = id;
    if (probs) probs[row * ld_probs] = 1.f / s;
    if (mask) mask[row] = id != 0 ? 1 : 0;
}

static size_t t1_align256(size_t x) { return (x + 255) & ~(size_t)255; }

static int top1_validate(const dc_vocab_top1_desc* d) {
    DC_REQUIRE(d != nullptr, DC_EINVAL, "dc_vocab_top1: null descriptor");
    DC_REQUIRE(d->M > 0 && d->V > 0 && d->K > 0 && d->X && d->W && d->tokens, DC_EINVAL, "dc_vocab_top1: bad arguments");
    DC_REQUIRE((d->K & 31) == 0 && (d->ldx & 3) == 0 && (d->ldw & 3) == 0, DC_EALIGN,
               "dc_vocab_top1: K must be a multiple of 32 and ldx, ldw multiples of 4");
    DC_REQUIRE(d->ldx >= d->K && d->ldw >= (d->V + 3) / 4 * 4, DC_EINVAL, "dc_vocab_top1: ldx < K or ldw < V rounded up to 4");
    DC_REQUIRE(aligned16(d->X) && aligned16(d->W) && (!d->bias || aligned16(d->bias)), DC_EALIGN, "dc_vocab_top1: X, W, bias must be 16-byte aligned");
    DC_REQUIRE((size_t)d->M * d->ldx * 4 < (size_t)0xFFFFFFF0u && (size_t)d->K * d->ldw * 4 < (size_t)0xFFFFFFF0u, DC_EINVAL,
               "dc_vocab_top1: operands must span < 4 GiB");
    DC_REQUIRE((!d->ids || d->ld_ids >= 1) && (!d->probs || d->ld_probs >= 1), DC_EINVAL, "dc_vocab_top1: ld_ids / ld_probs must be >= 1");
    return DC_OK;
}

}  // namespace dcap

using namespace dcap;

extern "C" size_t dc_vocab_top1_workspace_bytes(int M, int V) {
    if (M <= 0 || V <= 0) return 0;
    return t1_align256((size_t)M * ((V + 127) / 128) * T1_ST * sizeof(float));
}

extern "C" int dc_vocab_top1_f32(const dc_vocab_top1_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = top1_validate(d);
    if (rc) return rc;
    const size_t need = dc_vocab_top1_workspace_bytes(d->M, d->V);
    DC_REQUIRE(workspace && workspace_bytes >= need, DC_EWORKSPACE, "dc_vocab_top1: needs %zu workspace bytes, got %zu", need, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Top1Args ta{};
    ta.M = d->M; ta.V = d->V;
    ta.tiles_m = (d->M + 127) / 128;
    ta.tiles_n = (d->V + 127) / 128;
    ta.bias = d->bias;
    ta.stats = static_cast<float*>(workspace);
    // the B loader reads whole 16-byte column quads: the columns V .. round4(V) - 1 it then also reads lie inside the row (ldw >= round4(V))
    // and feed only the tile's guarded-off lanes
    T1A al{d->X, d->ldx, d->M, nullptr};
    T1B bl{d->W, d->ldw, (d->V + 3) / 4 * 4, nullptr};
    DC_ENSURE_DYN_LDS((&vocab_top1_f32_kernel), 160 * 1024);
    constexpr size_t lds = igemm_lds_bytes<128, 128, T1A, T1B>();
    hipLaunchKernelGGL(vocab_top1_f32_kernel, dim3(ta.tiles_m * ta.tiles_n), dim3(256), lds, s, al, bl, ta, d->K);
    rc = check_launch("vocab_top1_f32_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(vocab_top1_rows_kernel, dim3((d->M + 3) / 4), dim3(256), 0, s, d->M, ta.tiles_n, ta.stats, d->tokens, d->ids,
                       (long)d->ld_ids, d->probs, (long)d->ld_probs, d->mask);
    return check_launch("vocab_top1_rows_kernel");
}

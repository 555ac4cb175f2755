// vocab_topk.hip -- greedy and beam-search decoding on the device:
//   dc_vocab_top1_f32   the vocabulary projection FUSED with the row top-1 (greedy decoding): the next token, its softmax probability
//                       and the mask byte;
//   dc_vocab_topk_f32   the vocabulary projection FUSED with the row top-k (k <= 8) and the softmax probabilities of those k words;
//   dc_vocab_top1_bf16 / dc_vocab_topk_bf16   the same contract on bf16 operands and the bf16 matrix pipe (the arithmetic a bf16 model
//                       trains its vocabulary layer in: dc_vocab_ce's bf16 branch), on one of two tiles.  128 x 128 (bgemm_core.h): the
//                       main loop leaves the fp32 loop's accumulator layout, so the tile ends in the SAME epilogue.  256 x 256
//                       (bgemm256_core.h): the 128 accumulator registers of a lane are never transposed through LDS; every wave
//                       reduces its own 64-column slice in registers and writes its own cells (ceil(V/64) cells per row instead of
//                       ceil(V/128); no cross-wave combine, no barrier after the main loop), and the row kernel, generic over the
//                       number of cells per row, combines them unchanged.
//   dc_vocab_sample_f32 / dc_vocab_sample_bf16   the vocabulary projection FUSED with one draw per row from softmax(z / t) (stochastic
//                       decoding): the Gumbel-max argmax as one more reduction of the 128 x 128 tile's epilogue, counter-based noise;
//                       with top_k, the top-k tile kernels unchanged and a row kernel that perturbs the k winners;
//   dc_beam_step_f32    per RoI, the k best of the k beams' proposals (score + p or score + log p; a beam that has produced the end
//                       token proposes only itself, with token 0), with the parents' rows of up to four state tensors gathered into
//                       the next state buffers;  dc_beam_select_f32: the same kernel with one (h, c) pair and no end token;
//   dc_beam_backtrace   the [steps,R,k] parent / token history -> [R,k,steps] sequences.
//
// Replaces, per decoded token, Dense(V, activation='softmax') + tf.argmax + the chosen word's probability of the reference's
// ROICaptionInferenceLayer (dense_img_cap_separate_models/text_generation_model.py:192-232; dense_img_cap/dense_model.py:820), and
// the reference's beam loop (image captioning/test.py:23-64: per beam a full model.predict on the pre-padded prefix, a host argsort of
// the [V] probability row, a host sort of the k*k candidates) for the v2 decoders (text_generation_model_v2.py:140-166).
// Both vocabulary entry points run one kernel pair; top-1 is top-k at k = 1.  The fp32 MFMA main loop of dc_vocab_ce (igemm_core.h,
// 128 x 128 tiles, row tiles fastest, xcd_remap) runs ONCE over the output tiles, and each tile ends in a reduction epilogue while it
// sits in LDS: per (row, 128-column tile) the max, the sum of exp(z - max) and the tile's k best (value, column) pairs -- found in k
// threshold rounds of a 32-lane shuffle reduction, each round taking the best pair that comes after the previous round's winner in
// the order (value descending, column ascending), so no per-lane lists are needed.  A row kernel (one wave per row) runs the same
// rounds over the row's tiles_n * k candidates in an order that does not depend on M.  The [M,V] logits are never written.  No
// persistent grid, no cross-block spin: an ordinary grid plus one combine launch.
#include "bgemm256_core.h"
#include <algorithm>
#include <climits>

namespace dcap {

constexpr int TK_MAX = 8;

struct TopkArgs {
    int M, V, tiles_m, tiles_n, k;
    const float* bias;                   // [V] or null
    float2* cells;                       // [M][tiles_n][1 + k]: (max, sum exp), then k (value, column (int bits)); column INT_MAX = none
};

// (v, c) comes strictly after (tv, tc) in the order value descending, column ascending.  NaN never does.
__device__ __forceinline__ bool tk_after(float v, int c, float tv, int tc) {
    return v < tv || (v == tv && c > tc);
}

// the better of two (value, column) pairs: the larger value, the lower column on equal values.  -inf / NaN columns never win against
// a finite logit (NaN compares false both ways).
__device__ __forceinline__ void tk_take(float& m, int& i, float om, int oi) {
    if (om > m || (om == m && oi < i)) { m = om; i = oi; }
}

__device__ __forceinline__ void topk_epilogue(f32x16 (&acc)[2][2], float* Cs, const TopkArgs& ta, int m0, int n0, int wm, int wn, int tile_n) {
    constexpr int LDC = 128 + 4;
    const int tid = threadIdx.x;
    stage_acc_tile<2, 2, LDC>(acc, Cs, wm, wn);
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
    for (int p = 0; p < 16; ++p) {
        const int lr = p * 8 + rp, row = m0 + lr;
        float4 z = *reinterpret_cast<const float4*>(&Cs[lr * LDC + 4 * c4]);
        z.x += b4.x; z.y += b4.y; z.z += b4.z; z.w += b4.w;
        float2* out = ta.cells + ((long)row * ta.tiles_n + tile_n) * (ta.k + 1);
        float tv = INFINITY, mx = -INFINITY;
        int tc = INT_MIN;
        for (int r = 0; r < ta.k; ++r) {                       // round r: the tile's (r+1)-th best pair
            float bm = -INFINITY;
            int bi = INT_MAX;
            if (v0 && tk_after(z.x, col, tv, tc)) tk_take(bm, bi, z.x, col);
            if (v1 && tk_after(z.y, col + 1, tv, tc)) tk_take(bm, bi, z.y, col + 1);
            if (v2 && tk_after(z.z, col + 2, tv, tc)) tk_take(bm, bi, z.z, col + 2);
            if (v3 && tk_after(z.w, col + 3, tv, tc)) tk_take(bm, bi, z.w, col + 3);
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {
                const float om = __shfl_xor(bm, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                tk_take(bm, bi, om, oi);
            }
            if (r == 0) mx = bm;
            if (row < ta.M && c4 == 0) out[1 + r] = make_float2(bm, __int_as_float(bi));
            tv = bm; tc = bi;                                  // (no pair left: (-inf, INT_MAX), after which nothing comes)
        }
        float s = (v0 ? expf(z.x - mx) : 0.f) + (v1 ? expf(z.y - mx) : 0.f) + (v2 ? expf(z.z - mx) : 0.f) + (v3 ? expf(z.w - mx) : 0.f);
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (row < ta.M && c4 == 0) out[0] = make_float2(mx, s);
    }
}

using TKA = DenseKCT<true>;
using TKB = DenseMCT<true>;

// Row tiles fastest: the tiles_m blocks that share a column panel of W run side by side, so W streams from HBM about once.
__global__ __launch_bounds__(256, 2) void vocab_topk_f32_kernel(TKA al, TKB bl, TopkArgs ta, int K) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_m = lid % ta.tiles_m, tile_n = lid / ta.tiles_m;
    const int m0 = tile_m * 128, n0 = tile_n * 128;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    f32x16 acc[2][2];
    igemm_mainloop<128, 128, TKA, TKB>(al, bl, smem, m0, n0, 0, K, acc, wm, wn);
    topk_epilogue(acc, smem, ta, m0, n0, wm, wn, tile_n);
}

__global__ __launch_bounds__(256, 2) void vocab_topk_bf16_kernel(BOperand a, BOperand b, TopkArgs ta, int K) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_m = lid % ta.tiles_m, tile_n = lid / ta.tiles_m;
    const int m0 = tile_m * 128, n0 = tile_n * 128;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    f32x16 acc[2][2];
    bgemm_mainloop<true, false>(a, b, reinterpret_cast<char*>(smem), m0, n0, 0, K, acc, wm, wn);
    topk_epilogue(acc, smem, ta, m0, n0, wm, wn, tile_n);
}

// Epilogue of one 256 x 256 bf16 tile, straight from the accumulators (layout: bgemm256_core.h, mainloop).  Lane l of wave (group,
// wcol) holds, for each of its 8 rows (mt), 16 logits of the wave's 64-column slice: columns 32 (nt >> 1) + 16 (nt & 1) + 4 (l >> 4) + j;
// the lanes l, l ^ 16, l ^ 32, l ^ 48 share a row.  A threshold round is 16 in-lane comparisons and two shuffles; the sum of exp is 16
// in-lane terms in a fixed order and the same two shuffles.  The wave writes cell (row, n0 / 64 + wcol) in the 128-tile's cell format
// (ta.tiles_n = cells per row = ceil(V / 64)); a slice that starts at or past V writes nothing (no cell of that index exists).
__device__ __forceinline__ void topk_epilogue256(b256::f32x4 (&acc)[8][4], const TopkArgs& ta, int m0, int n0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int group = wave >> 2, wcol = wave & 3, i = lane & 15, q = lane >> 4;
    const int c0 = n0 + 64 * wcol;
    if (c0 >= ta.V) return;                                    // wave-uniform; nothing after the main loop synchronises the block
    const int cell = c0 >> 6;
    int col[4];
    float bias[4][4];
    unsigned live = 0;                                         // bit 4 nt + j: the column lies inside V
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        col[nt] = c0 + 32 * (nt >> 1) + 16 * (nt & 1) + 4 * q;
        float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ta.bias && col[nt] + 3 < ta.V) b4 = *reinterpret_cast<const float4*>(ta.bias + col[nt]);
        else if (ta.bias) {
            if (col[nt] < ta.V) b4.x = ta.bias[col[nt]];
            if (col[nt] + 1 < ta.V) b4.y = ta.bias[col[nt] + 1];
            if (col[nt] + 2 < ta.V) b4.z = ta.bias[col[nt] + 2];
        }
        bias[nt][0] = b4.x; bias[nt][1] = b4.y; bias[nt][2] = b4.z; bias[nt][3] = b4.w;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (col[nt] + j < ta.V) live |= 1u << (4 * nt + j);
    }
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
        const int row = m0 + 128 * group + 64 * (mt >> 2) + 16 * (mt & 3) + i;
        const bool wr = row < ta.M && q == 0;
        float2* out = ta.cells + ((long)row * ta.tiles_n + cell) * (ta.k + 1);
        float z[4][4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int j = 0; j < 4; ++j) z[nt][j] = acc[mt][nt][j] + bias[nt][j];
        float tv = INFINITY, mx = -INFINITY;
        int tc = INT_MIN;
        for (int r = 0; r < ta.k; ++r) {                       // round r: the slice's (r+1)-th best pair
            float bm = -INFINITY;
            int bi = INT_MAX;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((live >> (4 * nt + j) & 1u) && tk_after(z[nt][j], col[nt] + j, tv, tc)) tk_take(bm, bi, z[nt][j], col[nt] + j);
#pragma unroll
            for (int o = 16; o <= 32; o <<= 1) {
                const float om = __shfl_xor(bm, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                tk_take(bm, bi, om, oi);
            }
            if (r == 0) mx = bm;
            if (wr) out[1 + r] = make_float2(bm, __int_as_float(bi));
            tv = bm; tc = bi;                                  // (no pair left: (-inf, INT_MAX), after which nothing comes)
        }
        float s = 0.f;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int j = 0; j < 4; ++j) s += (live >> (4 * nt + j) & 1u) ? expf(z[nt][j] - mx) : 0.f;
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (wr) out[0] = make_float2(mx, s);
    }
}

// Tile ids walk down the row tiles of a column panel first (b256::tile_coords), so W streams from HBM about once.
__global__ __launch_bounds__(b256::NTHREADS, 2) void vocab_topk_bf16_256_kernel(BOperand a, BOperand b, TopkArgs ta, int K, int tiles_m, int tiles_n) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int tile_m, tile_n;
    b256::tile_coords(xcd_remap(blockIdx.x, gridDim.x), tiles_m, tiles_n, tile_m, tile_n);
    const int m0 = tile_m * b256::BM, n0 = tile_n * b256::BN;
    BLoadDense<b256::Geo, true, true> la;
    BLoadDense<b256::Geo, false, false> lb;
    la.init(a, m0, lane, wave);
    lb.init(b, n0, lane, wave);
    b256::f32x4 acc[8][4];
    b256::mainloop(la, lb, reinterpret_cast<char*>(smem), 0, K, acc);
    topk_epilogue256(acc, ta, m0, n0);
}

// One wave per row.  k threshold rounds over the tiles_n * k candidates, each a scan strided over the tiles (a lane takes all k
// candidates of its tiles) + a 64-lane xor reduction; lane r keeps round r's winner (z_r, id_r), and round 0's value is the row
// maximum m (every tile's maximum is among its candidates).  Then s = sum_j s_j exp(m_j - m) (lane-strided over j, then a fixed xor
// tree).  The top k of a strict total order does not depend on the scan order, and s is summed in an order fixed by tiles_n alone:
// the result is the same at every M.
// Lane r < k writes ids[row * ld_ids + r] and probs[row * ld_probs + r] = exp(z_r - m) / s (either may be null).  A top-1 call
// (dc_vocab_top1_f32: k = 1, tokens given) also writes tokens[row] and the optional mask[row] = id != 0, and its probability is
// 1 / s: the same value (z_0 = m), and also what it reports for a row without an orderable logit.
__global__ __launch_bounds__(256) void vocab_topk_rows_kernel(int M, int tiles_n, int k, const float2* __restrict__ cells,
                                                              int32_t* __restrict__ ids, long ld_ids,
                                                              float* __restrict__ probs, long ld_probs, int32_t* __restrict__ tokens,
                                                              uint8_t* __restrict__ mask) {
    const int row = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (row >= M) return;
    const float2* cl = cells + (long)row * tiles_n * (k + 1);
    float tv = INFINITY, m = -INFINITY, z = -INFINITY;
    int tc = INT_MIN, id = INT_MAX;
    for (int r = 0; r < k; ++r) {
        float bm = -INFINITY;
        int bi = INT_MAX;
        for (int j = lane; j < tiles_n; j += 64)
            for (int i = 1; i <= k; ++i) {
                const float2 q = cl[j * (k + 1) + i];
                const int c = __float_as_int(q.y);
                if (c != INT_MAX && tk_after(q.x, c, tv, tc)) tk_take(bm, bi, q.x, c);
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float om = __shfl_xor(bm, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            tk_take(bm, bi, om, oi);
        }
        if (r == 0) m = bm;
        if (lane == r) { z = bm; id = bi; }
        tv = bm; tc = bi;                                      // (no pair left: (-inf, INT_MAX), after which nothing comes)
    }
    float s = 0.f;
    for (int j = lane; j < tiles_n; j += 64) {
        const float2 q = cl[j * (k + 1)];
        s += q.y * expf(q.x - m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane >= k) return;
    const bool none = id == INT_MAX;                           // (a row with fewer than k orderable logits: tf.argmax's first column)
    if (none) id = 0;
    if (ids) ids[row * ld_ids + lane] = id;
    if (probs) probs[row * ld_probs + lane] = tokens ? 1.f / s : (none ? 0.f : expf(z - m) / s);
    if (tokens) {
        tokens[row] = id;
        if (mask) mask[row] = id != 0 ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ Gumbel-max sampling
// dc_vocab_sample_f32 / _bf16 (include/dcap.h): the word argmax_v fma(z_v, inv_t, g(row, v)) is an exact draw from softmax(z inv_t).
// The noise g is a pure function of (seed, offset + row, v) -- Philox-2x32-10 on the counter (v >> 1, offset + row), both words kept,
// so a lane's four columns (4 c4 .. 4 c4 + 3) cost two Philox calls -- and nothing else enters it: not M, not the tile, not the grid.
struct SampleArgs {
    TopkArgs t;                          // t.k is unused; t.cells: [M][tiles_n][3]: (max, sum exp), (y, column (int bits)), (z of that column, 0)
    float inv_t;
    unsigned seed, offset;
};

// standard Gumbel noise from 32 random bits: u = ((r >> 9) + 0.5) 2^-23 lies in [2^-24, 1 - 2^-24] and is exact; the accurate logf twice
__device__ __forceinline__ float sm_gumbel(unsigned r) {
    const float u = ((float)(r >> 9) + 0.5f) * 1.1920928955078125e-07f;
    return -logf(-logf(u));
}

__device__ __forceinline__ float sm_noise(unsigned seed, unsigned ctr, int v) {
    const uint2 r = philox2x32_pair((unsigned)v >> 1, ctr, seed);
    return sm_gumbel((v & 1) ? r.y : r.x);
}

// The epilogue of one 128 x 128 tile, topk_epilogue's staging and lane map.  The unperturbed (max, sum exp) of a row are
// topk_epilogue's at k = 1 (the same maximum, the same terms in the same order), so the reported probabilities are the greedy
// decoder's to rounding.  The perturbed pair takes one more 32-lane reduction; the lane that owns the winning column writes its logit.
__device__ __forceinline__ void sample_epilogue(f32x16 (&acc)[2][2], float* Cs, const SampleArgs& sa, int m0, int n0, int wm, int wn, int tile_n) {
    constexpr int LDC = 128 + 4;
    const TopkArgs& ta = sa.t;
    const int tid = threadIdx.x;
    stage_acc_tile<2, 2, LDC>(acc, Cs, wm, wn);
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
    const unsigned pc = (unsigned)col >> 1;                    // Philox counter word 0 of columns col, col + 1; pc + 1: col + 2, col + 3
    for (int p = 0; p < 16; ++p) {
        const int lr = p * 8 + rp, row = m0 + lr;
        float4 z = *reinterpret_cast<const float4*>(&Cs[lr * LDC + 4 * c4]);
        z.x += b4.x; z.y += b4.y; z.z += b4.z; z.w += b4.w;
        float2* out = ta.cells + ((long)row * ta.tiles_n + tile_n) * 3;
        float mx = -INFINITY;
        if (v0 && z.x > mx) mx = z.x;
        if (v1 && z.y > mx) mx = z.y;
        if (v2 && z.z > mx) mx = z.z;
        if (v3 && z.w > mx) mx = z.w;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            const float om = __shfl_xor(mx, o, 64);
            if (om > mx) mx = om;
        }
        float s = (v0 ? expf(z.x - mx) : 0.f) + (v1 ? expf(z.y - mx) : 0.f) + (v2 ? expf(z.z - mx) : 0.f) + (v3 ? expf(z.w - mx) : 0.f);
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        float bm = -INFINITY;
        int bi = INT_MAX;
        if (row < ta.M && v0) {                                // (a lane past V, or a row past M, proposes nothing)
            const unsigned ctr = sa.offset + (unsigned)row;
            const uint2 ra = philox2x32_pair(pc, ctr, sa.seed), rb = philox2x32_pair(pc + 1u, ctr, sa.seed);
            tk_take(bm, bi, fmaf(z.x, sa.inv_t, sm_gumbel(ra.x)), col);
            if (v1) tk_take(bm, bi, fmaf(z.y, sa.inv_t, sm_gumbel(ra.y)), col + 1);
            if (v2) tk_take(bm, bi, fmaf(z.z, sa.inv_t, sm_gumbel(rb.x)), col + 2);
            if (v3) tk_take(bm, bi, fmaf(z.w, sa.inv_t, sm_gumbel(rb.y)), col + 3);
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            const float om = __shfl_xor(bm, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            tk_take(bm, bi, om, oi);
        }
        if (row < ta.M) {
            if (c4 == 0) {
                out[0] = make_float2(mx, s);
                out[1] = make_float2(bm, __int_as_float(bi));
            }
            const unsigned own = (unsigned)(bi - col);         // (no pair: INT_MAX - col >= 4, no lane owns it)
            if (own < 4u) out[2] = make_float2(own == 0 ? z.x : own == 1 ? z.y : own == 2 ? z.z : z.w, 0.f);
        }
    }
}

// The tile loops of vocab_topk_f32_kernel / vocab_topk_bf16_kernel, ending in the sampling epilogue.
__global__ __launch_bounds__(256, 2) void vocab_sample_f32_kernel(TKA al, TKB bl, SampleArgs sa, int K) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_m = lid % sa.t.tiles_m, tile_n = lid / sa.t.tiles_m;
    const int m0 = tile_m * 128, n0 = tile_n * 128;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    f32x16 acc[2][2];
    igemm_mainloop<128, 128, TKA, TKB>(al, bl, smem, m0, n0, 0, K, acc, wm, wn);
    sample_epilogue(acc, smem, sa, m0, n0, wm, wn, tile_n);
}

__global__ __launch_bounds__(256, 2) void vocab_sample_bf16_kernel(BOperand a, BOperand b, SampleArgs sa, int K) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_m = lid % sa.t.tiles_m, tile_n = lid / sa.t.tiles_m;
    const int m0 = tile_m * 128, n0 = tile_n * 128;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    f32x16 acc[2][2];
    bgemm_mainloop<true, false>(a, b, reinterpret_cast<char*>(smem), m0, n0, 0, K, acc, wm, wn);
    sample_epilogue(acc, smem, sa, m0, n0, wm, wn, tile_n);
}

// One wave per row; lane 0 writes.  m and s come from the cells exactly as in vocab_topk_rows_kernel (the maximum of the tile
// maxima; s = sum_j s_j exp(m_j - m), lane-strided over j, then a fixed xor tree), in an order fixed by tiles_n alone.
// k = 0 (whole vocabulary; cells of sample_epilogue): the best of the tiles' perturbed pairs, and the winner's logit from its tile's cell.
// k >= 1 (cells of the top-k tile kernels at that k): vocab_topk_rows_kernel's k threshold rounds leave the row's r-th best (z_r, id_r) in
// lane r; those k lanes perturb their own candidate and a 64-lane reduction takes the best (y, id), its logit carried along.
// probs = exp(z_w - m) / s, 1 / s when z_w == m (the top-1 kernel's value, bit for bit) or when the row has no orderable logit (id 0).
__global__ __launch_bounds__(256) void vocab_sample_rows_kernel(int M, int tiles_n, int k, const float2* __restrict__ cells, float inv_t,
                                                                unsigned seed, unsigned offset, int32_t* __restrict__ ids, long ld_ids,
                                                                float* __restrict__ probs, long ld_probs, int32_t* __restrict__ tokens,
                                                                uint8_t* __restrict__ mask) {
    const int row = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (row >= M) return;
    const int cw = k ? k + 1 : 3;                              // float2 per cell
    const float2* cl = cells + (long)row * tiles_n * cw;
    float m = -INFINITY, z = -INFINITY, by = -INFINITY;
    int id = INT_MAX;
    if (k == 0) {
        for (int j = lane; j < tiles_n; j += 64) {
            const float mj = cl[j * 3].x;
            const float2 q = cl[j * 3 + 1];
            const int c = __float_as_int(q.y);
            if (mj > m) m = mj;
            if (c != INT_MAX) tk_take(by, id, q.x, c);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float om = __shfl_xor(m, o, 64), oy = __shfl_xor(by, o, 64);
            const int oi = __shfl_xor(id, o, 64);
            if (om > m) m = om;
            tk_take(by, id, oy, oi);
        }
        if (id != INT_MAX) z = cl[(id >> 7) * 3 + 2].x;        // the 128-column tile that proposed the winner kept its logit
    } else {
        float tv = INFINITY, zr = -INFINITY;
        int tc = INT_MIN, idr = INT_MAX;
        for (int r = 0; r < k; ++r) {
            float bm = -INFINITY;
            int bi = INT_MAX;
            for (int j = lane; j < tiles_n; j += 64)
                for (int i = 1; i <= k; ++i) {
                    const float2 q = cl[j * (k + 1) + i];
                    const int c = __float_as_int(q.y);
                    if (c != INT_MAX && tk_after(q.x, c, tv, tc)) tk_take(bm, bi, q.x, c);
                }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float om = __shfl_xor(bm, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                tk_take(bm, bi, om, oi);
            }
            if (r == 0) m = bm;
            if (lane == r) { zr = bm; idr = bi; }
            tv = bm; tc = bi;
        }
        if (idr != INT_MAX) {                                  // (lanes >= k and ranks past the orderable logits propose nothing)
            by = fmaf(zr, inv_t, sm_noise(seed, offset + (unsigned)row, idr));
            id = idr;
            z = zr;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float oy = __shfl_xor(by, o, 64), oz = __shfl_xor(z, o, 64);
            const int oi = __shfl_xor(id, o, 64);
            if (oy > by || (oy == by && oi < id)) { by = oy; id = oi; z = oz; }
        }
    }
    float s = 0.f;
    for (int j = lane; j < tiles_n; j += 64) {
        const float2 q = cl[j * cw];
        s += q.y * expf(q.x - m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane != 0) return;
    const bool none = id == INT_MAX;
    if (none) id = 0;
    if (ids) ids[row * ld_ids] = id;
    if (probs) probs[row * ld_probs] = none || z == m ? 1.f / s : expf(z - m) / s;
    tokens[row] = id;
    if (mask) mask[row] = id != 0 ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ beam selection
// One block of four waves per RoI.  Every wave repeats the decision: lane l < nb * k holds candidate (beam b = l / k, rank i = l % k)
// of the beam-major candidate rows b * R + roi: score = scores_in[roi][b] + (p or log p).  A beam that finished_in marks proposes ONE
// candidate, in its rank-0 lane: token 0 at its own score, nothing added; its candidate rows are not read.  k threshold rounds in the
// order (score descending, parent ascending, word id ascending) give the new beams best first; wave 0 writes beam q's score, history
// entries, next token, mask and finished byte.  After the first step there are always at least k candidates (a live beam brings k, and
// at worst k finished beams bring one each), so the "no candidate left" fallback (beam 0, token 0) is met only with NaN probabilities,
// as before.  Then the block copies the parents' rows of every row set into rows q * R + roi of the set's destination, the float4
// chunks of all k rows spread over the 256 threads (lane q of every wave keeps beam q's parent; four loads in flight per thread).
__device__ __forceinline__ bool bs_before(float s, int b, int t, float os, int ob, int ot) {
    return s > os || (s == os && (b < ob || (b == ob && t < ot)));
}

__global__ __launch_bounds__(256) void beam_step_kernel(dc_beam_step_desc d) {
    const int roi = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int k = d.k, R = d.R;
    float s = -INFINITY;
    int b = INT_MAX, t = INT_MAX, fin = 0;
    if (lane < d.nb * k) {
        const int lb = lane / k, i = lane - lb * k;
        fin = d.finished_in && d.finished_in[(long)lb * R + roi] ? 1 : 0;
        if (fin) {
            if (i == 0) { b = lb; t = 0; s = d.scores_in ? d.scores_in[roi * k + lb] : 0.f; }
        } else {
            const long c = ((long)lb * R + roi) * k + i;
            b = lb;
            t = d.cand_ids[c];
            const float p = d.cand_probs[c];
            s = (d.scores_in ? d.scores_in[roi * k + lb] : 0.f) + (d.log_score ? logf(p) : p);
        }
    }
    float ts = INFINITY;
    int tb = INT_MIN, tt = INT_MIN, par = 0;                   // par: lane q < k keeps new beam q's parent
    for (int q = 0; q < k; ++q) {
        const bool ok = bs_before(ts, tb, tt, s, b, t);       // this lane's candidate comes after the previous winner
        float bs = ok ? s : -INFINITY;
        int bb = ok ? b : INT_MAX, bt = ok ? t : INT_MAX;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(bs, o, 64);
            const int ob = __shfl_xor(bb, o, 64), ot = __shfl_xor(bt, o, 64);
            if (bs_before(os, ob, ot, bs, bb, bt)) { bs = os; bb = ob; bt = ot; }
        }
        ts = bs; tb = bb; tt = bt;
        if (bb == INT_MAX) { bb = 0; bt = 0; }                // (no candidate left, only with NaN probabilities: beam 0, token 0)
        const int pfin = __shfl(fin, bb * k, 64);             // the parent's finished flag sits in its rank-0 lane
        if (lane == q) par = bb;
        if (tid == 0) {
            const long dst = (long)q * R + roi, hix = ((long)d.j * R + roi) * k + q;
            d.scores_out[roi * k + q] = bs;
            d.parents[hix] = bb;
            d.tokens_hist[hix] = bt;
            if (d.tokens) d.tokens[dst] = bt;
            if (d.mask) d.mask[dst] = bt != 0 ? 1 : 0;
            if (d.finished_out) d.finished_out[dst] = pfin || bt == d.end_id ? 1 : 0;
        }
    }
#pragma unroll
    for (int si = 0; si < DC_BEAM_MAX_SETS; ++si) {
        if (si >= d.n_sets) break;
        const int n4 = d.U[si] >> 2, items = k * n4;
        const float4* __restrict__ src = reinterpret_cast<const float4*>(d.src[si]);
        float4* __restrict__ dst = reinterpret_cast<float4*>(d.dst[si]);
        // chunk i of the set's k * n4: row q = i / n4 of the new beams, from the row of q's parent (named registers, not arrays: an
        // indexed private array here is placed in LDS)
        auto load = [&](int i, float4& v) -> long {
            const int q = i < items ? i / n4 : 0;
            const int p = __shfl(par, q, 64);
            const int u = i - q * n4;
            if (i >= items) return -1;
            v = src[((long)p * R + roi) * n4 + u];
            return ((long)q * R + roi) * n4 + u;
        };
        for (int base = tid; base - tid < items; base += 1024) {
            float4 v0, v1, v2, v3;
            const long o0 = load(base, v0), o1 = load(base + 256, v1), o2 = load(base + 512, v2), o3 = load(base + 768, v3);
            if (o0 >= 0) dst[o0] = v0;
            if (o1 >= 0) dst[o1] = v1;
            if (o2 >= 0) dst[o2] = v2;
            if (o3 >= 0) dst[o3] = v3;
        }
    }
}

// One thread per (roi, beam): walk the parents from the last step back.
__global__ __launch_bounds__(256) void beam_backtrace_kernel(const int32_t* __restrict__ parents, const int32_t* __restrict__ tokens_hist,
                                                             int steps, int R, int k, int32_t* __restrict__ seq) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R * k) return;
    const int roi = i / k;
    int cur = i - roi * k;
    int32_t* out = seq + (long)i * steps;
    for (int j = steps - 1; j >= 0; --j) {
        const long hix = ((long)j * R + roi) * k + cur;
        out[j] = tokens_hist[hix];
        cur = parents[hix];
    }
}

static size_t tk_align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The operand checks of both vocabulary entry points; fn names the entry point in the messages.
static int vocab_f32_validate(const char* fn, const dc_vocab_topk_desc& d) {
    DC_REQUIRE((d.K & 31) == 0 && (d.ldx & 3) == 0 && (d.ldw & 3) == 0, DC_EALIGN, "%s: K must be a multiple of 32 and ldx, ldw multiples of 4", fn);
    DC_REQUIRE(d.ldx >= d.K && d.ldw >= (d.V + 3) / 4 * 4, DC_EINVAL, "%s: ldx < K or ldw < V rounded up to 4", fn);
    DC_REQUIRE(aligned16(d.X) && aligned16(d.W) && (!d.bias || aligned16(d.bias)), DC_EALIGN, "%s: X, W, bias must be 16-byte aligned", fn);
    DC_REQUIRE((size_t)d.M * d.ldx * 4 < (size_t)0xFFFFFFF0u && (size_t)d.K * d.ldw * 4 < (size_t)0xFFFFFFF0u, DC_EINVAL,
               "%s: operands must span < 4 GiB", fn);
    return DC_OK;
}

// bf16 operands: the rules of dc_vocab_ce's bf16 branch, but any V (W's rows readable up to V rounded up to 8).
static int vocab_bf16_validate(const char* fn, const dc_vocab_topk_bf16_desc& d) {
    DC_REQUIRE(d.tile == 0 || d.tile == 128 || d.tile == 256, DC_EINVAL, "%s: tile must be 0 (automatic), 128 or 256, got %d", fn, d.tile);
    DC_REQUIRE((d.K & 7) == 0 && (d.ldx & 7) == 0 && (d.ldw & 7) == 0, DC_EALIGN, "%s: K, ldx, ldw must be multiples of 8", fn);
    DC_REQUIRE(d.ldx >= d.K && d.ldw >= (d.V + 7) / 8 * 8, DC_EINVAL, "%s: ldx < K or ldw < V rounded up to 8", fn);
    DC_REQUIRE(aligned16(d.X) && aligned16(d.W) && (!d.bias || aligned16(d.bias)), DC_EALIGN, "%s: X, W, bias must be 16-byte aligned", fn);
    DC_REQUIRE((size_t)d.M * d.ldx * 2 < (size_t)0x7FFFFFF0u && (size_t)d.K * d.ldw * 2 < (size_t)0x7FFFFFF0u, DC_EINVAL,
               "%s: operands must span < 2 GiB", fn);
    return DC_OK;
}

// 0 (automatic) -> the tile dc_vocab_ce's bf16 branch would run this problem on (ce_big()); V counts rounded up to 8, as W is read
static int tk_bf16_tile(int M, int V, int K, int tile) {
    if (tile) return tile;
    return b256::prefer(M, (V + 7) / 8 * 8, K, 1) ? 256 : 128;
}
// cells per row: one per 128-column tile, or one per 64-column wave slice of the 256-column tile
static int tk_bf16_cells(int V, int tile) { return tile == 256 ? (V + 63) / 64 : (V + 127) / 128; }

}  // namespace dcap

using namespace dcap;

extern "C" size_t dc_vocab_topk_workspace_bytes(int M, int V, int k) {
    if (M <= 0 || V <= 0 || k <= 0) return 0;
    return tk_align256((size_t)M * ((V + 127) / 128) * (k + 1) * sizeof(float2));
}

// Both entry points: the tile kernel, then the row kernel with the caller's output strides (and, for top-1, tokens and mask).
static int vocab_topk_run(const char* fn, const dc_vocab_topk_desc& d, long ld_ids, long ld_probs, int32_t* tokens, uint8_t* mask,
                          void* workspace, size_t workspace_bytes, void* stream) {
    int rc = vocab_f32_validate(fn, d);
    if (rc) return rc;
    const size_t need = dc_vocab_topk_workspace_bytes(d.M, d.V, d.k);
    DC_REQUIRE(workspace && workspace_bytes >= need, DC_EWORKSPACE, "%s: needs %zu workspace bytes, got %zu", fn, need, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    TopkArgs ta{};
    ta.M = d.M; ta.V = d.V; ta.k = d.k;
    ta.tiles_m = (d.M + 127) / 128;
    ta.tiles_n = (d.V + 127) / 128;
    ta.bias = d.bias;
    ta.cells = static_cast<float2*>(workspace);
    // the B loader reads whole 16-byte column quads: the columns V .. round4(V) - 1 it then also reads lie inside the row (ldw >= round4(V))
    // and feed only the tile's guarded-off lanes
    TKA al{d.X, d.ldx, d.M, nullptr};
    TKB bl{d.W, d.ldw, (d.V + 3) / 4 * 4, nullptr};
    DC_ENSURE_DYN_LDS((&vocab_topk_f32_kernel), 160 * 1024);
    constexpr size_t lds = igemm_lds_bytes<128, 128, TKA, TKB>();
    hipLaunchKernelGGL(vocab_topk_f32_kernel, dim3(ta.tiles_m * ta.tiles_n), dim3(256), lds, s, al, bl, ta, d.K);
    rc = check_launch("vocab_topk_f32_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(vocab_topk_rows_kernel, dim3((d.M + 3) / 4), dim3(256), 0, s, d.M, ta.tiles_n, d.k, ta.cells, d.ids, ld_ids, d.probs,
                       ld_probs, tokens, mask);
    return check_launch("vocab_topk_rows_kernel");
}

extern "C" int dc_vocab_topk_f32(const dc_vocab_topk_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    DC_REQUIRE(d != nullptr, DC_EINVAL, "dc_vocab_topk: null descriptor");
    DC_REQUIRE(d->M > 0 && d->V > 0 && d->K > 0 && d->X && d->W && d->ids && d->probs, DC_EINVAL, "dc_vocab_topk: bad arguments");
    DC_REQUIRE(d->k >= 1 && d->k <= TK_MAX && d->V >= d->k, DC_EINVAL, "dc_vocab_topk: need 1 <= k <= 8 and V >= k (k = %d, V = %d)", d->k, d->V);
    return vocab_topk_run("dc_vocab_topk", *d, d->k, d->k, nullptr, nullptr, workspace, workspace_bytes, stream);
}

extern "C" size_t dc_vocab_top1_workspace_bytes(int M, int V) { return dc_vocab_topk_workspace_bytes(M, V, 1); }

extern "C" int dc_vocab_top1_f32(const dc_vocab_top1_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    DC_REQUIRE(d != nullptr, DC_EINVAL, "dc_vocab_top1: null descriptor");
    DC_REQUIRE(d->M > 0 && d->V > 0 && d->K > 0 && d->X && d->W && d->tokens, DC_EINVAL, "dc_vocab_top1: bad arguments");
    DC_REQUIRE((!d->ids || d->ld_ids >= 1) && (!d->probs || d->ld_probs >= 1), DC_EINVAL, "dc_vocab_top1: ld_ids / ld_probs must be >= 1");
    const dc_vocab_topk_desc tk{d->M, d->V, d->K, 1, d->X, d->ldx, d->W, d->ldw, d->bias, d->ids, d->probs};
    return vocab_topk_run("dc_vocab_top1", tk, d->ld_ids, d->ld_probs, d->tokens, d->mask, workspace, workspace_bytes, stream);
}

extern "C" int dc_vocab_topk_bf16_tile(int M, int V, int K) {
    if (M <= 0 || V <= 0 || K <= 0) return 0;
    return tk_bf16_tile(M, V, K, 0);
}

extern "C" size_t dc_vocab_topk_bf16_workspace_bytes(int M, int V, int K, int k, int tile) {
    if (M <= 0 || V <= 0 || K <= 0 || k <= 0 || (tile != 0 && tile != 128 && tile != 256)) return 0;
    return tk_align256((size_t)M * tk_bf16_cells(V, tk_bf16_tile(M, V, K, tile)) * (k + 1) * sizeof(float2));
}

extern "C" size_t dc_vocab_top1_bf16_workspace_bytes(int M, int V, int K, int tile) { return dc_vocab_topk_bf16_workspace_bytes(M, V, K, 1, tile); }

// Both bf16 entry points: the tile kernel of the chosen shape, then the row kernel over that shape's cells.
static int vocab_topk_bf16_run(const char* fn, const dc_vocab_topk_bf16_desc& d, long ld_ids, long ld_probs, int32_t* tokens, uint8_t* mask,
                               void* workspace, size_t workspace_bytes, void* stream) {
    int rc = vocab_bf16_validate(fn, d);
    if (rc) return rc;
    const size_t need = dc_vocab_topk_bf16_workspace_bytes(d.M, d.V, d.K, d.k, d.tile);
    DC_REQUIRE(workspace && workspace_bytes >= need, DC_EWORKSPACE, "%s: needs %zu workspace bytes, got %zu", fn, need, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int T = tk_bf16_tile(d.M, d.V, d.K, d.tile);
    TopkArgs ta{};
    ta.M = d.M; ta.V = d.V; ta.k = d.k;
    ta.tiles_m = (d.M + T - 1) / T;
    ta.tiles_n = tk_bf16_cells(d.V, T);
    ta.bias = d.bias;
    ta.cells = static_cast<float2*>(workspace);
    // the W loader reads whole 16-byte chunks of 8 columns: the columns V .. round8(V) - 1 lie inside the row (ldw >= round8(V)) and feed
    // only guarded-off lanes; the buffer ranges end with the last element the rules above make readable
    const int Vp = (d.V + 7) / 8 * 8;
    BOperand a{static_cast<const unsigned short*>(d.X), d.ldx, d.M, nullptr, (unsigned)(((size_t)(d.M - 1) * d.ldx + d.K) * 2)};
    BOperand b{static_cast<const unsigned short*>(d.W), d.ldw, Vp, nullptr, (unsigned)(((size_t)(d.K - 1) * d.ldw + Vp) * 2)};
    if (T == 256) {
        const int tiles_n = (d.V + 255) / 256;
        DC_ENSURE_DYN_LDS((&vocab_topk_bf16_256_kernel), 160 * 1024);
        hipLaunchKernelGGL(vocab_topk_bf16_256_kernel, dim3(ta.tiles_m * tiles_n), dim3(b256::NTHREADS), b256::LDS_BYTES, s, a, b, ta, d.K,
                           ta.tiles_m, tiles_n);
        rc = check_launch("vocab_topk_bf16_256_kernel");
    } else {
        DC_ENSURE_DYN_LDS((&vocab_topk_bf16_kernel), 160 * 1024);
        hipLaunchKernelGGL(vocab_topk_bf16_kernel, dim3(ta.tiles_m * ta.tiles_n), dim3(256), bgemm_lds_bytes(), s, a, b, ta, d.K);
        rc = check_launch("vocab_topk_bf16_kernel");
    }
    if (rc) return rc;
    hipLaunchKernelGGL(vocab_topk_rows_kernel, dim3((d.M + 3) / 4), dim3(256), 0, s, d.M, ta.tiles_n, d.k, ta.cells, d.ids, ld_ids, d.probs,
                       ld_probs, tokens, mask);
    return check_launch("vocab_topk_rows_kernel");
}

extern "C" int dc_vocab_topk_bf16(const dc_vocab_topk_bf16_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    DC_REQUIRE(d != nullptr, DC_EINVAL, "dc_vocab_topk_bf16: null descriptor");
    DC_REQUIRE(d->M > 0 && d->V > 0 && d->K > 0 && d->X && d->W && d->ids && d->probs, DC_EINVAL, "dc_vocab_topk_bf16: bad arguments");
    DC_REQUIRE(d->k >= 1 && d->k <= TK_MAX && d->V >= d->k, DC_EINVAL, "dc_vocab_topk_bf16: need 1 <= k <= 8 and V >= k (k = %d, V = %d)", d->k,
               d->V);
    return vocab_topk_bf16_run("dc_vocab_topk_bf16", *d, d->k, d->k, nullptr, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int dc_vocab_top1_bf16(const dc_vocab_top1_bf16_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    DC_REQUIRE(d != nullptr, DC_EINVAL, "dc_vocab_top1_bf16: null descriptor");
    DC_REQUIRE(d->M > 0 && d->V > 0 && d->K > 0 && d->X && d->W && d->tokens, DC_EINVAL, "dc_vocab_top1_bf16: bad arguments");
    DC_REQUIRE((!d->ids || d->ld_ids >= 1) && (!d->probs || d->ld_probs >= 1), DC_EINVAL, "dc_vocab_top1_bf16: ld_ids / ld_probs must be >= 1");
    const dc_vocab_topk_bf16_desc tk{d->M, d->V, d->K, 1, d->X, d->ldx, d->W, d->ldw, d->bias, d->ids, d->probs, d->tile};
    return vocab_topk_bf16_run("dc_vocab_top1_bf16", tk, d->ld_ids, d->ld_probs, d->tokens, d->mask, workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------------ sampling entry points
// What both sampling entry points ask beyond the operand checks; fn names the entry point in the messages.
static int vocab_sample_validate(const char* fn, int V, bool tokens, int ld_ids_ok, float inv_t, int top_k) {
    DC_REQUIRE(tokens, DC_EINVAL, "%s: bad arguments", fn);
    DC_REQUIRE(ld_ids_ok, DC_EINVAL, "%s: ld_ids / ld_probs must be >= 1", fn);
    DC_REQUIRE(inv_t > 0.f && inv_t < INFINITY, DC_EINVAL, "%s: inv_t = 1 / temperature must be finite and > 0, got %g", fn, (double)inv_t);
    DC_REQUIRE(top_k >= 0 && top_k <= TK_MAX && V >= top_k, DC_EINVAL,
               "%s: top_k must be 0 (the whole vocabulary) or 1 <= top_k <= 8 with V >= top_k (top_k = %d, V = %d)", fn, top_k, V);
    return DC_OK;
}

extern "C" size_t dc_vocab_sample_workspace_bytes(int M, int V, int top_k) {
    if (M <= 0 || V <= 0 || top_k < 0) return 0;
    if (top_k) return dc_vocab_topk_workspace_bytes(M, V, top_k);
    return tk_align256((size_t)M * ((V + 127) / 128) * 3 * sizeof(float2));
}

// whole vocabulary: always the 128 tile (0 means 128 here); top_k: the top-k kernels' rule
extern "C" size_t dc_vocab_sample_bf16_workspace_bytes(int M, int V, int K, int top_k, int tile) {
    if (M <= 0 || V <= 0 || K <= 0 || top_k < 0 || (tile != 0 && tile != 128 && tile != 256)) return 0;
    if (top_k) return dc_vocab_topk_bf16_workspace_bytes(M, V, K, top_k, tile);
    return tile == 256 ? 0 : dc_vocab_sample_workspace_bytes(M, V, 0);
}

extern "C" int dc_vocab_sample_f32(const dc_vocab_sample_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "dc_vocab_sample";
    DC_REQUIRE(d != nullptr, DC_EINVAL, "dc_vocab_sample: null descriptor");
    DC_REQUIRE(d->M > 0 && d->V > 0 && d->K > 0 && d->X && d->W, DC_EINVAL, "dc_vocab_sample: bad arguments");
    int rc = vocab_sample_validate(fn, d->V, d->tokens != nullptr, (!d->ids || d->ld_ids >= 1) && (!d->probs || d->ld_probs >= 1), d->inv_t, d->top_k);
    if (rc) return rc;
    const dc_vocab_topk_desc tk{d->M, d->V, d->K, d->top_k, d->X, d->ldx, d->W, d->ldw, d->bias, nullptr, nullptr};
    rc = vocab_f32_validate(fn, tk);
    if (rc) return rc;
    const size_t need = dc_vocab_sample_workspace_bytes(d->M, d->V, d->top_k);
    DC_REQUIRE(workspace && workspace_bytes >= need, DC_EWORKSPACE, "%s: needs %zu workspace bytes, got %zu", fn, need, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    SampleArgs sa{};
    TopkArgs& ta = sa.t;
    ta.M = d->M; ta.V = d->V; ta.k = d->top_k;
    ta.tiles_m = (d->M + 127) / 128;
    ta.tiles_n = (d->V + 127) / 128;
    ta.bias = d->bias;
    ta.cells = static_cast<float2*>(workspace);
    sa.inv_t = d->inv_t; sa.seed = d->seed; sa.offset = d->offset;
    TKA al{d->X, d->ldx, d->M, nullptr};                        // (operands: as vocab_topk_run)
    TKB bl{d->W, d->ldw, (d->V + 3) / 4 * 4, nullptr};
    constexpr size_t lds = igemm_lds_bytes<128, 128, TKA, TKB>();
    if (d->top_k) {
        DC_ENSURE_DYN_LDS((&vocab_topk_f32_kernel), 160 * 1024);
        hipLaunchKernelGGL(vocab_topk_f32_kernel, dim3(ta.tiles_m * ta.tiles_n), dim3(256), lds, s, al, bl, ta, d->K);
        rc = check_launch("vocab_topk_f32_kernel");
    } else {
        DC_ENSURE_DYN_LDS((&vocab_sample_f32_kernel), 160 * 1024);
        hipLaunchKernelGGL(vocab_sample_f32_kernel, dim3(ta.tiles_m * ta.tiles_n), dim3(256), lds, s, al, bl, sa, d->K);
        rc = check_launch("vocab_sample_f32_kernel");
    }
    if (rc) return rc;
    hipLaunchKernelGGL(vocab_sample_rows_kernel, dim3((d->M + 3) / 4), dim3(256), 0, s, d->M, ta.tiles_n, d->top_k, ta.cells, sa.inv_t, sa.seed,
                       sa.offset, d->ids, (long)d->ld_ids, d->probs, (long)d->ld_probs, d->tokens, d->mask);
    return check_launch("vocab_sample_rows_kernel");
}

extern "C" int dc_vocab_sample_bf16(const dc_vocab_sample_bf16_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "dc_vocab_sample_bf16";
    DC_REQUIRE(d != nullptr, DC_EINVAL, "dc_vocab_sample_bf16: null descriptor");
    DC_REQUIRE(d->M > 0 && d->V > 0 && d->K > 0 && d->X && d->W, DC_EINVAL, "dc_vocab_sample_bf16: bad arguments");
    int rc = vocab_sample_validate(fn, d->V, d->tokens != nullptr, (!d->ids || d->ld_ids >= 1) && (!d->probs || d->ld_probs >= 1), d->inv_t, d->top_k);
    if (rc) return rc;
    const dc_vocab_topk_bf16_desc tk{d->M, d->V, d->K, d->top_k, d->X, d->ldx, d->W, d->ldw, d->bias, nullptr, nullptr, d->tile};
    rc = vocab_bf16_validate(fn, tk);
    if (rc) return rc;
    DC_REQUIRE(d->top_k || d->tile != 256, DC_EINVAL,
               "%s: sampling over the whole vocabulary (top_k = 0) runs on the 128 x 128 tile only: pass tile = 0 or 128, got 256", fn);
    const size_t need = dc_vocab_sample_bf16_workspace_bytes(d->M, d->V, d->K, d->top_k, d->tile);
    DC_REQUIRE(workspace && workspace_bytes >= need, DC_EWORKSPACE, "%s: needs %zu workspace bytes, got %zu", fn, need, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int T = d->top_k ? tk_bf16_tile(d->M, d->V, d->K, d->tile) : 128;
    SampleArgs sa{};
    TopkArgs& ta = sa.t;
    ta.M = d->M; ta.V = d->V; ta.k = d->top_k;
    ta.tiles_m = (d->M + T - 1) / T;
    ta.tiles_n = tk_bf16_cells(d->V, T);
    ta.bias = d->bias;
    ta.cells = static_cast<float2*>(workspace);
    sa.inv_t = d->inv_t; sa.seed = d->seed; sa.offset = d->offset;
    const int Vp = (d->V + 7) / 8 * 8;                          // (operands: as vocab_topk_bf16_run)
    BOperand a{static_cast<const unsigned short*>(d->X), d->ldx, d->M, nullptr, (unsigned)(((size_t)(d->M - 1) * d->ldx + d->K) * 2)};
    BOperand b{static_cast<const unsigned short*>(d->W), d->ldw, Vp, nullptr, (unsigned)(((size_t)(d->K - 1) * d->ldw + Vp) * 2)};
    if (!d->top_k) {
        DC_ENSURE_DYN_LDS((&vocab_sample_bf16_kernel), 160 * 1024);
        hipLaunchKernelGGL(vocab_sample_bf16_kernel, dim3(ta.tiles_m * ta.tiles_n), dim3(256), bgemm_lds_bytes(), s, a, b, sa, d->K);
        rc = check_launch("vocab_sample_bf16_kernel");
    } else if (T == 256) {
        const int tiles_n = (d->V + 255) / 256;
        DC_ENSURE_DYN_LDS((&vocab_topk_bf16_256_kernel), 160 * 1024);
        hipLaunchKernelGGL(vocab_topk_bf16_256_kernel, dim3(ta.tiles_m * tiles_n), dim3(b256::NTHREADS), b256::LDS_BYTES, s, a, b, ta, d->K,
                           ta.tiles_m, tiles_n);
        rc = check_launch("vocab_topk_bf16_256_kernel");
    } else {
        DC_ENSURE_DYN_LDS((&vocab_topk_bf16_kernel), 160 * 1024);
        hipLaunchKernelGGL(vocab_topk_bf16_kernel, dim3(ta.tiles_m * ta.tiles_n), dim3(256), bgemm_lds_bytes(), s, a, b, ta, d->K);
        rc = check_launch("vocab_topk_bf16_kernel");
    }
    if (rc) return rc;
    hipLaunchKernelGGL(vocab_sample_rows_kernel, dim3((d->M + 3) / 4), dim3(256), 0, s, d->M, ta.tiles_n, d->top_k, ta.cells, sa.inv_t, sa.seed,
                       sa.offset, d->ids, (long)d->ld_ids, d->probs, (long)d->ld_probs, d->tokens, d->mask);
    return check_launch("vocab_sample_rows_kernel");
}

static bool bs_overlap(const void* a, const void* b, size_t bytes_a, size_t bytes_b) {
    const char* x = static_cast<const char*>(a);
    const char* y = static_cast<const char*>(b);
    return x < y + bytes_b && y < x + bytes_a;
}

// The checks and the launch of both beam entry points; fn names the entry point in the messages.
static int beam_step_run(const char* fn, const dc_beam_step_desc& d, void* stream) {
    DC_REQUIRE(d.R > 0 && d.k >= 1 && d.k <= TK_MAX && d.nb >= 1 && d.nb <= d.k && d.j >= 0 && d.j < d.steps, DC_EINVAL,
               "%s: need R > 0, 1 <= nb <= k <= 8, 0 <= j < steps", fn);
    DC_REQUIRE(d.cand_ids && d.cand_probs && d.scores_out && d.parents && d.tokens_hist, DC_EINVAL, "%s: null pointer", fn);
    DC_REQUIRE(d.scores_out != d.scores_in, DC_EINVAL, "%s: scores_out must not alias scores_in", fn);
    DC_REQUIRE(d.end_id >= -1, DC_EINVAL, "%s: end_id is a word id or -1 (none), got %d", fn, d.end_id);
    DC_REQUIRE(d.end_id < 0 || d.finished_out, DC_EINVAL, "%s: an end token needs finished_out", fn);
    DC_REQUIRE(!d.finished_out || d.finished_out != d.finished_in, DC_EINVAL, "%s: finished_out must not alias finished_in", fn);
    DC_REQUIRE(d.n_sets >= 0 && d.n_sets <= DC_BEAM_MAX_SETS, DC_EINVAL, "%s: 0 to %d row sets, got %d", fn, DC_BEAM_MAX_SETS, d.n_sets);
    const size_t rows = (size_t)d.k * d.R * sizeof(float);
    for (int i = 0; i < d.n_sets; ++i) {
        DC_REQUIRE(d.src[i] && d.dst[i] && d.U[i] > 0 && (d.U[i] & 3) == 0, DC_EINVAL, "%s: row set %d needs src, dst and U %% 4 == 0", fn, i);
        DC_REQUIRE(aligned16(d.src[i]) && aligned16(d.dst[i]), DC_EALIGN, "%s: row set %d must be 16-byte aligned", fn, i);
        for (int o = 0; o < d.n_sets; ++o)
            DC_REQUIRE(!bs_overlap(d.dst[i], d.src[o], rows * d.U[i], rows * d.U[o]) &&
                           (o == i || !bs_overlap(d.dst[i], d.dst[o], rows * d.U[i], rows * d.U[o])),
                       DC_EINVAL, "%s: dst of row set %d must not alias a src or another dst (set %d)", fn, i, o);
    }
    hipLaunchKernelGGL(beam_step_kernel, dim3(d.R), dim3(256), 0, static_cast<hipStream_t>(stream), d);
    return check_launch("beam_step_kernel");
}

extern "C" int dc_beam_step_f32(const dc_beam_step_desc* d, void* stream) {
    DC_REQUIRE(d != nullptr, DC_EINVAL, "dc_beam_step: null descriptor");
    return beam_step_run("dc_beam_step", *d, stream);
}

// The earlier entry point: its h / c pair is two row sets of one width, and there is no end token.
extern "C" int dc_beam_select_f32(const dc_beam_select_desc* d, void* stream) {
    DC_REQUIRE(d != nullptr, DC_EINVAL, "dc_beam_select: null descriptor");
    dc_beam_step_desc s{};
    s.R = d->R, s.k = d->k, s.nb = d->nb, s.steps = d->steps, s.j = d->j, s.log_score = d->log_score;
    s.cand_ids = d->cand_ids, s.cand_probs = d->cand_probs, s.scores_in = d->scores_in, s.scores_out = d->scores_out;
    s.parents = d->parents, s.tokens_hist = d->tokens_hist, s.tokens = d->tokens, s.mask = d->mask;
    s.end_id = -1;
    if (d->h_in) {
        DC_REQUIRE(d->c_in && d->h_out && d->c_out && d->U > 0 && (d->U & 3) == 0, DC_EINVAL, "dc_beam_select: h/c rows need U %% 4 == 0 and four buffers");
        s.n_sets = 2;
        s.U[0] = s.U[1] = d->U;
        s.src[0] = d->h_in, s.dst[0] = d->h_out, s.src[1] = d->c_in, s.dst[1] = d->c_out;
    }
    return beam_step_run("dc_beam_select", s, stream);
}

extern "C" int dc_beam_backtrace(const int32_t* parents, const int32_t* tokens_hist, int steps, int R, int k, int32_t* seq, void* stream) {
    DC_REQUIRE(parents && tokens_hist && seq && steps > 0 && R > 0 && k >= 1 && k <= TK_MAX, DC_EINVAL, "dc_beam_backtrace: bad arguments");
    hipLaunchKernelGGL(beam_backtrace_kernel, dim3((R * k + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), parents, tokens_hist,
                       steps, R, k, seq);
    return check_launch("beam_backtrace_kernel");
}

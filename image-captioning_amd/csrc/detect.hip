// detect.hip -- what Mask R-CNN's inference path needs behind the shared RoI head (mask_rcnn/mask_rcnn_model.py: fpn_classifier_graph's
// softmax + refine_detections :684-688, build_fpn_mask_graph's mrcnn_mask_deconv + mrcnn_mask, utils.unmold_mask):
//
//   dc_class_select_f32     per RoI: the winning class (lowest index of the maximal logit), its softmax probability and its four box
//                           deltas.  One wave per row, classes on the lanes; the maximum and the sum of exp(z - max) are xor-butterfly
//                           reductions, so the order of every operation is fixed by C alone.
//   dc_mask_head_tail_f32   Conv2DTranspose(2x2, stride 2) + ReLU + the 1x1 mrcnn_mask convolution + sigmoid, for each RoI's OWN
//                           class only.  The transposed convolution is the product [N P P, Cin] x [Cin, 4 Cmid] (a quadrant (dy, dx)
//                           of an input pixel is a block of Cmid columns); it runs on v_mfma_f32_32x32x2_f32 in the layout of
//                           conv_pw.hip -- channels on the MFMA's M side from an LDS slice of the weights, pixels on the N side with
//                           the lane's half of the K run held in registers for the block's whole life -- and the epilogue of each
//                           32-channel slice folds ReLU(acc + bias) into a dot product with the class column of the pixel's RoI.
//                           After the last slice of a quadrant the two lane halves are summed, the sigmoid applied and ONE float
//                           stored: neither the [N,2P,2P,Cmid] map nor an all-class map exists anywhere.
//   dc_mask_paste_u8        utils.unmold_mask for the detections of one image: scipy's bytescale on the mask's own range, PIL's 8-bit
//                           bilinear resize to the box (the coefficient code of resize_core.h, shared with resize.hip), threshold at
//                           128, pasted into a zeroed [H][W] plane.  Every byte of the output is written.
//   dc_mask_rle_u32         the same planes as COCO run lengths without ever storing them: the paste's first three launches, then
//                           one wave per box column takes the transitions of 64 rows a step from a ballot, two prefix sums place
//                           them, a second walk stores their positions and a last launch differences them into counts.
#include "igemm_core.h"
#include "resize_core.h"
#include <limits.h>

namespace dcap {

// ------------------------------------------------------------------------------------------------ class select
constexpr int CS_THREADS = 256, CS_ROWS = CS_THREADS / 64;

__global__ __launch_bounds__(CS_THREADS) void class_select_kernel(const float* __restrict__ z, int ldz, const float* __restrict__ dl, int ldd, int R,
                                                                 int C, int* __restrict__ ids, float* __restrict__ scores,
                                                                 float* __restrict__ dout) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * CS_ROWS + (threadIdx.x >> 6);
    if (row >= R) return;                                        // whole waves leave: the shuffles below see full waves
    const float* zr = z + (size_t)row * ldz;
    float best = -INFINITY;
    int bi = INT_MAX;
    for (int j = lane; j < C; j += 64) {
        const float v = zr[j];
        if (v > best) { best = v; bi = j; }                      // strictly greater: the lowest index of a lane's equal values stays
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const float ov = __shfl_xor(best, off);
        const int oi = __shfl_xor(bi, off);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    float s = 0.f;
    for (int j = lane; j < C; j += 64) s += expf(zr[j] - best);
#pragma unroll
    for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
    if (bi == INT_MAX) bi = 0;                                   // (only a row without one finite-comparable logit: not expected)
    if (lane == 0) {
        ids[row] = bi;
        scores[row] = 1.f / s;
    }
    if (lane < 4) dout[(size_t)row * 4 + lane] = dl[(size_t)row * ldd + 4 * (size_t)bi + lane];
}

// ------------------------------------------------------------------------------------------------ mask head tail
constexpr int MT_THREADS = 256, MT_CH = 32, MT_KMAX = 256, MT_ROWS = 128;      // 4 waves x 32 pixels; a weight slice is 32 channels
constexpr int MT_PRE = MT_CH * (MT_KMAX / 4) / MT_THREADS;                       // 16-byte words of a slice per thread: 8

// four consecutive floats: one 16-byte load where the caller knows the base allows it, four 4-byte loads otherwise
template <bool A16>
__device__ __forceinline__ f4 load4(const float* p) {
    if constexpr (A16) return *reinterpret_cast<const f4*>(p);
    return f4{p[0], p[1], p[2], p[3]};
}

__device__ __forceinline__ float sigmoid_f32(float z) {
    const float e = expf(-fabsf(z));                              // in (0, 1]: exp never overflows, |z| = 200 gives 0
    const float r = 1.f / (1.f + e);
    return z >= 0.f ? r : e * r;
}

template <bool A16>
__global__ __launch_bounds__(MT_THREADS, 2) void mask_head_tail_kernel(const float* __restrict__ x, const float* __restrict__ wd,
                                                                      const float* __restrict__ bd, const float* __restrict__ wmt,
                                                                      const float* __restrict__ bm, const int* __restrict__ class_ids,
                                                                      float* __restrict__ out, int M, int P, int Cin, int Cmid, int C) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int LDW = Cin + 4, KH = Cin / 2, K4 = Cin / 4;
    float* const Ws = smem;                                       // [MT_CH][LDW]
    float* const bds = smem + MT_CH * LDW;                        // [Cmid]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int PP = P * P;
    const int prow = (blockIdx.x * 4 + wave) * 32 + i;
    const bool pv = prow < M;
    const int p = min(prow, M - 1);
    const int n = p / PP, rem = p - n * PP, py = rem / P, px = rem - py * P;
    const int kraw = class_ids[n];
    const bool kv = kraw >= 0 && kraw < C;                        // an id outside [0, C): zeros for that RoI, nothing else read with it
    const int k = kv ? kraw : 0;
    const float* const wrow = wmt + (size_t)k * Cmid + 4 * h;
    const float bmk = bm[k];

    // the lane's half of its pixel's K run: the MFMA B operands, loaded once
    f4 xs[MT_KMAX / 8];
    const float* xr = x + (size_t)p * Cin + KH * h;
#pragma unroll
    for (int j = 0; j < MT_KMAX / 8; ++j) xs[j] = 4 * j < KH ? load4<A16>(xr + 4 * j) : f4{0.f, 0.f, 0.f, 0.f};
    for (int c = tid; c < Cmid; c += MT_THREADS) bds[c] = bd[c];

    // slice s = rows 32 s .. 32 s + 31 of the [4 Cmid][Cin] weight matrix; each thread carries its MT_PRE words of the NEXT slice in
    // registers while the MFMAs of the current one run
    const int slices = 4 * Cmid / MT_CH, per_quadrant = Cmid / MT_CH, words = MT_CH * K4;
    f4 pre[MT_PRE];
#pragma unroll
    for (int u = 0; u < MT_PRE; ++u) {
        const int idx = tid + u * MT_THREADS;
        if (idx < words) pre[u] = load4<A16>(wd + 4 * (size_t)idx);
    }
    float part = 0.f;
    for (int s = 0; s < slices; ++s) {
#pragma unroll
        for (int u = 0; u < MT_PRE; ++u) {
            const int idx = tid + u * MT_THREADS;
            if (idx < words) {
                const int c = idx / K4, k4 = idx - c * K4;
                *reinterpret_cast<f4*>(&Ws[c * LDW + 4 * k4]) = pre[u];
            }
        }
        __syncthreads();
        if (s + 1 < slices) {
            const float* next = wd + (size_t)(s + 1) * MT_CH * Cin;
#pragma unroll
            for (int u = 0; u < MT_PRE; ++u) {
                const int idx = tid + u * MT_THREADS;
                if (idx < words) pre[u] = load4<A16>(next + 4 * (size_t)idx);
            }
        }
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float* wa = &Ws[i * LDW + KH * h];
#pragma unroll
        for (int j = 0; j < MT_KMAX / 8; ++j) {
            if (4 * j < KH) {                                     // uniform: Cin is the block's
                const f4 a = *reinterpret_cast<const f4*>(wa + 4 * j);
                const f4 b = xs[j];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
            }
        }
        // accumulator quad q of lane (i, h) = channels cb + 8 q + 4 h .. + 3 of the slice's quadrant, pixel i
        const int quadrant = s / per_quadrant, cb = (s - quadrant * per_quadrant) * MT_CH;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f4 b4 = *reinterpret_cast<const f4*>(&bds[cb + 8 * q + 4 * h]);
            const f4 w4 = load4<A16>(wrow + cb + 8 * q);
            part += fmaxf(acc[4 * q] + b4.x, 0.f) * w4.x;
            part += fmaxf(acc[4 * q + 1] + b4.y, 0.f) * w4.y;
            part += fmaxf(acc[4 * q + 2] + b4.z, 0.f) * w4.z;
            part += fmaxf(acc[4 * q + 3] + b4.w, 0.f) * w4.w;
        }
        if (cb + MT_CH == Cmid) {                                 // the quadrant is complete: the two halves' sums, sigmoid, one store
            const float tot = part + __shfl_xor(part, 32);
            const float v = sigmoid_f32(bmk + tot);
            const int dy = quadrant >> 1, dx = quadrant & 1;
            if (pv && h == 0) out[((size_t)n * 2 * P + 2 * py + dy) * 2 * P + 2 * px + dx] = kv ? v : 0.f;
            part = 0.f;
        }
        __syncthreads();                                          // every wave is done with Ws before the next slice lands
    }
}

// ------------------------------------------------------------------------------------------------ mask paste
constexpr int MP_THREADS = 256, MP_MAX_SIDE = 64, MP_MAX_GRID = 65535;

struct PasteWs {
    size_t bytes, mids, tables, total;      // byte offsets of the three regions; ax / ay ints per detection in the table region
    int ax, ay;
};

__device__ __forceinline__ bool paste_box(const int* __restrict__ boxes, int m, int H, int W, int& y1, int& x1, int& bh, int& bw) {
    const int* b = boxes + 4 * (size_t)m;
    y1 = b[0], x1 = b[1];
    const int y2 = b[2], x2 = b[3];
    bh = y2 - y1, bw = x2 - x1;
    return y1 >= 0 && x1 >= 0 && y2 <= H && x2 <= W && y1 < y2 && x1 < x2;
}

// bytescale(mask) with the mask's own minimum and maximum, in float32 with one rounding per operation
__global__ __launch_bounds__(MP_THREADS) void paste_bytescale_kernel(const float* __restrict__ masks, uint8_t* __restrict__ bytes, int hw) {
#pragma clang fp contract(off)
    __shared__ float lo_s[MP_THREADS / 64], hi_s[MP_THREADS / 64];
    const float* mk = masks + (size_t)blockIdx.x * hw;
    float lo = INFINITY, hi = -INFINITY;
    for (int j = threadIdx.x; j < hw; j += MP_THREADS) {
        const float v = mk[j];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off));
        hi = fmaxf(hi, __shfl_xor(hi, off));
    }
    if ((threadIdx.x & 63) == 0) { lo_s[threadIdx.x >> 6] = lo; hi_s[threadIdx.x >> 6] = hi; }
    __syncthreads();
    lo = lo_s[0], hi = hi_s[0];
#pragma unroll
    for (int wv = 1; wv < MP_THREADS / 64; ++wv) { lo = fminf(lo, lo_s[wv]); hi = fmaxf(hi, hi_s[wv]); }
    float range = hi - lo;
    if (range == 0.f) range = 1.f;
    const float scale = (float)(255.0 / (double)range);
    uint8_t* o = bytes + (size_t)blockIdx.x * hw;
    for (int j = threadIdx.x; j < hw; j += MP_THREADS) {
        float v = (mk[j] - lo) * scale;
        v = v < 0.f ? 0.f : v > 255.f ? 255.f : v;
        o[j] = (uint8_t)(int)(v + 0.5f);
    }
}

__global__ __launch_bounds__(MP_THREADS) void paste_coef_kernel(const int* __restrict__ boxes, int* __restrict__ tables, int h, int w, int H, int W,
                                                               int ax, int ay) {
    const int m = blockIdx.z, axis = blockIdx.y;
    int y1, x1, bh, bw;
    if (!paste_box(boxes, m, H, W, y1, x1, bh, bw)) return;
    const int in_size = axis == 0 ? w : h, out_size = axis == 0 ? bw : bh;
    const int xx = blockIdx.x * MP_THREADS + threadIdx.x;
    if (xx >= out_size) return;
    int* bounds = tables + (size_t)m * (ax + ay) + (axis == 0 ? 0 : ax);
    resize_axis_coefs(in_size, out_size, xx, bounds, bounds + 2 * (size_t)out_size);
}

// mid[m][y][xx] = clip8((1 << 21) + sum_t k[t][xx] * bytes[m][y][xmin + t]) for xx < box width; a row of mid is W bytes apart
__global__ __launch_bounds__(MP_THREADS) void paste_h_kernel(const int* __restrict__ boxes, const int* __restrict__ tables,
                                                            const uint8_t* __restrict__ bytes, uint8_t* __restrict__ mids, int h, int w, int H,
                                                            int W, int ax, int ay) {
    const int m = blockIdx.z, y = blockIdx.y;
    int y1, x1, bh, bw;
    if (!paste_box(boxes, m, H, W, y1, x1, bh, bw)) return;
    const int xx = blockIdx.x * MP_THREADS + threadIdx.x;
    if (xx >= bw) return;
    const int* bounds = tables + (size_t)m * (ax + ay);
    const int* coefs = bounds + 2 * (size_t)bw;
    const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
    const uint8_t* p = bytes + ((size_t)m * h + y) * w + xmin;
    int acc = 1 << (RS_PRECISION_BITS - 1);
    for (int t = 0; t < n; ++t) acc += coefs[(size_t)t * bw + xx] * (int)p[t];
    mids[((size_t)m * h + y) * W + xx] = resize_clip8(acc);
}

// out[m][yy][x] = (vertical pass over mid's column x - x1 at row yy - y1) >= 128 inside the box, 0 outside it
__global__ __launch_bounds__(MP_THREADS) void paste_v_kernel(const int* __restrict__ boxes, const int* __restrict__ tables,
                                                            const uint8_t* __restrict__ mids, uint8_t* __restrict__ out, int h, int H, int W,
                                                            int ax, int ay) {
    const int m = blockIdx.z;
    const int x = blockIdx.x * MP_THREADS + threadIdx.x;
    if (x >= W) return;
    int y1, x1, bh, bw;
    const bool ok = paste_box(boxes, m, H, W, y1, x1, bh, bw);
    const bool in_x = ok && x >= x1 && x < x1 + bw;
    const int* bounds = tables + (size_t)m * (ax + ay) + ax;
    const int* coefs = bounds + 2 * (size_t)(ok ? bh : 0);
    const uint8_t* mid = mids + (size_t)m * h * W + (in_x ? x - x1 : 0);
    uint8_t* o = out + (size_t)m * H * W + x;
    for (int yy = blockIdx.y; yy < H; yy += gridDim.y) {
        const int y = yy - y1;
        uint8_t v = 0;
        if (in_x && y >= 0 && y < bh) {
            const int ymin = bounds[2 * y], n = bounds[2 * y + 1];
            const uint8_t* p = mid + (size_t)ymin * W;
            int acc = 1 << (RS_PRECISION_BITS - 1);
            for (int t = 0; t < n; ++t) acc += coefs[(size_t)t * bh + y] * (int)p[(size_t)t * W];
            v = resize_clip8(acc) >= 128 ? 1 : 0;
        }
        o[(size_t)yy * W] = v;
    }
}

static void paste_layout(int M_, int h, int w, int H, int W, PasteWs* L) {
    const size_t M = (size_t)M_;
    // a table of `out` entries from `in` source samples holds out * (2 + ksize) ints with ksize <= 2 in / out + 3 taps when shrinking
    // and 3 when not: never more than 2 in + 5 out, and out is at most the image's side
    L->ax = 2 * w + 5 * W;
    L->ay = 2 * h + 5 * H;
    L->bytes = 0;
    L->mids = (M * h * w + 15) & ~(size_t)15;
    L->tables = (L->mids + M * h * W + 15) & ~(size_t)15;
    L->total = L->tables + M * ((size_t)L->ax + L->ay) * sizeof(int);
}

static unsigned paste_blocks(int n) { return (unsigned)((n + MP_THREADS - 1) / MP_THREADS); }

// the three launches dc_mask_paste_u8 and dc_mask_rle_u32 share: byte images, both axes' coefficient tables, the horizontal pass
static void paste_front(const float* masks, const int32_t* boxes, int M, int h, int w, int H, int W, const PasteWs& L, uint8_t* base, hipStream_t s) {
    uint8_t* bytes = base + L.bytes;
    uint8_t* mids = base + L.mids;
    int* tables = reinterpret_cast<int*>(base + L.tables);
    const int side = H > W ? H : W;
    hipLaunchKernelGGL(paste_bytescale_kernel, dim3(M), dim3(MP_THREADS), 0, s, masks, bytes, h * w);
    hipLaunchKernelGGL(paste_coef_kernel, dim3(paste_blocks(side), 2, M), dim3(MP_THREADS), 0, s, boxes, tables, h, w, H, W, L.ax, L.ay);
    hipLaunchKernelGGL(paste_h_kernel, dim3(paste_blocks(W), h, M), dim3(MP_THREADS), 0, s, boxes, tables, bytes, mids, h, w, H, W, L.ax, L.ay);
}

static int paste_plan(const dc_mask_paste_desc* d, PasteWs* L) {
    DC_REQUIRE(d, DC_EINVAL, "dc_mask_paste_u8: null descriptor");
    DC_REQUIRE(d->M >= 0 && d->M <= MP_MAX_GRID, DC_EINVAL, "dc_mask_paste_u8: M in 0..%d, got %d", MP_MAX_GRID, d->M);
    DC_REQUIRE(d->h >= 1 && d->h <= MP_MAX_SIDE && d->w >= 1 && d->w <= MP_MAX_SIDE, DC_EINVAL,
               "dc_mask_paste_u8: a mask of 1 x 1 to %d x %d, got %d x %d", MP_MAX_SIDE, MP_MAX_SIDE, d->h, d->w);
    DC_REQUIRE(d->H >= 1 && d->W >= 1 && d->H <= (1 << 24) && d->W <= (1 << 24) && (size_t)d->H * d->W < ((size_t)1 << 31), DC_EINVAL,
               "dc_mask_paste_u8: an image of at least 1 x 1, sides of at most 2^24 and fewer than 2^31 pixels, got %d x %d", d->H, d->W);
    DC_REQUIRE(d->M == 0 || (d->masks && d->boxes && d->out), DC_EINVAL, "dc_mask_paste_u8: null masks, boxes or output");
    DC_REQUIRE((reinterpret_cast<uintptr_t>(d->masks) & 3u) == 0 && (reinterpret_cast<uintptr_t>(d->boxes) & 3u) == 0, DC_EINVAL,
               "dc_mask_paste_u8: masks (float32) and boxes (int32) must sit on 4-byte boundaries");
    paste_layout(d->M, d->h, d->w, d->H, d->W, L);
    return DC_OK;
}

// ------------------------------------------------------------------------------------------------ mask run lengths
// The plane of detection m is never stored.  Slot s of a detection is column x1 + s of its box for s < bw, and for s = bw the column
// right of the box, which can hold one transition only (the end of a run of ones that reaches the image's last row).  Slots are
// numbered 0..W per detection whatever the box is (the host cannot know the boxes); those behind the box count zero.
constexpr int RL_THREADS = 256, RL_WAVES = RL_THREADS / 64, RL_DIFF_BLOCKS = 8;

struct RleWs {
    PasteWs paste;
    size_t slots, totals, pos, total;      // byte offsets: int [M][W + 1], int [M], uint32 [capacity]
};

// One wave per (detection, slot).  COUNT: slot_n[m][s] = the slot's transitions.  Otherwise slot_n holds the exclusive prefix sums
// within the detection and transition j of the slot stores its pixel index at pos[offsets[m] + slot_n[m][s] + j], below capacity only.
template <bool COUNT>
__global__ __launch_bounds__(RL_THREADS) void rle_walk_kernel(const int* __restrict__ boxes, const int* __restrict__ tables,
                                                             const uint8_t* __restrict__ mids, int* __restrict__ slot_n,
                                                             const int* __restrict__ offsets, uint32_t* __restrict__ pos, int capacity, int h,
                                                             int H, int W, int ax, int ay) {
    const int m = blockIdx.z, lane = threadIdx.x & 63;
    const int s = blockIdx.x * RL_WAVES + (threadIdx.x >> 6);
    if (s > W) return;                                            // whole waves leave: the ballots below see full waves
    int y1, x1, bh, bw;
    const bool ok = paste_box(boxes, m, H, W, y1, x1, bh, bw);
    int* const mine = slot_n + (size_t)m * (W + 1) + s;
    if (!ok || s > bw || (s == bw && x1 + bw == W)) {             // (wave-uniform)
        if (COUNT && lane == 0) *mine = 0;
        return;
    }
    const int* bounds = tables + (size_t)m * (ax + ay) + ax;
    const int* coefs = bounds + 2 * (size_t)bh;
    const uint8_t* mid = mids + (size_t)m * h * W;
    // paste_v_kernel's arithmetic for box pixel (y, xx)
    auto bit = [&](int y, int xx) -> bool {
        const int ymin = bounds[2 * y], n = bounds[2 * y + 1];
        const uint8_t* p = mid + (size_t)ymin * W + xx;
        int acc = 1 << (RS_PRECISION_BITS - 1);
        for (int t = 0; t < n; ++t) acc += coefs[(size_t)t * bh + y] * (int)p[(size_t)t * W];
        return resize_clip8(acc) >= 128;
    };
    // the pixel before this column's first: the last row of the column to the left, set only where the box reaches that row
    const bool pred = s > 0 && y1 + bh == H && bit(bh - 1, s - 1);
    const int base = (x1 + s) * H;                                // (x1 + s < W here: below H * W < 2^31)
    const int at = COUNT ? 0 : offsets[m] + *mine;
    auto store = [&](int j, int index) {
        if (at + j < capacity) pos[at + j] = (uint32_t)index;
    };
    int n = 0;
    if (s == bw || y1 > 0) {                                      // row 0 of this column is outside the box: a zero
        if (pred) {
            if (!COUNT && lane == 0) store(0, base);
            n = 1;
        }
    }
    if (s < bw) {
        unsigned long long carry = y1 > 0 ? 0ull : (unsigned long long)pred;
        const int rows = bh + 1 < H - y1 ? bh + 1 : H - y1;      // box rows, and the zero below the box where the image has that row
        for (int y0 = 0; y0 < rows; y0 += 64) {
            const int y = y0 + lane;
            const unsigned long long bits = __ballot(y < bh && bit(y, s));
            const unsigned long long valid = rows - y0 >= 64 ? ~0ull : (1ull << (rows - y0)) - 1;
            const unsigned long long trans = (bits ^ ((bits << 1) | carry)) & valid;
            carry = bits >> 63;
            if (!COUNT && ((trans >> lane) & 1)) store(n + __popcll(trans & ((1ull << lane) - 1)), base + y1 + y);
            n += __popcll(trans);
        }
    }
    if (COUNT && lane == 0) *mine = n;
}

// exclusive prefix sum of one value per thread over the block, and the block's total; part holds RL_WAVES ints
__device__ __forceinline__ int rle_block_scan(int v, int* part, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(x, off);
        if (lane >= off) x += up;
    }
    if (lane == 63) part[wave] = x;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int wv = 0; wv < RL_WAVES; ++wv) {
        if (wv < wave) before += part[wv];
        total += part[wv];
    }
    __syncthreads();                                              // part is free again
    return before + x - v;
}

// block m: slot_n[m][0..W] becomes its own exclusive prefix sums, totals[m] the detection's transitions
__global__ __launch_bounds__(RL_THREADS) void rle_scan_slots_kernel(int* __restrict__ slot_n, int* __restrict__ totals, int W) {
    __shared__ int part[RL_WAVES];
    int* row = slot_n + (size_t)blockIdx.x * (W + 1);
    int carry = 0;
    for (int c0 = 0; c0 <= W; c0 += RL_THREADS) {
        const int i = c0 + threadIdx.x;
        int total;
        const int e = rle_block_scan(i <= W ? row[i] : 0, part, total);
        if (i <= W) row[i] = carry + e;
        carry += total;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// one block: offsets[m] = the entries of the detections before m, each its transitions + 1
__global__ __launch_bounds__(RL_THREADS) void rle_scan_dets_kernel(const int* __restrict__ totals, int* __restrict__ offsets, int M) {
    __shared__ int part[RL_WAVES];
    int carry = 0;
    for (int c0 = 0; c0 < M; c0 += RL_THREADS) {
        const int i = c0 + threadIdx.x;
        int total;
        const int e = rle_block_scan(i < M ? totals[i] + 1 : 0, part, total);
        if (i < M) offsets[i] = carry + e;
        carry += total;
    }
    if (threadIdx.x == 0) offsets[M] = carry;
}

// counts[j] = t - t' with t the position at j (H W at a detection's last entry) and t' the one before (0 at its first)
__global__ __launch_bounds__(RL_THREADS) void rle_diff_kernel(const int* __restrict__ offsets, const uint32_t* __restrict__ pos,
                                                             uint32_t* __restrict__ counts, int capacity, int HW) {
    const int m = blockIdx.y;
    const int lo = offsets[m], hi = offsets[m + 1];
    const int end = hi < capacity ? hi : capacity;
    for (int j = lo + blockIdx.x * RL_THREADS + threadIdx.x; j < end; j += gridDim.x * RL_THREADS) {
        const uint32_t t = j == hi - 1 ? (uint32_t)HW : pos[j];
        counts[j] = t - (j == lo ? 0u : pos[j - 1]);
    }
}

static int rle_plan(const dc_mask_rle_desc* d, RleWs* L) {
    DC_REQUIRE(d, DC_EINVAL, "dc_mask_rle_u32: null descriptor");
    DC_REQUIRE(d->M >= 0 && d->M <= MP_MAX_GRID, DC_EINVAL, "dc_mask_rle_u32: M in 0..%d, got %d", MP_MAX_GRID, d->M);
    DC_REQUIRE(d->h >= 1 && d->h <= MP_MAX_SIDE && d->w >= 1 && d->w <= MP_MAX_SIDE, DC_EINVAL,
               "dc_mask_rle_u32: a mask of 1 x 1 to %d x %d, got %d x %d", MP_MAX_SIDE, MP_MAX_SIDE, d->h, d->w);
    DC_REQUIRE(d->H >= 1 && d->W >= 1 && d->H <= (1 << 24) && d->W <= (1 << 24) && (size_t)d->H * d->W < ((size_t)1 << 31), DC_EINVAL,
               "dc_mask_rle_u32: an image of at least 1 x 1, sides of at most 2^24 and fewer than 2^31 pixels, got %d x %d", d->H, d->W);
    DC_REQUIRE((size_t)d->M * ((size_t)d->H * d->W + 1) < ((size_t)1 << 31), DC_EINVAL,
               "dc_mask_rle_u32: M * (H * W + 1) must stay below 2^31 (the int32 offsets), got M %d, %d x %d", d->M, d->H, d->W);
    DC_REQUIRE(d->capacity >= 0, DC_EINVAL, "dc_mask_rle_u32: capacity must not be negative, got %d", d->capacity);
    DC_REQUIRE(d->offsets && (d->counts || d->capacity == 0), DC_EINVAL, "dc_mask_rle_u32: null offsets or counts");
    DC_REQUIRE(d->M == 0 || (d->masks && d->boxes), DC_EINVAL, "dc_mask_rle_u32: null masks or boxes");
    DC_REQUIRE(((reinterpret_cast<uintptr_t>(d->masks) | reinterpret_cast<uintptr_t>(d->boxes) | reinterpret_cast<uintptr_t>(d->offsets) |
                 reinterpret_cast<uintptr_t>(d->counts)) & 3u) == 0, DC_EINVAL,
               "dc_mask_rle_u32: masks (float32), boxes and offsets (int32) and counts (uint32) must sit on 4-byte boundaries");
    const size_t M = (size_t)d->M;
    paste_layout(d->M, d->h, d->w, d->H, d->W, &L->paste);
    L->slots = (L->paste.total + 15) & ~(size_t)15;
    L->totals = L->slots + ((M * ((size_t)d->W + 1) * sizeof(int) + 15) & ~(size_t)15);
    L->pos = L->totals + ((M * sizeof(int) + 15) & ~(size_t)15);
    L->total = L->pos + (size_t)d->capacity * sizeof(uint32_t);
    return DC_OK;
}

}  // namespace dcap

using namespace dcap;

extern "C" int dc_class_select_f32(const float* logits, int ld_logits, const float* deltas, int ld_deltas, int R, int C, int32_t* class_ids,
                                   float* scores, float* deltas_out, void* stream) {
    DC_REQUIRE(logits && deltas && class_ids && scores && deltas_out, DC_EINVAL, "dc_class_select_f32: null logits, deltas or output");
    DC_REQUIRE(R >= 1 && C >= 2 && C <= (1 << 24), DC_EINVAL, "dc_class_select_f32: R >= 1 and C in 2..2^24, got R %d, C %d", R, C);
    DC_REQUIRE(R <= INT_MAX - CS_ROWS, DC_EINVAL, "dc_class_select_f32: R %d is too large", R);
    DC_REQUIRE((long)ld_logits >= C && (long)ld_deltas >= 4L * C, DC_EINVAL,
               "dc_class_select_f32: row strides below the row lengths (logits %d < %d or deltas %d < %ld)", ld_logits, C, ld_deltas, 4L * C);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(deltas) | reinterpret_cast<uintptr_t>(class_ids) |
                           reinterpret_cast<uintptr_t>(scores) | reinterpret_cast<uintptr_t>(deltas_out);
    DC_REQUIRE((bits & 3u) == 0, DC_EINVAL, "dc_class_select_f32: every pointer must sit on a 4-byte boundary");
    hipLaunchKernelGGL(class_select_kernel, dim3((R + CS_ROWS - 1) / CS_ROWS), dim3(CS_THREADS), 0, static_cast<hipStream_t>(stream), logits,
                       ld_logits, deltas, ld_deltas, R, C, class_ids, scores, deltas_out);
    return check_launch("class_select_kernel");
}

extern "C" int dc_mask_head_tail_f32(const dc_mask_head_tail_desc* d, void* stream) {
    DC_REQUIRE(d && d->x && d->wd && d->bd && d->wm_t && d->bm && d->class_ids && d->out, DC_EINVAL,
               "dc_mask_head_tail_f32: null descriptor, input, weights, class ids or output");
    DC_REQUIRE(d->N >= 1 && d->P >= 1 && d->P <= 16 && d->C >= 1, DC_EINVAL, "dc_mask_head_tail_f32: N >= 1, P in 1..16, C >= 1, got N %d, P %d, C %d",
               d->N, d->P, d->C);
    DC_REQUIRE(d->Cin >= 32 && d->Cin <= MT_KMAX && d->Cin % 32 == 0, DC_EINVAL,
               "dc_mask_head_tail_f32: Cin must be a multiple of 32 in 32..%d (a lane keeps half a pixel's inputs in registers), got %d", MT_KMAX,
               d->Cin);
    DC_REQUIRE(d->Cmid >= 32 && d->Cmid <= 4096 && d->Cmid % 32 == 0, DC_EINVAL, "dc_mask_head_tail_f32: Cmid must be a multiple of 32 in 32..4096, got %d",
               d->Cmid);
    const size_t rows = (size_t)d->N * d->P * d->P;
    DC_REQUIRE(rows < ((size_t)1 << 31) - MT_ROWS, DC_EINVAL, "dc_mask_head_tail_f32: N * P * P = %zu rows must stay below 2^31", rows);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(d->x) | reinterpret_cast<uintptr_t>(d->wd) | reinterpret_cast<uintptr_t>(d->wm_t) |
                           reinterpret_cast<uintptr_t>(d->bd) | reinterpret_cast<uintptr_t>(d->bm) | reinterpret_cast<uintptr_t>(d->class_ids) |
                           reinterpret_cast<uintptr_t>(d->out);
    DC_REQUIRE((bits & 3u) == 0, DC_EINVAL, "dc_mask_head_tail_f32: every pointer must sit on a 4-byte boundary");
    const bool a16 = aligned16(d->x) && aligned16(d->wd) && aligned16(d->wm_t);      // rows are multiples of 32 floats: the bases decide
    const size_t lds = ((size_t)MT_CH * (d->Cin + 4) + d->Cmid) * sizeof(float);
    const unsigned blocks = (unsigned)((rows + MT_ROWS - 1) / MT_ROWS);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int M = (int)rows;
    if (a16)
        hipLaunchKernelGGL(mask_head_tail_kernel<true>, dim3(blocks), dim3(MT_THREADS), lds, s, d->x, d->wd, d->bd, d->wm_t, d->bm, d->class_ids,
                           d->out, M, d->P, d->Cin, d->Cmid, d->C);
    else
        hipLaunchKernelGGL(mask_head_tail_kernel<false>, dim3(blocks), dim3(MT_THREADS), lds, s, d->x, d->wd, d->bd, d->wm_t, d->bm, d->class_ids,
                           d->out, M, d->P, d->Cin, d->Cmid, d->C);
    return check_launch("mask_head_tail_kernel");
}

extern "C" size_t dc_mask_paste_u8_workspace_bytes(const dc_mask_paste_desc* d) {
    PasteWs L;
    if (paste_plan(d, &L)) return 0;
    return L.total;
}

extern "C" int dc_mask_paste_u8(const dc_mask_paste_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    PasteWs L;
    int rc = paste_plan(d, &L);
    if (rc) return rc;
    if (d->M == 0) return DC_OK;
    DC_REQUIRE(workspace && workspace_bytes >= L.total && aligned16(workspace), DC_EWORKSPACE,
               "dc_mask_paste_u8: needs %zu workspace bytes (16-byte aligned), got %zu", L.total, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* base = static_cast<uint8_t*>(workspace);
    paste_front(d->masks, d->boxes, d->M, d->h, d->w, d->H, d->W, L, base, s);
    hipLaunchKernelGGL(paste_v_kernel, dim3(paste_blocks(d->W), d->H < MP_MAX_GRID ? d->H : MP_MAX_GRID, d->M), dim3(MP_THREADS), 0, s, d->boxes,
                       reinterpret_cast<int*>(base + L.tables), base + L.mids, d->out, d->h, d->H, d->W, L.ax, L.ay);
    return check_launch("mask_paste kernels");
}

extern "C" size_t dc_mask_rle_workspace_bytes(const dc_mask_rle_desc* d) {
    RleWs L;
    if (rle_plan(d, &L)) return 0;
    return L.total;
}

extern "C" int dc_mask_rle_u32(const dc_mask_rle_desc* d, void* stream) {
    RleWs L;
    int rc = rle_plan(d, &L);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int M = d->M;
    if (M == 0) {
        const hipError_t e = hipMemsetAsync(d->offsets, 0, sizeof(int32_t), s);
        DC_REQUIRE(e == hipSuccess, DC_ELAUNCH, "dc_mask_rle_u32: hipMemsetAsync: %s", hipGetErrorString(e));
        return DC_OK;
    }
    DC_REQUIRE(d->workspace && d->workspace_bytes >= L.total && aligned16(d->workspace), DC_EWORKSPACE,
               "dc_mask_rle_u32: needs %zu workspace bytes (16-byte aligned), got %zu", L.total, d->workspace_bytes);
    uint8_t* base = static_cast<uint8_t*>(d->workspace);
    const int* tables = reinterpret_cast<const int*>(base + L.paste.tables);
    const uint8_t* mids = base + L.paste.mids;
    int* slot_n = reinterpret_cast<int*>(base + L.slots);
    int* totals = reinterpret_cast<int*>(base + L.totals);
    uint32_t* pos = reinterpret_cast<uint32_t*>(base + L.pos);
    paste_front(d->masks, d->boxes, M, d->h, d->w, d->H, d->W, L.paste, base, s);
    const dim3 walk((unsigned)((d->W + 1 + RL_WAVES - 1) / RL_WAVES), 1, M);
    hipLaunchKernelGGL(rle_walk_kernel<true>, walk, dim3(RL_THREADS), 0, s, d->boxes, tables, mids, slot_n, d->offsets, pos, d->capacity, d->h, d->H,
                       d->W, L.paste.ax, L.paste.ay);
    hipLaunchKernelGGL(rle_scan_slots_kernel, dim3(M), dim3(RL_THREADS), 0, s, slot_n, totals, d->W);
    hipLaunchKernelGGL(rle_scan_dets_kernel, dim3(1), dim3(RL_THREADS), 0, s, totals, d->offsets, M);
    hipLaunchKernelGGL(rle_walk_kernel<false>, walk, dim3(RL_THREADS), 0, s, d->boxes, tables, mids, slot_n, d->offsets, pos, d->capacity, d->h,
                       d->H, d->W, L.paste.ax, L.paste.ay);
    hipLaunchKernelGGL(rle_diff_kernel, dim3(RL_DIFF_BLOCKS, M), dim3(RL_THREADS), 0, s, d->offsets, pos, d->counts, d->capacity, d->H * d->W);
    return check_launch("mask_rle kernels");
}

// RPN training targets on the device: build_rpn_targets (dense_img_cap/dense_model.py:1095-1183) for a batch of images, written in the
// packed form dc_rpn_loss_grad_f32 reads (counts, level / index / match of the chosen anchors, the positives' delta rows).
//
// Per image: the float64 IoU of every pyramid anchor against every ground-truth box with compute_overlaps' operations in its order
// (each rounded once: contraction is off for this file, as in proposal.hip), the first argmax per anchor, negatives below 0.3, every
// anchor that attains a box's column maximum positive (a column maximum of 0 claims every anchor with IoU 0, as on the host), 0.7 and
// above positive.  np.random.choice is replaced by counter-based keys: key(a) = Philox-2x32-10(a, offset, seed); the budget / 2
// positives and the budget - (positives kept) negatives with the smallest (key, a) pairs stay, the rest becomes neutral.
//
// A chain of eight small launches on the caller's stream (blockIdx.y = image, one thread per anchor), no grid barrier, no host read:
//   1 column-max partials   per block and box: the maximum IoU of the block's 256 anchors        (also clears the histograms)
//   2 column-max finish     per box: the maximum of the partials (a maximum does not depend on the order)
//   3 classify              per anchor: best box, class; histogram of the top key byte per class
//   4-6 radix passes        histogram of the next key byte among the keys that share the prefix chosen so far
//   7 count                 per block: chosen-for-sure and on-the-threshold anchors per class
//   8 write                 ordered compaction: output slot = chosen anchors before this one (earlier images, blocks, lanes)
// Every pass after the third starts by picking the previous pass's byte from its finished histogram (every block repeats the same
// 256-bin scan; block 0 stores the result for the next launch).  Histograms are integer atomics: order-independent, so two calls
// give identical bits.  The number of boxes is a device word per image; no launch shape depends on it.
#include "dcap_internal.h"

#pragma clang fp contract(off)

using namespace dcap;

namespace {

constexpr int RT_THREADS = 256, RT_WAVES = RT_THREADS / 64, RT_MAX_GT = 512, RT_MAX_BUDGET = 1024, RT_MAX_BATCH = 64, RT_PASSES = 4;
constexpr unsigned RT_IMAGE_SEED_STEP = 0x85EBCA6Bu;      // image b draws from key seed + b * this (as the detection targets' keys do)

// Radix-select state of one image after a pass, per class (0 positive, 1 negative): the key prefix chosen so far, how many of the keys
// that share it are still to be taken, and k = the class's final count.
struct RtState {
    unsigned prefix[2];
    int need[2];
    int k[2];
    int pad[2];
};

struct RtWorkspace {
    double* partial;      // [B][nblk][cap]
    double* colmax;       // [B][cap]
    int* info;            // [B][A]  best_gt * 4 + (class + 1)
    int* hist;            // [B][RT_PASSES][2][256]
    RtState* state;       // [B][RT_PASSES + 1]
    int* blockcnt;        // [B][nblk][4]
};

inline int rt_blocks(int A) { return (A + RT_THREADS - 1) / RT_THREADS; }

size_t rt_layout(const dc_rpn_targets_desc* d, void* base, RtWorkspace* w) {
    const size_t B = d->B, nblk = rt_blocks(d->A), cap = d->gt_capacity, A = d->A;
    size_t off = 0;
    char* p = static_cast<char*>(base);
    auto take = [&](size_t bytes) {
        char* q = p ? p + off : nullptr;
        off += (bytes + 15) / 16 * 16;
        return q;
    };
    double* partial = reinterpret_cast<double*>(take(B * nblk * cap * sizeof(double)));
    double* colmax = reinterpret_cast<double*>(take(B * cap * sizeof(double)));
    int* info = reinterpret_cast<int*>(take(B * A * sizeof(int)));
    int* hist = reinterpret_cast<int*>(take(B * RT_PASSES * 512 * sizeof(int)));
    RtState* state = reinterpret_cast<RtState*>(take(B * (RT_PASSES + 1) * sizeof(RtState)));
    int* blockcnt = reinterpret_cast<int*>(take(B * nblk * 4 * sizeof(int)));
    if (w) *w = RtWorkspace{partial, colmax, info, hist, state, blockcnt};
    return off;
}

// compute_overlaps (utils.compute_overlaps of the reference) for one pair: min, max, subtract, clip at 0, multiply, add, divide.
__device__ __forceinline__ double rt_iou(double a0, double a1, double a2, double a3, double area_a, const double* g) {
    const double g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3];
    double ih = (a2 < g2 ? a2 : g2) - (a0 > g0 ? a0 : g0);
    ih = ih > 0.0 ? ih : 0.0;
    double iw = (a3 < g3 ? a3 : g3) - (a1 > g1 ? a1 : g1);
    iw = iw > 0.0 ? iw : 0.0;
    const double inter = ih * iw;
    const double area_g = (g2 - g0) * (g3 - g1);
    return inter / (area_a + area_g - inter);
}

__device__ __forceinline__ double rt_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double t = __shfl_xor(v, o);
        v = t > v ? t : v;
    }
    return v;
}

__device__ __forceinline__ int rt_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int rt_box_count(const dc_rpn_targets_desc& d, int b) {
    const int g = d.gt_counts[b];
    return g < 0 ? 0 : (g > d.gt_capacity ? d.gt_capacity : g);
}

__device__ __forceinline__ unsigned rt_key(const dc_rpn_targets_desc& d, int b, int a) {
    const unsigned offset = d.offset + (d.offset_dev ? d.offset_dev[0] : 0u);
    return philox2x32((unsigned)a, offset, d.seed + (unsigned)b * RT_IMAGE_SEED_STEP);
}

// Inclusive scan over the block's 256 values; s[0..255] holds the result until the caller's next barrier.
__device__ __forceinline__ int rt_scan256(int v, int* s) {
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int o = 1; o < RT_THREADS; o <<= 1) {
        const int t = tid >= o ? s[tid - o] : 0;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
    return s[tid];
}

// The byte of the finished histogram `hist` ([2][256], the pass behind `prev`; prev == nullptr: the first pass, whose totals also
// fix how many of each class are kept) that holds the need-th smallest key, per class.  s: 258 ints of LDS.  The same in every block.
__device__ RtState rt_pick(const int* hist, const RtState* prev, int budget, int* s) {
    const int tid = threadIdx.x;
    RtState st;
    st.pad[0] = st.pad[1] = 0;
    for (int c = 0; c < 2; ++c) {
        const int h = hist[c * 256 + tid];
        const int cum = rt_scan256(h, s);
        const int total = s[RT_THREADS - 1];
        int need;
        unsigned prefix;
        if (prev == nullptr) {
            const int room = c == 0 ? budget / 2 : budget - st.k[0];
            st.k[c] = need = total < room ? total : room;
            prefix = 0u;
        } else {
            need = prev->need[c];
            prefix = prev->prefix[c];
            st.k[c] = prev->k[c];
        }
        __syncthreads();
        const bool chosen = need == 0 ? tid == 0 : (cum >= need && cum - h < need);
        if (chosen) {
            s[256] = tid;
            s[257] = need == 0 ? 0 : need - (cum - h);
        }
        __syncthreads();
        st.prefix[c] = (prefix << 8) | (unsigned)s[256];
        st.need[c] = s[257];
        __syncthreads();
    }
    return st;
}

__device__ __forceinline__ void rt_flush_hist(const int* lds, int* global) {
    for (int i = threadIdx.x; i < 512; i += RT_THREADS)
        if (lds[i]) atomicAdd(&global[i], lds[i]);
}

__global__ __launch_bounds__(RT_THREADS) void rt_colmax_partial_kernel(dc_rpn_targets_desc d, RtWorkspace w, int nblk) {
    __shared__ double box[RT_MAX_GT * 4];
    __shared__ double wmax[RT_WAVES][RT_MAX_GT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, cap = d.gt_capacity;
    const int G = rt_box_count(d, b);
    if (blockIdx.x == 0)
        for (int i = tid; i < RT_PASSES * 512; i += RT_THREADS) w.hist[(size_t)b * RT_PASSES * 512 + i] = 0;
    for (int i = tid; i < G * 4; i += RT_THREADS) box[i] = d.gt_boxes[(size_t)b * cap * 4 + i];
    __syncthreads();
    const int a = blockIdx.x * RT_THREADS + tid;
    const bool valid = a < d.A;                                        // the last block's tail
    const double* an = d.anchors + (size_t)(valid ? a : d.A - 1) * 4;
    const double a0 = an[0], a1 = an[1], a2 = an[2], a3 = an[3];
    const double area_a = (a2 - a0) * (a3 - a1);
    for (int g = 0; g < G; ++g) {
        const double v = rt_wave_max(valid ? rt_iou(a0, a1, a2, a3, area_a, box + 4 * g) : -1.0);
        if (lane == 0) wmax[wave][g] = v;
    }
    __syncthreads();
    for (int g = tid; g < G; g += RT_THREADS) {
        double m = wmax[0][g];
#pragma unroll
        for (int k = 1; k < RT_WAVES; ++k) m = wmax[k][g] > m ? wmax[k][g] : m;
        w.partial[((size_t)b * nblk + blockIdx.x) * cap + g] = m;
    }
}

__global__ __launch_bounds__(RT_THREADS) void rt_colmax_finish_kernel(dc_rpn_targets_desc d, RtWorkspace w, int nblk) {
    __shared__ double red[RT_WAVES];
    const int tid = threadIdx.x, g = blockIdx.x, b = blockIdx.y, cap = d.gt_capacity;
    if (g >= rt_box_count(d, b)) return;                               // (the whole block)
    double m = -1.0;
    for (int k = tid; k < nblk; k += RT_THREADS) {
        const double v = w.partial[((size_t)b * nblk + k) * cap + g];
        m = v > m ? v : m;
    }
    m = rt_wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < RT_WAVES; ++k) m = red[k] > m ? red[k] : m;
        w.colmax[(size_t)b * cap + g] = m;
    }
}

__global__ __launch_bounds__(RT_THREADS) void rt_classify_kernel(dc_rpn_targets_desc d, RtWorkspace w) {
    __shared__ double box[RT_MAX_GT * 4];
    __shared__ double cmax[RT_MAX_GT];
    __shared__ int hist[512];
    const int tid = threadIdx.x, b = blockIdx.y, cap = d.gt_capacity;
    const int G = rt_box_count(d, b);
    for (int i = tid; i < G * 4; i += RT_THREADS) box[i] = d.gt_boxes[(size_t)b * cap * 4 + i];
    for (int i = tid; i < G; i += RT_THREADS) cmax[i] = w.colmax[(size_t)b * cap + i];
    for (int i = tid; i < 512; i += RT_THREADS) hist[i] = 0;
    __syncthreads();
    const int a = blockIdx.x * RT_THREADS + tid;
    if (a < d.A) {
        const double* an = d.anchors + (size_t)a * 4;
        const double a0 = an[0], a1 = an[1], a2 = an[2], a3 = an[3];
        const double area_a = (a2 - a0) * (a3 - a1);
        double best = 0.0;
        int bg = 0;
        bool claimed = false;
        for (int g = 0; g < G; ++g) {
            const double iou = rt_iou(a0, a1, a2, a3, area_a, box + 4 * g);
            if (g == 0 || iou > best) {                                // the first maximum (np.argmax)
                best = iou;
                bg = g;
            }
            claimed = claimed || iou == cmax[g];                       // the same instructions produced cmax: equal means equal
        }
        int cls = -1;                                                  // no box at all: every anchor is a negative
        if (G > 0) {
            cls = best < 0.3 ? -1 : 0;
            if (claimed || best >= 0.7) cls = 1;
        }
        w.info[(size_t)b * d.A + a] = bg * 4 + (cls + 1);
        if (cls != 0) atomicAdd(&hist[(cls == 1 ? 0 : 256) + (int)(rt_key(d, b, a) >> 24)], 1);
    }
    __syncthreads();
    rt_flush_hist(hist, w.hist + (size_t)b * RT_PASSES * 512);
}

// Radix pass p (1..3): picks pass p - 1's byte, then counts byte p of the keys that share the prefix.
__global__ __launch_bounds__(RT_THREADS) void rt_radix_kernel(dc_rpn_targets_desc d, RtWorkspace w, int p) {
    __shared__ int s[258];
    __shared__ int hist[512];
    const int tid = threadIdx.x, b = blockIdx.y;
    int* hist_b = w.hist + (size_t)b * RT_PASSES * 512;
    RtState* state_b = w.state + (size_t)b * (RT_PASSES + 1);
    const RtState st = rt_pick(hist_b + (p - 1) * 512, p == 1 ? nullptr : state_b + (p - 1), d.budget, s);
    if (blockIdx.x == 0 && tid == 0) state_b[p] = st;
    for (int i = tid; i < 512; i += RT_THREADS) hist[i] = 0;
    __syncthreads();
    const int a = blockIdx.x * RT_THREADS + tid;
    if (a < d.A) {
        const int cls = (w.info[(size_t)b * d.A + a] & 3) - 1;
        if (cls != 0) {
            const int c = cls == 1 ? 0 : 1, shift = 32 - 8 * p;
            const unsigned key = rt_key(d, b, a);
            if ((key >> shift) == st.prefix[c]) atomicAdd(&hist[c * 256 + (int)((key >> (shift - 8)) & 255u)], 1);
        }
    }
    __syncthreads();
    rt_flush_hist(hist, hist_b + p * 512);
}

// The four conditions of an anchor against the final thresholds: {positive below, positive on, negative below, negative on}.
__device__ __forceinline__ void rt_flags(const dc_rpn_targets_desc& d, const RtState& st, int b, int a, int info, bool valid, bool f[4]) {
    const int cls = valid ? (info & 3) - 1 : 0;
    const unsigned key = cls != 0 ? rt_key(d, b, a) : 0u;
    f[0] = cls == 1 && key < st.prefix[0];
    f[1] = cls == 1 && key == st.prefix[0];
    f[2] = cls == -1 && key < st.prefix[1];
    f[3] = cls == -1 && key == st.prefix[1];
}

__global__ __launch_bounds__(RT_THREADS) void rt_count_kernel(dc_rpn_targets_desc d, RtWorkspace w, int nblk) {
    __shared__ int s[258];
    __shared__ int wc[RT_WAVES][4];
    const int tid = threadIdx.x, b = blockIdx.y;
    RtState* state_b = w.state + (size_t)b * (RT_PASSES + 1);
    const RtState st = rt_pick(w.hist + ((size_t)b * RT_PASSES + (RT_PASSES - 1)) * 512, state_b + (RT_PASSES - 1), d.budget, s);
    if (blockIdx.x == 0 && tid == 0) state_b[RT_PASSES] = st;
    const int a = blockIdx.x * RT_THREADS + tid;
    const bool valid = a < d.A;
    bool f[4];
    rt_flags(d, st, b, a, valid ? w.info[(size_t)b * d.A + a] : 0, valid, f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = __popcll(__ballot(f[j]));
        if ((tid & 63) == 0) wc[tid >> 6][j] = n;
    }
    __syncthreads();
    if (tid < 4) {
        int n = 0;
#pragma unroll
        for (int k = 0; k < RT_WAVES; ++k) n += wc[k][tid];
        w.blockcnt[((size_t)b * nblk + blockIdx.x) * 4 + tid] = n;
    }
}

__global__ __launch_bounds__(RT_THREADS) void rt_write_kernel(dc_rpn_targets_desc d, RtWorkspace w, int nblk) {
    __shared__ int red[RT_WAVES][4];
    __shared__ int wc[RT_WAVES][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const RtState st = w.state[(size_t)b * (RT_PASSES + 1) + RT_PASSES];
    // what the earlier images and all images chose
    int sel_base = 0, pos_base = 0, sel_all = 0, pos_all = 0;
    for (int i = 0; i < d.B; ++i) {
        const RtState* si = w.state + (size_t)i * (RT_PASSES + 1) + RT_PASSES;
        const int kp = si->k[0], kn = si->k[1];
        if (i < b) {
            sel_base += kp + kn;
            pos_base += kp;
        }
        sel_all += kp + kn;
        pos_all += kp;
    }
    // ... and the earlier blocks of this image
    int before[4] = {0, 0, 0, 0};
    for (int k = tid; k < (int)blockIdx.x; k += RT_THREADS) {
        const int* c = w.blockcnt + ((size_t)b * nblk + k) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) before[j] += c[j];
    }
    const int a = blockIdx.x * RT_THREADS + tid;
    const bool valid = a < d.A;
    const int info = valid ? w.info[(size_t)b * d.A + a] : 0;
    bool f[4];
    rt_flags(d, st, b, a, info, valid, f);
    unsigned long long bal[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        before[j] = rt_wave_sum(before[j]);
        bal[j] = __ballot(f[j]);
        if (lane == 0) {
            red[wave][j] = before[j];
            wc[wave][j] = __popcll(bal[j]);
        }
    }
    __syncthreads();
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int n = 0;
#pragma unroll
        for (int k = 0; k < RT_WAVES; ++k) n += red[k][j] + (k < wave ? wc[k][j] : 0);
        before[j] = n + __popcll(bal[j] & below);
    }
    const int rp = st.need[0], rn = st.need[1];
    const bool take = f[0] || (f[1] && before[1] < rp) || f[2] || (f[3] && before[3] < rn);
    const int pos_before = before[0] + (before[1] < rp ? before[1] : rp);
    const int o = sel_base + pos_before + before[2] + (before[3] < rn ? before[3] : rn);
    if (take && o < d.B * d.budget) {                                  // (o < sel_base + k[0] + k[1] by construction; the bound costs nothing)
        int level = 0, start = 0;
        while (level + 1 < d.n_levels && a >= start + d.level_sizes[level]) start += d.level_sizes[level++];
        const int cls = (info & 3) - 1;
        d.sel_level[o] = level;
        d.sel_index[o] = a - start + b * d.level_sizes[level];
        d.sel_match[o] = cls;
        if (cls == 1) {
            const double* an = d.anchors + (size_t)a * 4;
            const double* g = d.gt_boxes + ((size_t)b * d.gt_capacity + (info >> 2)) * 4;
            const double a0 = an[0], a1 = an[1], g0 = g[0], g1 = g[1];
            const double ah = an[2] - a0, aw = an[3] - a1, gh = g[2] - g0, gw = g[3] - g1;
            float* row = d.deltas + (size_t)(pos_base + pos_before) * 4;
            row[0] = (float)((((g0 + 0.5 * gh) - (a0 + 0.5 * ah)) / ah) / d.std_dev[0]);
            row[1] = (float)((((g1 + 0.5 * gw) - (a1 + 0.5 * aw)) / aw) / d.std_dev[1]);
            row[2] = (float)(log(gh / ah) / d.std_dev[2]);
            row[3] = (float)(log(gw / aw) / d.std_dev[3]);
        }
    }
    if (b == 0) {                                                      // the unused tail of the outputs, and the counts
        const int cap = d.B * d.budget;
        for (int i = blockIdx.x * RT_THREADS + tid; i < cap; i += gridDim.x * RT_THREADS) {
            if (i >= sel_all) d.sel_level[i] = d.sel_index[i] = d.sel_match[i] = 0;
            if (i >= pos_all) {
                float* row = d.deltas + (size_t)i * 4;
                row[0] = row[1] = row[2] = row[3] = 0.f;
            }
        }
        if (blockIdx.x == 0 && tid == 0) {
            d.counts[0] = sel_all;
            d.counts[1] = pos_all;
        }
    }
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

int rt_validate(const dc_rpn_targets_desc* d) {
    DC_REQUIRE(d && d->anchors && d->gt_boxes && d->gt_counts && d->counts && d->sel_level && d->sel_index && d->sel_match && d->deltas, DC_EINVAL,
               "dc_rpn_targets: null pointer");
    DC_REQUIRE(d->B >= 1 && d->B <= RT_MAX_BATCH && d->A >= 1, DC_EINVAL, "dc_rpn_targets: needs 1..%d images and at least one anchor", RT_MAX_BATCH);
    DC_REQUIRE(d->budget >= 2 && d->budget <= RT_MAX_BUDGET, DC_EINVAL, "dc_rpn_targets: the anchor budget must lie in 2..%d", RT_MAX_BUDGET);
    DC_REQUIRE(d->gt_capacity >= 1 && d->gt_capacity <= RT_MAX_GT, DC_EINVAL, "dc_rpn_targets: the box capacity must lie in 1..%d", RT_MAX_GT);
    DC_REQUIRE(d->n_levels >= 1 && d->n_levels <= 5, DC_EINVAL, "dc_rpn_targets: 1..5 pyramid levels");
    long long sum = 0;
    for (int l = 0; l < d->n_levels; ++l) {
        DC_REQUIRE(d->level_sizes[l] > 0, DC_EINVAL, "dc_rpn_targets: level %d has no anchors", l);
        sum += d->level_sizes[l];
    }
    DC_REQUIRE(sum == d->A, DC_EINVAL, "dc_rpn_targets: the level sizes sum to %lld, there are %d anchors", sum, d->A);
    DC_REQUIRE((long long)d->B * d->A < (1ll << 31), DC_EINVAL, "dc_rpn_targets: B * A must stay below 2^31");
    if (!aligned8(d->anchors) || !aligned8(d->gt_boxes)) {
        set_error("dc_rpn_targets: anchors and gt_boxes (float64) must be 8-byte aligned");
        return DC_EALIGN;
    }
    return DC_OK;
}

}  // namespace

extern "C" size_t dc_rpn_targets_workspace(const dc_rpn_targets_desc* d) {
    if (!d || d->B < 1 || d->A < 1 || d->gt_capacity < 1) return 0;
    return rt_layout(d, nullptr, nullptr);
}

extern "C" int dc_rpn_targets_f64(const dc_rpn_targets_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = rt_validate(d);
    if (rc != DC_OK) return rc;
    DC_REQUIRE(workspace != nullptr && workspace_bytes >= rt_layout(d, nullptr, nullptr), DC_EWORKSPACE,
               "dc_rpn_targets: the workspace holds %zu bytes, %zu are needed", workspace ? workspace_bytes : (size_t)0, rt_layout(d, nullptr, nullptr));
    if (!aligned16(workspace)) {
        set_error("dc_rpn_targets: the workspace must be 16-byte aligned");
        return DC_EALIGN;
    }
    RtWorkspace w;
    rt_layout(d, workspace, &w);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nblk = rt_blocks(d->A);
    const dim3 grid(nblk, d->B), block(RT_THREADS);
    hipLaunchKernelGGL(rt_colmax_partial_kernel, grid, block, 0, s, *d, w, nblk);
    hipLaunchKernelGGL(rt_colmax_finish_kernel, dim3(d->gt_capacity, d->B), block, 0, s, *d, w, nblk);
    hipLaunchKernelGGL(rt_classify_kernel, grid, block, 0, s, *d, w);
    for (int p = 1; p < RT_PASSES; ++p) hipLaunchKernelGGL(rt_radix_kernel, grid, block, 0, s, *d, w, p);
    hipLaunchKernelGGL(rt_count_kernel, grid, block, 0, s, *d, w, nblk);
    hipLaunchKernelGGL(rt_write_kernel, grid, block, 0, s, *d, w, nblk);
    return check_launch("rpn_targets kernels");
}

// Scoring detections against ground truth on the device (include/dcap.h: dc_rle_iou_f64, dc_box_iou_f64, dc_detection_ap_f64).
//
//   dc_rle_iou_f64       mask IoU of two packed sets of run-length encodings (the form dc_mask_rle_u32 writes): pycocotools' rleIou.
//                        Pass 1, one wave per mask: run ends and the set pixels below each, the area, the first and last set index.
//                        Pass 2, one wave per pair: the lanes take the shorter encoding's runs of ones and count the other's set
//                        pixels inside each by two binary searches in its run ends.
//   dc_box_iou_f64       utils.compute_overlaps on int32 boxes.
//   dc_detection_ap_f64  utils.compute_ap's matching and average precision on a given IoU matrix, one workgroup per (image, threshold).
//
// Integer and float64 work in a fixed order, no atomics: the same bytes on every run.  The host statements these are held to, bit for
// bit, are mask_rle.iou, utils.compute_overlaps and detection_eval.ap_from_overlaps.
#include "dcap_internal.h"
#include <limits.h>

// every product and sum below is one rounding, as NumPy's: no fused multiply-add
#pragma clang fp contract(off)

namespace dcap {

constexpr int EV_THREADS = 256, EV_WAVES = EV_THREADS / 64;
constexpr int EV_MAX = 1024;                                     // masks, boxes or predictions per set

__device__ __forceinline__ unsigned long long ev_wave_scan(unsigned long long v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_up(v, o);
        if (lane >= o) v += up;
    }
    return v;
}

__device__ __forceinline__ int ev_clip_int(unsigned long long v) { return v > 0x7fffffffull ? INT_MAX : (int)v; }

// either packed set needs more words than its buffer holds: nothing is walked, every result is NaN / -1
__device__ __forceinline__ bool ev_truncated(const int* __restrict__ offs_d, const int* __restrict__ offs_g, int D, int G, int cap_d, int cap_g) {
    return offs_d[D] > cap_d || offs_g[G] > cap_g;
}

// pass 1.  Wave m < D: detection m; wave D + m: ground truth m.  runs[j] = (the end of run j, the set pixels below that end) for
// count word j of the set (the ground truth's words behind the detections' cap_d); info[m] = (area or -1, first set index, last set
// index + 1, 1 when the counts sum to H W).  A mask whose offsets leave [0, capacity] or are not increasing reads nothing and is bad.
__global__ __launch_bounds__(EV_THREADS) void rle_prep_kernel(const int* __restrict__ offs_d, const uint32_t* __restrict__ cnt_d,
                                                             const int* __restrict__ offs_g, const uint32_t* __restrict__ cnt_g, int D, int G,
                                                             int cap_d, int cap_g, int HW, int2* __restrict__ runs, int4* __restrict__ info,
                                                             int* __restrict__ area_out) {
    const int wave = blockIdx.x * EV_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wave >= D + G) return;
    if (ev_truncated(offs_d, offs_g, D, G, cap_d, cap_g)) {
        if (lane == 0) {
            info[wave] = make_int4(-1, 0, 0, 0);
            if (area_out) area_out[wave] = -1;
        }
        return;
    }
    const bool gt = wave >= D;
    const int m = gt ? wave - D : wave, cap = gt ? cap_g : cap_d;
    const int* offs = gt ? offs_g : offs_d;
    const uint32_t* cnt = gt ? cnt_g : cnt_d;
    int2* out = runs + (gt ? cap_d : 0);
    const int lo = offs[m], hi = offs[m + 1];
    bool ok = lo >= 0 && hi > lo && hi <= cap;
    unsigned long long end_c = 0, ones_c = 0;
    int first = INT_MAX, last = 0;
    if (ok) {
        for (int j0 = lo; j0 < hi; j0 += 64) {
            const int j = j0 + lane;
            const bool in = j < hi, odd = (j - lo) & 1;
            const unsigned long long c = in ? cnt[j] : 0ull;
            const unsigned long long e = ev_wave_scan(c, lane) + end_c, o = ev_wave_scan(odd ? c : 0ull, lane) + ones_c;
            if (in) out[j] = make_int2(ev_clip_int(e), ev_clip_int(o));
            if (in && odd && c) {
                first = min(first, ev_clip_int(e - c));
                last = max(last, ev_clip_int(e));
            }
            end_c = __shfl(e, 63);
            ones_c = __shfl(o, 63);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        first = min(first, __shfl_xor(first, o));
        last = max(last, __shfl_xor(last, o));
    }
    ok = ok && end_c == (unsigned long long)HW;
    if (lane == 0) {
        const int area = ok ? (int)ones_c : -1;
        info[wave] = make_int4(area, first, last, ok ? 1 : 0);
        if (area_out) area_out[wave] = area;
    }
}

// the set pixels of one mask at indices below p: c = the runs that end at or before p; behind them p sits in run c, a run of ones
// exactly when c is odd
__device__ __forceinline__ int ev_below(const int2* __restrict__ r, int n, const int4 inf, int p) {
    if (p <= inf.y) return 0;
    if (p >= inf.z) return inf.x;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (r[mid].x <= p)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo == 0) return 0;
    const int2 at = r[lo - 1];
    return at.y + ((lo & 1) ? p - at.x : 0);
}

// pass 2: wave d * G + g
__global__ __launch_bounds__(EV_THREADS) void rle_iou_kernel(const int* __restrict__ offs_d, const int* __restrict__ offs_g, int D, int G, int cap_d,
                                                            int cap_g, const int* __restrict__ n_det, const uint8_t* __restrict__ iscrowd,
                                                            const int2* __restrict__ runs, const int4* __restrict__ info,
                                                            double* __restrict__ iou, int* __restrict__ inter, int ld) {
    const int pair = blockIdx.x * EV_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (pair >= D * G) return;
    const int d = pair / G, g = pair - d * G;
    const int rows = n_det ? n_det[0] : D;
    double out = 0.;
    int I = 0;
    if (ev_truncated(offs_d, offs_g, D, G, cap_d, cap_g)) {
        out = __longlong_as_double(0x7ff8000000000000ll);
        I = -1;
    } else if (d < rows) {
        const int4 id = info[d], ig = info[D + g];
        if (!id.w || !ig.w) {
            out = __longlong_as_double(0x7ff8000000000000ll);
            I = -1;
        } else {
            if (id.x > 0 && ig.x > 0 && id.y < ig.z && ig.y < id.z) {           // the set-index ranges meet
                const int lo_d = offs_d[d], n_d = offs_d[d + 1] - lo_d, lo_g = offs_g[g], n_g = offs_g[g + 1] - lo_g;
                const bool walk_d = n_d <= n_g;                                 // the lanes walk the shorter encoding
                const int2* rd = runs + lo_d;
                const int2* rg = runs + cap_d + lo_g;
                const int2* walked = walk_d ? rd : rg;
                const int2* other = walk_d ? rg : rd;
                const int nw = walk_d ? n_d : n_g, no = walk_d ? n_g : n_d;
                const int4 io = walk_d ? ig : id;
                int part = 0;
                for (int j0 = 1; j0 < nw; j0 += 128) {                          // count word j = 1, 3, 5, ...: the runs of ones
                    const int j = j0 + 2 * lane;
                    if (j < nw) {
                        const int s = walked[j - 1].x, e = walked[j].x;
                        if (e > s) part += ev_below(other, no, io, e) - ev_below(other, no, io, s);
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
                I = part;
            }
            const long long den = iscrowd && iscrowd[g] ? (long long)id.x : (long long)id.x + ig.x - I;
            out = den ? (double)I / (double)den : 0.;
        }
    }
    if (lane == 0) {
        iou[(size_t)d * ld + g] = out;
        if (inter) inter[(size_t)d * ld + g] = I;
    }
}

// one block.  status = (words the detections need when they outgrow capacity_d, else 0; the same for the ground truth; masks whose
// counts do not sum to H W; rows computed = min(n_det[0], D))
__global__ __launch_bounds__(EV_THREADS) void rle_status_kernel(const int* __restrict__ offs_d, const int* __restrict__ offs_g, int D, int G, int cap_d,
                                                               int cap_g, const int* __restrict__ n_det, const int4* __restrict__ info, int checked,
                                                               int* __restrict__ status) {
    __shared__ int part[EV_WAVES];
    const bool trunc = ev_truncated(offs_d, offs_g, D, G, cap_d, cap_g);
    int bad = 0;
    if (checked && !trunc)
        for (int m = threadIdx.x; m < D + G; m += EV_THREADS) bad += info[m].w == 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int rows = n_det ? n_det[0] : D;
        status[0] = offs_d[D] > cap_d ? offs_d[D] : 0;
        status[1] = offs_g[G] > cap_g ? offs_g[G] : 0;
        status[2] = part[0] + part[1] + part[2] + part[3];
        status[3] = rows < 0 ? 0 : rows < D ? rows : D;
    }
}

// utils.compute_overlaps / compute_iou on integers: one thread per (image, box, gt box)
__global__ __launch_bounds__(EV_THREADS) void box_iou_kernel(const int4* __restrict__ a, const int4* __restrict__ bx, int Dmax, int Gmax, int ld,
                                                            double* __restrict__ out, long total) {
    for (long i = (long)blockIdx.x * EV_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * EV_THREADS) {
        const int g = (int)(i % Gmax);
        const long bd = i / Gmax;                                              // image * Dmax + box
        const int4 p = a[bd], q = bx[(bd / Dmax) * Gmax + g];
        const long long ap = (long long)(p.z - p.x) * (p.w - p.y), aq = (long long)(q.z - q.x) * (q.w - q.y);
        const long long ih = max(min(p.z, q.z) - max(p.x, q.x), 0), iw = max(min(p.w, q.w) - max(p.y, q.y), 0);
        const long long inter = iw * ih, uni = ap + aq - inter;
        out[bd * ld + g] = (double)inter / (double)uni;                        // 0 / 0 is NumPy's NaN
    }
}

// a score's sort key: larger key = better; equal floats give equal keys (-0 as +0), every NaN ranks above every number, as
// np.argsort(...)[::-1] has them
__device__ __forceinline__ unsigned ap_key(float s) {
    if (s != s) return 0xffffffffu;
    const unsigned u = __float_as_uint(s + 0.f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(EV_THREADS) void detection_ap_kernel(dc_detection_ap_desc d) {
    __shared__ unsigned skey[EV_MAX];                // by prediction: the sort key; behind the sort, by ground truth: its class
    __shared__ int sorder[EV_MAX];                   // by rank: the prediction
    __shared__ int spm[EV_MAX];                      // by rank: the matched ground truth or -1
    __shared__ int sgm[EV_MAX];                      // by ground truth: the rank matched to it or -1
    __shared__ int shits[EV_MAX + 1];                // matches among the first i ranks
    __shared__ double sprec[EV_MAX + 2];             // the reference's padded precisions
    __shared__ double sterm[EV_MAX + 1];             // the terms of the final sum
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int n = min(max(d.n_det[b], 0), d.Dmax), G = min(max(d.n_gt[b], 0), d.Gmax);
    const double thr = d.thresholds[t];
    const double* ov = d.overlaps + (size_t)b * d.Dmax * d.ld;
    const int* pcls = d.pred_class + (size_t)b * d.Dmax;
    const float* psc = d.pred_score + (size_t)b * d.Dmax;
    const int* gcls = d.gt_class + (size_t)b * d.Gmax;

    for (int i = tid; i < n; i += EV_THREADS) skey[i] = ap_key(psc[i]);
    __syncthreads();
    // a prediction's rank = the predictions with a larger key, or the same key and a HIGHER index
    int my_rank[EV_MAX / EV_THREADS];
#pragma unroll
    for (int k = 0; k < EV_MAX / EV_THREADS; ++k) {
        const int i = tid + k * EV_THREADS;
        int rank = 0;
        if (i < n) {
            const unsigned mine = skey[i];
            for (int j = 0; j < n; ++j) {
                const unsigned o = skey[j];
                rank += (o > mine) || (o == mine && j > i);
            }
        }
        my_rank[k] = rank;
    }
    __syncthreads();                                 // the keys are read: skey takes the ground truth's classes
#pragma unroll
    for (int k = 0; k < EV_MAX / EV_THREADS; ++k) {
        const int i = tid + k * EV_THREADS;
        if (i < n) sorder[my_rank[k]] = i;
    }
    int* sgc = reinterpret_cast<int*>(skey);
    for (int g = tid; g < G; g += EV_THREADS) {
        sgc[g] = gcls[g];
        sgm[g] = -1;
    }
    __syncthreads();

    // the greedy matching, by wave 0 alone.  Lane l owns the ground truths l, l + 64, ...: bit k of `matched` is ground truth l + 64 k,
    // so the matched set sits in registers and the loop needs no barrier.
    if (tid < 64) {
        const int lane = tid;
        unsigned matched = 0u;
        for (int r = 0; r < n; ++r) {
            const int p = sorder[r], pc = pcls[p];
            const double* row = ov + (size_t)p * d.ld;
            double best = 0.;
            int bg = -1;
            for (int k = 0, g = lane; g < G; ++k, g += 64) {
                if ((matched >> k) & 1u) continue;
                const double v = row[g];
                if (v >= thr && sgc[g] == pc && (bg < 0 || v >= best)) {       // (a NaN fails v >= thr; g rises: on equal IoU the higher index)
                    best = v;
                    bg = g;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o);
                const int og = __shfl_xor(bg, o);
                if (og >= 0 && (bg < 0 || ob > best || (ob == best && og > bg))) {
                    best = ob;
                    bg = og;
                }
            }
            if (bg >= 0 && (bg & 63) == lane) matched |= 1u << (bg >> 6);
            if (lane == 0) {
                spm[r] = bg;
                if (bg >= 0) sgm[bg] = r;
            }
        }
    }
    __syncthreads();

    if (tid == 0) {
        double ap = __longlong_as_double(0x7ff8000000000000ll);                // no ground truth: NaN
        if (G > 0) {
            int c = 0;
            shits[0] = 0;
            sprec[0] = 0.;
            for (int r = 0; r < n; ++r) {
                c += spm[r] >= 0;
                shits[r + 1] = c;
                sprec[r + 1] = (double)c / (double)(r + 1);
            }
            sprec[n + 1] = 0.;
            for (int i = n; i >= 0; --i) sprec[i] = sprec[i] > sprec[i + 1] ? sprec[i] : sprec[i + 1];
            // recalls: a float32 quotient (formed in float64 and rounded once more, which for a quotient of two float32 is the float32
            // quotient), widened; [0] in front and [1] behind
            const double gf = (double)(float)G;
            int nt = 0;
            double before = 0.;
            for (int i = 1; i <= n + 1; ++i) {
                const double rec = i == n + 1 ? 1. : (double)(float)((double)(float)shits[i] / gf);
                if (rec != before) sterm[nt++] = (rec - before) * sprec[i];
                before = rec;
            }
            // NumPy's order for fewer than 128 terms, at any length
            if (nt < 8) {
                ap = 0.;
                for (int i = 0; i < nt; ++i) ap = ap + sterm[i];
            } else {
                double r0 = sterm[0], r1 = sterm[1], r2 = sterm[2], r3 = sterm[3], r4 = sterm[4], r5 = sterm[5], r6 = sterm[6], r7 = sterm[7];
                int i = 8;
                for (; i < nt - nt % 8; i += 8) {
                    r0 = r0 + sterm[i];
                    r1 = r1 + sterm[i + 1];
                    r2 = r2 + sterm[i + 2];
                    r3 = r3 + sterm[i + 3];
                    r4 = r4 + sterm[i + 4];
                    r5 = r5 + sterm[i + 5];
                    r6 = r6 + sterm[i + 6];
                    r7 = r7 + sterm[i + 7];
                }
                ap = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
                for (; i < nt; ++i) ap = ap + sterm[i];
            }
        }
        d.ap[(size_t)b * d.T + t] = ap;
    }
    if (d.pred_match) {
        int* pm = d.pred_match + ((size_t)b * d.T + t) * d.Dmax;
        for (int i = tid; i < d.Dmax; i += EV_THREADS) pm[i] = i < n ? spm[i] : -1;
    }
    if (d.gt_match) {
        int* gm = d.gt_match + ((size_t)b * d.T + t) * d.Gmax;
        for (int g = tid; g < d.Gmax; g += EV_THREADS) gm[g] = g < G ? sgm[g] : -1;
    }
    if (d.order && t == 0) {
        int* od = d.order + (size_t)b * d.Dmax;
        for (int i = tid; i < d.Dmax; i += EV_THREADS) od[i] = i < n ? sorder[i] : -1;
    }
}

struct RleIouWs {
    size_t info, total;
};

static bool off_boundary(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

static int rle_iou_plan(const dc_rle_iou_desc* d, RleIouWs* L) {
    DC_REQUIRE(d, DC_EINVAL, "dc_rle_iou_f64: null descriptor");
    DC_REQUIRE(d->D >= 0 && d->D <= EV_MAX && d->G >= 0 && d->G <= EV_MAX, DC_EINVAL, "dc_rle_iou_f64: D and G in 0..%d, got %d and %d", EV_MAX,
               d->D, d->G);
    DC_REQUIRE(d->H >= 1 && d->W >= 1 && (size_t)d->H * (size_t)d->W < ((size_t)1 << 31), DC_EINVAL,
               "dc_rle_iou_f64: an image of at least 1 x 1 and fewer than 2^31 pixels, got %d x %d", d->H, d->W);
    DC_REQUIRE(d->capacity_d >= 0 && d->capacity_g >= 0, DC_EINVAL, "dc_rle_iou_f64: a capacity must not be negative, got %d and %d",
               d->capacity_d, d->capacity_g);
    DC_REQUIRE(d->offsets_d && d->offsets_g && d->status, DC_EINVAL, "dc_rle_iou_f64: null offsets or status");
    DC_REQUIRE((d->counts_d || d->capacity_d == 0) && (d->counts_g || d->capacity_g == 0), DC_EINVAL,
               "dc_rle_iou_f64: null counts with a capacity above 0");
    DC_REQUIRE(d->iou || d->D == 0 || d->G == 0, DC_EINVAL, "dc_rle_iou_f64: null iou");
    DC_REQUIRE(d->ld >= d->G, DC_EINVAL, "dc_rle_iou_f64: ld %d is below G %d", d->ld, d->G);
    DC_REQUIRE(!off_boundary(d->offsets_d, 3) && !off_boundary(d->offsets_g, 3) && !off_boundary(d->counts_d, 3) && !off_boundary(d->counts_g, 3) &&
                   !off_boundary(d->n_det, 3) && !off_boundary(d->inter, 3) && !off_boundary(d->area, 3) && !off_boundary(d->status, 3) &&
                   !off_boundary(d->iou, 7),
               DC_EINVAL, "dc_rle_iou_f64: an int32 / uint32 pointer off a 4-byte boundary or iou off an 8-byte boundary");
    L->info = (((size_t)d->capacity_d + (size_t)d->capacity_g) * sizeof(int2) + 15) & ~(size_t)15;
    L->total = L->info + (size_t)(d->D + d->G) * sizeof(int4);
    return DC_OK;
}

}  // namespace dcap

using namespace dcap;

extern "C" size_t dc_rle_iou_workspace_bytes(const dc_rle_iou_desc* d) {
    RleIouWs L;
    if (rle_iou_plan(d, &L)) return 0;
    return d->D == 0 || d->G == 0 ? 0 : L.total;
}

extern "C" int dc_rle_iou_f64(const dc_rle_iou_desc* d, void* stream) {
    RleIouWs L;
    int rc = rle_iou_plan(d, &L);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int D = d->D, G = d->G;
    if (D == 0 || G == 0) {
        hipLaunchKernelGGL(rle_status_kernel, dim3(1), dim3(EV_THREADS), 0, s, d->offsets_d, d->offsets_g, D, G, d->capacity_d, d->capacity_g,
                           d->n_det, static_cast<const int4*>(nullptr), 0, d->status);
        return check_launch("rle_status_kernel");
    }
    DC_REQUIRE(d->workspace && d->workspace_bytes >= L.total && aligned16(d->workspace), DC_EWORKSPACE,
               "dc_rle_iou_f64: needs %zu workspace bytes (16-byte aligned), got %zu", L.total, d->workspace_bytes);
    uint8_t* base = static_cast<uint8_t*>(d->workspace);
    int2* runs = reinterpret_cast<int2*>(base);
    int4* info = reinterpret_cast<int4*>(base + L.info);
    hipLaunchKernelGGL(rle_prep_kernel, dim3((D + G + EV_WAVES - 1) / EV_WAVES), dim3(EV_THREADS), 0, s, d->offsets_d, d->counts_d, d->offsets_g,
                       d->counts_g, D, G, d->capacity_d, d->capacity_g, d->H * d->W, runs, info, d->area);
    hipLaunchKernelGGL(rle_iou_kernel, dim3((D * G + EV_WAVES - 1) / EV_WAVES), dim3(EV_THREADS), 0, s, d->offsets_d, d->offsets_g, D, G,
                       d->capacity_d, d->capacity_g, d->n_det, d->iscrowd, runs, info, d->iou, d->inter, d->ld);
    hipLaunchKernelGGL(rle_status_kernel, dim3(1), dim3(EV_THREADS), 0, s, d->offsets_d, d->offsets_g, D, G, d->capacity_d, d->capacity_g, d->n_det,
                       info, 1, d->status);
    return check_launch("rle_iou kernels");
}

extern "C" int dc_box_iou_f64(const int32_t* boxes, const int32_t* gt_boxes, int B, int Dmax, int Gmax, int ld, double* out, void* stream) {
    DC_REQUIRE(B >= 0 && B <= 65535 && Dmax >= 0 && Dmax <= EV_MAX && Gmax >= 0 && Gmax <= EV_MAX, DC_EINVAL,
               "dc_box_iou_f64: B in 0..65535, Dmax and Gmax in 0..%d, got %d, %d and %d", EV_MAX, B, Dmax, Gmax);
    DC_REQUIRE(ld >= Gmax, DC_EINVAL, "dc_box_iou_f64: ld %d is below Gmax %d", ld, Gmax);
    const long total = (long)B * Dmax * Gmax;
    if (total == 0) return DC_OK;
    DC_REQUIRE(boxes && gt_boxes && out, DC_EINVAL, "dc_box_iou_f64: null boxes, gt_boxes or out");
    DC_REQUIRE(!off_boundary(boxes, 15) && !off_boundary(gt_boxes, 15) && !off_boundary(out, 7), DC_EINVAL,
               "dc_box_iou_f64: the box arrays must sit on 16-byte boundaries (a box is read at once) and out on an 8-byte boundary");
    const long blocks = (total + EV_THREADS - 1) / EV_THREADS;
    hipLaunchKernelGGL(box_iou_kernel, dim3((unsigned)(blocks < 65535 ? blocks : 65535)), dim3(EV_THREADS), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const int4*>(boxes), reinterpret_cast<const int4*>(gt_boxes), Dmax, Gmax, ld, out, total);
    return check_launch("box_iou_kernel");
}

extern "C" int dc_detection_ap_f64(const dc_detection_ap_desc* d, void* stream) {
    DC_REQUIRE(d, DC_EINVAL, "dc_detection_ap_f64: null descriptor");
    DC_REQUIRE(d->B >= 0 && d->B <= 65535 && d->Dmax >= 0 && d->Dmax <= EV_MAX && d->Gmax >= 0 && d->Gmax <= EV_MAX, DC_EINVAL,
               "dc_detection_ap_f64: B in 0..65535, Dmax and Gmax in 0..%d, got %d, %d and %d", EV_MAX, d->B, d->Dmax, d->Gmax);
    DC_REQUIRE(d->T >= 1 && d->T <= 16, DC_EINVAL, "dc_detection_ap_f64: T in 1..16, got %d", d->T);
    DC_REQUIRE(d->ld >= d->Gmax, DC_EINVAL, "dc_detection_ap_f64: ld %d is below Gmax %d", d->ld, d->Gmax);
    if (d->B == 0) return DC_OK;
    DC_REQUIRE(d->n_det && d->n_gt && d->thresholds && d->ap, DC_EINVAL, "dc_detection_ap_f64: null n_det, n_gt, thresholds or ap");
    DC_REQUIRE((d->overlaps || d->Dmax == 0 || d->Gmax == 0) && ((d->pred_class && d->pred_score) || d->Dmax == 0) && (d->gt_class || d->Gmax == 0),
               DC_EINVAL, "dc_detection_ap_f64: null overlaps, pred_class, pred_score or gt_class");
    DC_REQUIRE(!off_boundary(d->overlaps, 7) && !off_boundary(d->thresholds, 7) && !off_boundary(d->ap, 7) && !off_boundary(d->n_det, 3) &&
                   !off_boundary(d->n_gt, 3) && !off_boundary(d->pred_class, 3) && !off_boundary(d->pred_score, 3) && !off_boundary(d->gt_class, 3) &&
                   !off_boundary(d->pred_match, 3) && !off_boundary(d->gt_match, 3) && !off_boundary(d->order, 3),
               DC_EINVAL, "dc_detection_ap_f64: a float64 pointer off an 8-byte boundary or a 4-byte one off a 4-byte boundary");
    hipLaunchKernelGGL(detection_ap_kernel, dim3(d->T, d->B), dim3(EV_THREADS), 0, static_cast<hipStream_t>(stream), *d);
    return check_launch("detection_ap_kernel");
}

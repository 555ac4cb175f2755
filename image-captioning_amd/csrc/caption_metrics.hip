// caption_metrics.hip -- BLEU-1..4 / ROUGE-L statistics and values (dc_caption_metrics_f64) and CIDEr (dc_caption_cider_f64) of
// caption records held as int32 token ids.  Small-integer, latency-bound work: one 64-lane wave per record, the candidate's
// positions on the lanes, the reference positions walked in a loop out of LDS (a broadcast read).  N-gram equality is equality of up
// to four ids -- nothing is hashed.  All floating point is float64 in a fixed order (butterfly shuffles, no atomics): a record's
// result depends on that record alone, two calls give identical bits.
#include "dcap_internal.h"
#include <math.h>

namespace dcap {

constexpr int kCapMaxTokens = DC_CAPTION_MAX_TOKENS;     // one wave holds a sentence: a position per lane
constexpr int kCapPad = 4;                                // LDS slack past the last position: a 4-gram read never leaves the array

__device__ __forceinline__ int cap_clamp_len(int len, int width) {
    const int hi = width < kCapMaxTokens ? width : kCapMaxTokens;
    return len < 0 ? 0 : (len > hi ? hi : len);
}
__device__ __forceinline__ int cap_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double cap_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// how many of the (up to four) leading tokens of two windows agree
__device__ __forceinline__ int cap_match_len(int a0, int a1, int a2, int a3, const int* b) {
    int m = 0;
    if (a0 == b[0]) {
        m = 1;
        if (a1 == b[1]) {
            m = 2;
            if (a2 == b[2]) m = a3 == b[3] ? 4 : 3;
        }
    }
    return m;
}

// One wave per record.  Padding sentinels: -1 past the candidate's end, -2 past a reference's (ids are >= 0), so a window that
// runs off a sentence stops matching there; a candidate window is only counted for the orders that fit (lane + k <= Lc).
__global__ __launch_bounds__(64) void caption_metrics_kernel(dc_caption_metrics_desc d) {
    __shared__ int sc[kCapMaxTokens + kCapPad], sr[kCapMaxTokens + kCapPad];
    const int rec = blockIdx.x, lane = threadIdx.x;
    const int Lc = cap_clamp_len(d.cand_len[rec], d.Tc);
    const int myc = lane < Lc ? d.cand[(size_t)rec * d.ld_cand + lane] : -1;
    sc[lane] = myc;
    if (lane < kCapPad) sc[kCapMaxTokens + lane] = -1;
    __syncthreads();
    const int c1 = sc[lane + 1], c2 = sc[lane + 2], c3 = sc[lane + 3];

    // the candidate against itself: the count of each of this lane's k-grams and whether an earlier lane holds the same one
    int cnt_c[4] = {0, 0, 0, 0};
    bool seen[4] = {false, false, false, false};
    for (int j = 0; j < Lc; ++j) {
        const int m = cap_match_len(myc, c1, c2, c3, sc + j);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cnt_c[k] += m > k;
            seen[k] = seen[k] || (m > k && j < lane);
        }
    }

    int r0 = d.ref_start[rec], r1 = d.ref_start[rec + 1];
    r0 = r0 < 0 ? 0 : (r0 > d.M ? d.M : r0);
    r1 = r1 < r0 ? r0 : (r1 > d.M ? d.M : r1);
    int max_r[4] = {0, 0, 0, 0};
    int best_diff = 0x7fffffff, reflen = 0, lcs_max = 0;
    double prec_max = 0.0, rec_max = 0.0;
    for (int r = r0; r < r1; ++r) {
        const int Lr = cap_clamp_len(d.ref_len[r], d.Tr);
        const int myr = lane < Lr ? d.refs[(size_t)r * d.ld_refs + lane] : -2;
        __syncthreads();                                  // the previous reference has been read by every lane
        sr[lane] = myr;
        if (lane < kCapPad) sr[kCapMaxTokens + lane] = -2;
        __syncthreads();
        int cnt_r[4] = {0, 0, 0, 0};
        for (int p = 0; p < Lr; ++p) {
            const int m = cap_match_len(myc, c1, c2, c3, sr + p);
#pragma unroll
            for (int k = 0; k < 4; ++k) cnt_r[k] += m > k;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) max_r[k] = cnt_r[k] > max_r[k] ? cnt_r[k] : max_r[k];
        const int diff = Lr > Lc ? Lr - Lc : Lc - Lr;
        if (diff < best_diff || (diff == best_diff && Lr < reflen)) {
            best_diff = diff;
            reflen = Lr;
        }

        int l;
        if (d.lcs) {
            // true LCS: row p of the table over the candidate's prefixes, a column per lane.  cur[j] = max(up[j], diag[j] + match,
            // cur[j - 1]) -- the last term is an inclusive prefix maximum over the lanes (six shuffles)
            int prev = 0;
            for (int p = 0; p < Lr; ++p) {
                const int rt = sr[p];
                int diag = __shfl_up(prev, 1, 64);
                if (lane == 0) diag = 0;
                int t = diag + (myc == rt);
                t = t > prev ? t : prev;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int u = __shfl_up(t, o, 64);
                    if (lane >= o && u > t) t = u;
                }
                prev = t;
            }
            l = Lc > 0 ? __shfl(prev, Lc - 1, 64) : 0;
        } else if (Lc <= Lr) {
            // the fork's my_lcs: positions of the SHORTER sentence (the candidate on equal lengths) whose token is in the longer
            l = __popcll(__ballot(lane < Lc && cnt_r[0] > 0));
        } else {
            bool hit = false;
            for (int i = 0; i < Lc; ++i) hit = hit || (sc[i] == myr);
            l = __popcll(__ballot(lane < Lr && hit));
        }
        lcs_max = l > lcs_max ? l : lcs_max;
        const double p_ = (double)l / (double)(Lc > 0 ? Lc : 1), r_ = (double)l / (double)(Lr > 0 ? Lr : 1);
        prec_max = p_ > prec_max ? p_ : prec_max;
        rec_max = r_ > rec_max ? r_ : rec_max;
    }

    int correct[4], guess[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool first = lane + k + 1 <= Lc && !seen[k];
        correct[k] = cap_wave_sum(first ? (cnt_c[k] < max_r[k] ? cnt_c[k] : max_r[k]) : 0);
        guess[k] = Lc - k > 0 ? Lc - k : 0;
    }
    if (lane != 0) return;
    int32_t* st = d.stats + (size_t)rec * 12;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        st[k] = correct[k];
        st[4 + k] = guess[k];
    }
    st[8] = Lc;
    st[9] = reflen;
    st[10] = lcs_max;
    st[11] = 0;
    const double tiny = 1e-15, small = 1e-9;
    const double ratio = ((double)Lc + tiny) / ((double)reflen + small);
    const double brevity = ratio < 1.0 ? exp(1.0 - 1.0 / ratio) : 1.0;
    double b = 1.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        b *= ((double)correct[k] + tiny) / ((double)guess[k] + small);
        const double v = pow(b, 1.0 / (double)(k + 1));
        d.bleu[(size_t)k * d.N + rec] = ratio < 1.0 ? v * brevity : v;
    }
    const double beta2 = 1.2 * 1.2;
    d.rouge[rec] = (prec_max != 0.0 && rec_max != 0.0) ? ((1.0 + beta2) * prec_max * rec_max) / (rec_max + beta2 * prec_max) : 0.0;
}

// CIDEr of one record per wave from dense n-gram ids (equal ids = equal n-grams of one group) and the document-frequency table.
// A gram's weight is tf * (log N - log max(1, df)); the norms and the clipped similarity sum over DISTINCT grams, found as in the
// kernel above (first lane that holds the id).  Sentinels: -1 / -2 where no n-gram starts.
__global__ __launch_bounds__(64) void caption_cider_kernel(dc_caption_cider_desc d) {
    __shared__ int sc[kCapMaxTokens], sr[kCapMaxTokens];
    const int rec = blockIdx.x, lane = threadIdx.x;
    const int M = d.S - d.N;
    int r0 = d.ref_start[rec], r1 = d.ref_start[rec + 1];
    r0 = r0 < 0 ? 0 : (r0 > M ? M : r0);
    r1 = r1 < r0 ? r0 : (r1 > M ? M : r1);
    const int Lc = cap_clamp_len(d.sent_len[rec], d.T);
    const int gn = d.group_n[rec];
    const double log_n = log((double)(gn > 1 ? gn : 1));
    double total = 0.0;
    for (int k = 0; k < 4; ++k) {
        const int G = (k < 3 ? d.df_off[k + 1] : d.df_len) - d.df_off[k];
        const int nc = Lc - k > 0 ? Lc - k : 0;                                   // n-grams of this order in the candidate
        int gc = lane < nc ? d.grams[((size_t)k * d.S + rec) * d.T + lane] : -1;
        if (gc < 0 || gc >= G) gc = -1;
        __syncthreads();
        sc[lane] = gc;
        __syncthreads();
        int tf_c = 0;
        bool first_c = gc >= 0;
        for (int j = 0; j < nc; ++j) {
            const bool same = sc[j] == gc;
            tf_c += same;
            first_c = first_c && !(same && j < lane);
        }
        const double idf_c = gc >= 0 ? log_n - log((double)max(1, d.df[d.df_off[k] + gc])) : 0.0;
        const double w_c = (double)tf_c * idf_c;
        const double norm_c = sqrt(cap_wave_sum(first_c ? w_c * w_c : 0.0));
        double score_k = 0.0;
        for (int r = r0; r < r1; ++r) {
            const int s = d.N + r;
            const int Lr = cap_clamp_len(d.sent_len[s], d.T);
            const int nr = Lr - k > 0 ? Lr - k : 0;
            int gr = lane < nr ? d.grams[((size_t)k * d.S + s) * d.T + lane] : -2;
            if (gr < 0 || gr >= G) gr = -2;
            __syncthreads();
            sr[lane] = gr;
            __syncthreads();
            int tf_r = 0, tf_cr = 0;                                              // of this lane's reference gram / candidate gram, in the reference
            bool first_r = gr >= 0;
            for (int j = 0; j < nr; ++j) {
                const int g = sr[j];
                tf_r += g == gr;
                first_r = first_r && !(g == gr && j < lane);
                tf_cr += g == gc;
            }
            const double idf_r = gr >= 0 ? log_n - log((double)max(1, d.df[d.df_off[k] + gr])) : 0.0;
            const double w_r = (double)tf_r * idf_r;
            const double norm_r = sqrt(cap_wave_sum(first_r ? w_r * w_r : 0.0));
            const double w_cr = (double)tf_cr * idf_c;                            // the candidate gram's weight in the reference
            double val = cap_wave_sum(first_c ? (w_c < w_cr ? w_c : w_cr) * w_cr : 0.0);
            if (norm_c != 0.0 && norm_r != 0.0) val /= norm_c * norm_r;
            const double delta = (double)((Lc > 1 ? Lc - 1 : 0) - (Lr > 1 ? Lr - 1 : 0));
            score_k += val * exp(-(delta * delta) / (2.0 * 6.0 * 6.0));
        }
        total += score_k;
    }
    if (lane == 0) d.cider[rec] = r1 > r0 ? total / 4.0 / (double)(r1 - r0) * 10.0 : 0.0;
}

}  // namespace dcap

using namespace dcap;

extern "C" int dc_caption_metrics_f64(const dc_caption_metrics_desc* d, void* stream) {
    DC_REQUIRE(d && d->N >= 1 && d->M >= 1 && d->cand && d->cand_len && d->refs && d->ref_len && d->ref_start && d->stats && d->bleu && d->rouge,
               DC_EINVAL, "dc_caption_metrics: bad arguments");
    DC_REQUIRE(d->Tc >= 1 && d->Tr >= 1 && (d->N == 1 || d->ld_cand >= d->Tc) && (d->M == 1 || d->ld_refs >= d->Tr), DC_EINVAL,
               "dc_caption_metrics: a width is below 1 or above its row stride");
    DC_REQUIRE(d->lcs == 0 || d->lcs == 1, DC_EINVAL, "dc_caption_metrics: lcs must be 0 or 1, got %d", d->lcs);
    hipLaunchKernelGGL(caption_metrics_kernel, dim3(d->N), dim3(64), 0, static_cast<hipStream_t>(stream), *d);
    return check_launch("caption_metrics_kernel");
}

extern "C" int dc_caption_cider_f64(const dc_caption_cider_desc* d, void* stream) {
    DC_REQUIRE(d && d->N >= 1 && d->S > d->N && d->T >= 1 && d->grams && d->sent_len && d->ref_start && d->df && d->group_n && d->cider, DC_EINVAL,
               "dc_caption_cider: bad arguments");
    DC_REQUIRE(d->df_off[0] == 0 && d->df_off[1] >= 0 && d->df_off[2] >= d->df_off[1] && d->df_off[3] >= d->df_off[2] && d->df_len >= d->df_off[3],
               DC_EINVAL, "dc_caption_cider: df_off must start at 0 and not decrease up to df_len");
    hipLaunchKernelGGL(caption_cider_kernel, dim3(d->N), dim3(64), 0, static_cast<hipStream_t>(stream), *d);
    return check_launch("caption_cider_kernel");
}

// roialign.hip -- PyramidROIAlign forward: FPN level routing + tf.image.crop_and_resize (bilinear,
// one sample per bin, extrapolation 0) as one HBM-bound gather kernel.
// One wave per output bin: the 64 lanes read the four corner pixels' channel vectors as float4
// (C = 256 -> one coalesced 1 KiB row per corner) and write the bin's 1 KiB row.
// Sample coordinates follow TF's float32 kernel operation by operation (mul, div, mul, add -- no fma
// contraction) so the in-range test and floor/ceil decisions match the reference's CPU path.
#include "dcap_internal.h"
#include <math.h>
#include <algorithm>

// Every float operation of this file is rounded on its own, as the TF float32 kernels it mirrors round theirs: the decisions taken on the
// results (a sample inside the map or not, floor/ceil, IoU > threshold, sort order) are discontinuous, and a multiply fused into the
// following add moves them.  HIP's __fmul_rn / __fadd_rn do not prevent that: they are plain operators in a header parsed before this
// pragma, so their operations stay fusable after inlining -- the helpers below are compiled under it.
#pragma clang fp contract(off)
namespace dcap {
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }      // correctly rounded: hipcc's default for fp32 division
}

namespace dcap {

__device__ __forceinline__ int roi_level(float y1, float x1, float y2, float x2, float image_area) {
    const float h = sub_rn(y2, y1), w = sub_rn(x2, x1);
    const float ratio = div_rn(__fsqrt_rn(mul_rn(h, w)), div_rn(224.0f, __fsqrt_rn(image_area)));
    const float lvl = div_rn(logf(ratio), logf(2.0f));
    if (!(lvl > -100.f)) return 2;          // log(0) = -inf, NaN: TF's int cast underflows, the clamp gives 2
    const int r = (int)rintf(lvl);          // round half to even, like tf.round
    return min(5, max(2, 4 + r));
}

// Sample coordinates of bin row / column `p` of a box on a map of extent n (TF's operation order).
__device__ __forceinline__ float roi_sample(float lo, float hi, int p, int n, int pool) {
    if (pool > 1) {
        const float step = div_rn(mul_rn(sub_rn(hi, lo), (float)(n - 1)), (float)(pool - 1));
        return add_rn(mul_rn(lo, (float)(n - 1)), mul_rn((float)p, step));
    }
    return mul_rn(mul_rn(0.5f, add_rn(lo, hi)), (float)(n - 1));
}

// The one sample of bin (py, px) of box bx = (y1, x1, y2, x2) on an H x W map: its coordinates, whether it lies inside the map (outside:
// the bin is zero and no pixel is read) and the rows / columns of its four corner pixels.  The forward kernel and the tile-group list
// (roi_tile_groups_kernel) take every decision here, so the list can never disagree with what the forward reads.
struct RoiBin {
    float in_y, in_x;
    bool ok;
    int top, bot, left, right;
};
__device__ __forceinline__ RoiBin roi_bin(const float4& bx, int py, int px, int H, int W, int pool) {
    RoiBin r;
    r.in_y = roi_sample(bx.x, bx.z, py, H, pool);
    r.in_x = roi_sample(bx.y, bx.w, px, W, pool);
    r.ok = (r.in_y >= 0.f) && (r.in_y <= (float)(H - 1)) && (r.in_x >= 0.f) && (r.in_x <= (float)(W - 1));
    r.top = (int)floorf(r.in_y);
    r.bot = (int)ceilf(r.in_y);
    r.left = (int)floorf(r.in_x);
    r.right = (int)ceilf(r.in_x);
    return r;
}

__global__ __launch_bounds__(256) void roi_align_kernel(dc_roialign_desc d) {
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    const int bins = d.pool * d.pool;
    const int total = d.B * d.R * bins;
    if (wave >= total) return;
    const int box = wave / bins, bin = wave - box * bins;
    const int py = bin / d.pool, px = bin - py * d.pool;
    const float4 bx = reinterpret_cast<const float4*>(d.boxes)[box];       // y1,x1,y2,x2
    const int lvl = roi_level(bx.x, bx.y, bx.z, bx.w, d.image_area);
    if (d.levels_out && bin == 0 && lane == 0) d.levels_out[box] = lvl;
    const int li = lvl - 2;
    const int H = d.Hs[li], W = d.Ws[li], C4 = d.C >> 2;
    const float* fm = d.maps[li] + (long)(box / d.R) * H * W * d.C;
    float4* out = reinterpret_cast<float4*>(d.out) + (long)wave * C4;

    const RoiBin sb = roi_bin(bx, py, px, H, W, d.pool);
    if (!sb.ok) {
        for (int c = lane; c < C4; c += 64) out[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const int top = sb.top, bot = sb.bot, left = sb.left, right = sb.right;
    const float ly = sb.in_y - (float)top, lx = sb.in_x - (float)left;
    const float4* tl = reinterpret_cast<const float4*>(fm + ((long)top * W + left) * d.C);
    const float4* tr = reinterpret_cast<const float4*>(fm + ((long)top * W + right) * d.C);
    const float4* bl = reinterpret_cast<const float4*>(fm + ((long)bot * W + left) * d.C);
    const float4* br = reinterpret_cast<const float4*>(fm + ((long)bot * W + right) * d.C);
    for (int c = lane; c < C4; c += 64) {
        const float4 a = tl[c], b = tr[c], e = bl[c], f = br[c];
        float4 o;
#define DC_LERP(k)                                  \
    {                                               \
        const float t = a.k + (b.k - a.k) * lx;     \
        const float u = e.k + (f.k - e.k) * lx;     \
        o.k = t + (u - t) * ly;                     \
    }
        DC_LERP(x) DC_LERP(y) DC_LERP(z) DC_LERP(w)
        out[c] = o;
    }
}

// backward, DETERMINISTIC (round 3): gather per destination pixel instead of an atomic scatter per bin.  One wave per pixel of
// a pyramid level: the lanes test 64 RoIs at a time (routed to this level? does its sampling grid come within one pixel of
// this one?), the hits are then visited in ascending (RoI, bin row, bin column) order -- the same order on every run and on
// every rank -- and each contributing bin adds  weight x its 256-channel gradient row  (four channels per lane) to a register
// accumulator that is added to the map with ONE plain read-modify-write.  weight = the bilinear corner weight the forward used:
//   wy = [y == floor(in_y)] (1 - ly) + [y == ceil(in_y)] ly,  wx likewise  (both terms when in_y is integral: 1).
// No float atomics: the joint model's FPN / RPN gradients become bit-reproducible (they were the only ones that were not).
constexpr int RA_MAX_POOL = 16;

__global__ __launch_bounds__(256) void roi_align_bwd_gather_kernel(dc_roialign_desc d, int li, long wave0) {
    const int lane = threadIdx.x & 63;
    const long wv = wave0 + (((long)blockIdx.x * 256 + threadIdx.x) >> 6);
    const int H = d.Hs[li], W = d.Ws[li];
    const long per_img = (long)H * W;
    if (wv >= (long)d.B * per_img) return;
    const int img = (int)(wv / per_img);
    const int pix = (int)(wv - (long)img * per_img);
    const int y = pix / W, x = pix - y * W;
    const float4* boxes = reinterpret_cast<const float4*>(d.boxes) + (long)img * d.R;
    const int bins = d.pool * d.pool;
    float4 acc[4];                                   // channels 4 lane .. 4 lane + 3 (+ 256 k): C <= 1024
    const int C4 = d.C >> 2, nchunk = (C4 + 63) >> 6;
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    bool any = false;
    for (int b0 = 0; b0 < d.R; b0 += 64) {
        const int bi = b0 + lane;
        bool hit = false;
        if (bi < d.R) {
            const float4 bx = boxes[bi];
            if (roi_level(bx.x, bx.y, bx.z, bx.w, d.image_area) - 2 == li) {
                // the sampling grid spans [in(0), in(pool - 1)] (either order for a flipped box): can it touch row y / column x?
                const float ya = roi_sample(bx.x, bx.z, 0, H, d.pool), yb = roi_sample(bx.x, bx.z, d.pool - 1, H, d.pool);
                const float xa = roi_sample(bx.y, bx.w, 0, W, d.pool), xb = roi_sample(bx.y, bx.w, d.pool - 1, W, d.pool);
                hit = fminf(ya, yb) < (float)y + 1.f && fmaxf(ya, yb) > (float)y - 1.f && fminf(xa, xb) < (float)x + 1.f && fmaxf(xa, xb) > (float)x - 1.f;
            }
        }
        unsigned long long m = __ballot(hit);
        while (m) {                                  // wave-uniform: ascending RoI index
            const int j = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int box = b0 + j;
            const float4 bx = boxes[box];            // same address in every lane: one broadcast load
            float wys[RA_MAX_POOL], wxs[RA_MAX_POOL];
#pragma unroll 1
            for (int p = 0; p < d.pool; ++p) {
                const float iy = roi_sample(bx.x, bx.z, p, H, d.pool), ix = roi_sample(bx.y, bx.w, p, W, d.pool);
                float wy = 0.f, wx = 0.f;
                if (iy >= 0.f && iy <= (float)(H - 1)) {
                    const float ly = iy - floorf(iy);
                    if ((int)floorf(iy) == y) wy += 1.f - ly;
                    if ((int)ceilf(iy) == y) wy += ly;
                } else {
                    wy = -1.f;                       // this bin row is outside the map: the forward wrote zeros, no gradient
                }
                if (ix >= 0.f && ix <= (float)(W - 1)) {
                    const float lx = ix - floorf(ix);
                    if ((int)floorf(ix) == x) wx += 1.f - lx;
                    if ((int)ceilf(ix) == x) wx += lx;
                } else {
                    wx = -1.f;
                }
                wys[p] = wy;
                wxs[p] = wx;
            }
            const float* go = d.out + ((long)(img * d.R + box) * bins) * d.C;
#pragma unroll 1
            for (int py = 0; py < d.pool; ++py) {
                if (!(wys[py] > 0.f)) continue;
#pragma unroll 1
                for (int px = 0; px < d.pool; ++px) {
                    if (!(wxs[px] > 0.f)) continue;
                    const float wgt = wys[py] * wxs[px];
                    const float4* row = reinterpret_cast<const float4*>(go + (long)(py * d.pool + px) * d.C);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < nchunk && lane + 64 * k < C4) {
                            const float4 g = row[lane + 64 * k];
                            acc[k].x += g.x * wgt; acc[k].y += g.y * wgt; acc[k].z += g.z * wgt; acc[k].w += g.w * wgt;
                        }
                    any = true;
                }
            }
        }
    }
    if (!any) return;
    float4* dst = reinterpret_cast<float4*>(const_cast<float*>(d.maps[li]) + ((long)img * per_img + pix) * d.C);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < nchunk && lane + 64 * k < C4) {
            float4 v = dst[lane + 64 * k];
            v.x += acc[k].x; v.y += acc[k].y; v.z += acc[k].z; v.w += acc[k].w;
            dst[lane + 64 * k] = v;
        }
}

// ------------------------------------------------------------------------------------------------------------------------
// The tile groups of the pyramid maps that roi_align_kernel reads for a set of boxes (dc_roi_tile_groups): the FPN output convolutions
// then compute those groups only (conv_wino.hip, wino32b_list_kernel).  ONE block: (1) clear the marks, one per group, the four levels
// end to end, (2) thread per (box, bin): the forward's own routing and sample (roi_level, roi_bin), a mark on the group of each of the
// four corner pixels at the routed level -- a sample outside the map marks nothing, as the forward reads nothing there --, (3) one
// ballot scan over all marks, RG_THREADS at a time: a marked group goes to its level's list at its rank among the level's marks, so
// every list is in ascending group index (image-major, group row, group column: the dense item walk's index), and counts[level] is
// the level's number of marks.  Plain stores only; the same lists in the same order on every run.  The marks live in LDS when they fit
// (RG_LDS_MARKS: 1360 groups at two 1024 x 1024 images) -- the launch is then two global round trips deep, the boxes in and the lists
// out -- and in the caller's scratch otherwise.
// (4) dc_roi_tile_groups_lateral only: the tiles of the level-2 LATERAL map (t2, the input of fpn_p2) that the list-driven fpn_p2 reads --
// every listed level-2 group plus whatever lies within one pixel of it: the group itself and its up to eight neighbours in the group
// grid of the SAME image (no wrap across a group row, none from one image into the next).  A second ballot scan over the level-2
// groups, each thread OR-ing the up to nine marks around its group; ascending list, device-side count, plain stores.
// ------------------------------------------------------------------------------------------------------------------------
constexpr int RG_THREADS = 1024, RG_WAVES = RG_THREADS / 64, RG_LDS_MARKS = 8192;
struct RoiGroupsArgs {
    dc_roi_groups_desc d;
    int gy[4], gx[4], off[5];        // tile groups per image (rows, columns); the level's first mark, off[4] = all marks
    int* lat_list;                   // optional: the level-2 lateral tile list (off[1] entries of room) and its count
    int* lat_count;
};

__global__ __launch_bounds__(RG_THREADS) void roi_tile_groups_kernel(RoiGroupsArgs a) {
    const dc_roi_groups_desc& d = a.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ int lds_marks[RG_LDS_MARKS];
    __shared__ int wsum[4][RG_WAVES];                    // per wave: marks of the chunk [0] in all, [l] below level l's first mark
    const int nmarks = a.off[4];
    int* marks = nmarks <= RG_LDS_MARKS ? lds_marks : d.marks;
    for (int i = tid; i < nmarks; i += RG_THREADS) marks[i] = 0;
    __syncthreads();
    const int bins = d.pool * d.pool, samples = d.B * d.R * bins;
    for (int s = tid; s < samples; s += RG_THREADS) {
        const int box = s / bins, bin = s - box * bins;
        const int py = bin / d.pool, px = bin - py * d.pool;
        const float4 bx = reinterpret_cast<const float4*>(d.boxes)[box];
        const int li = roi_level(bx.x, bx.y, bx.z, bx.w, d.image_area) - 2;
        const RoiBin sb = roi_bin(bx, py, px, d.Hs[li], d.Ws[li], d.pool);
        if (!sb.ok) continue;
        int* m = marks + a.off[li] + (box / d.R) * a.gy[li] * a.gx[li];
        const int gt = sb.top / kWinoGroupH * a.gx[li], gb = sb.bot / kWinoGroupH * a.gx[li];
        const int gl = sb.left / kWinoGroupW, gr = sb.right / kWinoGroupW;
        m[gt + gl] = 1;
        m[gt + gr] = 1;
        m[gb + gl] = 1;
        m[gb + gr] = 1;
    }
    __syncthreads();
    int below[4] = {0, 0, 0, 0};                         // marks seen so far: [0] in all, [l] below level l's first mark (block-uniform)
    for (int c0 = 0; c0 < nmarks; c0 += RG_THREADS) {
        const int i = c0 + tid;
        const bool on = i < nmarks && marks[i] != 0;
        const int l = i >= a.off[3] ? 3 : (i >= a.off[2] ? 2 : (i >= a.off[1] ? 1 : 0));
        const int first = l == 3 ? a.off[3] : (l == 2 ? a.off[2] : (l == 1 ? a.off[1] : 0));       // (a.off[0] = 0)
        const unsigned long long b = __ballot(on);
        const unsigned long long b1 = __ballot(on && i < a.off[1]), b2 = __ballot(on && i < a.off[2]), b3 = __ballot(on && i < a.off[3]);
        if (lane == 0) {
            wsum[0][wave] = __popcll(b);
            wsum[1][wave] = __popcll(b1);
            wsum[2][wave] = __popcll(b2);
            wsum[3][wave] = __popcll(b3);
        }
        __syncthreads();
        int before = 0, add[4] = {0, 0, 0, 0};
#pragma unroll
        for (int w = 0; w < RG_WAVES; ++w) {
            before += w < wave ? wsum[0][w] : 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) add[k] += wsum[k][w];
        }
        // rank among ALL marks, less the marks below this level's first one: they all lie in this chunk or an earlier one
        const int rank = below[0] + before + __popcll(b & ((1ull << lane) - 1ull));
        const int lower = l == 3 ? below[3] + add[3] : (l == 2 ? below[2] + add[2] : (l == 1 ? below[1] + add[1] : 0));
        if (on) d.lists[l][rank - lower] = i - first;
#pragma unroll
        for (int k = 0; k < 4; ++k) below[k] += add[k];
        __syncthreads();
    }
    if (tid < 4) {                                       // every mark below level l + 1's first one, less those below level l's
        const int lo = tid == 3 ? below[3] : (tid == 2 ? below[2] : (tid == 1 ? below[1] : 0));
        const int hi = tid == 3 ? below[0] : (tid == 2 ? below[3] : (tid == 1 ? below[2] : below[1]));
        d.counts[tid] = hi - lo;
    }
    if (a.lat_list == nullptr) return;                   // (block-uniform)
    // the main scan's last barrier is behind every thread: wsum[0] is free, the marks are final
    const int n0 = a.off[1], gy0 = a.gy[0], gx0 = a.gx[0], gpi0 = gy0 * gx0;
    int listed = 0;                                      // lateral tiles so far (block-uniform)
    for (int c0 = 0; c0 < n0; c0 += RG_THREADS) {
        const int i = c0 + tid;
        bool on = false;
        if (i < n0) {
            const int img = i / gpi0, gr = i - img * gpi0, y = gr / gx0, x = gr - y * gx0;
            const int* m = marks + img * gpi0;
            for (int yy = max(y - 1, 0); yy <= min(y + 1, gy0 - 1); ++yy)
                for (int xx = max(x - 1, 0); xx <= min(x + 1, gx0 - 1); ++xx) on = on || m[yy * gx0 + xx] != 0;
        }
        const unsigned long long b = __ballot(on);
        if (lane == 0) wsum[0][wave] = __popcll(b);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < RG_WAVES; ++w) {
            before += w < wave ? wsum[0][w] : 0;
            all += wsum[0][w];
        }
        if (on) a.lat_list[listed + before + __popcll(b & ((1ull << lane) - 1ull))] = i;
        listed += all;
        __syncthreads();
    }
    if (tid == 0) a.lat_count[0] = listed;
}

// ------------------------------------------------------------------------------------------------------------------------
// dc_row_mean_f32: out[b][c] = (((x[b][0][c] + x[b][1][c]) + x[b][2][c]) + ...) / K -- the image-level feature vector, the mean of the
// RoIAlign block over its RoIs, in the order np.mean(float32[K, ...], axis=0) adds: sequentially over k, then ONE correctly rounded
// division.  Only the columns are parallel (12 544 of them, 1000 dependent adds each), so a block owns RM_COLS = 64 columns (196 blocks
// at C = 12 544: one per CU on most of the chip) and separates the two jobs: all four waves LOAD -- 16 lanes x float4 cover the block's
// 256-byte piece of a row, a wave instruction fetches four rows, the block RM_ROWS = 128 rows (32 KiB) per tile, every load of a tile
// issued before the first is waited for -- and stage the tile in LDS; wave 0 then ADDS, lane = column, row after row out of LDS, while
// the loads of the next tile are already in flight (two LDS tiles, one barrier per tile).  VEC: the float4 loads, where x, ld and the
// batch stride keep every quad on a 16-byte boundary; otherwise (and for a quad that crosses C) the same walk with four guarded scalar
// loads per lane.  Rows past K are staged as zeros and never added.
// ------------------------------------------------------------------------------------------------------------------------
constexpr int RM_COLS = 64, RM_ROWS = 128, RM_THREADS = 256, RM_LOADS = RM_ROWS * (RM_COLS / 4) / RM_THREADS;      // 8 quads per lane and tile

template <bool VEC>
__device__ __forceinline__ void row_mean_load(const float* xb, long ld, int K, int C, int t0, int c, int r0, float4 (&v)[RM_LOADS]) {
#pragma unroll
    for (int j = 0; j < RM_LOADS; ++j) {
        const int row = t0 + r0 + 16 * j;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row >= K || c >= C) continue;
        const float* p = xb + (long)row * ld + c;
        if (VEC && c + 3 < C) {
            v[j] = *reinterpret_cast<const float4*>(p);
        } else {
            v[j].x = p[0];
            if (c + 1 < C) v[j].y = p[1];
            if (c + 2 < C) v[j].z = p[2];
            if (c + 3 < C) v[j].w = p[3];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(RM_THREADS) void row_mean_kernel(const float* x, int K, int C, long ld, long batch_stride, float* out, long ld_out) {
    __shared__ float4 tile[2][RM_ROWS][RM_COLS / 4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int c0 = blockIdx.x * RM_COLS;
    const float* xb = x + (long)blockIdx.y * batch_stride;
    const int r0 = wave * 4 + (lane >> 4), q = lane & 15;      // this lane's row within a round of 16, its quad of columns
    const int c = c0 + 4 * q;
    float4 v[RM_LOADS];
    row_mean_load<VEC>(xb, ld, K, C, 0, c, r0, v);
    float acc = 0.f;
    int buf = 0;
    for (int t0 = 0; t0 < K; t0 += RM_ROWS, buf ^= 1) {
#pragma unroll
        for (int j = 0; j < RM_LOADS; ++j) tile[buf][r0 + 16 * j][q] = v[j];
        __syncthreads();                                         // the tile is whole; wave 0 is done with the other one
        if (t0 + RM_ROWS < K) row_mean_load<VEC>(xb, ld, K, C, t0 + RM_ROWS, c, r0, v);
        if (wave == 0) {
            const float* col = reinterpret_cast<const float*>(&tile[buf][0][0]) + lane;
            const int rows = min(RM_ROWS, K - t0);
#pragma unroll 8
            for (int r = 0; r < rows; ++r) acc = add_rn(acc, col[r * RM_COLS]);
        }
    }
    if (wave == 0 && c0 + lane < C) out[(long)blockIdx.y * ld_out + c0 + lane] = div_rn(acc, (float)K);
}

}  // namespace dcap

using namespace dcap;

extern "C" int dc_row_mean_f32(const float* x, int B, int K, int C, long ld, long batch_stride, float* out, long ld_out, void* stream) {
    DC_REQUIRE(x && out, DC_EINVAL, "dc_row_mean: null pointer");
    DC_REQUIRE(B > 0 && B <= 65535 && K > 0 && K < (1 << 24) && C > 0, DC_EINVAL, "dc_row_mean: bad B/K/C (1 <= B <= 65535, 1 <= K < 2^24, C >= 1)");
    DC_REQUIRE(ld >= C && ld_out >= C && (B == 1 || batch_stride >= 0), DC_EINVAL, "dc_row_mean: a row stride below C or a negative batch stride");
    const dim3 grid((unsigned)((C + RM_COLS - 1) / RM_COLS), (unsigned)B);
    const bool vec = aligned16(x) && ld % 4 == 0 && (B == 1 || batch_stride % 4 == 0);
    if (vec)
        hipLaunchKernelGGL(row_mean_kernel<true>, grid, dim3(RM_THREADS), 0, static_cast<hipStream_t>(stream), x, K, C, ld, batch_stride, out, ld_out);
    else
        hipLaunchKernelGGL(row_mean_kernel<false>, grid, dim3(RM_THREADS), 0, static_cast<hipStream_t>(stream), x, K, C, ld, batch_stride, out, ld_out);
    return check_launch("row_mean_kernel");
}

static int roi_tile_groups_launch(const dc_roi_groups_desc* d, int32_t* lat_list, int32_t* lat_count, void* stream) {
    DC_REQUIRE(d && d->boxes && d->marks && d->counts, DC_EINVAL, "dc_roi_tile_groups: null pointer");
    DC_REQUIRE(d->B > 0 && d->R > 0 && d->pool > 0, DC_EINVAL, "dc_roi_tile_groups: bad B/R/pool");
    DC_REQUIRE(aligned16(d->boxes), DC_EALIGN, "dc_roi_tile_groups: boxes not 16-byte aligned");
    RoiGroupsArgs a;
    a.d = *d;
    a.lat_list = lat_list;
    a.lat_count = lat_count;
    long off = 0;
    for (int l = 0; l < 4; ++l) {
        DC_REQUIRE(d->lists[l] && d->Hs[l] > 0 && d->Ws[l] > 0, DC_EINVAL, "dc_roi_tile_groups: bad level %d", l);
        a.gy[l] = wino_groups_y(d->Hs[l]);
        a.gx[l] = wino_groups_x(d->Ws[l]);
        a.off[l] = (int)off;
        off += (long)d->B * a.gy[l] * a.gx[l];
    }
    a.off[4] = (int)off;
    DC_REQUIRE(off < (1l << 30) && (long)d->B * d->R * d->pool * d->pool < (1l << 30), DC_EINVAL, "dc_roi_tile_groups: too many groups / samples");
    hipLaunchKernelGGL(roi_tile_groups_kernel, dim3(1), dim3(RG_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("roi_tile_groups_kernel");
}

extern "C" int dc_roi_tile_groups(const dc_roi_groups_desc* d, void* stream) { return roi_tile_groups_launch(d, nullptr, nullptr, stream); }

extern "C" int dc_roi_tile_groups_lateral(const dc_roi_groups_desc* d, int32_t* lat_list, int32_t* lat_count, void* stream) {
    DC_REQUIRE(lat_list && lat_count, DC_EINVAL, "dc_roi_tile_groups_lateral: null lateral list / count");
    return roi_tile_groups_launch(d, lat_list, lat_count, stream);
}

extern "C" int dc_roi_align_pyramid_bwd_f32(const dc_roialign_desc* d, void* stream) {
    DC_REQUIRE(d && d->boxes && d->out, DC_EINVAL, "dc_roi_align_pyramid_bwd: null pointer");
    DC_REQUIRE(d->B > 0 && d->R > 0 && d->pool > 0 && d->pool <= RA_MAX_POOL && d->C > 0 && (d->C & 3) == 0 && d->C <= 1024, DC_EINVAL,
               "dc_roi_align_pyramid_bwd: bad B/R/pool/C (pool <= 16, C a multiple of 4 and <= 1024)");
    for (int l = 0; l < 4; ++l) {
        DC_REQUIRE(d->maps[l] && d->Hs[l] > 0 && d->Ws[l] > 0, DC_EINVAL, "dc_roi_align_pyramid_bwd: bad map %d", l);
        DC_REQUIRE(aligned16(d->maps[l]), DC_EALIGN, "dc_roi_align_pyramid_bwd: gradient map %d not 16-byte aligned", l);
    }
    DC_REQUIRE(aligned16(d->boxes) && aligned16(d->out), DC_EALIGN, "dc_roi_align_pyramid_bwd: boxes / dout not 16-byte aligned");
    for (int l = 0; l < 4; ++l) {
        const long waves = (long)d->B * d->Hs[l] * d->Ws[l];
        for (long w0 = 0; w0 < waves; w0 += 4L * 0x40000000) {       // (grids stay below 2^31 blocks)
            const long n = std::min(waves - w0, 4L * 0x40000000);
            hipLaunchKernelGGL(roi_align_bwd_gather_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), *d, l, w0);
        }
        int rc = check_launch("roi_align_bwd_gather_kernel");
        if (rc) return rc;
    }
    return DC_OK;
}

extern "C" int dc_roi_align_pyramid_f32(const dc_roialign_desc* d, void* stream) {
    DC_REQUIRE(d && d->boxes && d->out, DC_EINVAL, "dc_roi_align_pyramid: null pointer");
    DC_REQUIRE(d->B > 0 && d->R > 0 && d->pool > 0 && d->C > 0 && (d->C & 3) == 0, DC_EINVAL, "dc_roi_align_pyramid: bad B/R/pool/C");
    for (int l = 0; l < 4; ++l) {
        DC_REQUIRE(d->maps[l] && d->Hs[l] > 0 && d->Ws[l] > 0, DC_EINVAL, "dc_roi_align_pyramid: bad feature map %d", l);
        DC_REQUIRE(aligned16(d->maps[l]), DC_EALIGN, "dc_roi_align_pyramid: feature map %d not 16-byte aligned", l);
    }
    DC_REQUIRE(aligned16(d->boxes) && aligned16(d->out), DC_EALIGN, "dc_roi_align_pyramid: boxes/out not 16-byte aligned");
    const long waves = (long)d->B * d->R * d->pool * d->pool;
    const int blocks = (int)((waves + 3) / 4);
    hipLaunchKernelGGL(roi_align_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), *d);
    return check_launch("roi_align_kernel");
}

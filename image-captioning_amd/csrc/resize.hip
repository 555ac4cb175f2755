// Resize + zero-pad of raw uint8 RGB images into the encoder's [B][H][W][3] canvas, bit for bit what
// PIL.Image.resize((new_w, new_h), resample=BILINEAR) followed by np.pad gives (utils.resize_image: the host path this replaces).
//
// PIL's ImagingResample for 8-bit channels is two separable passes with integer coefficients: per axis and output index a window
// [xmin, xmin + n) of the source and n weights of the triangle filter, normalised in float64 and rounded to 22 fractional bits;
// a pixel is clamp(((1 << 21) + sum k * p) >> 22).  The horizontal pass runs first into a uint8 intermediate [h][new_w][3], the
// vertical pass reads that.  A pass whose size does not change comes out of the formulas as the identity (weights 2^22 and 0).
//
// Three launches serve the whole batch (blockIdx.z = image; an image smaller than the batch's largest leaves blocks idle):
//   resize_coef_kernel  one thread per (axis, output index): window and coefficients from the four sizes alone, into the workspace
//   resize_h_kernel     one thread per byte of the intermediate
//   resize_v_kernel     one thread per byte of the canvas: the vertical pass inside the image's window, 0 everywhere else
// Every access to the images and the canvas is a single byte, so neither has an alignment rule.
//
// dc_resize_pad_flip_u8 adds load_image_gt's augmentation, the mirror of the PADDED square (image[:, ::-1] behind np.pad), per image:
// the first two launches are the unflipped call's, and the vertical kernel's thread for canvas byte (x, c) of a flagged image computes
// the unflipped canvas' byte (W - 1 - x, c) -- the same window test, the same column of the intermediate, the same coefficients and
// sum -- and stores it at (x, c).  Nothing is resampled from a mirrored source, so the mirrored bytes are the unflipped pass's by
// construction.  The flags are an int32 [B] block inside the packed buffer (one upload); the old entry point passes none.
#include "dcap_internal.h"
#include "resize_core.h"
#include <math.h>

// The coefficients are the host C code's only if every operation rounds once: no fused multiply-add (resize_core.h, shared with
// detect.hip, says so for its own body; this keeps the whole file that way).
#pragma clang fp contract(off)

namespace dcap {

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_GRID_Y = 65535;
constexpr size_t RS_LIMIT = (size_t)1 << 31;       // every byte count and offset fits int32

// One axis' table in the workspace: bounds [out][2] = (xmin, n), then coefficients tap-major [tap][out] so that neighbouring output
// indices read neighbouring words.
struct ResizeAxis {
    const int* bounds;
    const int* coefs;
};

// Image b's tables: the x axis at slot b of the first region (ax ints per slot), the y axis at slot b of the second (ay ints).
__device__ __forceinline__ int* resize_axis_table(int* tables, int B, int b, int axis, int ax, int ay) {
    return axis == 0 ? tables + (size_t)b * ax : tables + (size_t)B * ax + (size_t)b * ay;
}

__global__ __launch_bounds__(RS_THREADS) void resize_coef_kernel(const int* __restrict__ rec, int* __restrict__ tables, int B, int ax, int ay) {
    const int b = blockIdx.z, axis = blockIdx.y;
    const int* r = rec + b * DC_RESIZE_RECORD_INTS;
    const int in_size = axis == 0 ? r[2] : r[1], out_size = axis == 0 ? r[4] : r[3];
    const int xx = blockIdx.x * RS_THREADS + threadIdx.x;
    if (xx >= out_size) return;
    int* bounds = resize_axis_table(tables, B, b, axis, ax, ay);
    int* coefs = bounds + 2 * (size_t)out_size;
    resize_axis_coefs(in_size, out_size, xx, bounds, coefs);
}

// mid[y][xx][c] = clip8((1 << 21) + sum_t k[t][xx] * src[y][xmin + t][c]); thread = byte j = xx * 3 + c of the row, rows grid-strided
__global__ __launch_bounds__(RS_THREADS) void resize_h_kernel(const uint8_t* __restrict__ packed, const int* __restrict__ rec,
                                                              const int* __restrict__ tables, uint8_t* __restrict__ mids, int B, int ax, int ay) {
    const int b = blockIdx.z;
    const int* r = rec + b * DC_RESIZE_RECORD_INTS;
    const int h = r[1], w = r[2], new_w = r[4];
    const int j = blockIdx.x * RS_THREADS + threadIdx.x;
    if (j >= new_w * 3) return;
    const int xx = j / 3, c = j - xx * 3;
    const int* bounds = tables + (size_t)b * ax;
    const int* coefs = bounds + 2 * (size_t)new_w;
    const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
    const uint8_t* src = packed + r[0] + xmin * 3 + c;
    uint8_t* mid = mids + r[7] + j;
    for (int y = blockIdx.y; y < h; y += gridDim.y) {
        const uint8_t* p = src + (size_t)y * w * 3;
        int acc = 1 << (RS_PRECISION_BITS - 1);
        for (int t = 0; t < n; ++t) acc += coefs[(size_t)t * new_w + xx] * (int)p[t * 3];
        mid[(size_t)y * new_w * 3] = resize_clip8(acc);
    }
}

// out[b][yy][j]: inside the window (rows top .. top + new_h, bytes left * 3 .. (left + new_w) * 3) the vertical pass over the
// intermediate's column j - left * 3, outside it 0.  The pass never looks at channels: a row is new_w * 3 independent columns.
// flips (null: no image is mirrored) holds one int32 per image; with flips[b] == 1 the thread of byte j = x * 3 + c computes the
// unflipped row's byte js = (W - 1 - x) * 3 + c and stores it at j.
__global__ __launch_bounds__(RS_THREADS) void resize_v_kernel(const int* __restrict__ rec, const int* __restrict__ tables,
                                                              const uint8_t* __restrict__ mids, uint8_t* __restrict__ out,
                                                              const int* __restrict__ flips, int B, int H, int W, int ax, int ay) {
    const int b = blockIdx.z;
    const int* r = rec + b * DC_RESIZE_RECORD_INTS;
    const int new_h = r[3], row = r[4] * 3, top = r[5], left = r[6] * 3;
    const int j = blockIdx.x * RS_THREADS + threadIdx.x;
    if (j >= W * 3) return;
    int js = j;
    if (flips != nullptr && flips[b] != 0) {
        const int x = j / 3;
        js = (W - 1 - x) * 3 + (j - x * 3);
    }
    const int* bounds = tables + (size_t)B * ax + (size_t)b * ay;
    const int* coefs = bounds + 2 * (size_t)new_h;
    const bool in_x = js >= left && js < left + row;
    const uint8_t* mid = mids + r[7] + (js - left);
    uint8_t* o = out + ((size_t)b * H * W) * 3 + j;
    for (int yy = blockIdx.y; yy < H; yy += gridDim.y) {
        const int y = yy - top;
        uint8_t v = 0;
        if (in_x && y >= 0 && y < new_h) {
            const int ymin = bounds[2 * y], n = bounds[2 * y + 1];
            const uint8_t* p = mid + (size_t)ymin * row;
            int acc = 1 << (RS_PRECISION_BITS - 1);
            for (int t = 0; t < n; ++t) acc += coefs[(size_t)t * new_h + y] * (int)p[(size_t)t * row];
            v = resize_clip8(acc);
        }
        o[(size_t)yy * W * 3] = v;
    }
}

struct ResizeWs {
    size_t mid_bytes, tables, total;      // the intermediates, then (16-byte aligned) the tables: B slots of ax ints, B slots of ay ints
    int ax, ay, max_h, max_mid_row;
};

// Everything the host decides, from ITS copy of the records; 0 and the layout in *L, or an error code.
static int resize_plan(const dc_resize_pad_desc* d, ResizeWs* L) {
    DC_REQUIRE(d && d->packed && d->records && d->out, DC_EINVAL, "dc_resize_pad_u8: null descriptor, packed buffer, records or canvas");
    DC_REQUIRE(d->B >= 1 && d->B <= RS_MAX_GRID_Y && d->H >= 1 && d->W >= 1, DC_EINVAL,
               "dc_resize_pad_u8: B in 1..%d and a canvas of at least 1 x 1, got B %d, canvas %d x %d", RS_MAX_GRID_Y, d->B, d->H, d->W);
    DC_REQUIRE((reinterpret_cast<uintptr_t>(d->packed) & 3u) == 0, DC_EINVAL,
               "dc_resize_pad_u8: the packed buffer starts with int32 records, so it must sit on a 4-byte boundary (the images in it need not)");
    const size_t head = (size_t)d->B * DC_RESIZE_RECORD_INTS * sizeof(int32_t);
    DC_REQUIRE(d->packed_bytes < RS_LIMIT && (size_t)d->B * d->H * d->W * 3 < RS_LIMIT, DC_EINVAL,
               "dc_resize_pad_u8: the packed buffer (%zu bytes) and the canvas must stay below 2^31 bytes", d->packed_bytes);
    size_t mid = 0, ax = 0, ay = 0;
    int max_h = 0, max_row = 0;
    for (int b = 0; b < d->B; ++b) {
        const int32_t* r = d->records + (size_t)b * DC_RESIZE_RECORD_INTS;
        const long off = r[0], h = r[1], w = r[2], nh = r[3], nw = r[4], top = r[5], left = r[6];
        DC_REQUIRE(h >= 1 && w >= 1 && nh >= 1 && nw >= 1, DC_EINVAL, "dc_resize_pad_u8: image %d has a zero size (%ld x %ld -> %ld x %ld)", b, h, w,
                   nh, nw);
        DC_REQUIRE(top >= 0 && left >= 0 && top + nh <= d->H && left + nw <= d->W, DC_EINVAL,
                   "dc_resize_pad_u8: image %d's window (%ld, %ld) + %ld x %ld leaves the %d x %d canvas", b, top, left, nh, nw, d->H, d->W);
        DC_REQUIRE((size_t)h * w * 3 < RS_LIMIT && off >= (long)head && (size_t)off + (size_t)h * w * 3 <= d->packed_bytes, DC_EINVAL,
                   "dc_resize_pad_u8: image %d's %ld x %ld x 3 bytes at offset %ld leave the packed buffer (records %zu, total %zu bytes)", b, h, w,
                   off, head, d->packed_bytes);
        DC_REQUIRE((size_t)r[7] == mid, DC_EINVAL, "dc_resize_pad_u8: image %d's intermediate must start at workspace byte %zu, its record says %d",
                   b, mid, r[7]);
        mid += (size_t)h * nw * 3;
        DC_REQUIRE(mid < RS_LIMIT, DC_EINVAL, "dc_resize_pad_u8: the intermediates must stay below 2^31 bytes");
        const size_t tx = (size_t)nw * (2 + resize_ksize((int)w, (int)nw)), ty = (size_t)nh * (2 + resize_ksize((int)h, (int)nh));
        ax = tx > ax ? tx : ax;
        ay = ty > ay ? ty : ay;
        max_h = h > max_h ? (int)h : max_h;
        max_row = nw * 3 > max_row ? (int)nw * 3 : max_row;
    }
    DC_REQUIRE(ax < RS_LIMIT / 4 && ay < RS_LIMIT / 4, DC_EINVAL, "dc_resize_pad_u8: a coefficient table must stay below 2^31 bytes");
    L->mid_bytes = mid;
    L->tables = (mid + 15) & ~(size_t)15;
    L->total = L->tables + (size_t)d->B * (ax + ay) * sizeof(int);
    L->ax = (int)ax, L->ay = (int)ay, L->max_h = max_h, L->max_mid_row = max_row;
    DC_REQUIRE(L->total < RS_LIMIT, DC_EINVAL, "dc_resize_pad_u8: the workspace must stay below 2^31 bytes");
    return DC_OK;
}

}  // namespace dcap

using namespace dcap;

extern "C" size_t dc_resize_pad_u8_workspace_bytes(const dc_resize_pad_desc* d) {
    ResizeWs L;
    if (resize_plan(d, &L)) return 0;
    return L.total;
}

// The three launches of both entry points; flips: the device's flag block, or null.
static int resize_launch(const dc_resize_pad_desc* d, const ResizeWs& L, const int* flips, void* workspace, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* mids = static_cast<uint8_t*>(workspace);
    int* tables = reinterpret_cast<int*>(mids + L.tables);
    const int* rec = reinterpret_cast<const int*>(d->packed);        // the device's copy of the records heads the packed buffer
    const int B = d->B;
    int max_out = 0;
    for (int b = 0; b < B; ++b) {
        const int32_t* r = d->records + (size_t)b * DC_RESIZE_RECORD_INTS;
        max_out = r[3] > max_out ? r[3] : max_out;
        max_out = r[4] > max_out ? r[4] : max_out;
    }
    auto blocks = [](int n) { return (unsigned)((n + RS_THREADS - 1) / RS_THREADS); };
    auto rows = [](int n) { return (unsigned)(n < RS_MAX_GRID_Y ? n : RS_MAX_GRID_Y); };
    hipLaunchKernelGGL(resize_coef_kernel, dim3(blocks(max_out), 2, B), dim3(RS_THREADS), 0, s, rec, tables, B, L.ax, L.ay);
    hipLaunchKernelGGL(resize_h_kernel, dim3(blocks(L.max_mid_row), rows(L.max_h), B), dim3(RS_THREADS), 0, s, d->packed, rec, tables, mids, B, L.ax,
                       L.ay);
    hipLaunchKernelGGL(resize_v_kernel, dim3(blocks(d->W * 3), rows(d->H), B), dim3(RS_THREADS), 0, s, rec, tables, mids, d->out, flips, B, d->H,
                       d->W, L.ax, L.ay);
    return check_launch("resize_pad kernels");
}

extern "C" int dc_resize_pad_u8(const dc_resize_pad_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    ResizeWs L;
    int rc = resize_plan(d, &L);
    if (rc) return rc;
    DC_REQUIRE(workspace && workspace_bytes >= L.total && aligned16(workspace), DC_EWORKSPACE,
               "dc_resize_pad_u8: needs %zu workspace bytes (16-byte aligned), got %zu", L.total, workspace_bytes);
    return resize_launch(d, L, nullptr, workspace, stream);
}

extern "C" int dc_resize_pad_flip_u8(const dc_resize_pad_desc* d, const int32_t* flips, size_t flips_offset, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    ResizeWs L;
    int rc = resize_plan(d, &L);
    if (rc) return rc;
    DC_REQUIRE(flips, DC_EINVAL, "dc_resize_pad_flip_u8: null flags (the host's copy of the B flags in the packed buffer)");
    const size_t head = (size_t)d->B * DC_RESIZE_RECORD_INTS * sizeof(int32_t), fbytes = (size_t)d->B * sizeof(int32_t);
    DC_REQUIRE((flips_offset & 3u) == 0, DC_EINVAL, "dc_resize_pad_flip_u8: the flags are int32, their block at byte %zu is off a 4-byte boundary",
               flips_offset);
    DC_REQUIRE(flips_offset >= head && flips_offset <= d->packed_bytes && fbytes <= d->packed_bytes - flips_offset, DC_EINVAL,
               "dc_resize_pad_flip_u8: the flags block [%zu, %zu) overlaps the records (%zu bytes) or leaves the packed buffer (%zu bytes)",
               flips_offset, flips_offset + fbytes, head, d->packed_bytes);
    for (int b = 0; b < d->B; ++b) {
        const int32_t* r = d->records + (size_t)b * DC_RESIZE_RECORD_INTS;
        const size_t off = (size_t)r[0], end = off + (size_t)r[1] * r[2] * 3;
        DC_REQUIRE(end <= flips_offset || off >= flips_offset + fbytes, DC_EINVAL,
                   "dc_resize_pad_flip_u8: the flags block [%zu, %zu) overlaps image %d's bytes [%zu, %zu)", flips_offset, flips_offset + fbytes, b, off,
                   end);
        DC_REQUIRE(flips[b] == 0 || flips[b] == 1, DC_EINVAL, "dc_resize_pad_flip_u8: image %d's flag is %d, a flag is 0 or 1", b, flips[b]);
    }
    DC_REQUIRE(workspace && workspace_bytes >= L.total && aligned16(workspace), DC_EWORKSPACE,
               "dc_resize_pad_flip_u8: needs %zu workspace bytes (16-byte aligned), got %zu", L.total, workspace_bytes);
    return resize_launch(d, L, reinterpret_cast<const int*>(d->packed + flips_offset), workspace, stream);
}

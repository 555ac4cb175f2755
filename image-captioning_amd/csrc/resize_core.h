// PIL's 8-bit bilinear resampling arithmetic, shared by resize.hip (RGB images into the encoder's canvas) and detect.hip (a detection's
// mask into its box): the per-axis window / coefficient computation of ImagingResample's precompute_coeffs + normalize_coeffs_8bpc and
// the pixel clamp.  One definition, so both callers carry the same bits.
#pragma once
#include <math.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace dcap {

constexpr int RS_PRECISION_BITS = 32 - 8 - 2;      // PIL's PRECISION_BITS: coefficients carry 22 fractional bits

// bilinear support is 1.0: the taps of one output index never exceed this (precompute_coeffs' ksize)
__host__ __device__ inline int resize_ksize(int in_size, int out_size) {
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(1.0 * fs) * 2 + 1;
}

// Output index xx of one axis (in_size -> out_size): bounds[2 xx] = (xmin, n) and the n coefficients tap-major at coefs[tap * out_size
// + xx].  The coefficients are the host C code's only if every operation rounds once: no fused multiply-add.
__device__ __forceinline__ void resize_axis_coefs(int in_size, int out_size, int xx, int* bounds, int* coefs) {
#pragma clang fp contract(off)
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs, ss = 1.0 / fs;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    const int n = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
        const double a = fabs((x + xmin - center + 0.5) * ss);
        ww += a < 1.0 ? 1.0 - a : 0.0;
    }
    for (int x = 0; x < n; ++x) {                    // the same weights again (same operations, same values), now normalised
        const double a = fabs((x + xmin - center + 0.5) * ss);
        double w = a < 1.0 ? 1.0 - a : 0.0;
        if (ww != 0.0) w /= ww;
        coefs[(size_t)x * out_size + xx] = (int)(0.5 + w * (double)(1 << RS_PRECISION_BITS));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = n;
}

__device__ __forceinline__ uint8_t resize_clip8(int acc) {
    const int v = acc >> RS_PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

}  // namespace dcap

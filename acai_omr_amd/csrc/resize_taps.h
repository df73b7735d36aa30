// The per-sample arithmetic of the bicubic antialiased resize, shared by resize.hip (one image per call) and page.hip (a table of boxes cut
// from pages per call) so that both write the same bits: the window of an output sample, its tap weights, the accumulation order and the
// nn.Unfold addressing of the patch form.  See resize.hip's header for the definitions (aten `_upsample_bicubic2d_aa`, align_corners = False).
#pragma once
#include "common.h"

namespace {

struct Axis {
    float scale, support, invscale;
    int in_size, max_taps;
};

__device__ __forceinline__ float cubic_aa(float x) {
    const float a = -0.5f;
    x = fabsf(x);
    if (x < 1.f) return ((a + 2.f) * x - (a + 3.f)) * x * x + 1.f;
    if (x < 2.f) return (((x - 5.f) * x + 8.f) * x - 4.f) * a;
    return 0.f;
}

__device__ __forceinline__ void window(const Axis &ax, int i, int &xmin, int &xsize, float &center) {
    center = (float)((double)ax.scale * ((double)i + 0.5));
    const long long lo = (long long)((double)(center - ax.support) + 0.5);
    const long long hi = (long long)((double)(center + ax.support) + 0.5);
    xmin = (int)(lo > 0 ? lo : 0);
    int n = (int)(hi < ax.in_size ? hi : ax.in_size) - xmin;
    xsize = n < 0 ? 0 : (n > ax.max_taps ? ax.max_taps : n);
}

__device__ __forceinline__ float tap_weight(const Axis &ax, int j, int xmin, float center) {
    return cubic_aa((float)(((double)((float)(j + xmin) - center) + 0.5) * (double)ax.invscale));
}

// Where the height pass puts its samples when it feeds the encoder directly ("direct packing into the token stream"): the
// crop window (DynamicResize's centre crop to the positional grid) of the resized image goes out as nn.Unfold(P, P) rows - sample (y, x) of
// the window -> row row0 + (y / P) (cw / P) + x / P, column (y % P) P + x % P - in fp32 or bf16: no image tensor, no patchify launch, no cast.
struct PatchOut {
    void *base;
    int ld, row0, P, top, left, ch, cw, bf16;
};

__device__ __forceinline__ float in_sample(const float *p) { return *p; }
__device__ __forceinline__ float in_sample(const unsigned char *p) { return (float)*p / 255.0f; }   // v2.ToDtype(torch.float32, scale=True) of a uint8 image

// Output sample i of an axis: the normalised taps over src[0], src[stride], ... where src points at element 0 of the resized axis.  This is
// the tap loop of resize_axis_kernel (resize.hip), statement for statement; that kernel keeps its own copy because routing it through here
// reorders its address arithmetic, and its generated code is held fixed.
template <typename TI>
__device__ __forceinline__ float resample(const Axis &ax, int i, const TI *src, size_t stride) {
    int xmin, xsize;
    float center;
    window(ax, i, xmin, xsize, center);
    float total = 0.f;
    for (int j = 0; j < xsize; ++j) total += tap_weight(ax, j, xmin, center);
    const float inv = total != 0.f ? 1.f / total : 0.f;
    src += (size_t)xmin * stride;
    float t = 0.f;
    for (int j = 0; j < xsize; ++j) {
        const float w = tap_weight(ax, j, xmin, center) * inv;
        t = j == 0 ? in_sample(src) * w : t + in_sample(src + (size_t)j * stride) * w;
    }
    return t;
}

// Sample (y, x) of the crop window's frame -> its element of the patch stream (the caller has checked it lies inside the window).
__device__ __forceinline__ void store_patch_sample(const PatchOut &po, int y, int xx, float t) {
    const size_t row = (size_t)po.row0 + (size_t)(y / po.P) * (po.cw / po.P) + xx / po.P;
    const int col = (y % po.P) * po.P + xx % po.P;
    if (po.bf16) reinterpret_cast<bf16_t *>(po.base)[row * po.ld + col] = f2bf(t);
    else reinterpret_cast<float *>(po.base)[row * po.ld + col] = t;
}

__host__ __device__ inline Axis make_axis(int in_size, int out_size) {
    Axis a;
    a.scale = (float)in_size / (float)out_size;
    a.support = a.scale >= 1.f ? 2.f * a.scale : 2.f;
    a.invscale = a.scale >= 1.f ? 1.f / a.scale : 1.f;
    a.in_size = in_size;
    a.max_taps = (int)ceilf(a.support) * 2 + 1;
    return a;
}

}  // namespace

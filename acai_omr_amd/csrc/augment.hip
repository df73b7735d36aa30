// Camera augmentation of the training input pipeline (acai_omr/train/pre_train.py:178-190, omr_teacher_force_train.py:320-331,
// omr_grpo_train.py:530-541): Gaussian blur, Gaussian noise, rotation, perspective warp, brightness / contrast jitter on one-channel fp32
// images, batched over a ragged list of images through a table of AcaiAugImage in device memory (include/acai_omr_hip.h has the arithmetic).
// Every kernel is one thread per output pixel, threads along x, grid (ceil(max W / 256), max H, images): a block outside its image's H x W,
// or of an image whose `apply` is 0, leaves at once, so one launch serves every image of the call.  HBM-bound and small next to the encoder:
// a stage reads and writes each image once (the 15 blur taps and the 4 bilinear corners of neighbouring threads hit L1 / L2).
// The warps evaluate their sampling coordinates in fp64 (a dozen DFMAs and, for the perspective, two divisions per pixel - nothing next to
// the memory time on this chip): fp32 coordinates near x = 2000 carry 1e-4 pixels of rounding, which a sharp staff line turns into 1e-4 of
// grey value.  The contrast mean is summed in a fixed order (per-thread strided fp64 sums, wave shuffles, ACAI_AUG_MEAN_PARTS partials per
// image added up in one order by every block of the last stage): no atomics, so a call is bit-reproducible.
#include "common.h"

namespace {

constexpr int TPB = 256;

__device__ __forceinline__ const float *slot_in(const AcaiAugImage &d, int slot) { return slot < 0 ? d.src : d.buf[slot]; }

// F.pad(mode="reflect") index: the edge pixel is not repeated.  Valid for -n < i < 2n - 1 (the host checks ktaps / 2 < n).
__device__ __forceinline__ int reflect(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

template <bool VERTICAL>
__global__ __launch_bounds__(TPB) void aug_blur_kernel(const AcaiAugImage *__restrict__ table, int in_slot, int out_slot, int add_noise) {
    const AcaiAugImage &d = table[blockIdx.z];
    const int x = blockIdx.x * TPB + threadIdx.x, y = blockIdx.y;
    if (!d.apply || y >= d.H || x >= d.W) return;
    const float *in = slot_in(d, in_slot);
    const int W = d.W, r = d.ktaps / 2;
    float acc = 0.f;
    for (int j = 0; j < d.ktaps; ++j) {
        const float v = VERTICAL ? in[(size_t)reflect(y + j - r, d.H) * W + x] : in[(size_t)y * W + reflect(x + j - r, W)];
        acc = fmaf(d.w[j], v, acc);
    }
    const size_t o = (size_t)y * W + x;
    if (VERTICAL && add_noise && d.noise) acc = clamp01(fmaf(d.noise_sigma, d.noise[o], acc));
    d.buf[out_slot][o] = acc;
}

// F.grid_sample(bilinear, padding_mode="zeros", align_corners=False) of the image and of an all-ones mask at pixel-index position (sx, sy),
// multiplied: corners outside the image contribute nothing to either.
__device__ __forceinline__ float sample_masked(const float *in, int H, int W, double sx, double sy) {
    if (!(sx > -1.0 && sx < (double)W && sy > -1.0 && sy < (double)H)) return 0.f;   // (also a NaN position: every corner is outside)
    const double fx0 = floor(sx), fy0 = floor(sy);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float tx = (float)(sx - fx0), ty = (float)(sy - fy0);
    const float wx[2] = {1.f - tx, tx}, wy[2] = {1.f - ty, ty};
    float img = 0.f, mask = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int xx = x0 + i, yy = y0 + j;
            if (xx >= 0 && xx < W && yy >= 0 && yy < H) {
                const float w = wx[i] * wy[j];
                img = fmaf(in[(size_t)yy * W + xx], w, img);
                mask += w;
            }
        }
    return img * mask;
}

template <bool PERSPECTIVE>
__global__ __launch_bounds__(TPB) void aug_warp_kernel(const AcaiAugImage *__restrict__ table, int in_slot, int out_slot) {
    const AcaiAugImage &d = table[blockIdx.z];
    const int x = blockIdx.x * TPB + threadIdx.x, y = blockIdx.y;
    if (!d.apply || y >= d.H || x >= d.W) return;
    const int H = d.H, W = d.W;
    double sx, sy;
    if (PERSPECTIVE) {
        const double X = x + 0.5, Y = y + 0.5;
        const double den = d.persp[6] * X + d.persp[7] * Y + 1.0;
        sx = (d.persp[0] * X + d.persp[1] * Y + d.persp[2]) / den - 0.5;
        sy = (d.persp[3] * X + d.persp[4] * Y + d.persp[5]) / den - 0.5;
    } else {
        const double xc = x + 0.5 - 0.5 * W, yc = y + 0.5 - 0.5 * H;
        sx = d.rot_cos * xc - d.rot_sin * yc + 0.5 * W - 0.5;
        sy = d.rot_sin * xc + d.rot_cos * yc + 0.5 * H - 0.5;
    }
    d.buf[out_slot][(size_t)y * W + x] = sample_masked(slot_in(d, in_slot), H, W, sx, sy);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Partial sums of the image the contrast step averages: the stage input, or clamp(input * fb) when brightness comes first.
// Block p of an image owns the contiguous p-th share of its pixels; every sum below runs in an order the launch shape fixes.
__global__ __launch_bounds__(TPB) void aug_mean_kernel(const AcaiAugImage *__restrict__ table, int in_slot) {
    const AcaiAugImage &d = table[blockIdx.z];
    if (!d.apply || !(d.jitter & ACAI_AUG_CONTRAST)) return;
    const float *in = slot_in(d, in_slot);
    const long long n = (long long)d.H * d.W, share = (n + ACAI_AUG_MEAN_PARTS - 1) / ACAI_AUG_MEAN_PARTS;
    const long long lo = blockIdx.x * share, hi = lo + share < n ? lo + share : n;
    const bool bright = (d.jitter & ACAI_AUG_BRIGHTNESS) && (d.jitter & ACAI_AUG_BRIGHTNESS_FIRST);
    double s = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += TPB) {
        const float v = in[i];
        s += (double)(bright ? clamp01(v * d.fb) : v);
    }
    s = wave_sum_f64(s);
    __shared__ double ws[TPB / 64];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) d.partials[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

struct AugPatchOut {
    void *base;   // nullptr: the image form
    int ld, P, bf16;
};

__global__ __launch_bounds__(TPB) void aug_jitter_out_kernel(const AcaiAugImage *__restrict__ table, int in_slot, int do_jitter, AugPatchOut po) {
    const AcaiAugImage &d = table[blockIdx.z];
    const int x = blockIdx.x * TPB + threadIdx.x, y = blockIdx.y;
    if (y >= d.H || blockIdx.x * TPB >= d.W) return;   // (whole blocks only: the barrier below is reached by every thread that stays)
    const bool jitter = d.apply && do_jitter;
    float mean = 0.f;
    if (jitter && (d.jitter & ACAI_AUG_CONTRAST)) {
        __shared__ float mean_s;
        if (threadIdx.x < 64) {
            static_assert(ACAI_AUG_MEAN_PARTS == 128, "two partials per lane of the first wave");
            const double t = wave_sum_f64(d.partials[threadIdx.x] + d.partials[threadIdx.x + 64]);
            if (threadIdx.x == 0) mean_s = (float)(t / ((double)d.H * (double)d.W));
        }
        __syncthreads();
        mean = mean_s;
    }
    if (x >= d.W) return;
    const int W = d.W;
    float v = (d.apply ? slot_in(d, in_slot) : d.src)[(size_t)y * W + x];
    if (jitter) {
        const bool b = d.jitter & ACAI_AUG_BRIGHTNESS, c = d.jitter & ACAI_AUG_CONTRAST;
        const float shift = (1.f - d.fc) * mean;
        if (d.jitter & ACAI_AUG_BRIGHTNESS_FIRST) {
            if (b) v = clamp01(v * d.fb);
            if (c) v = clamp01(fmaf(d.fc, v, shift));
        } else {
            if (c) v = clamp01(fmaf(d.fc, v, shift));
            if (b) v = clamp01(v * d.fb);
        }
    }
    if (po.base) {
        const size_t row = (size_t)d.row0 + (size_t)(y / po.P) * (W / po.P) + x / po.P;
        const int col = (y % po.P) * po.P + x % po.P;
        if (po.bf16) reinterpret_cast<bf16_t *>(po.base)[row * po.ld + col] = f2bf(v);
        else reinterpret_cast<float *>(po.base)[row * po.ld + col] = v;
    } else
        d.out[(size_t)y * W + x] = v;
}

int check_batch(const char *who, const AcaiAugImage *table, int n, int max_h, int max_w) {
    ACAI_CHECK_ARG(table, "%s: null descriptor table", who);
    ACAI_CHECK_ARG(n > 0 && n <= 65535 && max_h > 0 && max_h <= 65535 && max_w > 0, "%s: %d images of at most %d x %d (images and rows are grid dimensions, <= 65535)",
                   who, n, max_h, max_w);
    return 0;
}

dim3 pixel_grid(int n, int max_h, int max_w) { return dim3(cdiv(max_w, TPB), max_h, n); }

}  // namespace

extern "C" int acai_augment_blur_noise(const AcaiAugImage *table, int n_images, int max_h, int max_w, int in_slot, int tmp_slot, int out_slot,
                                       int do_blur, int do_noise, void *stream) {
    if (int rc = check_batch("acai_augment_blur_noise", table, n_images, max_h, max_w)) return rc;
    ACAI_CHECK_ARG(in_slot >= -1 && in_slot <= 1 && (out_slot == 0 || out_slot == 1) && in_slot != out_slot, "acai_augment_blur_noise: bad slots %d -> %d",
                   in_slot, out_slot);
    ACAI_CHECK_ARG(!do_blur || ((tmp_slot == 0 || tmp_slot == 1) && tmp_slot != in_slot && tmp_slot != out_slot),
                   "acai_augment_blur_noise: the row pass needs a scratch slot that is neither input (%d) nor output (%d), got %d", in_slot, out_slot, tmp_slot);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid = pixel_grid(n_images, max_h, max_w);
    if (do_blur) {
        hipLaunchKernelGGL((aug_blur_kernel<false>), grid, dim3(TPB), 0, st, table, in_slot, tmp_slot, 0);
        ACAI_LAUNCH_CHECK("acai_augment_blur_noise (rows)");
    }
    hipLaunchKernelGGL((aug_blur_kernel<true>), grid, dim3(TPB), 0, st, table, do_blur ? tmp_slot : in_slot, out_slot, do_noise ? 1 : 0);
    ACAI_LAUNCH_CHECK("acai_augment_blur_noise (columns)");
    return 0;
}

extern "C" int acai_augment_warp(const AcaiAugImage *table, int n_images, int max_h, int max_w, int in_slot, int out_slot, int perspective, void *stream) {
    if (int rc = check_batch("acai_augment_warp", table, n_images, max_h, max_w)) return rc;
    ACAI_CHECK_ARG(in_slot >= -1 && in_slot <= 1 && (out_slot == 0 || out_slot == 1) && in_slot != out_slot, "acai_augment_warp: bad slots %d -> %d", in_slot,
                   out_slot);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid = pixel_grid(n_images, max_h, max_w);
    if (perspective) hipLaunchKernelGGL((aug_warp_kernel<true>), grid, dim3(TPB), 0, st, table, in_slot, out_slot);
    else hipLaunchKernelGGL((aug_warp_kernel<false>), grid, dim3(TPB), 0, st, table, in_slot, out_slot);
    ACAI_LAUNCH_CHECK("acai_augment_warp");
    return 0;
}

extern "C" int acai_augment_jitter_out(const AcaiAugImage *table, int n_images, int max_h, int max_w, int in_slot, int do_jitter, void *patches, int ld,
                                       int P, int out_dtype, void *stream) {
    if (int rc = check_batch("acai_augment_jitter_out", table, n_images, max_h, max_w)) return rc;
    ACAI_CHECK_ARG(in_slot >= -1 && in_slot <= 1, "acai_augment_jitter_out: bad input slot %d", in_slot);
    ACAI_CHECK_ARG(!patches || (P > 0 && ld >= P * P && (out_dtype == ACAI_F32 || out_dtype == ACAI_BF16)),
                   "acai_augment_jitter_out: patch form needs P > 0, ld >= P*P and an fp32 / bf16 stream (P = %d, ld = %d, dtype %d)", P, ld, out_dtype);
    hipStream_t st = (hipStream_t)stream;
    if (do_jitter) {
        hipLaunchKernelGGL(aug_mean_kernel, dim3(ACAI_AUG_MEAN_PARTS, 1, n_images), dim3(TPB), 0, st, table, in_slot);
        ACAI_LAUNCH_CHECK("acai_augment_jitter_out (mean)");
    }
    const AugPatchOut po{patches, ld, patches ? P : 1, out_dtype == ACAI_BF16 ? 1 : 0};
    hipLaunchKernelGGL(aug_jitter_out_kernel, pixel_grid(n_images, max_h, max_w), dim3(TPB), 0, st, table, in_slot, do_jitter ? 1 : 0, po);
    ACAI_LAUNCH_CHECK("acai_augment_jitter_out");
    return 0;
}

// Blank-patch pruning ahead of the encoder (an extension; no reference counterpart): which patches of the packed patch stream are paper, and
// the stream without them.
//   acai_patch_ink        one wave per patch row: the number of its elements strictly below ink_level;
//   acai_patch_keep       one workgroup per image: inked = ink > max_ink, keep = an inked patch within Chebyshev distance halo inside the
//                         image's own grid (every patch of an image without ink), and the kept local indices in ascending order;
//   acai_patch_compact    after the host has read the kept counts: the kept rows copied bitwise into the exact-size stream, the packed kept
//                         indices and the rows of the positional table they gather;
//   acai_attn_map_expand  per-token maps over the kept patches scattered to the columns of the full grid.
// Integer counts, ballots and popcounts only: no floating-point arithmetic beyond the one comparison, no atomics, the same bits on every run.
#include "common.h"

namespace {

constexpr int INK_WAVES = 4;      // patch rows per workgroup of the ink and compact kernels
constexpr int KEEP_THREADS = 256; // patches per chunk of the keep kernel's scan
constexpr int KEEP_WAVES = KEEP_THREADS / 64;

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// T = float or bf16_t.  VEC: base and pitch are multiples of 16 bytes, so every row starts on a 16-byte boundary; lanes then read 16-byte units
// and the L % (16 / sizeof(T)) trailing elements one by one.
template <typename T, bool VEC>
__global__ __launch_bounds__(64 * INK_WAVES) void patch_ink_kernel(const T *patches, int64_t pitch, int M, int L, float level, int32_t *ink) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * INK_WAVES + (threadIdx.x >> 6);
    if (r >= M) return;   // wave-uniform; the kernel has no barrier
    const T *row = patches + (size_t)r * pitch;
    constexpr int PER = 16 / (int)sizeof(T);
    int cnt = 0, done = 0;
    if constexpr (VEC) {
        const int units = L / PER;
        for (int u = lane; u < units; u += 64) {
            const uint4 v = ld_nt16(row + (size_t)u * PER);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (sizeof(T) == 4) {
                    cnt += __uint_as_float(w[j]) < level ? 1 : 0;
                } else {
                    cnt += __uint_as_float(w[j] << 16) < level ? 1 : 0;
                    cnt += __uint_as_float(w[j] & 0xFFFF0000u) < level ? 1 : 0;
                }
            }
        }
        done = units * PER;
    }
    for (int e = done + lane; e < L; e += 64) cnt += DT<T>::ld(row + e) < level ? 1 : 0;
    cnt = wave_sum_i32(cnt);
    if (lane == 0) ink[r] = cnt;
}

// Per-image entry of the device table (int32 [B][ACAI_PRUNE_TABLE_COLS]): h_p, w_p, the image's first row in the full stream, the first row
// of its positional grid in the positional table and that grid's width.
struct PruneImage {
    int h, w, off, pe_base, pe_w;
};
__device__ __forceinline__ PruneImage prune_image(const int32_t *table, int i) {
    const int32_t *t = table + (size_t)i * ACAI_PRUNE_TABLE_COLS;
    return PruneImage{t[0], t[1], t[2], t[3], t[4]};
}

__global__ __launch_bounds__(KEEP_THREADS) void patch_keep_kernel(const int32_t *ink, const int32_t *table, int max_ink, int halo, int32_t *kept_local,
                                                                  int32_t *count) {
    __shared__ int wave_total[KEEP_WAVES];
    const PruneImage im = prune_image(table, blockIdx.x);
    const int n = im.h * im.w;
    const int32_t *iink = ink + im.off;
    int32_t *out = kept_local + im.off;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    int any = 0;
    for (int p = threadIdx.x; p < n; p += KEEP_THREADS) any |= iink[p] > max_ink ? 1 : 0;
    const bool all = !__syncthreads_or(any);   // an image without ink keeps every patch

    int base = 0;   // kept patches of the chunks before this one: the same value in every thread
    for (int p0 = 0; p0 < n; p0 += KEEP_THREADS) {
        const int p = p0 + threadIdx.x;
        bool keep = false;
        if (p < n) {
            keep = all;
            if (!all) {
                const int r = p / im.w, c = p - r * im.w;
                const int r0 = max(r - halo, 0), r1 = min(r + halo, im.h - 1), c0 = max(c - halo, 0), c1 = min(c + halo, im.w - 1);
                for (int rr = r0; rr <= r1; ++rr)
                    for (int cc = c0; cc <= c1; ++cc) keep |= iink[rr * im.w + cc] > max_ink;
            }
        }
        const unsigned long long mask = __ballot(keep);   // 64 bits: one per lane of the wave
        if (lane == 0) wave_total[wave] = __popcll(mask);
        __syncthreads();
        int before = base, total = 0;
#pragma unroll
        for (int w = 0; w < KEEP_WAVES; ++w) {
            const int t = wave_total[w];
            before += w < wave ? t : 0;
            total += t;
        }
        if (keep) out[before + __popcll(mask & ((1ull << lane) - 1ull))] = p;
        base += total;
        __syncthreads();   // wave_total is rewritten by the next chunk
    }
    if (threadIdx.x == 0) count[blockIdx.x] = base;
}

// The image of output row j: the largest i with cu_out[i] <= j, so an image without rows is stepped over.
__device__ __forceinline__ int image_of_row(const int32_t *cu_out, int B, int j) {
    int lo = 0, hi = B;   // cu_out[lo] <= j < cu_out[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cu_out[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

// One wave per kept row.  ES: bytes per element; VEC as in patch_ink_kernel, for the source and the destination both.
template <int ES, bool VEC>
__global__ __launch_bounds__(64 * INK_WAVES) void patch_compact_kernel(const char *patches, int64_t pitch_bytes, int L, const int32_t *table,
                                                                       const int32_t *kept_local, const int32_t *cu_out, int B, int total,
                                                                       char *out, int32_t *kept, int32_t *pe_idx) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * INK_WAVES + (threadIdx.x >> 6);
    if (j >= total) return;   // wave-uniform; the kernel has no barrier
    const int i = image_of_row(cu_out, B, j);
    const PruneImage im = prune_image(table, i);
    const int local = kept_local[im.off + (j - cu_out[i])];
    const char *src = patches + (size_t)(im.off + local) * pitch_bytes;
    char *dst = out + (size_t)j * L * ES;
    const int bytes = L * ES;
    int done = 0;
    if constexpr (VEC) {
        const int units = bytes >> 4;
        for (int u = lane; u < units; u += 64) *reinterpret_cast<uint4 *>(dst + ((size_t)u << 4)) = ld_nt16(src + ((size_t)u << 4));
        done = units << 4;
    }
    for (int e = done + lane * ES; e < bytes; e += 64 * ES) {
        if constexpr (ES == 4) *reinterpret_cast<uint32_t *>(dst + e) = *reinterpret_cast<const uint32_t *>(src + e);
        else *reinterpret_cast<uint16_t *>(dst + e) = *reinterpret_cast<const uint16_t *>(src + e);
    }
    if (lane == 0) {
        kept[j] = local;
        const int r = local / im.w, c = local - r * im.w;
        pe_idx[j] = im.pe_base + r * im.pe_w + c;
    }
}

constexpr int EXPAND_COLS = 256;

// Row t of image b: out_b[t][kept_b[j]] = in_b[t][j].
__global__ __launch_bounds__(EXPAND_COLS) void attn_map_expand_kernel(const float *in, const int64_t *in_off, float *out, const int64_t *out_off,
                                                                      const int32_t *cu_q, const int32_t *cu_kept, const int32_t *cu_full,
                                                                      const int32_t *kept) {
    const int b = blockIdx.z, t = blockIdx.y;
    const int T = cu_q[b + 1] - cu_q[b];
    const int k0 = cu_kept[b], K = cu_kept[b + 1] - k0;
    const int S = cu_full[b + 1] - cu_full[b];
    const int j = blockIdx.x * EXPAND_COLS + threadIdx.x;
    if (t >= T || j >= K) return;
    const int col = kept[k0 + j];
    if (col < 0 || col >= S) return;   // (checked on the host side of the product path; never write outside the image's block)
    out[out_off[b] + (int64_t)t * S + col] = in[in_off[b] + (int64_t)t * K + j];
}

}  // namespace

extern "C" int acai_patch_ink(const void *patches, int dtype, int M, int L, int64_t pitch, float ink_level, int32_t *ink, void *stream) {
    ACAI_CHECK_ARG(dtype == ACAI_F32 || dtype == ACAI_BF16, "acai_patch_ink: dtype %d (fp32 or bf16)", dtype);
    ACAI_CHECK_ARG(M >= 0 && L >= 1 && pitch >= L, "acai_patch_ink: bad dims M=%d L=%d pitch=%lld", M, L, (long long)pitch);
    ACAI_CHECK_ARG(!(ink_level != ink_level), "acai_patch_ink: ink_level is NaN");
    if (M == 0) return 0;
    ACAI_CHECK_ARG(patches && ink, "acai_patch_ink: null operand");
    const int es = dtype == ACAI_F32 ? 4 : 2;
    const bool vec = aligned16(patches) && (pitch * es) % 16 == 0;
    const dim3 grid(cdiv(M, INK_WAVES)), block(64 * INK_WAVES);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ACAI_F32) {
        if (vec) hipLaunchKernelGGL((patch_ink_kernel<float, true>), grid, block, 0, st, (const float *)patches, pitch, M, L, ink_level, ink);
        else hipLaunchKernelGGL((patch_ink_kernel<float, false>), grid, block, 0, st, (const float *)patches, pitch, M, L, ink_level, ink);
    } else {
        if (vec) hipLaunchKernelGGL((patch_ink_kernel<bf16_t, true>), grid, block, 0, st, (const bf16_t *)patches, pitch, M, L, ink_level, ink);
        else hipLaunchKernelGGL((patch_ink_kernel<bf16_t, false>), grid, block, 0, st, (const bf16_t *)patches, pitch, M, L, ink_level, ink);
    }
    ACAI_LAUNCH_CHECK("acai_patch_ink");
    return 0;
}

extern "C" int acai_patch_keep(const int32_t *ink, const int32_t *table, int B, int max_grid, int max_ink, int halo, int32_t *kept_local,
                               int32_t *count, void *stream) {
    ACAI_CHECK_ARG(B >= 0 && B <= ACAI_PRUNE_MAX_IMAGES, "acai_patch_keep: %d images (at most %d)", B, ACAI_PRUNE_MAX_IMAGES);
    ACAI_CHECK_ARG(halo >= 0 && halo <= ACAI_PRUNE_MAX_HALO, "acai_patch_keep: halo=%d (0 .. %d)", halo, ACAI_PRUNE_MAX_HALO);
    ACAI_CHECK_ARG(max_ink >= 0, "acai_patch_keep: max_ink=%d (must not be negative)", max_ink);
    ACAI_CHECK_ARG(max_grid >= 0 && max_grid <= ACAI_PRUNE_MAX_GRID, "acai_patch_keep: a grid of %d patches (at most %d)", max_grid,
                   ACAI_PRUNE_MAX_GRID);
    if (B == 0) return 0;
    ACAI_CHECK_ARG(ink && table && kept_local && count, "acai_patch_keep: null operand");
    hipLaunchKernelGGL(patch_keep_kernel, dim3(B), dim3(KEEP_THREADS), 0, (hipStream_t)stream, ink, table, max_ink, halo, kept_local, count);
    ACAI_LAUNCH_CHECK("acai_patch_keep");
    return 0;
}

extern "C" int acai_patch_compact(const void *patches, int dtype, int L, int64_t pitch, const int32_t *table, const int32_t *kept_local,
                                  const int32_t *cu_out, int B, int total, void *out, int32_t *kept, int32_t *pe_idx, void *stream) {
    ACAI_CHECK_ARG(dtype == ACAI_F32 || dtype == ACAI_BF16, "acai_patch_compact: dtype %d (fp32 or bf16)", dtype);
    ACAI_CHECK_ARG(B >= 0 && B <= ACAI_PRUNE_MAX_IMAGES && total >= 0 && L >= 1 && pitch >= L, "acai_patch_compact: bad dims B=%d total=%d L=%d pitch=%lld",
                   B, total, L, (long long)pitch);
    if (total == 0) return 0;
    ACAI_CHECK_ARG(B >= 1 && patches && table && kept_local && cu_out && out && kept && pe_idx, "acai_patch_compact: null operand");
    ACAI_CHECK_ARG(out != patches, "acai_patch_compact: out must not be the input stream");
    const int es = dtype == ACAI_F32 ? 4 : 2;
    const bool vec = aligned16(patches) && aligned16(out) && (pitch * es) % 16 == 0 && ((int64_t)L * es) % 16 == 0;
    const dim3 grid(cdiv(total, INK_WAVES)), block(64 * INK_WAVES);
    hipStream_t st = (hipStream_t)stream;
#define ACAI_COMPACT(ES, VEC)                                                                                                                 \
    hipLaunchKernelGGL((patch_compact_kernel<ES, VEC>), grid, block, 0, st, (const char *)patches, pitch * es, L, table, kept_local, cu_out, B, \
                       total, (char *)out, kept, pe_idx)
    if (es == 4) {
        if (vec) ACAI_COMPACT(4, true);
        else ACAI_COMPACT(4, false);
    } else {
        if (vec) ACAI_COMPACT(2, true);
        else ACAI_COMPACT(2, false);
    }
#undef ACAI_COMPACT
    ACAI_LAUNCH_CHECK("acai_patch_compact");
    return 0;
}

extern "C" int acai_attn_map_expand(const float *in, const int64_t *in_off, float *out, const int64_t *out_off, const int32_t *cu_q,
                                    const int32_t *cu_kept, const int32_t *cu_full, const int32_t *kept, int B, int max_q, int max_kept,
                                    void *stream) {
    ACAI_CHECK_ARG(B >= 0 && B <= ACAI_PRUNE_MAX_IMAGES && max_q >= 0 && max_q <= 65535 && max_kept >= 0,
                   "acai_attn_map_expand: bad dims B=%d max_q=%d max_kept=%d", B, max_q, max_kept);
    if (B == 0 || max_q == 0 || max_kept == 0) return 0;
    ACAI_CHECK_ARG(in && in_off && out && out_off && cu_q && cu_kept && cu_full && kept, "acai_attn_map_expand: null operand");
    ACAI_CHECK_ARG(in != out, "acai_attn_map_expand: out must not be the input buffer");
    hipLaunchKernelGGL(attn_map_expand_kernel, dim3(cdiv(max_kept, EXPAND_COLS), max_q, B), dim3(EXPAND_COLS), 0, (hipStream_t)stream, in, in_off,
                       out, out_off, cu_q, cu_kept, cu_full, kept);
    ACAI_LAUNCH_CHECK("acai_attn_map_expand");
    return 0;
}

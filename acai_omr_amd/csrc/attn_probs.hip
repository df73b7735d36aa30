// Token-to-image alignment: the attention the flash-style kernels never materialise (attn_varlen.hip, decode_attn.hip), written out.
//
// acai_attn_probs_mean: out[t][s] (+)= sum_h head_w[h] * exp2(q_h[t] . k_h[s] * log2(e) / sqrt(dh) - lse[h][t]) per image, the weighted
//   mean over heads of the cross-attention probabilities.  lse is what acai_attn_varlen_fwd wrote for the same q and k, so one pass over
//   the scores is enough: no row maximum, no second sweep.  Heads are summed in index order inside one thread: the same bits every run.
//   * bf16, d_h 32 / 64, 16-byte aligned rows: probs_mfma_kernel.  A workgroup of 2 x 2 waves owns 128 queries x 128 keys of one image,
//     a wave 64 x 64 as 2 x 2 v_mfma_f32_32x32x16_bf16 tiles with the queries as A and the keys as B: the result has the key on the lane
//     and the query in the register, so every store instruction writes two 128-byte runs of one map row.  The Q / K fragments of a head
//     are exactly 16 contiguous bytes per lane and go global -> VGPR (no LDS, no barrier: a wave whose tile is empty just leaves).  The map
//     accumulators (64 registers) live across the head loop; the map is read (accumulate) and written once.  Per score: one FMA, one
//     v_exp_f32, one FMA.  Bound by the fragment loads from L2 (4 bytes per score and head at this tile) and by the map write.
//   * everything else (fp32, other d_h, unaligned views): probs_fma_kernel, 16 queries x 64 keys per workgroup, the head's Q / K tile
//     widened to fp32 in LDS and plain FMA chains over d_h - the fp32 form never rounds an operand to bf16.
//
// acai_attn_map_locate: one wave per map row reduces it to (arg-max patch, row sum, peak, centroid, spread) in two sweeps (sums, then
//   the second moments around the centroid).  Each lane walks its keys in ascending order and the lanes are combined by a fixed butterfly,
//   so the result is the same bits every run; on equal values the lower index wins.
#include "common.h"

#include <math.h>

namespace {

struct ProbsArgs {
    const void *q, *k;
    const int32_t *cu_q, *cu_k;
    const float *lse, *head_w;
    const int64_t *map_off;
    float *out;
    int ldq, ldk, H, dh, total_q, accumulate;
    float scale_log2e;
};

constexpr int WQ = 64, WK = 64;     // a wave's tile: 2 x 2 MFMA results of 32 x 32
constexpr int BQ = 128, BK = 128;   // a workgroup's: 2 x 2 waves

template <int DH>
__global__ __launch_bounds__(256) void probs_mfma_kernel(const ProbsArgs a) {
    constexpr int KS = DH / 16;   // k-steps of 16 per head
    const int b = blockIdx.z;
    const int q_start = a.cu_q[b], lq = a.cu_q[b + 1] - q_start;
    const int k_start = a.cu_k[b], lk = a.cu_k[b + 1] - k_start;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q0 = blockIdx.y * BQ + (wave >> 1) * WQ;
    const int k0 = blockIdx.x * BK + (wave & 1) * WK;
    if (q0 >= lq || k0 >= lk) return;   // wave-uniform, and the kernel has no barrier
    const int r = lane & 31, lh = lane >> 5;

    // fragment rows: lane (r, lh) holds elements 8 lh .. 8 lh + 7 of each k-step of row r.  Rows past the ragged end are clamped to the
    // last valid one (finite values, never stored).
    const bf16_t *qrow[2], *krow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        qrow[i] = (const bf16_t *)a.q + (size_t)(q_start + min(q0 + 32 * i + r, lq - 1)) * a.ldq + lh * 8;
        krow[i] = (const bf16_t *)a.k + (size_t)(k_start + min(k0 + 32 * i + r, lk - 1)) * a.ldk + lh * 8;
    }
    // result layout: register e of lane (r, lh) is query (e & 3) + 8 (e >> 2) + 4 lh, key r
    int trow[2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) trow[i][e] = q0 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * lh;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const float c = a.scale_log2e;
    for (int h = 0; h < a.H; ++h) {
        const float w = a.head_w[h];
        if (w == 0.f) continue;
        bf16x8 qf[2][KS], kf[2][KS];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                qf[i][s] = *reinterpret_cast<const bf16x8 *>(qrow[i] + h * DH + s * 16);
                kf[i][s] = *reinterpret_cast<const bf16x8 *>(krow[i] + h * DH + s * 16);
            }
        const float *lse_h = a.lse + (size_t)h * a.total_q + q_start;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float nl[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) nl[e] = -lse_h[min(trow[i][e], lq - 1)];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                f32x16 s;
#pragma unroll
                for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[i][ks], kf[j][ks], s, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = fmaf(w, fast_exp2(fmaf(s[e], c, nl[e])), acc[i][j][e]);
            }
        }
    }

    float *map = a.out + a.map_off[b];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int s_idx = k0 + 32 * j + r;
            if (s_idx >= lk) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int t = trow[i][e];
                if (t < lq) {
                    float *p = map + (size_t)t * lk + s_idx;
                    *p = a.accumulate ? *p + acc[i][j][e] : acc[i][j][e];
                }
            }
        }
}

constexpr int FQ = 16, FK = 64;   // the FMA form's tile: thread (key = tid & 63, group = tid >> 6) owns queries 4 group .. 4 group + 3

template <typename T>
__global__ __launch_bounds__(256) void probs_fma_kernel(const ProbsArgs a) {
    __shared__ float qs[FQ][65], ks[FK][65];
    const int b = blockIdx.z;
    const int q_start = a.cu_q[b], lq = a.cu_q[b + 1] - q_start;
    const int k_start = a.cu_k[b], lk = a.cu_k[b + 1] - k_start;
    const int q0 = blockIdx.y * FQ, k0 = blockIdx.x * FK;
    if (q0 >= lq || k0 >= lk) return;   // uniform over the workgroup
    const int tid = threadIdx.x, key = tid & 63, grp = tid >> 6, dh = a.dh;
    const T *Q = (const T *)a.q, *K = (const T *)a.k;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int h = 0; h < a.H; ++h) {
        const float w = a.head_w[h];
        if (w == 0.f) continue;   // uniform: every thread reads the same weight
        __syncthreads();          // the previous head's tiles are no longer read
        for (int x = tid; x < FQ * dh; x += 256) {
            const int row = x / dh, d = x - row * dh;
            qs[row][d] = DT<T>::ld(Q + (size_t)(q_start + min(q0 + row, lq - 1)) * a.ldq + h * dh + d);
        }
        for (int x = tid; x < FK * dh; x += 256) {
            const int row = x / dh, d = x - row * dh;
            ks[row][d] = DT<T>::ld(K + (size_t)(k_start + min(k0 + row, lk - 1)) * a.ldk + h * dh + d);
        }
        __syncthreads();
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int d = 0; d < dh; ++d) {
            const float kv = ks[key][d];
#pragma unroll
            for (int i = 0; i < 4; ++i) s[i] = fmaf(qs[4 * grp + i][d], kv, s[i]);
        }
        const float *lse_h = a.lse + (size_t)h * a.total_q + q_start;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float l = lse_h[min(q0 + 4 * grp + i, lq - 1)];
            acc[i] = fmaf(w, fast_exp2(fmaf(s[i], a.scale_log2e, -l)), acc[i]);
        }
    }
    if (k0 + key >= lk) return;
    float *map = a.out + a.map_off[b];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = q0 + 4 * grp + i;
        if (t < lq) {
            float *p = map + (size_t)t * lk + k0 + key;
            *p = a.accumulate ? *p + acc[i] : acc[i];
        }
    }
}

// ---- locate ---------------------------------------------------------------------------------------------------------------------------
constexpr int LOC_MAX_B = 512;   // images per call: their grid widths travel as kernel arguments
struct LocateArgs {
    const float *map;
    const int64_t *map_off;
    const int32_t *cu_q, *cu_k;
    int32_t *patch;
    float *loc;
    int32_t grid_w[LOC_MAX_B];
};

__device__ __forceinline__ float wave_sum_fixed(float v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);   // a + b is commutative: every lane ends with the same bits
    return v;
}

__global__ __launch_bounds__(256) void map_locate_kernel(const LocateArgs a) {
    const int b = blockIdx.y;
    const int q_start = a.cu_q[b], lq = a.cu_q[b + 1] - q_start;
    const int S = a.cu_k[b + 1] - a.cu_k[b];
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= lq) return;   // wave-uniform; no barrier
    const int w = a.grid_w[b];
    const float *row = a.map + a.map_off[b] + (size_t)t * S;
    float m = 0.f, mx = 0.f, my = 0.f, best = -1.f;
    int arg = 0x7fffffff;
    for (int s = lane; s < S; s += 64) {
        const float p = row[s];
        const int y = s / w, x = s - y * w;
        m += p;
        mx = fmaf(p, (float)x + 0.5f, mx);
        my = fmaf(p, (float)y + 0.5f, my);
        if (p > best) { best = p; arg = s; }   // ascending s: the first of equal values stays
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float ob = __shfl_xor(best, o);
        const int oa = __shfl_xor(arg, o);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    m = wave_sum_fixed(m), mx = wave_sum_fixed(mx), my = wave_sum_fixed(my);
    const bool empty = !(m > 0.f);
    const float cx = empty ? 0.f : mx / m, cy = empty ? 0.f : my / m;
    float vx = 0.f, vy = 0.f;
    for (int s = lane; s < S; s += 64) {
        const float p = row[s];
        const int y = s / w, x = s - y * w;
        const float dx = (float)x + 0.5f - cx, dy = (float)y + 0.5f - cy;
        vx = fmaf(p, dx * dx, vx);
        vy = fmaf(p, dy * dy, vy);
    }
    vx = wave_sum_fixed(vx), vy = wave_sum_fixed(vy);
    if (lane == 0) {
        a.patch[q_start + t] = (empty || S == 0) ? 0 : arg;
        float *o = a.loc + (size_t)(q_start + t) * 6;
        o[0] = m;
        o[1] = S > 0 ? fmaxf(best, 0.f) : 0.f;
        o[2] = cx;
        o[3] = cy;
        o[4] = empty ? 0.f : sqrtf(vx / m);
        o[5] = empty ? 0.f : sqrtf(vy / m);
    }
}

}  // namespace

extern "C" int acai_attn_probs_mean(const void *q, int ldq, const void *k, int ldk, const int32_t *cu_q, const int32_t *cu_k, int B, int H, int dh,
                                    int max_q, int max_k, int dtype, const float *lse, int total_q, const float *head_w, const int64_t *map_off,
                                    float *out, int accumulate, void *stream) {
    ACAI_CHECK_ARG(q && k && cu_q && cu_k && lse && head_w && map_off && out, "acai_attn_probs_mean: null operand");
    ACAI_CHECK_ARG(B > 0 && H >= 1 && dh > 0 && dh <= 64 && max_q > 0 && max_k > 0 && total_q > 0,
                   "acai_attn_probs_mean: bad dims B=%d H=%d dh=%d max_q=%d max_k=%d total_q=%d (dh <= 64)", B, H, dh, max_q, max_k, total_q);
    ACAI_CHECK_ARG(ldq >= H * dh && ldk >= H * dh, "acai_attn_probs_mean: row stride smaller than H*dh");
    ACAI_CHECK_ARG(B <= 65535, "acai_attn_probs_mean: grid too large");
    ACAI_CHECK_ARG(dtype == ACAI_BF16 || dtype == ACAI_F32, "acai_attn_probs_mean: bad dtype %d", dtype);
    ProbsArgs a{q, k, cu_q, cu_k, lse, head_w, map_off, out, ldq, ldk, H, dh, total_q, accumulate ? 1 : 0, 1.4426950408889634f / sqrtf((float)dh)};
    hipStream_t st = (hipStream_t)stream;
    const bool mfma = dtype == ACAI_BF16 && (dh == 32 || dh == 64) && ldq % 8 == 0 && ldk % 8 == 0 && aligned16(q) && aligned16(k);
    if (mfma) {
        dim3 grid(cdiv(max_k, BK), cdiv(max_q, BQ), B);
        ACAI_CHECK_ARG(grid.y <= 65535, "acai_attn_probs_mean: grid too large");
        if (dh == 32)
            hipLaunchKernelGGL(probs_mfma_kernel<32>, grid, dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL(probs_mfma_kernel<64>, grid, dim3(256), 0, st, a);
    } else {
        dim3 grid(cdiv(max_k, FK), cdiv(max_q, FQ), B);
        ACAI_CHECK_ARG(grid.y <= 65535, "acai_attn_probs_mean: grid too large");
        if (dtype == ACAI_BF16)
            hipLaunchKernelGGL(probs_fma_kernel<bf16_t>, grid, dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL(probs_fma_kernel<float>, grid, dim3(256), 0, st, a);
    }
    ACAI_LAUNCH_CHECK("acai_attn_probs_mean");
    return 0;
}

extern "C" int acai_attn_map_locate(const float *map, const int64_t *map_off, const int32_t *cu_q, const int32_t *cu_k, const int32_t *grid_w,
                                    int B, int max_q, int32_t *patch, float *loc, void *stream) {
    ACAI_CHECK_ARG(map && map_off && cu_q && cu_k && grid_w && patch && loc, "acai_attn_map_locate: null operand");
    ACAI_CHECK_ARG(B > 0 && B <= LOC_MAX_B && max_q > 0, "acai_attn_map_locate: bad dims B=%d max_q=%d (B <= %d)", B, max_q, LOC_MAX_B);
    LocateArgs a{map, map_off, cu_q, cu_k, patch, loc, {}};
    for (int b = 0; b < B; ++b) {
        ACAI_CHECK_ARG(grid_w[b] >= 1, "acai_attn_map_locate: grid_w[%d] = %d (must be >= 1)", b, grid_w[b]);
        a.grid_w[b] = grid_w[b];
    }
    dim3 grid(cdiv(max_q, 4), B);
    ACAI_CHECK_ARG(grid.x <= 0x7fffffffu / 4, "acai_attn_map_locate: grid too large");
    hipLaunchKernelGGL(map_locate_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    ACAI_LAUNCH_CHECK("acai_attn_map_locate");
    return 0;
}

// GRPO objective + entropy bonus over the policy's teacher-forced logits, forward and backward (acai_omr/train/omr_grpo_train.py:240-283:
// calc_grpo_objective, calc_policy_theta_entropy, calc_entropy_bonus; under autocast the bf16 logits go through log_softmax / softmax in fp32).
//
// Positions n = r * T + t of logits [R][T][V] (contiguous, fp32 or bf16).  Position n is live when mask[n] == 0; its action is a = rollouts[r][t+1].
//   lse = logsumexp(x), lp = x[a] - lse, ratio = exp(lp - old_lp[r][t+1]), s = min(ratio A_r, clamp(ratio, 1-eps, 1+eps) A_r), H = sum_c p_c (lse - x_c)
//   objective = sum_r (sum_t s / len_r) / num_groups,   bonus = mean_r (sum_t H / len_r) / log(V)
//
// Three launches, no float atomics, so both passes are bitwise repeatable:
//   grpo_rows_kernel    one workgroup per 16 consecutive positions: the chunk (16 V elements, a multiple of 16 bytes) is staged into LDS with
//                       16-byte loads, each wave then takes four positions and writes (lse, H, s, ds/dlp) to `stats`;
//   grpo_reduce_kernel  ONE workgroup: per rollout a wave sums its positions in a fixed order (rowstat = (S_r/len_r, H_r/len_r, len_r)), then
//                       the rollouts are summed in a fixed order into out[0] = objective, out[1] = bonus;
//   grpo_bwd_kernel     the rows kernel's layout again: dlogits = g_obj w_r ds/dlp (d_ca - p_c) + g_bonus u_r (-p_c (x_c - lse + H)),
//                       w_r = 1 / (len_r num_groups), u_r = 1 / (R len_r log V); the two incoming gradients are read from device memory.
// ds/dlp follows torch's autograd of the reference formula: torch.minimum hands a tie half to each input, clamp passes the gradient on the closed
// band [1-eps, 1+eps] - so inside the band (unclipped == clipped bit for bit) the whole gradient flows, outside it only the unclipped branch's
// when it is the smaller one.
// Deviation (documented): an entropy term with p_c == 0 counts 0 (the reference's 0 * (-inf) = NaN for -inf logits, its KAT uses them), and
// such classes get a zero gradient.  Real unembed logits are never -inf.  len_r == 0 gives NaN, as in the reference.
//
// Size: the forward reads the logits once, the backward reads them and writes dlogits: 29 MB / 58 MB at R = 128, T = 500, V = 227, bf16.
// Measured on one MI355X (rocprofv3 kernel trace of tools/bench_grpo.py, profiles/grpo_update_kernel_stats.csv): rows 44.8 us (0.65 TB/s,
// 8 % of the 8 TB/s HBM peak), reduce 43.7 us (one workgroup: latency, not bandwidth), backward 30.0 us (1.94 TB/s, 24 %).  Far from the
// roof - both passes together are 0.1 % of an update epoch (180 ms), so they were left simple; the single-workgroup reduce is the first thing
// to split if that changes.
#include "common.h"

namespace {

constexpr int GRPO_POS = 16;   // positions per workgroup (16 V elements are a whole number of 16-byte vectors for any V, fp32 and bf16)

// chunk [e0, e1) of the flat logits into LDS as fp32; e0 is 16-byte aligned (base aligned, checked on the host)
template <typename LT>
__device__ __forceinline__ void stage_chunk(const LT *__restrict__ x, long e0, long e1, float *lds) {
    constexpr int EPV = 16 / sizeof(LT);
    const int n = (int)(e1 - e0), nvec = n / EPV;
    const uint4 *src = reinterpret_cast<const uint4 *>(x + e0);
    for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
        const uint4 v = src[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        if constexpr (sizeof(LT) == 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lds[i * 8 + 2 * j] = __uint_as_float(w[j] << 16);
                lds[i * 8 + 2 * j + 1] = __uint_as_float(w[j] & 0xFFFF0000u);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) lds[i * 4 + j] = __uint_as_float(w[j]);
        }
    }
    for (int i = nvec * EPV + threadIdx.x; i < n; i += blockDim.x) lds[i] = DT<LT>::ld(x + e0 + i);
}

template <typename LT>
__device__ __forceinline__ void store_chunk(LT *__restrict__ y, long e0, long e1, const float *lds) {
    constexpr int EPV = 16 / sizeof(LT);
    const int n = (int)(e1 - e0), nvec = n / EPV;
    uint4 *dst = reinterpret_cast<uint4 *>(y + e0);
    for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
        uint4 v;
        if constexpr (sizeof(LT) == 2) {
            v = make_uint4(pack_bf16(lds[i * 8], lds[i * 8 + 1]), pack_bf16(lds[i * 8 + 2], lds[i * 8 + 3]), pack_bf16(lds[i * 8 + 4], lds[i * 8 + 5]),
                           pack_bf16(lds[i * 8 + 6], lds[i * 8 + 7]));
        } else {
            v = make_uint4(__float_as_uint(lds[i * 4]), __float_as_uint(lds[i * 4 + 1]), __float_as_uint(lds[i * 4 + 2]), __float_as_uint(lds[i * 4 + 3]));
        }
        dst[i] = v;
    }
    for (int i = nvec * EPV + threadIdx.x; i < n; i += blockDim.x) DT<LT>::st(y + e0 + i, lds[i]);
}

// the wave's row x[0..V) in LDS: lse and H (terms with p_c == 0 count 0)
__device__ __forceinline__ void row_lse_entropy(const float *x, int V, int lane, float &lse, float &H) {
    float m = -INFINITY;
    for (int c = lane; c < V; c += 64) m = fmaxf(m, x[c]);
    m = wave_max(m);
    float se = 0.f;
    for (int c = lane; c < V; c += 64) se += expf(x[c] - m);
    lse = m + logf(wave_sum(se));
    float h = 0.f;
    for (int c = lane; c < V; c += 64) {
        const float p = expf(x[c] - lse);
        if (p > 0.f) h += p * (lse - x[c]);
    }
    H = wave_sum(h);
}

template <typename LT>
__global__ __launch_bounds__(256) void grpo_rows_kernel(const LT *__restrict__ logits, const int64_t *__restrict__ rollouts, int ld_roll,
                                                        const float *__restrict__ old_lp, int ld_old, const unsigned char *__restrict__ mask,
                                                        const float *__restrict__ adv, int N, int T, int V, float lo, float hi, float4 *stats) {
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = blockIdx.x * GRPO_POS, n1 = min(n0 + GRPO_POS, N);
    bool any = false;
    for (int n = n0; n < n1; ++n) any |= mask[n] == 0;
    if (any) stage_chunk(logits, (long)n0 * V, (long)n1 * V, lds);
    __syncthreads();
    for (int n = n0 + wave; n < n1; n += 4) {
        if (mask[n]) {
            if (lane == 0) stats[n] = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const float *x = lds + (n - n0) * V;
        float lse, H;
        row_lse_entropy(x, V, lane, lse, H);
        if (lane == 0) {
            const int r = n / T, t = n - r * T;
            const int64_t a = rollouts[(size_t)r * ld_roll + t + 1];
            const float lp = (a >= 0 && a < V ? x[a] : NAN) - lse;   // (an out-of-vocabulary action gives NaN, not an out-of-bounds read)
            const float ratio = expf(lp - old_lp[(size_t)r * ld_old + t + 1]);
            const float A = adv[r];
            const float u = ratio * A, c = fminf(fmaxf(ratio, lo), hi) * A;
            // autograd of min(u, c): a tie splits in half; c passes on to ratio on the closed band only
            const float gu = u < c ? 1.f : (u == c ? 0.5f : 0.f);
            const float gc = (ratio >= lo && ratio <= hi) ? (c < u ? 1.f : (u == c ? 0.5f : 0.f)) : 0.f;
            stats[n] = make_float4(lse, H, isnan(ratio) ? ratio : fminf(u, c), ratio * A * (gu + gc));   // (torch.minimum propagates NaN)
        }
    }
}

// one workgroup of 1024 threads: per rollout a fixed-order wave sum; wave w keeps the running sum of its rollouts w, w + 16, ... in order, and
// thread 0 adds the 16 wave sums in order
__global__ __launch_bounds__(1024) void grpo_reduce_kernel(const float4 *__restrict__ stats, const unsigned char *__restrict__ mask, int R, int T,
                                                           float num_groups, float logv, float4 *rowstat, float *out) {
    __shared__ float part[16][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float so = 0.f, sh = 0.f;
    for (int r = wave; r < R; r += 16) {
        float s = 0.f, h = 0.f, len = 0.f;
        for (int t = lane; t < T; t += 64) {
            const int n = r * T + t;
            if (!mask[n]) {
                const float4 st = stats[n];
                s += st.z;
                h += st.y;
                len += 1.f;
            }
        }
        s = wave_sum(s);
        h = wave_sum(h);
        len = wave_sum(len);
        so += s / len;
        sh += h / len;
        if (lane == 0) rowstat[r] = make_float4(s / len, h / len, len, 0.f);
    }
    if (lane == 0) {
        part[wave][0] = so;
        part[wave][1] = sh;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, b = 0.f;
        for (int w = 0; w < 16; ++w) {
            a += part[w][0];
            b += part[w][1];
        }
        out[0] = a / num_groups;
        out[1] = b / (float)R / logv;
    }
}

template <typename LT>
__global__ __launch_bounds__(256) void grpo_bwd_kernel(const LT *__restrict__ logits, const int64_t *__restrict__ rollouts, int ld_roll,
                                                       const unsigned char *__restrict__ mask, const float4 *__restrict__ stats,
                                                       const float4 *__restrict__ rowstat, const float *__restrict__ gout, int N, int T, int V, int R,
                                                       float num_groups, float logv, LT *dlogits) {
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = blockIdx.x * GRPO_POS, n1 = min(n0 + GRPO_POS, N);
    stage_chunk(logits, (long)n0 * V, (long)n1 * V, lds);
    __syncthreads();
    const float g_obj = gout[0], g_bonus = gout[1];
    for (int n = n0 + wave; n < n1; n += 4) {
        float *x = lds + (n - n0) * V;
        if (mask[n]) {
            for (int c = lane; c < V; c += 64) x[c] = 0.f;
            continue;
        }
        const int r = n / T, t = n - r * T;
        const float4 st = stats[n];
        const float len = rowstat[r].z;
        const float wv = g_obj * st.w / (len * num_groups);
        const float ub = g_bonus / ((float)R * len * logv);
        const int a = (int)rollouts[(size_t)r * ld_roll + t + 1];
        const float lse = st.x, H = st.y;
        for (int c = lane; c < V; c += 64) {
            const float xc = x[c], p = expf(xc - lse);
            const float d = c == a ? wv : 0.f;
            x[c] = p > 0.f ? d - wv * p - ub * p * (xc - lse + H) : d;
        }
    }
    __syncthreads();
    store_chunk(dlogits, (long)n0 * V, (long)n1 * V, lds);
}

}  // namespace

extern "C" int acai_grpo_objective_fwd(const void *logits, int dtype, const int64_t *rollouts, int ld_roll, const float *old_lp, int ld_old,
                                       const unsigned char *mask, const float *adv, int R, int T, int V, float clip_lo, float clip_hi, int num_groups,
                                       float logv, float *stats, float *rowstat, float *out, void *stream) {
    ACAI_CHECK_ARG(logits && rollouts && old_lp && mask && adv && stats && rowstat && out && R > 0 && T > 0 && V > 0 && V <= 1024 && ld_roll > T &&
                   ld_old > T && num_groups > 0 && (dtype == ACAI_F32 || dtype == ACAI_BF16) && aligned16(logits) && aligned16(stats) && aligned16(rowstat),
                   "acai_grpo_objective_fwd: bad arguments");
    const int N = R * T;
    const size_t lds = (size_t)GRPO_POS * V * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == ACAI_BF16)
        hipLaunchKernelGGL(grpo_rows_kernel<bf16_t>, dim3(cdiv(N, GRPO_POS)), dim3(256), lds, s, (const bf16_t *)logits, rollouts, ld_roll, old_lp, ld_old,
                           mask, adv, N, T, V, clip_lo, clip_hi, (float4 *)stats);
    else
        hipLaunchKernelGGL(grpo_rows_kernel<float>, dim3(cdiv(N, GRPO_POS)), dim3(256), lds, s, (const float *)logits, rollouts, ld_roll, old_lp, ld_old,
                           mask, adv, N, T, V, clip_lo, clip_hi, (float4 *)stats);
    ACAI_LAUNCH_CHECK("acai_grpo_objective_fwd rows");
    hipLaunchKernelGGL(grpo_reduce_kernel, dim3(1), dim3(1024), 0, s, (const float4 *)stats, mask, R, T, (float)num_groups, logv, (float4 *)rowstat, out);
    ACAI_LAUNCH_CHECK("acai_grpo_objective_fwd reduce");
    return 0;
}

extern "C" int acai_grpo_objective_bwd(const void *logits, int dtype, const int64_t *rollouts, int ld_roll, const unsigned char *mask, const float *stats,
                                       const float *rowstat, const float *grad_out, int R, int T, int V, int num_groups, float logv, void *dlogits,
                                       void *stream) {
    ACAI_CHECK_ARG(logits && rollouts && mask && stats && rowstat && grad_out && dlogits && R > 0 && T > 0 && V > 0 && V <= 1024 && ld_roll > T &&
                   num_groups > 0 && (dtype == ACAI_F32 || dtype == ACAI_BF16) && aligned16(logits) && aligned16(dlogits) && aligned16(stats) &&
                   aligned16(rowstat), "acai_grpo_objective_bwd: bad arguments");
    const int N = R * T;
    const size_t lds = (size_t)GRPO_POS * V * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == ACAI_BF16)
        hipLaunchKernelGGL(grpo_bwd_kernel<bf16_t>, dim3(cdiv(N, GRPO_POS)), dim3(256), lds, s, (const bf16_t *)logits, rollouts, ld_roll, mask,
                           (const float4 *)stats, (const float4 *)rowstat, grad_out, N, T, V, R, (float)num_groups, logv, (bf16_t *)dlogits);
    else
        hipLaunchKernelGGL(grpo_bwd_kernel<float>, dim3(cdiv(N, GRPO_POS)), dim3(256), lds, s, (const float *)logits, rollouts, ld_roll, mask,
                           (const float4 *)stats, (const float4 *)rowstat, grad_out, N, T, V, R, (float)num_groups, logv, (float *)dlogits);
    ACAI_LAUNCH_CHECK("acai_grpo_objective_bwd");
    return 0;
}

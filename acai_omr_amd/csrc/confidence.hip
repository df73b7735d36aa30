// Per-token confidence after decoding (an extension; no reference counterpart): what the selection launches of a decode step throw away.
//   acai_token_confidence       one wave per logit row: log-probability of a given token, entropy, the token's rank and the first K tokens
//                               of the row's order with their log-probabilities;
//   acai_attn_map_weighted_sum  the maps of acai_attn_probs_mean summed over the token axis with one weight per token: a heat map per image.
// Plain VALU and shuffle work; both give the same bits on every run (no floating-point atomics, fixed reduction orders).
#include "common.h"

#include <math.h>

namespace {

constexpr int CONF_MAX_K = 8;
constexpr int CONF_WAVES = 4;     // rows per workgroup
constexpr int CONF_REG = 4;       // V <= 64 * CONF_REG: the row stays in registers

struct ConfArgs {
    const float *logits;
    const int64_t *chosen;
    float *log_prob, *entropy;
    int32_t *rank, *top_ids;
    float *top_lp;
    int N, V, K;
    float tau;
};

// The row's order: raw logit descending, then index ascending (row_argmax_sumexp's and torch.argmax's first-index rule).  -inf entries
// compare equal to each other, so they come last, by index.
__device__ __forceinline__ bool before(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Wave-wide first element of the order among the lanes' candidates (ci == 0x7fffffff: the lane has none).
__device__ __forceinline__ void wave_first(float &cv, int &ci) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(cv, o);
        const int oi = __shfl_xor(ci, o);
        if (before(ov, oi, cv, ci)) {
            cv = ov;
            ci = oi;
        }
    }
}

// REG: lane owns entries lane, lane + 64, ... of a row of at most 64 * CONF_REG logits and reads them once; otherwise every sweep re-reads
// the row (it stays in L2: the sweeps of one wave follow each other).  All comparisons are on the raw logits, so rank and top_ids do not
// depend on the arithmetic of the sums.
template <bool REG>
__global__ __launch_bounds__(64 * CONF_WAVES) void token_confidence_kernel(const ConfArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * CONF_WAVES + (threadIdx.x >> 6);
    if (r >= a.N) return;   // wave-uniform; the kernel has no barrier
    const int V = a.V;
    const float *lg = a.logits + (size_t)r * V;
    const int nj = REG ? CONF_REG : (V + 63) >> 6;
    float reg[CONF_REG];
    if constexpr (REG) {
#pragma unroll
        for (int j = 0; j < CONF_REG; ++j) reg[j] = (lane + 64 * j < V) ? lg[lane + 64 * j] : -INFINITY;
    }
    auto at = [&](int j) -> float {
        if constexpr (REG) return reg[j];
        else return lg[lane + 64 * j];
    };
    const int c = (int)a.chosen[r];   // checked on the host: 0 <= c < V
    const float vc = lg[c];

    // sweep 1: the maximum (at its first index: top-1) and the chosen token's rank
    float best = -INFINITY;
    int bi = 0x7fffffff, cnt = 0;
#pragma unroll 4
    for (int j = 0; j < nj; ++j) {
        const int i = lane + 64 * j;
        if (i < V) {
            const float v = at(j);
            if (before(v, i, best, bi)) {
                best = v;
                bi = i;
            }
            cnt += before(v, i, vc, c) ? 1 : 0;
        }
    }
    wave_first(best, bi);
    cnt = wave_sum_int(cnt);

    // sweep 2: with d = (logit - max) / tau <= 0:  se = sum exp(d),  sd = sum exp(d) d;  lse - z_max = log se,  entropy = log se - sd / se
    const float tau = a.tau;
    float se = 0.f, sd = 0.f;
#pragma unroll 4
    for (int j = 0; j < nj; ++j) {
        const int i = lane + 64 * j;
        if (i < V) {
            const float d = (at(j) - best) / tau;
            const float e = expf(d);
            se += e;
            sd += e > 0.f ? e * d : 0.f;   // p = 0 (a -inf logit, or underflow) contributes 0, not 0 * -inf
        }
    }
    se = wave_sum(se);
    sd = wave_sum(sd);
    const float lse = logf(se);   // se >= 1: the maximum's own term
    if (lane == 0) {
        a.log_prob[r] = (vc - best) / tau - lse;
        a.entropy[r] = lse - sd / se;
        a.rank[r] = cnt;
    }

    // K rounds: the first element of the order that comes after the previous pick.  Nothing is marked as taken, so -inf entries can be
    // picked like any other.  Round 0 is sweep 1's arg-max.
    float pv = best;
    int pi = bi;
    for (int k = 0;; ++k) {
        if (lane == 0) {
            a.top_ids[(size_t)r * a.K + k] = pi;
            a.top_lp[(size_t)r * a.K + k] = (pv - best) / tau - lse;
        }
        if (k + 1 >= a.K) break;
        float cv = -INFINITY;
        int ci = 0x7fffffff;
#pragma unroll 4
        for (int j = 0; j < nj; ++j) {
            const int i = lane + 64 * j;
            if (i < V) {
                const float v = at(j);
                if (before(pv, pi, v, i) && before(v, i, cv, ci)) {
                    cv = v;
                    ci = i;
                }
            }
        }
        wave_first(cv, ci);
        pv = cv;
        pi = ci;   // K <= V (checked on the host): a next element exists
    }
}

constexpr int WS_COLS = 256;   // columns per workgroup, one per thread: a wave reads 256 contiguous bytes of a map row
constexpr int WS_ROWS = 32;    // tokens per split: 512 tokens x 4096 patches of ONE image are 16 x 16 workgroups

struct WsumArgs {
    const float *map;
    const int64_t *map_off;
    const int32_t *cu_q, *cu_k;
    const float *weights;
    float *dst;        // nsplit == 1: the result; otherwise the partial sums [nsplit][total_k]
    size_t total_k;
};

// Stage 1: split y of image z sums its WS_ROWS tokens in ascending order.  Split 0 always writes (an image without tokens gets zeros).
__global__ __launch_bounds__(WS_COLS) void map_wsum_partial_kernel(const WsumArgs a) {
    const int b = blockIdx.z;
    const int q0 = a.cu_q[b], T = a.cu_q[b + 1] - q0;
    const int k0 = a.cu_k[b], S = a.cu_k[b + 1] - k0;
    const int s = blockIdx.x * WS_COLS + threadIdx.x;
    const int t0 = blockIdx.y * WS_ROWS, t1 = min(t0 + WS_ROWS, T);
    if (s >= S || (blockIdx.y > 0 && t0 >= T)) return;
    const float *col = a.map + a.map_off[b] + s;
    const float *w = a.weights + q0;
    float acc = 0.f;
#pragma unroll 8
    for (int t = t0; t < t1; ++t) acc = fmaf(w[t], col[(size_t)t * S], acc);
    a.dst[(size_t)blockIdx.y * a.total_k + k0 + s] = acc;
}

// Stage 2: the splits that stage 1 wrote for the image, added in ascending order.
__global__ __launch_bounds__(WS_COLS) void map_wsum_final_kernel(const float *partial, const int32_t *cu_q, const int32_t *cu_k, size_t total_k,
                                                                float *out) {
    const int b = blockIdx.y;
    const int T = cu_q[b + 1] - cu_q[b];
    const int k0 = cu_k[b], S = cu_k[b + 1] - k0;
    const int s = blockIdx.x * WS_COLS + threadIdx.x;
    if (s >= S) return;
    const int n = max(1, (T + WS_ROWS - 1) / WS_ROWS);
    float acc = partial[(size_t)k0 + s];
    for (int j = 1; j < n; ++j) acc += partial[(size_t)j * total_k + k0 + s];
    out[(size_t)k0 + s] = acc;
}

}  // namespace

extern "C" int acai_token_confidence(const float *logits, const int64_t *chosen, int N, int V, int top_k, float temperature, float *log_prob,
                                     float *entropy, int32_t *rank, int32_t *top_ids, float *top_log_probs, void *stream) {
    ACAI_CHECK_ARG(N >= 0 && V >= 1, "acai_token_confidence: bad dims N=%d V=%d", N, V);
    ACAI_CHECK_ARG(top_k >= 1 && top_k <= CONF_MAX_K && top_k <= V, "acai_token_confidence: top_k=%d (1 <= top_k <= min(%d, V=%d))", top_k,
                   CONF_MAX_K, V);
    ACAI_CHECK_ARG(temperature > 0.f && isfinite(temperature), "acai_token_confidence: temperature=%g (must be positive and finite)",
                   (double)temperature);
    if (N == 0) return 0;
    ACAI_CHECK_ARG(logits && chosen && log_prob && entropy && rank && top_ids && top_log_probs, "acai_token_confidence: null operand");
    ConfArgs a{logits, chosen, log_prob, entropy, rank, top_ids, top_log_probs, N, V, top_k, temperature};
    const dim3 grid(cdiv(N, CONF_WAVES)), block(64 * CONF_WAVES);
    if (V <= 64 * CONF_REG)
        hipLaunchKernelGGL(token_confidence_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(token_confidence_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
    ACAI_LAUNCH_CHECK("acai_token_confidence");
    return 0;
}

extern "C" int acai_attn_map_weighted_sum(const float *map, const int64_t *map_off, const int32_t *cu_q, const int32_t *cu_k, const float *weights,
                                          int B, int max_q, int max_k, int64_t total_k, float *partial, float *out, void *stream) {
    ACAI_CHECK_ARG(map && map_off && cu_q && cu_k && weights && out, "acai_attn_map_weighted_sum: null operand");
    ACAI_CHECK_ARG(B > 0 && B <= 65535 && max_q > 0 && max_k > 0 && total_k > 0, "acai_attn_map_weighted_sum: bad dims B=%d max_q=%d max_k=%d total_k=%lld",
                   B, max_q, max_k, (long long)total_k);
    const int nsplit = cdiv(max_q, WS_ROWS);
    ACAI_CHECK_ARG(nsplit <= 65535, "acai_attn_map_weighted_sum: max_q=%d is too large", max_q);
    ACAI_CHECK_ARG(nsplit == 1 || partial, "acai_attn_map_weighted_sum: max_q=%d needs a partial buffer of %d x total_k floats", max_q, nsplit);
    hipStream_t st = (hipStream_t)stream;
    WsumArgs a{map, map_off, cu_q, cu_k, weights, nsplit == 1 ? out : partial, (size_t)total_k};
    hipLaunchKernelGGL(map_wsum_partial_kernel, dim3(cdiv(max_k, WS_COLS), nsplit, B), dim3(WS_COLS), 0, st, a);
    if (nsplit > 1)
        hipLaunchKernelGGL(map_wsum_final_kernel, dim3(cdiv(max_k, WS_COLS), B), dim3(WS_COLS), 0, st, partial, cu_q, cu_k, (size_t)total_k, out);
    ACAI_LAUNCH_CHECK("acai_attn_map_weighted_sum");
    return 0;
}

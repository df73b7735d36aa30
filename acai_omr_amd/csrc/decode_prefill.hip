// Prompt prefill of the KV-cached decode (see decode.hip): after one teacher-forced pass over the C prompt tokens that all rows share, the
// pass's self-attention K/V rows go into the decode's caches (prefill_self_kv_kernel) and its logits become the sequence state that C
// prompt steps would have left (prefill_arm_kernel), so the prompt-mode loop starts at index C + 1.
#include "decode_internal.h"

namespace {

// k_self / v_self [B][H][Tmax][dhp] <- columns E .. 3E of qkv [(b * C + p)][ld], p < C, d < dh.  One thread moves VEC elements of K and the
// same of V (VEC elements = 16 bytes, or 1 where dh, ld or a base address does not allow that).  Positions >= C, pad columns d >= dh and
// rows >= B are not touched.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void prefill_self_kv_kernel(const T *qkv, int ld, T *kc, T *vc, int B, int C, int E, int H, int dh, int dhp,
                                                              int Tmax) {
    struct alignas(sizeof(T) * VEC) Pack {
        T v[VEC];
    };
    const int per_row = E / VEC;
    const long long n = (long long)B * C * per_row;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int row = (int)(i / per_row), col = (int)(i % per_row) * VEC;   // row = b * C + p
    const int b = row / C, p = row % C, h = col / dh, d = col % dh;
    const T *src = qkv + (size_t)row * ld + E + col;
    const size_t dst = (((size_t)b * H + h) * Tmax + p) * dhp + d;
    *reinterpret_cast<Pack *>(kc + dst) = *reinterpret_cast<const Pack *>(src);
    *reinterpret_cast<Pack *>(vc + dst) = *reinterpret_cast<const Pack *>(src + E);
}

// The state C prompt steps leave, from the pass's logits [(b * C + j)][V] (row b * C + j scores output index j + 1): one wave per (row,
// index) writes seqs[b][j + 1] and logprobs[b][j + 1] as greedy_select_kernel's PROMPT form does (same reduction, same rounding); the wave of index C
// also writes finished[b] and the next step's input x[b] = emb[token] + pos[C + 1]; wave 0 writes seqs[.][0] = <bos>'s column through its
// own row, and thread 0 of workgroup 0 the shared words: finished[B] (that form's count at t = C: a row with C < len[b] is
// unfinished) and step.  A table entry that gives no token (index past len[b], id outside [0, V)) falls back to the row's own arg-max, as
// the prompt step does at that index, so no table content indexes out of bounds - but unlike there the later indices do not see it: the
// host refuses such a prompt.
__global__ __launch_bounds__(256) void prefill_arm_kernel(const float *logits, int V, int B, int C, int64_t *seqs, float *logprobs, int max_len,
                                                          int32_t *step, int32_t *finished, int bos, int eos, int round_lp,
                                                          const int32_t *ptok, const int32_t *plen, int ppitch, const float *emb,
                                                          const float *pos, float *x, int E, int Tmax) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);   // wave-uniform
    if (w < B * C) {
        const int b = w / C, j = w % C, t = j + 1;
        const float *lg = logits + (size_t)w * V;
        float best;
        int bi;
        const float se = row_argmax_sumexp(lg, V, lane, best, bi);
        const int P = prompt_len(plen, b, ppitch, max_len);
        const int forced = prompt_token(ptok, b, ppitch, t, P, V);
        const int tok = forced >= 0 ? forced : min(bi, V - 1);   // (bi stays at its start value when every logit is NaN)
        float lp = -(logf(se) - (lg[tok] - best));
        if (round_lp) lp = round_bf16(lp);
        if (lane == 0) {
            if (j == 0) seqs[(size_t)b * max_len] = bos;
            seqs[(size_t)b * max_len + t] = tok;
            logprobs[(size_t)b * max_len + t] = lp;
            if (t == C) finished[b] = tok == eos ? 1 : 0;
        }
        if (t == C && C + 1 < Tmax)   // the input of step C + 1 (quirk Q1: the token at index C is embedded with position C + 1)
            for (int i = lane; i < E; i += 64) x[(size_t)b * E + i] = emb[(size_t)tok * E + i] + pos[(size_t)(C + 1) * E + i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int tot = 0;
        for (int b = 0; b < B; ++b) {
            const int P = prompt_len(plen, b, ppitch, max_len);
            const bool fin = prompt_token(ptok, b, ppitch, C, P, V) == eos;
            tot += (fin && C >= P) ? 0 : 1;
        }
        finished[B] = tot;
        step[0] = C + 1;
        step[1] = C;
    }
}

template <typename T>
int launch_prefill_self_kv_t(const AcaiDecoder *d, int layer, const void *qkv, int ld, int C, hipStream_t st) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const AcaiDecLayer *ly = d->layers + layer;
    const bool wide = d->dh % VEC == 0 && ld % VEC == 0 && d->E % VEC == 0 && aligned16(qkv) && aligned16(ly->k_self) && aligned16(ly->v_self);
    const long long n = (long long)d->B * C * (d->E / (wide ? VEC : 1));
    const dim3 grid((unsigned)((n + 255) / 256));
    if (wide)
        hipLaunchKernelGGL((prefill_self_kv_kernel<T, VEC>), grid, dim3(256), 0, st, (const T *)qkv, ld, (T *)ly->k_self, (T *)ly->v_self, d->B,
                           C, d->E, d->H, d->dh, d->dhp, d->Tmax);
    else
        hipLaunchKernelGGL((prefill_self_kv_kernel<T, 1>), grid, dim3(256), 0, st, (const T *)qkv, ld, (T *)ly->k_self, (T *)ly->v_self, d->B, C,
                           d->E, d->H, d->dh, d->dhp, d->Tmax);
    ACAI_LAUNCH_CHECK("prefill_self_kv");
    return 0;
}

}  // namespace

int launch_prefill_self_kv(const AcaiDecoder *d, int layer, const void *qkv, int ld, int C, hipStream_t st) {
    return d->dtype == ACAI_BF16 ? launch_prefill_self_kv_t<bf16_t>(d, layer, qkv, ld, C, st)
                                 : launch_prefill_self_kv_t<float>(d, layer, qkv, ld, C, st);
}

int launch_prefill_arm(const AcaiDecoder *d, const AcaiPrompt *pr, const float *logits, int C, hipStream_t st) {
    hipLaunchKernelGGL(prefill_arm_kernel, dim3((unsigned)cdiv(d->B * C, 4)), dim3(256), 0, st, logits, d->V, d->B, C, d->seqs, d->logprobs,
                       d->max_len, d->step, d->finished, d->bos, d->eos, (d->flags & ACAI_GEMM_ROUND_BF16) ? 1 : 0, pr->tok, pr->len, pr->pitch,
                       d->emb, d->pos, d->x, d->E, d->Tmax);
    ACAI_LAUNCH_CHECK("prefill_arm");
    return 0;
}

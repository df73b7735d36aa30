// Token selection of a decode step (see decode.hip): embedding, greedy / sampled / slot / speculative / beam / grammar-constrained selection and their
// bookkeeping, each with the host helper that launches it from the decoder descriptor.
#include "decode_internal.h"

namespace {

// x[b,:] = vocab_embedding[token_b] + pos_embedding[t]; token from `tokens` or seqs[b, t-1] (quirk Q1: M:576)
__global__ __launch_bounds__(256) void embed_kernel(const float *emb, const float *pos, const int64_t *tokens, const int64_t *seqs,
                                                    const int32_t *step, int max_len, float *x, int E) {
    const int b = blockIdx.x, t = step[0];
    const int64_t tok = tokens ? tokens[b] : seqs[(size_t)b * max_len + t - 1];
    for (int i = threadIdx.x; i < E; i += 256) x[(size_t)b * E + i] = emb[(size_t)tok * E + i] + pos[(size_t)t * E + i];
}

__global__ void set_step_kernel(int32_t *step, int t) { step[0] = t; }

// (row_argmax_sumexp, the row maximum / arg-max / sum of exponentials all selection kernels start from, is in common.h)
// cached_get_next_token (M:579-581) + loop bookkeeping (M:606-611).  One workgroup, wave w takes rows w, w+4, ...
// With `emb`: the wave that chose row b's token also writes the NEXT step's input x[b] = vocab_embedding[token] + pos_embedding[t + 1]
// (quirk Q1: the token at index t is embedded with position t + 1, M:576), so a token step needs no embed launch of its own.
__global__ __launch_bounds__(1024) void argmax_logprob_kernel(const float *logits, int V, int B, int64_t *seqs, float *logprobs,
                                                             int max_len, int32_t *step, int32_t *finished, int eos, int round_lp,
                                                             int bookkeeping, const float *emb, const float *pos, float *x, int E, int Tmax) {
    __shared__ int unfinished[16];   // up to 16 waves: one row per wave for the usual batch sizes (the rows of a wave run back to back)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = step[0];
    int cnt = 0;
    const int nw = blockDim.x >> 6;
    for (int b = wave; b < B; b += nw) {
        const float *lg = logits + (size_t)b * V;
        float best;
        int bi;
        const float se = row_argmax_sumexp(lg, V, lane, best, bi);
        float lp = -logf(se);  // logit[argmax] - logsumexp
        if (round_lp) lp = round_bf16(lp);
        if (bookkeeping) {
            int fin = finished[b];
            if (bi == eos) fin = 1;
            if (lane == 0) {
                seqs[(size_t)b * max_len + t] = bi;
                logprobs[(size_t)b * max_len + t] = lp;
                finished[b] = fin;
            }
            cnt += fin ? 0 : 1;
            if (emb && t + 1 < Tmax)
                for (int i = lane * 4; i < E; i += 256) {
                    const float4 ev = *reinterpret_cast<const float4 *>(emb + (size_t)bi * E + i), pv = *reinterpret_cast<const float4 *>(pos + (size_t)(t + 1) * E + i);
                    *reinterpret_cast<float4 *>(x + (size_t)b * E + i) = make_float4(ev.x + pv.x, ev.y + pv.y, ev.z + pv.z, ev.w + pv.w);
                }
        } else if (lane == 0) {
            seqs[b] = bi;
            logprobs[b] = lp;
        }
    }
    if (lane == 0) unfinished[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < nw; ++w) tot += unfinished[w];
        if (bookkeeping) finished[B] = tot;
        step[0] = t + 1;
        step[1] = step[1] + 1;
    }
}

// ---- prompted decoding (an extension: the reference starts every sequence from <bos> alone) -----------------------------------------------
// (prompt_len / prompt_token, the clamped reads of the prompt tables, are in common.h: decode_prefill.hip shares them)
// argmax_logprob_kernel (with its bookkeeping) whose token at index t <= len[b] is the prompt's.  The log-prob of token k is
// -(logf(se) - (logit[k] - max)): for the arg-max the inner difference is exactly 0 and the value is argmax_logprob_kernel's -logf(se) bit for
// bit (beam_select_kernel's form).  A row inside its prompt (t < len[b]) counts as unfinished.
__global__ __launch_bounds__(1024) void prompt_logprob_kernel(const float *logits, int V, int B, int64_t *seqs, float *logprobs, int max_len,
                                                             int32_t *step, int32_t *finished, int eos, int round_lp, const int32_t *ptok,
                                                             const int32_t *plen, int ppitch, const float *emb, const float *pos, float *x,
                                                             int E, int Tmax) {
    __shared__ int unfinished[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = step[0];
    int cnt = 0;
    const int nw = blockDim.x >> 6;
    for (int b = wave; b < B; b += nw) {
        const float *lg = logits + (size_t)b * V;
        float best;
        int bi;
        const float se = row_argmax_sumexp(lg, V, lane, best, bi);
        const int P = prompt_len(plen, b, ppitch, max_len);
        const int forced = prompt_token(ptok, b, ppitch, t, P, V);
        const int tok = forced >= 0 ? forced : bi;
        float lp = -(logf(se) - (lg[tok] - best));
        if (round_lp) lp = round_bf16(lp);
        int fin = finished[b];
        if (tok == eos) fin = 1;
        if (lane == 0) {
            seqs[(size_t)b * max_len + t] = tok;
            logprobs[(size_t)b * max_len + t] = lp;
            finished[b] = fin;
        }
        cnt += (fin && t >= P) ? 0 : 1;
        if (emb && t + 1 < Tmax)   // next step's input (see argmax_logprob_kernel)
            for (int i = lane * 4; i < E; i += 256) {
                const float4 ev = *reinterpret_cast<const float4 *>(emb + (size_t)tok * E + i), pv = *reinterpret_cast<const float4 *>(pos + (size_t)(t + 1) * E + i);
                *reinterpret_cast<float4 *>(x + (size_t)b * E + i) = make_float4(ev.x + pv.x, ev.y + pv.y, ev.z + pv.z, ev.w + pv.w);
            }
    }
    if (lane == 0) unfinished[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < nw; ++w) tot += unfinished[w];
        finished[B] = tot;
        step[0] = t + 1;
        step[1] = step[1] + 1;
    }
}

// GRPOViTOMR.cached_forward_rollout_policy (M:988-1049), one sampling step: top-k filter, softmax with temperature over the kept logits,
// draw from that distribution, log-prob of the drawn token under the UN-tempered softmax of the kept logits (the reference takes
// log_softmax(top_k_logits), M:1017).  torch.multinomial's Philox stream is not reproducible here; the draw is the inverse CDF of a caller
// supplied uniform u[b][t] over the kept logits in descending order (ties: lower vocabulary index first), so a step is a pure function of
// (logits, u) that the oracle restates.  One wave per row: k rounds of a wave-wide arg-max build the sorted top-k (k <= 64).
// The per-row part, shared by the static and the slot sampler so that a sequence draws the same tokens in either: wave-wide, `sv` / `si` are
// the wave's own 64 LDS entries.  Returns the drawn token; lp = log_softmax(kept)[drawn] (not rounded).
__device__ __forceinline__ int topk_draw_row(const float *lg, int V, int lane, float *sv, int *si, int top_k, float inv_temperature, float u,
                                             float &lp) {
    // lane owns vocabulary entries lane, lane + 64, ... (V <= 512)
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (lane + 64 * j < V) ? lg[lane + 64 * j] : -INFINITY;
    const int k = min(top_k, V);
    for (int r = 0; r < k; ++r) {
        float best = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (v[j] > best) {   // ascending j = ascending index: first maximum wins
                best = v[j];
                bi = lane + 64 * j;
            }
        if (best == -INFINITY) bi = 0x7fffffff;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o);
            const int oi = __shfl_xor(bi, o);
            if (ov > best || (ov == best && oi < bi)) {
                best = ov;
                bi = oi;
            }
        }
        if ((bi & 63) == lane) {   // owner removes the winner
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (bi == lane + 64 * j) v[j] = -INFINITY;
        }
        if (lane == 0) {
            sv[r] = best;
            si[r] = bi;
        }
    }
    // same wave wrote and reads: LDS operations of a wave complete in order
    const bool in = lane < k;
    const float x = in ? sv[lane] : -INFINITY, m = sv[0];
    const float pT = in ? expf((x - m) * inv_temperature) : 0.f;   // softmax(top_k_logits / temperature), unnormalised
    const float p1 = in ? expf(x - m) : 0.f;                       // softmax(top_k_logits), unnormalised
    const float sumT = wave_sum(pT), sum1 = wave_sum(p1);
    float cdf = pT;                                                // inclusive prefix sum over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(cdf, o);
        if (lane >= o) cdf += up;
    }
    const float target = u * sumT;
    const unsigned long long hit = __ballot(in && cdf > target);
    const int r = hit ? __builtin_ctzll(hit) : k - 1;              // rounding at the top of the CDF: last kept entry
    lp = (sv[r] - m) - logf(sum1);
    return si[r];
}

__global__ __launch_bounds__(256) void sample_logprob_kernel(const float *logits, int V, int B, int64_t *seqs, float *logprobs, int max_len,
                                                             const int32_t *step, int32_t *finished, int eos, int round_lp,
                                                             const float *uniforms, int top_k, float inv_temperature, const float *emb,
                                                             const float *pos, float *xnext, int E, int Tmax) {
    __shared__ float sv[4][64];
    __shared__ int si[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + wave;
    if (b >= B) return;
    const int t = step[0];
    float lp;
    const int tok = topk_draw_row(logits + (size_t)b * V, V, lane, sv[wave], si[wave], top_k, inv_temperature,
                                  uniforms[(size_t)b * max_len + t], lp);
    if (round_lp) lp = round_bf16(lp);
    if (lane == 0) {
        seqs[(size_t)b * max_len + t] = tok;
        logprobs[(size_t)b * max_len + t] = lp;
        if (tok == eos) finished[b] = 1;
    }
    if (emb && t + 1 < Tmax)   // next step's input (see argmax_logprob_kernel)
        for (int i = lane * 4; i < E; i += 256) {
            const float4 ev = *reinterpret_cast<const float4 *>(emb + (size_t)tok * E + i), pv = *reinterpret_cast<const float4 *>(pos + (size_t)(t + 1) * E + i);
            *reinterpret_cast<float4 *>(xnext + (size_t)b * E + i) = make_float4(ev.x + pv.x, ev.y + pv.y, ev.z + pv.z, ev.w + pv.w);
        }
}

// loop bookkeeping after a sampling step: unfinished count, advance position and cache length
__global__ __launch_bounds__(64) void sample_bookkeeping_kernel(int B, int32_t *step, int32_t *finished) {
    int cnt = 0;
    for (int b = threadIdx.x; b < B; b += 64) cnt += finished[b] ? 0 : 1;
    cnt = (int)wave_sum((float)cnt);
    if (threadIdx.x == 0) {
        finished[B] = cnt;
        step[0] = step[0] + 1;
        step[1] = step[1] + 1;
    }
}

__global__ void advance_cache_kernel(int32_t *step) { step[1] = step[1] + 1; }

// ---- continuous batching (slot mode; an extension: the reference decodes one static batch) --------------------------------------------
// The greedy token of every unfinished row at its OWN local time t = slot_t[b] (argmax_logprob_kernel's reduction, so a row decodes as it
// would in a greedy batch): seqs / logprobs at index t, then either the row finishes (<eos>, or t has reached its cap - 1) and from then on
// writes nothing, or t advances and the wave writes the row's next input emb[token] + pos[t + 1] (quirk Q1).  Thread 0 publishes the
// unfinished count finished[B] and advances the shared ring write index step[1] modulo Tmax.  step[0] is not used in slot mode.
__global__ __launch_bounds__(1024) void slot_argmax_kernel(const float *logits, int V, int B, int64_t *seqs, float *logprobs, int max_len,
                                                          int32_t *step, int32_t *finished, int32_t *slot_t, const int32_t *slot_cap, int eos,
                                                          int round_lp, const float *emb, const float *pos, float *x, int E, int Tmax) {
    __shared__ int unfinished[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int cnt = 0;
    const int nw = blockDim.x >> 6;
    for (int b = wave; b < B; b += nw) {
        if (finished[b]) continue;   // wave-uniform: a finished or idle row writes nothing
        const int t = slot_t[b];
        const float *lg = logits + (size_t)b * V;
        float best;
        int bi;
        const float se = row_argmax_sumexp(lg, V, lane, best, bi);
        float lp = -logf(se);
        if (round_lp) lp = round_bf16(lp);
        const bool fin = bi == eos || t >= slot_cap[b] - 1;
        if (lane == 0) {
            seqs[(size_t)b * max_len + t] = bi;
            logprobs[(size_t)b * max_len + t] = lp;
            if (fin) finished[b] = 1;
            else slot_t[b] = t + 1;
        }
        if (!fin) {   // t + 1 <= cap - 1 < max_len <= Tmax
            cnt += 1;
            for (int i = lane * 4; i < E; i += 256) {
                const float4 ev = *reinterpret_cast<const float4 *>(emb + (size_t)bi * E + i), pv = *reinterpret_cast<const float4 *>(pos + (size_t)(t + 1) * E + i);
                *reinterpret_cast<float4 *>(x + (size_t)b * E + i) = make_float4(ev.x + pv.x, ev.y + pv.y, ev.z + pv.z, ev.w + pv.w);
            }
        }
    }
    if (lane == 0) unfinished[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < nw; ++w) tot += unfinished[w];
        finished[B] = tot;
        const int nxt = step[1] + 1;
        step[1] = nxt >= Tmax ? 0 : nxt;
    }
}

// The sampling form of slot_argmax_kernel: the token of every unfinished row is topk_draw_row's at the row's local time t = slot_t[b], with
// the uniform uniforms[urow[b]][t] of the sequence the slot decodes (urow is set when the slot is armed), so a sequence draws what it draws
// alone in sample_logprob_kernel whichever slot and step it runs in.  One wave per row over gridDim.x workgroups of four (the k rounds of
// a row are a serial chain: one workgroup for every row would put them end to end).  With more than one workgroup the unfinished count and
// the ring index are written by the workgroup that arrives last at `ticket` (zero between launches, re-armed here): every workgroup
// publishes its rows' flags with agent-scope atomic stores before it takes its ticket, and the last one reads all flags the same way.
__global__ __launch_bounds__(256) void slot_sample_kernel(const float *logits, int V, int B, int64_t *seqs, float *logprobs, int max_len,
                                                          int32_t *step, int32_t *finished, int32_t *slot_t, const int32_t *slot_cap, int eos,
                                                          int round_lp, const float *uniforms, int ld_uniforms, const int32_t *urow, int top_k,
                                                          float inv_temperature, const float *emb, const float *pos, float *x, int E, int Tmax,
                                                          unsigned *ticket) {
    __shared__ float sv[4][64];
    __shared__ int si[4][64];
    __shared__ int is_last;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = blockIdx.x * 4 + wave; b < B; b += gridDim.x * 4) {
        if (finished[b]) continue;   // wave-uniform: a finished or idle row writes nothing
        const int t = slot_t[b];
        float lp;
        const int tok = topk_draw_row(logits + (size_t)b * V, V, lane, sv[wave], si[wave], top_k, inv_temperature,
                                      uniforms[(size_t)urow[b] * ld_uniforms + t], lp);
        if (round_lp) lp = round_bf16(lp);
        const bool fin = tok == eos || t >= slot_cap[b] - 1;
        if (lane == 0) {
            seqs[(size_t)b * max_len + t] = tok;
            logprobs[(size_t)b * max_len + t] = lp;
            if (fin) __hip_atomic_store(finished + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else slot_t[b] = t + 1;
        }
        if (!fin)   // t + 1 <= cap - 1 < max_len <= Tmax
            for (int i = lane * 4; i < E; i += 256) {
                const float4 ev = *reinterpret_cast<const float4 *>(emb + (size_t)tok * E + i), pv = *reinterpret_cast<const float4 *>(pos + (size_t)(t + 1) * E + i);
                *reinterpret_cast<float4 *>(x + (size_t)b * E + i) = make_float4(ev.x + pv.x, ev.y + pv.y, ev.z + pv.z, ev.w + pv.w);
            }
    }
    if (gridDim.x > 1) {
        __threadfence();   // this thread's flag stores are visible device-wide before the workgroup's ticket
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned n = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            is_last = n == gridDim.x - 1;
            if (is_last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    if (gridDim.x > 1 && !is_last) return;
    if (wave == 0) {
        int cnt = 0;
        for (int b = lane; b < B; b += 64) cnt += __hip_atomic_load(finished + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 0 : 1;
        cnt = (int)wave_sum((float)cnt);
        if (lane == 0) {
            finished[B] = cnt;
            const int nxt = step[1] + 1;
            step[1] = nxt >= Tmax ? 0 : nxt;
        }
    }
}

// Arms row rows[i] (one workgroup each) for a new sequence: <bos> then <pad>, log-probs 0, unfinished, local time 1 starting at the current
// ring write index step[1], cap rows[n + i] (clamped to [2, max_len]) and the first input emb[<bos>] + pos[1].  Rows outside [0, B) are
// ignored.
__global__ __launch_bounds__(256) void slot_arm_kernel(const int32_t *rows, int n, int B, int max_len, int64_t *seqs, float *logprobs,
                                                       int32_t *finished, int32_t *slot_t, int32_t *slot_first, int32_t *slot_cap,
                                                       const int32_t *step, int bos, int pad, const float *emb,
                                                       const float *pos, float *x, int E) {
    const int r = rows[blockIdx.x];
    if (r < 0 || r >= B) return;
    const int cap = min(max(rows[n + blockIdx.x], 2), max_len);
    for (int p = threadIdx.x; p < max_len; p += 256) {
        seqs[(size_t)r * max_len + p] = p == 0 ? bos : pad;
        logprobs[(size_t)r * max_len + p] = 0.f;
    }
    for (int i = threadIdx.x; i < E; i += 256) x[(size_t)r * E + i] = emb[(size_t)bos * E + i] + pos[(size_t)E + i];
    if (threadIdx.x == 0) {
        finished[r] = 0;
        slot_t[r] = 1;
        slot_first[r] = step[1];
        slot_cap[r] = cap;
    }
}

// What every slot wrote since the caller last looked (acai_decode_slot_flush; the steps leave t at the last token of a finished row and
// past the last token of a running one).  One wave per slot, four to a workgroup: the lanes stride over the slot's n new entries, so the
// int64 reads and the int32 / fp32 writes of a wave are consecutive addresses; lanes 0 .. 3 write the header as one 16-byte run.  mark[s]
// has one reader and one writer, this wave, and every lane has read it before lane 0 stores it.  Nothing but mark and the outputs is
// written.
__global__ __launch_bounds__(256) void slot_flush_kernel(const int64_t *seqs, const float *logprobs, int max_len, const int32_t *slot_t,
                                                         const int32_t *finished, int32_t *mark, int B, int ld, int32_t *out_tok,
                                                         float *out_lp, int32_t *hdr) {
    const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= B) return;   // wave-uniform
    const int fin = finished[s] != 0, m = mark[s];
    const int end = min(slot_t[s] + fin, max_len);               // (never past the row, whatever t holds)
    const int n = m < 0 ? 0 : min(max(end - m, 0), ld);          // (a mark below 0 is no index of the row: nothing is read)
    const int64_t *tok = seqs + (size_t)s * max_len + m;
    const float *lp = logprobs + (size_t)s * max_len + m;
    for (int i = lane; i < n; i += 64) {
        out_tok[(size_t)s * ld + i] = (int32_t)tok[i];
        out_lp[(size_t)s * ld + i] = lp[i];
    }
    if (lane < 4) hdr[4 * s + lane] = lane == 0 ? n : lane == 1 ? m : lane == 2 ? fin : 0;
    if (lane == 0) mark[s] = m + n;
}

// ---- speculative greedy decoding (an extension: the reference emits one token per step) -------------------------------------------------
// An image owns R = D + 1 consecutive decode rows.  Before a verify step, next[i][0] is the image's last emitted token (index t - 1) and
// next[i][1..D] the draft tokens for indices t .. t + D - 1 (-1 = none); row j consumed next[i][j] at position t + j (quirk Q1) and its
// logits predict index t + j.  One workgroup closes the step (and, with arm set, opens the run):
//   1. wave w: the greedy token and log-prob of rows w, w + nw, ... (argmax_logprob_kernel's reduction) into LDS;
//   2. wave w: images w, w + nw, ...: accept - g_0, then g_j while draft j equals g_{j-1} - written at t .. t + n, cut at the first <eos>
//      and at cap - 1; t, finished[i], steps[i];
//   3. the same wave drafts the next step: from the injected table drafts[i][index] when given, else by prompt lookup - for m = ngram .. 1
//      the most recent earlier occurrence of the sequence's last m tokens, the first m that has one proposes the up to D tokens after it -
//      and writes next[i][], the table entries of indices t - 1 .. t - 1 + D (row j at the NEXT write index) and every row's input x;
//   4. thread 0: the unfinished count finished[B] and the shared write index step[1].
// Every loop is bounded by cap <= max_len or by B.
struct SpecArgs {
    const float *logits;
    int V, B, R, E, Tmax, ld, eos, pad, round_lp, ngram, arm, pitch;
    int64_t *seqs;
    float *logprobs;
    int32_t *step, *finished;
    const float *emb, *pos;
    float *x;
    int32_t *t, *steps, *tab, *next;
    const int32_t *cap, *drafts;
};

// A prompted run (acai_decode_spec_prompt_step): the verify step with image i's prompt row i.  Row j at write index t emits the prompt's token
// while t + j <= len[i], with prompt_logprob_kernel's log-prob, and while the new t <= len[i] the next step's drafts are the prompt's tokens
// of indices <= len[i] (none beyond), so that they are all accepted.  The kernel is a template over its argument struct: the unprompted
// instantiation compiles to what it was.
struct SpecPromptArgs : SpecArgs {
    const int32_t *ptok, *plen;
    int ppitch;
};
template <typename A> struct spec_prompted { static constexpr bool value = false; };
template <> struct spec_prompted<SpecPromptArgs> { static constexpr bool value = true; };

template <typename A>
__global__ __launch_bounds__(1024) void spec_accept_kernel(A a) {
    constexpr bool PROMPT = spec_prompted<A>::value;
    extern __shared__ int spec_dyn[];   // [B] greedy tokens, [B] their log-probs
    __shared__ int unfinished[16];
    int *g_tok = spec_dyn;
    float *g_lp = reinterpret_cast<float *>(spec_dyn + a.B);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int R = a.R, nimg = a.B / R;
    if (!a.arm)
        for (int b = wave; b < a.B; b += nw) {
            float best;
            int bi;
            const float se = row_argmax_sumexp(a.logits + (size_t)b * a.V, a.V, lane, best, bi);
            float lp = -logf(se);
            if constexpr (PROMPT) {   // row b predicts index t + b % R of image b / R
                const int img = b / R;
                const int forced = prompt_token(a.ptok, img, a.ppitch, a.t[img] + b % R, prompt_len(a.plen, img, a.ppitch, a.ld), a.V);
                if (forced >= 0) {
                    lp = -(logf(se) - (a.logits[(size_t)b * a.V + forced] - best));
                    bi = forced;
                }
            }
            if (a.round_lp) lp = round_bf16(lp);
            if (lane == 0) {
                g_tok[b] = bi;
                g_lp[b] = lp;
            }
        }
    __syncthreads();   // (also orders the a.t reads above before the writes below)
    const int wnext = min(a.step[1] + (a.arm ? 0 : 1), a.Tmax - 1);   // the cache position the next step's rows write
    int cnt = 0;
    for (int img = wave; img < nimg; img += nw) {
        int64_t *sq = a.seqs + (size_t)img * a.ld;
        float *lq = a.logprobs + (size_t)img * a.ld;
        int32_t *nx = a.next + (size_t)img * 8;
        const int cap = min(a.cap[img], min(a.ld, a.pitch));
        int t = a.t[img], fin = a.finished[img];
        if (t < 1 || t >= cap) fin = 1;   // (an armed, unfinished image has 1 <= t <= cap - 1)
        if (!a.arm && !fin) {
            int n = 0;
            for (int j = 0; j < R; ++j) {   // wave-uniform
                if (j > 0 && nx[j] != g_tok[img * R + j - 1]) break;   // draft j was wrong (or none): row j saw another sequence
                if (t + j >= cap) break;
                const int tok = g_tok[img * R + j];
                if (lane == 0) {
                    sq[t + j] = tok;
                    lq[t + j] = g_lp[img * R + j];
                }
                n = j + 1;
                if (tok == a.eos) {
                    fin = 1;
                    break;
                }
            }
            t += n;
            if (t >= cap) fin = 1;
            if (lane == 0) {
                a.t[img] = t;
                a.steps[img] += 1;
            }
            __threadfence();   // lane 0's tokens are read back by every lane of this wave below
        }
        if (lane == 0) a.finished[img] = fin;
        if (fin) continue;
        cnt += 1;
        // the next step's inputs: lane j < R holds the token row j consumes (index t - 1 + j), -1 = none
        int mine = -1;
        bool in_prompt = false;
        if constexpr (PROMPT) {
            const int P = prompt_len(a.plen, img, a.ppitch, a.ld);
            in_prompt = t <= P;   // wave-uniform
            if (in_prompt && lane >= 1 && lane < R && t + lane < cap) mine = prompt_token(a.ptok, img, a.ppitch, t - 1 + lane, P, a.V);
        }
        if (in_prompt) {
        } else if (a.drafts) {
            const int idx = t - 1 + lane;
            if (lane >= 1 && lane < R && t + lane < cap) {   // (a row whose prediction index would reach cap is idle)
                const int v = a.drafts[(size_t)img * a.pitch + idx];
                mine = (v >= 0 && v < a.V) ? v : -1;
            }
        } else {
            int e_found = -1;
            for (int m = min(a.ngram, t - 1); m >= 1 && e_found < 0; --m)
                for (int base = t - 1; base >= m; base -= 64) {   // candidate ends e (exclusive) from the most recent down
                    const int e = base - lane;
                    bool ok = e >= m;
                    if (ok)
                        for (int i = 0; i < m; ++i)
                            if (sq[e - m + i] != sq[t - m + i]) {
                                ok = false;
                                break;
                            }
                    const unsigned long long hit = __ballot(ok);
                    if (hit) {
                        e_found = base - __builtin_ctzll(hit);
                        break;
                    }
                }
            if (e_found >= 0 && lane >= 1 && lane < R && e_found + lane - 1 < t && t + lane < cap) mine = (int)sq[e_found + lane - 1];
        }
        if (lane == 0) mine = (int)sq[t - 1];
        if (lane < R) {
            nx[lane] = mine;
            const int idx = t - 1 + lane;
            if (idx < a.pitch) a.tab[(size_t)img * a.pitch + idx] = wnext * 8 + lane;
        }
        for (int j = 0; j < R; ++j) {
            const int tk = __shfl(mine, j), tok = tk < 0 ? a.pad : tk, p = min(t + j, a.Tmax - 1);
            float *xr = a.x + (size_t)(img * R + j) * a.E;
            for (int i = lane; i < a.E; i += 64) xr[i] = a.emb[(size_t)tok * a.E + i] + a.pos[(size_t)p * a.E + i];
        }
    }
    if (lane == 0) unfinished[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < nw; ++w) tot += unfinished[w];
        a.finished[a.B] = tot;
        if (!a.arm) a.step[1] = min(a.step[1] + 1, a.Tmax - 1);
    }
}

// ---- beam search (an extension: the reference decodes greedily) ------------------------------------------------------------------------

struct BeamArgs {
    const float *logits;
    int V, K, E, Tmax, pitch, eos, pad, round_lp;
    const int32_t *step;
    int32_t *finished;
    const float *emb, *pos;
    float *x;
    int32_t *anc;
    int64_t *tok;
    float *lp;
    long long bstride;   // elements between the two parity copies of the lineage
    float *cum;
    int32_t *len;
};

// One workgroup per image (rows r0 .. r0 + K - 1), step t = step[0]; lineage copy (t & 1) is read, copy (t + 1) & 1 written.
//   1. the K rows' (cum, finished, len) into LDS (this workgroup is their only writer);
//   2. wave w builds the candidates of rows w, w + 4, ...: a live row its K best tokens by raw logit in K rounds of a wave-wide arg-max (lower
//      index first on ties, sample_logprob_kernel's pattern), score cum + lp with greedy's row max / sum of exponentials; a finished row the
//      single candidate (itself + <pad>, lp 0, score cum); a row at cum = -inf none.  Candidate c = parent * K + rank;
//   3. thread c ranks its candidate against all K*K (score descending, then c ascending = parent slot, then rank): rank j < K -> slot j;
//   4. wave w fills new slots w, w + 4, ...: the parent's lineage up to position t - 1 plus (slot, token, lp) at t, cum, finished, len and the
//      next step's input emb[token] + pos[t + 1].
__global__ __launch_bounds__(256) void beam_select_kernel(BeamArgs a) {
    __shared__ float cs[BEAM_MAX * BEAM_MAX], clp[BEAM_MAX * BEAM_MAX];
    __shared__ int ctok[BEAM_MAX * BEAM_MAX];
    __shared__ float pcum[BEAM_MAX];
    __shared__ int pfin[BEAM_MAX], plen[BEAM_MAX], sel[BEAM_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, NC = K * K, r0 = blockIdx.x * K;
    const int t = a.step[0];
    const size_t cur = (size_t)(t & 1) * a.bstride, nxt = (size_t)((t + 1) & 1) * a.bstride;
    if (tid < K) {
        pcum[tid] = a.cum[r0 + tid];
        pfin[tid] = a.finished[r0 + tid];
        plen[tid] = a.len[r0 + tid];
        sel[tid] = -1;
    }
    if (tid < NC) cs[tid] = -INFINITY;
    __syncthreads();
    const int kv = min(K, a.V);
    for (int k = wave; k < K; k += 4) {
        const float c0 = pcum[k];
        if (c0 == -INFINITY) continue;
        if (pfin[k]) {
            if (lane == 0) {
                cs[k * K] = c0;
                ctok[k * K] = a.pad;
                clp[k * K] = 0.f;
            }
            continue;
        }
        const float *lg = a.logits + (size_t)(r0 + k) * a.V;
        float best;
        int bi;
        const float lse = logf(row_argmax_sumexp(lg, a.V, lane, best, bi));
        float v[8];   // lane owns vocabulary entries lane, lane + 64, ... (V <= 512)
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (lane + 64 * j < a.V) ? lg[lane + 64 * j] : -INFINITY;
        for (int r = 0; r < kv; ++r) {
            float bv = -INFINITY;
            int bj = 0x7fffffff;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (v[j] > bv) {
                    bv = v[j];
                    bj = lane + 64 * j;
                }
            if (bv == -INFINITY) bj = 0x7fffffff;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o);
                const int oi = __shfl_xor(bj, o);
                if (ov > bv || (ov == bv && oi < bj)) {
                    bv = ov;
                    bj = oi;
                }
            }
            if ((bj & 63) == lane) {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (bj == lane + 64 * j) v[j] = -INFINITY;
            }
            if (lane == 0 && bj < a.V) {
                const float l = -(lse - (bv - best));   // = (logit - max) - lse; -lse exactly for the arg-max (greedy's -logf(se))
                cs[k * K + r] = c0 + l;
                ctok[k * K + r] = bj;
                clp[k * K + r] = l;
            }
        }
    }
    __syncthreads();
    if (tid < NC) {
        const float sc = cs[tid];
        if (sc > -INFINITY) {
            int rank = 0;
            for (int c = 0; c < NC; ++c) {
                const float o = cs[c];
                rank += (o > sc || (o == sc && c < tid)) ? 1 : 0;
            }
            if (rank < K) sel[rank] = tid;
        }
    }
    __syncthreads();
    for (int j = wave; j < K; j += 4) {
        const int c = sel[j], row = r0 + j;
        int par = j, tk = a.pad, fin = 1, ln = 0;
        float l = 0.f, sc = -INFINITY;
        if (c >= 0) {   // (no candidate: a dead slot - it keeps its own lineage, extended by <pad>)
            par = c / K;
            tk = ctok[c];
            l = clp[c];
            sc = cs[c];
            if (pfin[par]) {
                ln = plen[par];
            } else if (tk == a.eos) {
                ln = t;
            } else {
                fin = 0;
            }
        }
        const size_t src = cur + (size_t)(r0 + par) * a.pitch, dst = nxt + (size_t)row * a.pitch;
        const int tc = min(t, a.pitch);
        for (int p = lane; p < tc; p += 64) {
            a.anc[dst + p] = a.anc[src + p];
            a.tok[dst + p] = a.tok[src + p];
            a.lp[dst + p] = a.lp[src + p];
        }
        if (lane == 0) {
            if (t < a.pitch) {
                a.anc[dst + t] = row;   // the next step writes this row's K/V at position t
                a.tok[dst + t] = tk;
                a.lp[dst + t] = a.round_lp ? round_bf16(l) : l;
            }
            a.cum[row] = sc;
            a.finished[row] = fin;
            a.len[row] = ln;
        }
        if (t + 1 < a.Tmax)   // next step's input (see argmax_logprob_kernel)
            for (int i = lane * 4; i < a.E; i += 256) {
                const float4 ev = *reinterpret_cast<const float4 *>(a.emb + (size_t)tk * a.E + i), pv = *reinterpret_cast<const float4 *>(a.pos + (size_t)(t + 1) * a.E + i);
                *reinterpret_cast<float4 *>(a.x + (size_t)row * a.E + i) = make_float4(ev.x + pv.x, ev.y + pv.y, ev.z + pv.z, ev.w + pv.w);
            }
    }
}

// ---- grammar-constrained decoding (an extension: the reference knows no grammar) -------------------------------------------------------------
// The selection kernels above are left exactly as they are; the constrained forms below are their copies with three additions: the row's
// table row (grammar_row), the masked reductions (row_argmax_sumexp_masked / topk_draw_row_masked: a token the state forbids counts as a -inf
// logit) and the state update (grammar_advance).  With a table that allows every token each computes what its plain form computes, bit for
// bit: a masked term is expf(-inf) = 0 exactly and the order of every reduction is the plain one's.
struct GrammarArgs {   // AcaiGrammar as the kernels take it
    const int16_t *next, *resync;
    int32_t *state;
    int states, start;
};

// Wave-uniform: the table row of decode row b's state (clamped to [0, states)), or null when that state allows no token - the row is then
// unconstrained at this step (a defensive path: the builders refuse such tables).
__device__ __forceinline__ const int16_t *grammar_row(const GrammarArgs &g, int b, int V, int lane) {
    const int s = min(max(g.state[b], 0), g.states - 1);
    const int16_t *row = g.next + (size_t)s * V;
    bool any = false;
    for (int i = lane; i < V; i += 64) any |= row[i] >= 0;
    return __ballot(any) ? row : nullptr;
}

// The state after `tok` was emitted from the state of `row` (grammar_row's result): the table's, resync[tok] out of a dead state.  A token
// outside [0, V) (no finite logit in the row) leads to start, so that no index leaves the tables.
__device__ __forceinline__ int grammar_advance(const GrammarArgs &g, const int16_t *row, int tok, int V) {
    if ((unsigned)tok >= (unsigned)V) return g.start;
    return row ? row[tok] : g.resync[tok];
}

// row_argmax_sumexp over the tokens with allow[i] >= 0 (allow null: every token)
__device__ __forceinline__ float row_argmax_sumexp_masked(const float *lg, int V, int lane, float &best, int &bi, const int16_t *allow) {
    best = -INFINITY;
    bi = 0x7fffffff;
    for (int i = lane; i < V; i += 64) {
        const float v = (allow && allow[i] < 0) ? -INFINITY : lg[i];
        if (v > best) {
            best = v;
            bi = i;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > best || (ov == best && oi < bi)) {
            best = ov;
            bi = oi;
        }
    }
    float se = 0.f;
    for (int i = lane; i < V; i += 64) se += expf(((allow && allow[i] < 0) ? -INFINITY : lg[i]) - best);
    return wave_sum(se);
}

// topk_draw_row over the tokens with allow[i] >= 0 (allow null: every token): with fewer than top_k of them the kept set is the allowed set -
// the trailing rounds find none - and the rounding fallback of the draw is the last entry that holds a token.
__device__ __forceinline__ int topk_draw_row_masked(const float *lg, int V, int lane, float *sv, int *si, int top_k, float inv_temperature,
                                                    float u, float &lp, const int16_t *allow) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (lane + 64 * j < V && !(allow && allow[lane + 64 * j] < 0)) ? lg[lane + 64 * j] : -INFINITY;
    const int k = min(top_k, V);
    for (int r = 0; r < k; ++r) {
        float best = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (v[j] > best) {
                best = v[j];
                bi = lane + 64 * j;
            }
        if (best == -INFINITY) bi = 0x7fffffff;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o);
            const int oi = __shfl_xor(bi, o);
            if (ov > best || (ov == best && oi < bi)) {
                best = ov;
                bi = oi;
            }
        }
        if ((bi & 63) == lane) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (bi == lane + 64 * j) v[j] = -INFINITY;
        }
        if (lane == 0) {
            sv[r] = best;
            si[r] = bi;
        }
    }
    const bool in = lane < k;
    const float x = in ? sv[lane] : -INFINITY, m = sv[0];
    const float pT = in ? expf((x - m) * inv_temperature) : 0.f;
    const float p1 = in ? expf(x - m) : 0.f;
    const float sumT = wave_sum(pT), sum1 = wave_sum(p1);
    float cdf = pT;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(cdf, o);
        if (lane >= o) cdf += up;
    }
    const float target = u * sumT;
    const unsigned long long hit = __ballot(in && cdf > target);
    const int last = max(__popcll(__ballot(in && x > -INFINITY)), 1) - 1;
    const int r = hit ? __builtin_ctzll(hit) : last;
    lp = (sv[r] - m) - logf(sum1);
    return si[r];
}

// argmax_logprob_kernel (with its bookkeeping) under the automaton: logprobs holds the log-softmax over the allowed tokens
__global__ __launch_bounds__(1024) void grammar_argmax_kernel(const float *logits, int V, int B, int64_t *seqs, float *logprobs, int max_len,
                                                             int32_t *step, int32_t *finished, int eos, int round_lp, const float *emb,
                                                             const float *pos, float *x, int E, int Tmax, GrammarArgs g) {
    __shared__ int unfinished[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = step[0];
    int cnt = 0;
    const int nw = blockDim.x >> 6;
    for (int b = wave; b < B; b += nw) {
        const float *lg = logits + (size_t)b * V;
        float best;
        int bi;
        const int16_t *allow = grammar_row(g, b, V, lane);
        const float se = row_argmax_sumexp_masked(lg, V, lane, best, bi, allow);
        float lp = -logf(se);
        if (round_lp) lp = round_bf16(lp);
        int fin = finished[b];
        if (bi == eos) fin = 1;
        if (lane == 0) {
            seqs[(size_t)b * max_len + t] = bi;
            logprobs[(size_t)b * max_len + t] = lp;
            finished[b] = fin;
            g.state[b] = grammar_advance(g, allow, bi, V);
        }
        cnt += fin ? 0 : 1;
        if (emb && t + 1 < Tmax)
            for (int i = lane * 4; i < E; i += 256) {
                const float4 ev = *reinterpret_cast<const float4 *>(emb + (size_t)bi * E + i), pv = *reinterpret_cast<const float4 *>(pos + (size_t)(t + 1) * E + i);
                *reinterpret_cast<float4 *>(x + (size_t)b * E + i) = make_float4(ev.x + pv.x, ev.y + pv.y, ev.z + pv.z, ev.w + pv.w);
            }
    }
    if (lane == 0) unfinished[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < nw; ++w) tot += unfinished[w];
        finished[B] = tot;
        step[0] = t + 1;
        step[1] = step[1] + 1;
    }
}

// sample_logprob_kernel under the automaton
__global__ __launch_bounds__(256) void grammar_sample_kernel(const float *logits, int V, int B, int64_t *seqs, float *logprobs, int max_len,
                                                             const int32_t *step, int32_t *finished, int eos, int round_lp,
                                                             const float *uniforms, int top_k, float inv_temperature, const float *emb,
                                                             const float *pos, float *xnext, int E, int Tmax, GrammarArgs g) {
    __shared__ float sv[4][64];
    __shared__ int si[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + wave;
    if (b >= B) return;
    const int t = step[0];
    float lp;
    const int16_t *allow = grammar_row(g, b, V, lane);
    const int tok = topk_draw_row_masked(logits + (size_t)b * V, V, lane, sv[wave], si[wave], top_k, inv_temperature,
                                         uniforms[(size_t)b * max_len + t], lp, allow);
    if (round_lp) lp = round_bf16(lp);
    if (lane == 0) {
        seqs[(size_t)b * max_len + t] = tok;
        logprobs[(size_t)b * max_len + t] = lp;
        if (tok == eos) finished[b] = 1;
        g.state[b] = grammar_advance(g, allow, tok, V);
    }
    if (emb && t + 1 < Tmax)
        for (int i = lane * 4; i < E; i += 256) {
            const float4 ev = *reinterpret_cast<const float4 *>(emb + (size_t)tok * E + i), pv = *reinterpret_cast<const float4 *>(pos + (size_t)(t + 1) * E + i);
            *reinterpret_cast<float4 *>(xnext + (size_t)b * E + i) = make_float4(ev.x + pv.x, ev.y + pv.y, ev.z + pv.z, ev.w + pv.w);
        }
}

// slot_argmax_kernel under the automaton: a finished or idle row reads and writes no state
__global__ __launch_bounds__(1024) void slot_grammar_argmax_kernel(const float *logits, int V, int B, int64_t *seqs, float *logprobs, int max_len,
                                                                  int32_t *step, int32_t *finished, int32_t *slot_t, const int32_t *slot_cap,
                                                                  int eos, int round_lp, const float *emb, const float *pos, float *x, int E,
                                                                  int Tmax, GrammarArgs g) {
    __shared__ int unfinished[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int cnt = 0;
    const int nw = blockDim.x >> 6;
    for (int b = wave; b < B; b += nw) {
        if (finished[b]) continue;   // wave-uniform
        const int t = slot_t[b];
        const float *lg = logits + (size_t)b * V;
        float best;
        int bi;
        const int16_t *allow = grammar_row(g, b, V, lane);
        const float se = row_argmax_sumexp_masked(lg, V, lane, best, bi, allow);
        float lp = -logf(se);
        if (round_lp) lp = round_bf16(lp);
        const bool fin = bi == eos || t >= slot_cap[b] - 1;
        if (lane == 0) {
            seqs[(size_t)b * max_len + t] = bi;
            logprobs[(size_t)b * max_len + t] = lp;
            if (fin) finished[b] = 1;
            else slot_t[b] = t + 1;
            g.state[b] = grammar_advance(g, allow, bi, V);
        }
        if (!fin) {   // t + 1 <= cap - 1 < max_len <= Tmax
            cnt += 1;
            for (int i = lane * 4; i < E; i += 256) {
                const float4 ev = *reinterpret_cast<const float4 *>(emb + (size_t)bi * E + i), pv = *reinterpret_cast<const float4 *>(pos + (size_t)(t + 1) * E + i);
                *reinterpret_cast<float4 *>(x + (size_t)b * E + i) = make_float4(ev.x + pv.x, ev.y + pv.y, ev.z + pv.z, ev.w + pv.w);
            }
        }
    }
    if (lane == 0) unfinished[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < nw; ++w) tot += unfinished[w];
        finished[B] = tot;
        const int nxt = step[1] + 1;
        step[1] = nxt >= Tmax ? 0 : nxt;
    }
}

// slot_sample_kernel under the automaton (the same ticket hand-off closes the step)
__global__ __launch_bounds__(256) void slot_grammar_sample_kernel(const float *logits, int V, int B, int64_t *seqs, float *logprobs, int max_len,
                                                                  int32_t *step, int32_t *finished, int32_t *slot_t, const int32_t *slot_cap,
                                                                  int eos, int round_lp, const float *uniforms, int ld_uniforms,
                                                                  const int32_t *urow, int top_k, float inv_temperature, const float *emb,
                                                                  const float *pos, float *x, int E, int Tmax, unsigned *ticket, GrammarArgs g) {
    __shared__ float sv[4][64];
    __shared__ int si[4][64];
    __shared__ int is_last;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = blockIdx.x * 4 + wave; b < B; b += gridDim.x * 4) {
        if (finished[b]) continue;   // wave-uniform
        const int t = slot_t[b];
        float lp;
        const int16_t *allow = grammar_row(g, b, V, lane);
        const int tok = topk_draw_row_masked(logits + (size_t)b * V, V, lane, sv[wave], si[wave], top_k, inv_temperature,
                                             uniforms[(size_t)urow[b] * ld_uniforms + t], lp, allow);
        if (round_lp) lp = round_bf16(lp);
        const bool fin = tok == eos || t >= slot_cap[b] - 1;
        if (lane == 0) {
            seqs[(size_t)b * max_len + t] = tok;
            logprobs[(size_t)b * max_len + t] = lp;
            if (fin) __hip_atomic_store(finished + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else slot_t[b] = t + 1;
            g.state[b] = grammar_advance(g, allow, tok, V);
        }
        if (!fin)
            for (int i = lane * 4; i < E; i += 256) {
                const float4 ev = *reinterpret_cast<const float4 *>(emb + (size_t)tok * E + i), pv = *reinterpret_cast<const float4 *>(pos + (size_t)(t + 1) * E + i);
                *reinterpret_cast<float4 *>(x + (size_t)b * E + i) = make_float4(ev.x + pv.x, ev.y + pv.y, ev.z + pv.z, ev.w + pv.w);
            }
    }
    if (gridDim.x > 1) {
        __threadfence();
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned n = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            is_last = n == gridDim.x - 1;
            if (is_last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    if (gridDim.x > 1 && !is_last) return;
    if (wave == 0) {
        int cnt = 0;
        for (int b = lane; b < B; b += 64) cnt += __hip_atomic_load(finished + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 0 : 1;
        cnt = (int)wave_sum((float)cnt);
        if (lane == 0) {
            finished[B] = cnt;
            const int nxt = step[1] + 1;
            step[1] = nxt >= Tmax ? 0 : nxt;
        }
    }
}

}  // namespace

static int round_lp(const AcaiDecoder *d) { return (d->flags & ACAI_GEMM_ROUND_BF16) ? 1 : 0; }
// one workgroup closes the step, one wave per row for the usual batch sizes
static dim3 row_waves(const AcaiDecoder *d) { return dim3(d->B > 8 ? 1024 : (d->B > 4 ? 512 : 256)); }

int launch_embed(const AcaiDecoder *d, const int64_t *tokens, hipStream_t st) {
    hipLaunchKernelGGL(embed_kernel, dim3(d->B), dim3(256), 0, st, (const float *)d->emb, (const float *)d->pos, tokens, (const int64_t *)d->seqs,
                       (const int32_t *)d->step, d->max_len, d->x, d->E);
    ACAI_LAUNCH_CHECK("embed");
    return 0;
}

int launch_set_step(const AcaiDecoder *d, int t, hipStream_t st) {
    hipLaunchKernelGGL(set_step_kernel, dim3(1), dim3(1), 0, st, d->step, t);
    ACAI_LAUNCH_CHECK("set_step");
    return 0;
}

int launch_advance_cache(const AcaiDecoder *d, hipStream_t st) {
    hipLaunchKernelGGL(advance_cache_kernel, dim3(1), dim3(1), 0, st, d->step);
    ACAI_LAUNCH_CHECK("advance_cache");
    return 0;
}

// `chained`: the kernel also writes the next step's input x
int launch_argmax_logprob(const AcaiDecoder *d, bool chained, hipStream_t st) {
    hipLaunchKernelGGL(argmax_logprob_kernel, dim3(1), row_waves(d), 0, st, d->logits, d->V, d->B, d->seqs, d->logprobs, d->max_len, d->step,
                       d->finished, d->eos, round_lp(d), 1, chained ? (const float *)d->emb : nullptr, (const float *)d->pos, d->x, d->E, d->Tmax);
    ACAI_LAUNCH_CHECK("argmax_logprob");
    return 0;
}

static GrammarArgs grammar_args(const AcaiGrammar *gr) { return GrammarArgs{gr->next, gr->resync, gr->state, gr->states, gr->start}; }

// the grammar-constrained forms of launch_argmax_logprob / launch_sample_logprob / launch_slot_argmax / launch_slot_sample
int launch_grammar_argmax(const AcaiDecoder *d, const AcaiGrammar *gr, bool chained, hipStream_t st) {
    hipLaunchKernelGGL(grammar_argmax_kernel, dim3(1), row_waves(d), 0, st, d->logits, d->V, d->B, d->seqs, d->logprobs, d->max_len, d->step,
                       d->finished, d->eos, round_lp(d), chained ? (const float *)d->emb : nullptr, (const float *)d->pos, d->x, d->E, d->Tmax,
                       grammar_args(gr));
    ACAI_LAUNCH_CHECK("grammar_argmax");
    return 0;
}

int launch_grammar_sample(const AcaiDecoder *d, const AcaiGrammar *gr, const float *uniforms, int top_k, float temperature, bool chained,
                          hipStream_t st) {
    hipLaunchKernelGGL(grammar_sample_kernel, dim3(cdiv(d->B, 4)), dim3(256), 0, st, d->logits, d->V, d->B, d->seqs, d->logprobs, d->max_len,
                       d->step, d->finished, d->eos, round_lp(d), uniforms, top_k, 1.0f / temperature,
                       chained ? (const float *)d->emb : nullptr, (const float *)d->pos, d->x, d->E, d->Tmax, grammar_args(gr));
    hipLaunchKernelGGL(sample_bookkeeping_kernel, dim3(1), dim3(64), 0, st, d->B, d->step, d->finished);
    ACAI_LAUNCH_CHECK("grammar_sample");
    return 0;
}

int launch_slot_grammar_argmax(const AcaiDecoder *d, const AcaiSlots *sl, const AcaiGrammar *gr, hipStream_t st) {
    hipLaunchKernelGGL(slot_grammar_argmax_kernel, dim3(1), row_waves(d), 0, st, d->logits, d->V, d->B, d->seqs, d->logprobs, d->max_len, d->step,
                       d->finished, sl->t, (const int32_t *)sl->cap, d->eos, round_lp(d), (const float *)d->emb, (const float *)d->pos, d->x,
                       d->E, d->Tmax, grammar_args(gr));
    ACAI_LAUNCH_CHECK("slot_grammar_argmax");
    return 0;
}

int launch_slot_grammar_sample(const AcaiDecoder *d, const AcaiSlots *sl, const AcaiGrammar *gr, const float *uniforms, int ld_uniforms,
                               const int32_t *urow, int top_k, float temperature, hipStream_t st) {
    hipLaunchKernelGGL(slot_grammar_sample_kernel, dim3(d->tickets ? cdiv(d->B, 4) : 1), dim3(256), 0, st, d->logits, d->V, d->B, d->seqs,
                       d->logprobs, d->max_len, d->step, d->finished, sl->t, (const int32_t *)sl->cap, d->eos, round_lp(d), uniforms,
                       ld_uniforms, urow, top_k, 1.0f / temperature, (const float *)d->emb, (const float *)d->pos, d->x, d->E, d->Tmax,
                       (unsigned *)d->tickets, grammar_args(gr));
    ACAI_LAUNCH_CHECK("slot_grammar_sample");
    return 0;
}

// the prompted form of launch_argmax_logprob
int launch_prompt_logprob(const AcaiDecoder *d, const AcaiPrompt *pr, bool chained, hipStream_t st) {
    hipLaunchKernelGGL(prompt_logprob_kernel, dim3(1), row_waves(d), 0, st, d->logits, d->V, d->B, d->seqs, d->logprobs, d->max_len, d->step,
                       d->finished, d->eos, round_lp(d), pr->tok, pr->len, pr->pitch, chained ? (const float *)d->emb : nullptr,
                       (const float *)d->pos, d->x, d->E, d->Tmax);
    ACAI_LAUNCH_CHECK("prompt_logprob");
    return 0;
}

// the sampling kernel, then the loop bookkeeping
int launch_sample_logprob(const AcaiDecoder *d, const float *uniforms, int top_k, float temperature, bool chained, hipStream_t st) {
    hipLaunchKernelGGL(sample_logprob_kernel, dim3(cdiv(d->B, 4)), dim3(256), 0, st, d->logits, d->V, d->B, d->seqs, d->logprobs, d->max_len, d->step,
                       d->finished, d->eos, round_lp(d), uniforms, top_k, 1.0f / temperature,
                       chained ? (const float *)d->emb : nullptr, (const float *)d->pos, d->x, d->E, d->Tmax);
    hipLaunchKernelGGL(sample_bookkeeping_kernel, dim3(1), dim3(64), 0, st, d->B, d->step, d->finished);
    ACAI_LAUNCH_CHECK("sample_logprob");
    return 0;
}

// the beam selection, then the loop bookkeeping
int launch_beam_select(const AcaiDecoder *d, const AcaiBeam *bs, hipStream_t st) {
    BeamArgs a{};
    a.logits = d->logits; a.V = d->V; a.K = bs->K; a.E = d->E; a.Tmax = d->Tmax; a.pitch = bs->pitch; a.eos = d->eos; a.pad = d->pad;
    a.round_lp = round_lp(d);
    a.step = d->step; a.finished = d->finished; a.emb = d->emb; a.pos = d->pos; a.x = d->x;
    a.anc = bs->anc; a.tok = bs->tok; a.lp = bs->lp; a.bstride = (long long)bs->rows * bs->pitch; a.cum = bs->cum; a.len = bs->len;
    hipLaunchKernelGGL(beam_select_kernel, dim3(d->B / bs->K), dim3(256), 0, st, a);
    ACAI_LAUNCH_CHECK("beam_select");
    hipLaunchKernelGGL(sample_bookkeeping_kernel, dim3(1), dim3(64), 0, st, d->B, d->step, d->finished);
    ACAI_LAUNCH_CHECK("beam_bookkeeping");
    return 0;
}

int launch_slot_arm(const AcaiDecoder *d, const AcaiSlots *sl, const int32_t *rows, int n, hipStream_t st) {
    hipLaunchKernelGGL(slot_arm_kernel, dim3(n), dim3(256), 0, st, rows, n, d->B, d->max_len, d->seqs, d->logprobs,
                       d->finished, sl->t, sl->first, sl->cap, (const int32_t *)d->step, d->bos, d->pad,
                       (const float *)d->emb, (const float *)d->pos, d->x, d->E);
    ACAI_LAUNCH_CHECK("slot_arm");
    return 0;
}

int launch_slot_argmax(const AcaiDecoder *d, const AcaiSlots *sl, hipStream_t st) {
    hipLaunchKernelGGL(slot_argmax_kernel, dim3(1), row_waves(d), 0, st, d->logits, d->V, d->B, d->seqs,
                       d->logprobs, d->max_len, d->step, d->finished, sl->t, (const int32_t *)sl->cap, d->eos,
                       round_lp(d), (const float *)d->emb, (const float *)d->pos, d->x, d->E, d->Tmax);
    ACAI_LAUNCH_CHECK("slot_argmax");
    return 0;
}

int launch_slot_sample(const AcaiDecoder *d, const AcaiSlots *sl, const float *uniforms, int ld_uniforms, const int32_t *urow, int top_k,
                       float temperature, hipStream_t st) {
    // one wave per row; without arrival counters (d->tickets) one workgroup takes every row and closes the step itself
    hipLaunchKernelGGL(slot_sample_kernel, dim3(d->tickets ? cdiv(d->B, 4) : 1), dim3(256), 0, st, d->logits, d->V, d->B, d->seqs, d->logprobs,
                       d->max_len, d->step, d->finished, sl->t, (const int32_t *)sl->cap, d->eos, round_lp(d),
                       uniforms, ld_uniforms, urow, top_k, 1.0f / temperature, (const float *)d->emb, (const float *)d->pos, d->x, d->E, d->Tmax,
                       (unsigned *)d->tickets);
    ACAI_LAUNCH_CHECK("slot_sample");
    return 0;
}

// arm != 0 opens a run (no logits are read), arm == 0 closes a verify step
int launch_spec_accept(const AcaiDecoder *d, const AcaiSpec *sp, int arm, hipStream_t st) {
    SpecArgs a{};
    a.logits = d->logits; a.V = d->V; a.B = d->B; a.R = sp->D + 1; a.E = d->E; a.Tmax = d->Tmax; a.ld = d->max_len; a.eos = d->eos; a.pad = d->pad;
    a.round_lp = round_lp(d); a.ngram = sp->ngram; a.arm = arm; a.pitch = sp->pitch;
    a.seqs = d->seqs; a.logprobs = d->logprobs; a.step = d->step; a.finished = d->finished; a.emb = d->emb; a.pos = d->pos; a.x = d->x;
    a.t = sp->t; a.steps = sp->steps; a.tab = sp->tab; a.next = sp->next; a.cap = sp->cap; a.drafts = sp->drafts;
    hipLaunchKernelGGL(spec_accept_kernel<SpecArgs>, dim3(1), row_waves(d), sizeof(int) * 2 * (size_t)d->B, st, a);
    ACAI_LAUNCH_CHECK("spec_accept");
    return 0;
}

// launch_spec_accept with the prompt tables
int launch_spec_prompt_accept(const AcaiDecoder *d, const AcaiSpec *sp, const AcaiPrompt *pr, int arm, hipStream_t st) {
    SpecPromptArgs a{};
    a.logits = d->logits; a.V = d->V; a.B = d->B; a.R = sp->D + 1; a.E = d->E; a.Tmax = d->Tmax; a.ld = d->max_len; a.eos = d->eos; a.pad = d->pad;
    a.round_lp = round_lp(d); a.ngram = sp->ngram; a.arm = arm; a.pitch = sp->pitch;
    a.seqs = d->seqs; a.logprobs = d->logprobs; a.step = d->step; a.finished = d->finished; a.emb = d->emb; a.pos = d->pos; a.x = d->x;
    a.t = sp->t; a.steps = sp->steps; a.tab = sp->tab; a.next = sp->next; a.cap = sp->cap; a.drafts = sp->drafts;
    a.ptok = pr->tok; a.plen = pr->len; a.ppitch = pr->pitch;
    hipLaunchKernelGGL(spec_accept_kernel<SpecPromptArgs>, dim3(1), row_waves(d), sizeof(int) * 2 * (size_t)d->B, st, a);
    ACAI_LAUNCH_CHECK("spec_prompt_accept");
    return 0;
}

// (declared and documented in acai_omr_hip.h; it takes the slot state as bare pointers, not through the decoder descriptor, so that it can
// be driven over any rows laid out as the slot steps lay them out)
extern "C" int acai_decode_slot_flush(const int64_t *seqs, const float *logprobs, int max_len, const int32_t *slot_t, const int32_t *finished,
                                      int32_t *mark, int rows, int B, int ld, int32_t *out_tok, float *out_lp, int32_t *hdr, void *stream) {
    ACAI_CHECK_ARG(seqs && logprobs && slot_t && finished && mark && out_tok && out_lp && hdr, "acai_decode_slot_flush: null operand");
    ACAI_CHECK_ARG(B >= 1 && rows >= B, "acai_decode_slot_flush: %d slots over state of %d rows (needs 1 <= B <= rows)", B, rows);
    ACAI_CHECK_ARG(max_len >= 1 && ld >= 1 && ld <= max_len, "acai_decode_slot_flush: ld %d outside [1, max_len = %d]", ld, max_len);
    hipLaunchKernelGGL(slot_flush_kernel, dim3(cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, seqs, logprobs, max_len, slot_t, finished, mark,
                       B, ld, out_tok, out_lp, hdr);
    ACAI_LAUNCH_CHECK("slot_flush");
    return 0;
}

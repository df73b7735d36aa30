// Token selection of a decode step (see decode.hip): embedding, greedy / sampled / slot / speculative / beam / grammar-constrained selection and their
// bookkeeping, each with the host helper that launches it from the decoder descriptor.
#include "decode_internal.h"

#include <type_traits>

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

// The NEXT step's input of row b, written by the wave that chose its token: x[b] = vocab_embedding[tok] + pos_embedding[t1], 16 bytes a lane
// (E % 4 == 0).  Quirk Q1: the token at index t is embedded with position t1 = t + 1 (M:576).  With it a token step needs no embed launch.
__device__ __forceinline__ void write_next_input(const float *emb, const float *pos, float *x, int E, int b, int tok, int t1, int lane) {
    for (int i = lane * 4; i < E; i += 256) {
        const float4 ev = *reinterpret_cast<const float4 *>(emb + (size_t)tok * E + i), pv = *reinterpret_cast<const float4 *>(pos + (size_t)t1 * E + i);
        *reinterpret_cast<float4 *>(x + (size_t)b * E + i) = make_float4(ev.x + pv.x, ev.y + pv.y, ev.z + pv.z, ev.w + pv.w);
    }
}

// GRPOViTOMR.cached_forward_rollout_policy (M:988-1049), one sampling step: top-k filter, softmax with temperature over the kept logits,
// draw from that distribution, log-prob of the drawn token under the UN-tempered softmax of the kept logits (the reference takes
// log_softmax(top_k_logits), M:1017).  torch.multinomial's Philox stream is not reproducible here; the draw is the inverse CDF of a caller
// supplied uniform u[b][t] over the kept logits in descending order (ties: lower vocabulary index first), so a step is a pure function of
// (logits, u) that the oracle restates.  One wave per row: k rounds of a wave-wide arg-max build the sorted top-k (k <= 64).
// The per-row part, shared by the static and the slot sampler so that a sequence draws the same tokens in either: wave-wide, `sv` / `si` are
// the wave's own 64 LDS entries.  Returns the drawn token; lp = log_softmax(kept)[drawn] (not rounded).
// MASKED (grammar-constrained selection): only over the tokens with allow[i] >= 0 (allow null: every token).  With fewer than top_k of them
// the kept set is the allowed set - the trailing rounds find none - and the rounding fallback of the draw is the last entry that holds a token.
template <bool MASKED = false>
__device__ __forceinline__ int topk_draw_row(const float *lg, int V, int lane, float *sv, int *si, int top_k, float inv_temperature, float u,
                                             float &lp, const int16_t *allow = nullptr) {
    // lane owns vocabulary entries lane, lane + 64, ... (V <= 512)
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        bool keep = lane + 64 * j < V;
        if constexpr (MASKED) keep = keep && !(allow && allow[lane + 64 * j] < 0);
        v[j] = keep ? lg[lane + 64 * j] : -INFINITY;
    }
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
    // MASKED: the entries past the allowed set hold no token and take no part in the draw.  Their prefix sums add zeros to the last real
    // entry's, but in another order of additions (the scan pairs differently per lane), so one of them can exceed a target near the top of
    // the CDF that the last real entry's own prefix does not: it must not be hit, and the rounding fallback is not k - 1.
    // (Unmasked, every one of the k entries holds a token.  Where the tail's expf underflows to 0 - a low temperature - the same rounding, or
    // the fallback k - 1, can draw a tail entry of fp32 probability 0 at a u within an ulp or so of 1: a valid kept token, accepted.)
    bool live = in;
    if constexpr (MASKED) live = in && x > -INFINITY;
    const unsigned long long hit = __ballot(live && cdf > target);
    int last = k - 1;                                              // rounding at the top of the CDF: last kept entry
    if constexpr (MASKED) last = max(__popcll(__ballot(live)), 1) - 1;
    const int r = hit ? __builtin_ctzll(hit) : last;
    lp = (sv[r] - m) - logf(sum1);
    return si[r];
}

// ---- the selection of a step: greedy_select_kernel / sample_select_kernel ---------------------------------------------------------------
// Each is ONE template over what a step may add to plain selection, and a feature is an `if constexpr` branch with an argument struct of its
// own, so that an instantiation without it compiles without it and loads nothing for it (NoArgs in the struct's place):
//   SLOT    continuous batching (an extension: the reference decodes one static batch).  A row runs at its OWN local time t = slot_t[b] instead
//           of step[0]; a finished or idle row is skipped and writes nothing; a row finishes on <eos> or when t has reached its cap - 1, else t
//           advances; the step closes by advancing the shared ring write index step[1] modulo Tmax (step[0] is not used in slot mode).
//   GRAMMAR grammar-constrained decoding (an extension: the reference knows no grammar).  The row's table row (grammar_row) masks the reduction
//           - a token the state forbids counts as a -inf logit, so logprobs holds the log-softmax over the allowed tokens - and the state is
//           updated (grammar_advance).  With a table that allows every token the step computes what the plain one computes, bit for bit.
//   PROMPT  prompted decoding (an extension: the reference starts every sequence from <bos> alone; greedy only, without SLOT or GRAMMAR).  The
//           token at index t <= len[b] is the prompt's (prompt_len / prompt_token, the clamped reads of the prompt tables, are in common.h).
//   LOOP    the loop guard (an extension: the reference lets a row repeat itself up to its cap; without GRAMMAR or PROMPT).  The wave that
//           chose the row's token also keeps, in lane p - 1, the length run[b][p - 1] of the run of indices i ending at t with
//           seq[i] == seq[i - p] (loop_check); the row ends at the first t where a period's run reaches need(p) = max((R - 1) p, M), the
//           way a cap ends it.  With a guard that cannot fire the step computes what the plain one computes, bit for bit.
// Only the combinations an entry point launches are instantiated.
struct SelArgs {   // what every form takes, from AcaiDecoder
    const float *logits;
    int V, B, max_len, eos, round_lp, E, Tmax;
    int64_t *seqs;
    float *logprobs;
    int32_t *step, *finished;
    const float *emb, *pos;   // emb null (static forms only): the kernel does not write the next step's input
    float *x;
};
struct NoArgs {};
struct SlotArgs {   // AcaiSlots
    int32_t *t;
    const int32_t *cap;
};
struct PromptArgs {   // AcaiPrompt
    const int32_t *tok, *len;
    int pitch;
};
struct GrammarArgs {   // AcaiGrammar
    const int16_t *next, *resync;
    int32_t *state;
    int states, start;
};
struct DrawArgs {   // a sampling step's draw: row b at time t takes uniforms[(SLOT ? urow[b] : b) * ld + t]
    const float *uniforms;
    int ld;
    const int32_t *urow;   // SLOT: the sequence each slot decodes (set when the slot is armed), so that a sequence draws what it draws alone
    int top_k;
    float inv_temperature;
    unsigned *ticket;      // SLOT with more than one workgroup: the arrival counter (zero between launches)
};
struct LoopArgs {   // AcaiLoop; R and M clamped to max_len + 1 by loop_args (a need above max_len never fires), so need(p) fits an int
    int32_t *run, *stop, *period, *start;
    int P, R, M;
};
template <bool ON, typename T> using part = std::conditional_t<ON, T, NoArgs>;

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

// The loop guard's part of a step, for the wave that chose `tok` for index t of row b (wave-uniform result): lane p - 1 compares the token
// p indices back (one coalesced read of the row; only indices >= 1 take part, index 0 is <bos>) with the token in its register and counts
// its run, +1 on a match, 0 otherwise - lanes past P and indices before 1 + p hold 0.  The verdict is one ballot over run >= need(p); the
// lowest set bit is the smallest period.  Returns that period, or 0; an <eos> never counts as a loop stop (the row ends on it as it does
// without a guard).  On a hit lane 0 writes the report: stop = t, the period, and start = t - need(p) - p + 1, the first index of the
// periodic stretch.  O(1) a step: the row is not scanned again.
__device__ __forceinline__ int loop_check(const LoopArgs &l, const int64_t *row, int b, int t, int tok, int eos, int lane) {
    const int p = lane + 1;
    const bool cmp = p <= l.P && t - p >= 1;
    const int64_t prev = cmp ? row[t - p] : -1;
    int32_t *run = l.run + (size_t)b * 64 + lane;
    const int r = (cmp && prev == (int64_t)tok) ? *run + 1 : 0;
    *run = r;
    const int need = max((l.R - 1) * p, l.M);
    const unsigned long long hit = __ballot(p <= l.P && r >= need);
    if (!hit || tok == eos) return 0;
    const int per = __builtin_ctzll(hit) + 1;
    if (lane == 0) {
        l.stop[b] = t;
        l.period[b] = per;
        l.start[b] = t - max((l.R - 1) * per, l.M) - per + 1;
    }
    return per;
}

// slot mode: the shared ring write index after a step
__device__ __forceinline__ void advance_ring(int32_t *step, int Tmax) {
    const int nxt = step[1] + 1;
    step[1] = nxt >= Tmax ? 0 : nxt;
}

// cached_get_next_token (M:579-581) + loop bookkeeping (M:606-611).  One workgroup, wave w takes rows w, w + nw, ... (up to 16 waves: one row
// per wave for the usual batch sizes, the rows of a wave run back to back): the arg-max token and its log-prob into seqs / logprobs at index
// t, the finished flag, the row's next input (write_next_input), then thread 0 publishes the unfinished count finished[B] and advances the
// step.  PROMPT: the log-prob of token k is -(logf(se) - (logit[k] - max)); for the arg-max the inner difference is exactly 0 and the value is
// the plain form's -logf(se) bit for bit (beam_select_kernel's form).  A row inside its prompt (t < len[b]) counts as unfinished.
// LOOP: a row that is already finished is not examined and its counters stand; a row the guard stops is finished from this step on.
template <bool SLOT, bool GRAMMAR, bool PROMPT, bool LOOP = false>
__global__ __launch_bounds__(1024) void greedy_select_kernel(SelArgs a, part<SLOT, SlotArgs> s, part<GRAMMAR, GrammarArgs> g,
                                                            part<PROMPT, PromptArgs> p, part<LOOP, LoopArgs> l) {
    __shared__ int unfinished[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int t = 0, cnt = 0;
    if constexpr (!SLOT) t = a.step[0];
    for (int b = wave; b < a.B; b += nw) {
        if constexpr (SLOT) {
            if (a.finished[b]) continue;   // wave-uniform
            t = s.t[b];
        }
        const float *lg = a.logits + (size_t)b * a.V;
        const int16_t *allow = nullptr;
        if constexpr (GRAMMAR) allow = grammar_row(g, b, a.V, lane);
        float best;
        int tok;
        const float se = row_argmax_sumexp<GRAMMAR>(lg, a.V, lane, best, tok, allow);
        float lp = -logf(se);  // logit[argmax] - logsumexp
        bool in_prompt = false;
        if constexpr (PROMPT) {
            const int P = prompt_len(p.len, b, p.pitch, a.max_len);
            const int forced = prompt_token(p.tok, b, p.pitch, t, P, a.V);
            if (forced >= 0) tok = forced;
            lp = -(logf(se) - (lg[tok] - best));
            in_prompt = t < P;
        }
        if (a.round_lp) lp = round_bf16(lp);
        int fin;
        if constexpr (SLOT) {
            fin = tok == a.eos || t >= s.cap[b] - 1;
        } else {
            fin = a.finished[b];
            if constexpr (LOOP) {
                if (!fin && loop_check(l, a.seqs + (size_t)b * a.max_len, b, t, tok, a.eos, lane)) fin = 1;   // wave-uniform
            }
            if (tok == a.eos) fin = 1;
        }
        if constexpr (SLOT && LOOP) {
            if (loop_check(l, a.seqs + (size_t)b * a.max_len, b, t, tok, a.eos, lane)) fin = 1;
        }
        if (lane == 0) {
            a.seqs[(size_t)b * a.max_len + t] = tok;
            a.logprobs[(size_t)b * a.max_len + t] = lp;
            if constexpr (SLOT) {
                if (fin) a.finished[b] = 1;
                else s.t[b] = t + 1;
            } else {
                a.finished[b] = fin;
            }
            if constexpr (GRAMMAR) g.state[b] = grammar_advance(g, allow, tok, a.V);
        }
        cnt += (fin && !in_prompt) ? 0 : 1;
        // SLOT: an unfinished row has t + 1 <= cap - 1 < max_len <= Tmax, and a slot step is always chained
        if (SLOT ? !fin : (a.emb && t + 1 < a.Tmax)) write_next_input(a.emb, a.pos, a.x, a.E, b, tok, t + 1, lane);
    }
    if (lane == 0) unfinished[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < nw; ++w) tot += unfinished[w];
        a.finished[a.B] = tot;
        if constexpr (SLOT) {
            advance_ring(a.step, a.Tmax);
        } else {
            a.step[0] = t + 1;
            a.step[1] = a.step[1] + 1;
        }
    }
}

// The sampling step: the token of row b is topk_draw_row's.  One wave per row over gridDim.x workgroups of four (the k rounds of a row are a
// serial chain: one workgroup for every row would put them end to end).  A static step is followed by sample_bookkeeping_kernel.  A slot
// step closes itself: with more than one workgroup the unfinished count and the ring index are written by the workgroup that arrives last
// at `ticket` (zero between launches, re-armed here) - every workgroup publishes its rows' flags with agent-scope atomic stores before it
// takes its ticket, and the last one reads all flags the same way.
template <bool SLOT, bool GRAMMAR>
__global__ __launch_bounds__(256) void sample_select_kernel(SelArgs a, DrawArgs d, part<SLOT, SlotArgs> s, part<GRAMMAR, GrammarArgs> g) {
    __shared__ float sv[4][64];
    __shared__ int si[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const auto select_row = [&](int b) {
        int t, urow = b;
        if constexpr (SLOT) {
            if (a.finished[b]) return;   // wave-uniform
            t = s.t[b];
            urow = d.urow[b];
        } else {
            t = a.step[0];
        }
        const int16_t *allow = nullptr;
        if constexpr (GRAMMAR) allow = grammar_row(g, b, a.V, lane);
        float lp;
        const int tok = topk_draw_row<GRAMMAR>(a.logits + (size_t)b * a.V, a.V, lane, sv[wave], si[wave], d.top_k, d.inv_temperature,
                                               d.uniforms[(size_t)urow * d.ld + t], lp, allow);
        if (a.round_lp) lp = round_bf16(lp);
        bool fin = tok == a.eos;
        if constexpr (SLOT) fin = fin || t >= s.cap[b] - 1;
        if (lane == 0) {
            a.seqs[(size_t)b * a.max_len + t] = tok;
            a.logprobs[(size_t)b * a.max_len + t] = lp;
            if constexpr (SLOT) {
                if (fin) __hip_atomic_store(a.finished + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else s.t[b] = t + 1;
            } else {
                if (fin) a.finished[b] = 1;
            }
            if constexpr (GRAMMAR) g.state[b] = grammar_advance(g, allow, tok, a.V);
        }
        if (SLOT ? !fin : (a.emb && t + 1 < a.Tmax)) write_next_input(a.emb, a.pos, a.x, a.E, b, tok, t + 1, lane);
    };
    const int b0 = blockIdx.x * 4 + wave;
    if constexpr (!SLOT) {   // a wave for every row: no row loop - with it the static draw took 2 us longer
        if (b0 < a.B) select_row(b0);
    } else {
        for (int b = b0; b < a.B; b += gridDim.x * 4) select_row(b);
        __shared__ int is_last;
        if (gridDim.x > 1) {
            __threadfence();   // this thread's flag stores are visible device-wide before the workgroup's ticket
            __syncthreads();
            if (threadIdx.x == 0) {
                const unsigned n = __hip_atomic_fetch_add(d.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
                is_last = n == gridDim.x - 1;
                if (is_last) __hip_atomic_store(d.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();
        if (gridDim.x > 1 && !is_last) return;
        if (wave == 0) {
            int cnt = 0;
            for (int b = lane; b < a.B; b += 64) cnt += __hip_atomic_load(a.finished + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 0 : 1;
            cnt = (int)wave_sum((float)cnt);
            if (lane == 0) {
                a.finished[a.B] = cnt;
                advance_ring(a.step, a.Tmax);
            }
        }
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
//   1. wave w: the greedy token and log-prob of rows w, w + nw, ... (greedy_select_kernel's reduction) into LDS;
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
// while t + j <= len[i], with greedy_select_kernel's PROMPT log-prob, and while the new t <= len[i] the next step's drafts are the prompt's tokens
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
//      index first on ties, topk_draw_row's pattern), score cum + lp with greedy's row max / sum of exponentials; a finished row the
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
        if (t + 1 < a.Tmax) write_next_input(a.emb, a.pos, a.x, a.E, row, tk, t + 1, lane);
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

// ---- the selection launches: the kernels' argument structs from the descriptors, once ---------------------------------------------------
// `chained`: the kernel also writes the next step's input x (a slot step always does)
static SelArgs select_args(const AcaiDecoder *d, bool chained) {
    return SelArgs{d->logits, d->V, d->B, d->max_len, d->eos, round_lp(d), d->E, d->Tmax, d->seqs, d->logprobs, d->step, d->finished,
                   chained ? d->emb : nullptr, d->pos, d->x};
}
static SlotArgs slot_args(const AcaiSlots *sl) { return SlotArgs{sl->t, sl->cap}; }
static PromptArgs prompt_args(const AcaiPrompt *pr) { return PromptArgs{pr->tok, pr->len, pr->pitch}; }
static GrammarArgs grammar_args(const AcaiGrammar *gr) { return GrammarArgs{gr->next, gr->resync, gr->state, gr->states, gr->start}; }
// a static step draws row b's uniforms[b][t] (pitch max_len); a slot step uniforms[urow[b]][t]
static DrawArgs draw_args(const AcaiDecoder *d, const float *uniforms, int ld, const int32_t *urow, int top_k, float temperature) {
    return DrawArgs{uniforms, ld, urow, top_k, 1.0f / temperature, (unsigned *)d->tickets};
}

static LoopArgs loop_args(const AcaiDecoder *d, const AcaiLoop *lp) {
    const int top = d->max_len + 1;
    return LoopArgs{lp->run, lp->stop, lp->period, lp->start, lp->max_period, min(lp->min_repeats, top), min(lp->min_tokens, top)};
}

template <bool SLOT, bool GRAMMAR, bool PROMPT, bool LOOP = false>
static int launch_greedy(const AcaiDecoder *d, bool chained, part<SLOT, SlotArgs> s, part<GRAMMAR, GrammarArgs> g, part<PROMPT, PromptArgs> p,
                         const char *name, hipStream_t st, part<LOOP, LoopArgs> l = {}) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(greedy_select_kernel<SLOT, GRAMMAR, PROMPT, LOOP>), dim3(1), row_waves(d), 0, st, select_args(d, chained), s, g,
                       p, l);
    ACAI_LAUNCH_CHECK(name);
    return 0;
}

// One wave per row.  A static step is followed by the loop bookkeeping; a slot step without arrival counters (d->tickets) is one workgroup
// that takes every row and closes the step itself.
template <bool SLOT, bool GRAMMAR>
static int launch_sample(const AcaiDecoder *d, bool chained, DrawArgs w, part<SLOT, SlotArgs> s, part<GRAMMAR, GrammarArgs> g, const char *name,
                         hipStream_t st) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(sample_select_kernel<SLOT, GRAMMAR>), dim3(SLOT && !d->tickets ? 1 : cdiv(d->B, 4)), dim3(256), 0, st,
                       select_args(d, chained), w, s, g);
    if (!SLOT) hipLaunchKernelGGL(sample_bookkeeping_kernel, dim3(1), dim3(64), 0, st, d->B, d->step, d->finished);
    ACAI_LAUNCH_CHECK(name);
    return 0;
}

int launch_argmax_logprob(const AcaiDecoder *d, bool chained, hipStream_t st) {
    return launch_greedy<false, false, false>(d, chained, {}, {}, {}, "argmax_logprob", st);
}
int launch_prompt_logprob(const AcaiDecoder *d, const AcaiPrompt *pr, bool chained, hipStream_t st) {
    return launch_greedy<false, false, true>(d, chained, {}, {}, prompt_args(pr), "prompt_logprob", st);
}
int launch_grammar_argmax(const AcaiDecoder *d, const AcaiGrammar *gr, bool chained, hipStream_t st) {
    return launch_greedy<false, true, false>(d, chained, {}, grammar_args(gr), {}, "grammar_argmax", st);
}
int launch_slot_argmax(const AcaiDecoder *d, const AcaiSlots *sl, hipStream_t st) {
    return launch_greedy<true, false, false>(d, true, slot_args(sl), {}, {}, "slot_argmax", st);
}
int launch_slot_grammar_argmax(const AcaiDecoder *d, const AcaiSlots *sl, const AcaiGrammar *gr, hipStream_t st) {
    return launch_greedy<true, true, false>(d, true, slot_args(sl), grammar_args(gr), {}, "slot_grammar_argmax", st);
}
int launch_loop_argmax(const AcaiDecoder *d, const AcaiLoop *lp, bool chained, hipStream_t st) {
    return launch_greedy<false, false, false, true>(d, chained, {}, {}, {}, "loop_argmax", st, loop_args(d, lp));
}
int launch_slot_loop_argmax(const AcaiDecoder *d, const AcaiSlots *sl, const AcaiLoop *lp, hipStream_t st) {
    return launch_greedy<true, false, false, true>(d, true, slot_args(sl), {}, {}, "slot_loop_argmax", st, loop_args(d, lp));
}
int launch_sample_logprob(const AcaiDecoder *d, const float *uniforms, int top_k, float temperature, bool chained, hipStream_t st) {
    return launch_sample<false, false>(d, chained, draw_args(d, uniforms, d->max_len, nullptr, top_k, temperature), {}, {}, "sample_logprob", st);
}
int launch_grammar_sample(const AcaiDecoder *d, const AcaiGrammar *gr, const float *uniforms, int top_k, float temperature, bool chained,
                          hipStream_t st) {
    return launch_sample<false, true>(d, chained, draw_args(d, uniforms, d->max_len, nullptr, top_k, temperature), {}, grammar_args(gr),
                                      "grammar_sample", st);
}
int launch_slot_sample(const AcaiDecoder *d, const AcaiSlots *sl, const float *uniforms, int ld_uniforms, const int32_t *urow, int top_k,
                       float temperature, hipStream_t st) {
    return launch_sample<true, false>(d, true, draw_args(d, uniforms, ld_uniforms, urow, top_k, temperature), slot_args(sl), {}, "slot_sample", st);
}
int launch_slot_grammar_sample(const AcaiDecoder *d, const AcaiSlots *sl, const AcaiGrammar *gr, const float *uniforms, int ld_uniforms,
                               const int32_t *urow, int top_k, float temperature, hipStream_t st) {
    return launch_sample<true, true>(d, true, draw_args(d, uniforms, ld_uniforms, urow, top_k, temperature), slot_args(sl), grammar_args(gr),
                                     "slot_grammar_sample", st);
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

// Test entry (declared and documented in acai_omr_hip.h): ONE selection launch on the logits the caller wrote, through the launch helper the
// step of that form calls.  No layer runs and check_decoder is not applied: the descriptor holds the fields selection reads and nothing else.
// The time index a kernel reads on the device (step[0], a slot's t) is the caller's to keep inside the rows, as it is for the steps.
extern "C" int acai_debug_decode_select(int form, const AcaiDecoder *d, const AcaiSlots *sl, const AcaiGrammar *g, const AcaiPrompt *pr,
                                        const AcaiBeam *bs, const float *uniforms, int ld_uniforms, const int32_t *urow, int top_k,
                                        float temperature, int chained, void *stream) {
    const char *fn = "acai_debug_decode_select";
    ACAI_CHECK_ARG(form >= ACAI_SELECT_ARGMAX && form <= ACAI_SELECT_BEAM, "%s: form %d outside [0, 9]", fn, form);
    const bool beam = form == ACAI_SELECT_BEAM;
    const bool slot = form == ACAI_SELECT_SLOT_ARGMAX || form == ACAI_SELECT_SLOT_GRAMMAR_ARGMAX || form == ACAI_SELECT_SLOT_SAMPLE ||
                      form == ACAI_SELECT_SLOT_GRAMMAR_SAMPLE;
    const bool grammar = form == ACAI_SELECT_GRAMMAR_ARGMAX || form == ACAI_SELECT_SLOT_GRAMMAR_ARGMAX || form == ACAI_SELECT_GRAMMAR_SAMPLE ||
                         form == ACAI_SELECT_SLOT_GRAMMAR_SAMPLE;
    const bool sampled = form >= ACAI_SELECT_SAMPLE && form <= ACAI_SELECT_SLOT_GRAMMAR_SAMPLE;
    ACAI_CHECK_ARG(d, "%s: null decoder", fn);
    ACAI_CHECK_ARG(d->logits && d->step && d->finished, "%s: null logits / step / finished", fn);
    ACAI_CHECK_ARG(beam || (d->seqs && d->logprobs), "%s: null seqs / logprobs", fn);
    ACAI_CHECK_ARG(d->B >= 1 && d->V >= 1 && d->E >= 1 && d->Tmax >= 1 && d->max_len > 1, "%s: bad dims B=%d V=%d E=%d Tmax=%d max_len=%d", fn,
                   d->B, d->V, d->E, d->Tmax, d->max_len);
    ACAI_CHECK_ARG(chained || !(slot || beam), "%s: a slot or beam selection always writes the next input (chained = 0 with form %d)", fn, form);
    ACAI_CHECK_ARG(!chained || (d->emb && d->pos && d->x), "%s: a chained selection needs emb, pos and x", fn);
    ACAI_CHECK_ARG(!chained || d->E % 4 == 0, "%s: a chained selection needs E %% 4 == 0 (E=%d)", fn, d->E);
    if (slot) {
        ACAI_CHECK_ARG(sl && sl->t && sl->cap && sl->rows >= d->B, "%s: null slot state or rows < B", fn);
        ACAI_CHECK_ARG(d->max_len <= d->Tmax, "%s: a slot selection needs max_len <= Tmax (max_len=%d Tmax=%d)", fn, d->max_len, d->Tmax);
    }
    if (grammar) {   // (acai_decode_grammar_step's conditions but its vocabulary bound, which is the sampled forms': check_draw below)
        ACAI_CHECK_ARG(g && g->next && g->resync && g->state, "%s: null grammar tables or state", fn);
        ACAI_CHECK_ARG(g->states >= 1 && g->states <= 32767, "%s: states %d outside [1, 32767]", fn, g->states);
        ACAI_CHECK_ARG(g->start >= 0 && g->start < g->states, "%s: start %d outside [0, states = %d)", fn, g->start, g->states);
        ACAI_CHECK_ARG(g->rows >= d->B, "%s: grammar rows %d below B = %d", fn, g->rows, d->B);
    }
    if (form == ACAI_SELECT_PROMPT) {
        ACAI_CHECK_ARG(pr && pr->tok && pr->len, "%s: null prompt tables", fn);
        ACAI_CHECK_ARG(pr->pitch >= d->max_len && pr->rows >= d->B, "%s: needs prompt pitch >= max_len and rows >= B (pitch=%d max_len=%d rows=%d)",
                       fn, pr->pitch, d->max_len, pr->rows);
    }
    if (sampled) {
        int rc = check_draw(d, fn, uniforms, top_k, temperature, slot ? 1 : 0, ld_uniforms, urow);
        if (rc) return rc;
    }
    if (beam) {
        ACAI_CHECK_ARG(bs && bs->anc && bs->tok && bs->lp && bs->cum && bs->len, "%s: null beam state", fn);
        ACAI_CHECK_ARG(bs->K >= 1 && bs->K <= BEAM_MAX && d->B % bs->K == 0 && bs->rows >= d->B && bs->pitch >= d->max_len && d->V <= 512,
                       "%s: needs 1 <= K <= 16 dividing B, rows >= B, pitch >= max_len, vocabulary <= 512 (K=%d B=%d rows=%d pitch=%d V=%d)", fn,
                       bs->K, d->B, bs->rows, bs->pitch, d->V);
    }
    hipStream_t st = (hipStream_t)stream;
    const bool ch = chained != 0;
    switch (form) {
        case ACAI_SELECT_ARGMAX: return launch_argmax_logprob(d, ch, st);
        case ACAI_SELECT_PROMPT: return launch_prompt_logprob(d, pr, ch, st);
        case ACAI_SELECT_GRAMMAR_ARGMAX: return launch_grammar_argmax(d, g, ch, st);
        case ACAI_SELECT_SLOT_ARGMAX: return launch_slot_argmax(d, sl, st);
        case ACAI_SELECT_SLOT_GRAMMAR_ARGMAX: return launch_slot_grammar_argmax(d, sl, g, st);
        case ACAI_SELECT_SAMPLE: return launch_sample_logprob(d, uniforms, top_k, temperature, ch, st);
        case ACAI_SELECT_GRAMMAR_SAMPLE: return launch_grammar_sample(d, g, uniforms, top_k, temperature, ch, st);
        case ACAI_SELECT_SLOT_SAMPLE: return launch_slot_sample(d, sl, uniforms, ld_uniforms, urow, top_k, temperature, st);
        case ACAI_SELECT_SLOT_GRAMMAR_SAMPLE: return launch_slot_grammar_sample(d, sl, g, uniforms, ld_uniforms, urow, top_k, temperature, st);
        default: return launch_beam_select(d, bs, st);
    }
}

// Test entry (declared and documented in acai_omr_hip.h): acai_debug_decode_select's counterpart for the two loop-guard forms.
extern "C" int acai_debug_decode_loop_select(int slot, const AcaiDecoder *d, const AcaiSlots *sl, const AcaiLoop *loop, int chained, void *stream) {
    const char *fn = "acai_debug_decode_loop_select";
    ACAI_CHECK_ARG(d, "%s: null decoder", fn);
    ACAI_CHECK_ARG(d->logits && d->step && d->finished && d->seqs && d->logprobs, "%s: null logits / step / finished / seqs / logprobs", fn);
    ACAI_CHECK_ARG(d->B >= 1 && d->V >= 1 && d->E >= 1 && d->Tmax >= 1 && d->max_len > 1, "%s: bad dims B=%d V=%d E=%d Tmax=%d max_len=%d", fn,
                   d->B, d->V, d->E, d->Tmax, d->max_len);
    ACAI_CHECK_ARG(chained || !slot, "%s: a slot selection always writes the next input (chained = 0 with slot = %d)", fn, slot);
    ACAI_CHECK_ARG(!chained || (d->emb && d->pos && d->x), "%s: a chained selection needs emb, pos and x", fn);
    ACAI_CHECK_ARG(!chained || d->E % 4 == 0, "%s: a chained selection needs E %% 4 == 0 (E=%d)", fn, d->E);
    if (slot) {
        ACAI_CHECK_ARG(sl && sl->t && sl->cap && sl->rows >= d->B, "%s: null slot state or rows < B", fn);
        ACAI_CHECK_ARG(d->max_len <= d->Tmax, "%s: a slot selection needs max_len <= Tmax (max_len=%d Tmax=%d)", fn, d->max_len, d->Tmax);
    }
    int rc = check_loop(d, loop, fn);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    return slot ? launch_slot_loop_argmax(d, sl, loop, st) : launch_loop_argmax(d, loop, chained != 0, st);
}

// Test entry (declared and documented in acai_omr_hip.h): ONE launch of spec_accept_kernel on the state and logits the caller wrote, through
// the helper the speculative steps call.  No layer runs; check_decoder, check_unembed and the x-valid contract are not applied: what is
// checked is what this launch reads - check_spec's conditions on the speculative state and, with a prompt, check_prompt's for one row per image.
extern "C" int acai_debug_decode_spec_accept(const AcaiDecoder *d, const AcaiSpec *sp, const AcaiPrompt *pr, int arm, void *stream) {
    const char *fn = "acai_debug_decode_spec_accept";
    ACAI_CHECK_ARG(d, "%s: null decoder", fn);
    ACAI_CHECK_ARG(d->seqs && d->logprobs && d->step && d->finished, "%s: null seqs / logprobs / step / finished", fn);
    ACAI_CHECK_ARG(d->emb && d->pos && d->x, "%s: null emb / pos / x", fn);
    ACAI_CHECK_ARG(arm || d->logits, "%s: a verify step (arm = 0) needs logits", fn);
    ACAI_CHECK_ARG(d->B >= 1 && d->V >= 1 && d->E >= 1, "%s: bad dims B=%d V=%d E=%d", fn, d->B, d->V, d->E);
    ACAI_CHECK_ARG(d->max_len > 1 && d->max_len <= d->Tmax, "%s: max_len outside [2, Tmax] (max_len=%d Tmax=%d)", fn, d->max_len, d->Tmax);
    ACAI_CHECK_ARG(sp && sp->t && sp->cap && sp->steps && sp->tab && sp->next, "%s: null speculative state", fn);
    ACAI_CHECK_ARG(sp->D >= 1 && sp->D <= 7, "%s: draft length %d outside [1, 7]", fn, sp->D);
    ACAI_CHECK_ARG(d->B % (sp->D + 1) == 0, "%s: needs B %% (D + 1) == 0 (B=%d D=%d)", fn, d->B, sp->D);
    ACAI_CHECK_ARG(sp->rows >= d->B / (sp->D + 1) && sp->pitch >= d->max_len && sp->pitch <= d->Tmax, "%s: needs rows >= B / (D + 1) and "
                   "max_len <= pitch <= Tmax (rows=%d pitch=%d)", fn, sp->rows, sp->pitch);
    ACAI_CHECK_ARG(sp->drafts || (sp->ngram >= 1 && sp->ngram <= 8), "%s: without a drafts table ngram must be in [1, 8] (got %d)", fn, sp->ngram);
    if (pr) {
        const int rows = d->B / (sp->D + 1);
        ACAI_CHECK_ARG(pr->tok && pr->len, "%s: null prompt tables", fn);
        ACAI_CHECK_ARG(pr->pitch >= d->max_len && pr->rows >= rows, "%s: needs prompt pitch >= max_len and rows >= %d (pitch=%d max_len=%d rows=%d)",
                       fn, rows, pr->pitch, d->max_len, pr->rows);
        return launch_spec_prompt_accept(d, sp, pr, arm, (hipStream_t)stream);
    }
    return launch_spec_accept(d, sp, arm, (hipStream_t)stream);
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

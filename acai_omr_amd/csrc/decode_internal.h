// Internal interface between the decode sources (decode.hip, decode_gemv.hip, decode_attn.hip, decode_select.hip, decode_prefill.hip).  Not installed and
// not part of the C ABI (include/acai_omr_hip.h).  No __device__ helper lives here: what the decode kernels share is in common.h.
#pragma once
#include <stdlib.h>

#include "common.h"

constexpr int SKM_MAXK = 4096;   // largest K of the MFMA skinny GEMM
constexpr int BEAM_MAX = 16;     // largest beam width of beam_select_kernel

struct SkinnyArgs {
    const float *x;        // [B, ldx] fp32
    const void *W;         // [N, ldw]
    const float *bias;     // [N] or null
    const float *residual; // [B, ldr] or null
    float *y;              // [B, ldy]
    int ldx, ldw, ldr, ldy, B, N, K, flags;
    // optional KV append (self-attention in_proj): columns E..3E also go to the caches at position step[1]
    void *k_cache, *v_cache;
    const int32_t *step;
    int E, H, dh, dhp, Tmax;
    // optional fused LayerNorm (MFMA kernel only): x := LN(x) on load (dim == K); the per-row (mean, rstd) can be
    // published for a later launch; residual := LN(residual) from published statistics
    const float *ln_w, *ln_b;
    float ln_eps;
    float *stats_out;        // [B][2]
    const float *rln_w, *rln_b, *rstats;
    int x_bf16, y_bf16;      // activation in / out stored as bf16 (x: row stride ldx in bf16 elements)
    int rows_per_block;      // MFMA kernel: weight rows per workgroup (set by the launcher)
    int w_cached;            // non-zero: default-policy (cacheable) weight loads instead of non-temporal ones (ACAI_SKINNY_NT, an A/B aid)
    const float *ln2_w, *ln2_b;   // chain kernel only: a SECOND LayerNorm applied to the normalised row (last layer's norm3, then the stack's final norm)
    float ln2_eps;
    unsigned long long *stamps;   // diagnostic (acai_debug_stamps): [workgroup][8] s_memrealtime stamps (100 MHz) of the kernel's stages, else null
};

struct DAttnArgs {
    const float *q;   // [B, ldq] fp32, head h at column h*dh
    const void *kc, *vc;
    const int64_t *seq_off;  // per-sequence element offset (ragged cross K/V) or null
    const int32_t *seq_len;  // per-sequence length (cross) or null; SLOT (with seq_off null): per-row key count
    const int32_t *step;     // self-attention: length = step[1] + 1, layout [B][H][Tmax][dhp]
    float *partial;          // [B][H][nsplit][dhp + 2]
    int ldq, H, dh, dhp, Tmax, chunk, nsplit;
    float scale_log2e;
    float *out;              // nsplit == 1: the workgroup writes softmax(qK^T)V itself to out[b, h*dh + d] (no combine launch)
    int ldo, round_out;
    unsigned *tickets;       // [B*H] arrival counters (zero between launches): the LAST workgroup of a (b, h) merges the splits
    // beam search (ANC instantiation only): key p of row b lives in cache row anc[b][p] of the parity copy (step[0] & 1) of the ancestor table.
    // Continuous batching (SLOT instantiation only): row b has seq_len[b] keys, key j at ring position (slot_first[b] + j) % Tmax.  The two
    // share a slot so that the struct - and with it every existing kernel's argument offsets - stays as it was.
    // Speculative greedy decoding (SPEC instantiation only): the R = anc_bstride rows of image b / R share the image's key table
    // spec_tab[b / R][anc_pitch]; entry p = 8 * (cache position) + (row of the image) holds key p; row b attends over seq_len[b / R] + b % R
    // keys.  It rides the same slot, and anc_pitch / anc_bstride / seq_len, for the same reason.
    union {
        const int32_t *anc;  // [2][rows][anc_pitch]
        const int32_t *slot_first;
        const int32_t *spec_tab;
    };
    int anc_pitch;
    long long anc_bstride;   // elements between the two parity copies (rows * anc_pitch); SPEC: rows per image
    // FP8 memory cache (fp8e4m3_t instantiation only): one fp32 power-of-two scale per K row and per V row, at the row's element offset / dhp
    const float *k_scale, *v_scale;
    // decode_attn_kernel only: out holds bf16 rows (ldo in bf16 elements) - the fused step's values are bf16-representable already (round_out),
    // and the out / cross-out GEMV then stages half the bytes.  Appended, so that every other member keeps its offset.
    int out_bf16;
};

// Element type of an FP8 (OCP e4m3fn) cross K/V cache: a stored value is q * 2^e, 2^e the row's scale (acai_cross_kv_quantize_fp8)
struct fp8e4m3_t {
    uint8_t bits;
};

// ---- decode_gemv.hip ----------------------------------------------------------------------------------------------------------------
bool skinny_mfma_ok(const SkinnyArgs &a);   // the bf16 MFMA forms take these operands (K, leading dimensions, alignment)
template <typename TW>                      // TW = float or bf16_t (the weight type); instantiated for both in decode_gemv.hip
int launch_skinny(const SkinnyArgs &a, hipStream_t st);

// ---- decode_attn.hip ----------------------------------------------------------------------------------------------------------------
template <typename TC>                      // TC = float or bf16_t (the cache type); instantiated for both in decode_attn.hip
int launch_dattn(const DAttnArgs &a, int B, bool spec, hipStream_t st);
int launch_dattn_fp8(const DAttnArgs &a, int B, hipStream_t st);
int launch_dattn_group(const DAttnArgs &a, int B, int group, hipStream_t st);
int launch_attn_combine(const float *partial, float *out, int ldo, int B, int H, int dh, int dhp, int nsplit, int round_out, hipStream_t st);
// may the splits of decode_attn_kernel<dtype's cache type, dhp> be merged inside the launch (tickets)?  dtype: ACAI_F32 / ACAI_BF16 / ACAI_FP8_E4M3
bool dattn_merge_in_launch(int dtype, int dhp);

// ---- decode_select.hip: one launch helper per selection form, operands from the descriptors (the nine greedy / sampled forms are
// instantiations of greedy_select_kernel / sample_select_kernel) --------------------------------------------------------------------------
int launch_embed(const AcaiDecoder *d, const int64_t *tokens, hipStream_t st);
int launch_set_step(const AcaiDecoder *d, int t, hipStream_t st);
int launch_advance_cache(const AcaiDecoder *d, hipStream_t st);
int launch_argmax_logprob(const AcaiDecoder *d, bool chained, hipStream_t st);
int launch_sample_logprob(const AcaiDecoder *d, const float *uniforms, int top_k, float temperature, bool chained, hipStream_t st);
int launch_beam_select(const AcaiDecoder *d, const AcaiBeam *bs, hipStream_t st);
int launch_slot_arm(const AcaiDecoder *d, const AcaiSlots *sl, const int32_t *rows, int n, hipStream_t st);
int launch_slot_argmax(const AcaiDecoder *d, const AcaiSlots *sl, hipStream_t st);
int launch_slot_sample(const AcaiDecoder *d, const AcaiSlots *sl, const float *uniforms, int ld_uniforms, const int32_t *urow, int top_k,
                       float temperature, hipStream_t st);
int launch_spec_accept(const AcaiDecoder *d, const AcaiSpec *sp, int arm, hipStream_t st);
int launch_prompt_logprob(const AcaiDecoder *d, const AcaiPrompt *pr, bool chained, hipStream_t st);
int launch_spec_prompt_accept(const AcaiDecoder *d, const AcaiSpec *sp, const AcaiPrompt *pr, int arm, hipStream_t st);
int launch_grammar_argmax(const AcaiDecoder *d, const AcaiGrammar *gr, bool chained, hipStream_t st);
int launch_grammar_sample(const AcaiDecoder *d, const AcaiGrammar *gr, const float *uniforms, int top_k, float temperature, bool chained,
                          hipStream_t st);
int launch_slot_grammar_argmax(const AcaiDecoder *d, const AcaiSlots *sl, const AcaiGrammar *gr, hipStream_t st);
int launch_slot_grammar_sample(const AcaiDecoder *d, const AcaiSlots *sl, const AcaiGrammar *gr, const float *uniforms, int ld_uniforms,
                               const int32_t *urow, int top_k, float temperature, hipStream_t st);

int launch_loop_argmax(const AcaiDecoder *d, const AcaiLoop *lp, bool chained, hipStream_t st);
int launch_slot_loop_argmax(const AcaiDecoder *d, const AcaiSlots *sl, const AcaiLoop *lp, hipStream_t st);

// ---- decode.hip: the checks of a sampling step's draw (`fn` names the entry point in the message), shared with the selection test entry ----
int check_draw(const AcaiDecoder *d, const char *fn, const float *uniforms, int top_k, float temperature, int slot = 0, int ld_uniforms = 0,
               const int32_t *urow = nullptr);
// the checks of a loop-guard descriptor, shared with the loop selection test entry
int check_loop(const AcaiDecoder *d, const AcaiLoop *loop, const char *fn);

// ---- decode_prefill.hip: the prompt's self K/V rows and the state its steps would leave, from one teacher-forced pass ------------------
int launch_prefill_self_kv(const AcaiDecoder *d, int layer, const void *qkv, int ld, int C, hipStream_t st);
int launch_prefill_arm(const AcaiDecoder *d, const AcaiPrompt *pr, const float *logits, int C, hipStream_t st);

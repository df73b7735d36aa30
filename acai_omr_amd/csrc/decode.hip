// KV-cached greedy decode step: the HBM-bound half of the path.
// Reference: CachedTransformerDecoderLayer.cached_forward (acai_omr/models/kv_caching.py:190-223),
// KVCache.update (K:83-109), CachedTransformerDecoder.cached_generate (K:292-302),
// OMRDecoder.cached_generate (acai_omr/models/models.py:518-528), ViTOMR.cached_get_next_token (M:575-583),
// cached_greedy_generate loop body (M:603-611).
//
// gfx950 design: per step the bytes that matter are the decoder weights (read once) and, dominating, the
// cross-attention K/V of every sequence (12 layers x 2 x S x 1024 elements each).  Everything is a
// streaming kernel with 16-byte loads, fp32 accumulation and no host involvement: positions, lengths and
// the finished flags live in device memory, so one captured hipGraph replays for every token.
// The step driver lives here; its kernels are in decode_gemv.hip (skinny_gemm / skinny_mfma / skinny_chain), decode_attn.hip
// (decode_attn, attn_combine, the FP8 memory cache), decode_select.hip (embedding and token selection) and decode_prefill.hip (prompt
// prefill), behind decode_internal.h.
#include "decode_internal.h"

#include <mutex>
#include <unordered_map>

namespace {

// Host-side record of "d->x holds the chained step's input embedding" per decoder state (keyed by the x buffer): acai_decode_embed sets it,
// acai_decode_step / acai_decode_sample_step require it (they no longer embed by themselves: their input is what the previous step's argmax
// kernel wrote) and keep it, acai_decode_logits / acai_decode_hidden clear it (they overwrite x).  A C-ABI caller that mixes the stepwise and
// the chained entry points without re-embedding gets an argument error instead of a step on stale input.  (Replays of a captured graph do
// not pass through here: the capture-time call is what is checked - INTEGRATION.md.)
static std::mutex g_xv_mu;
static std::unordered_map<const void *, bool> g_x_valid;
static void x_valid_set(const AcaiDecoder *d, bool v) {
    std::lock_guard<std::mutex> lk(g_xv_mu);
    g_x_valid[d->x] = v;
}
static bool x_valid_get(const AcaiDecoder *d) {
    std::lock_guard<std::mutex> lk(g_xv_mu);
    auto it = g_x_valid.find(d->x);
    return it != g_x_valid.end() && it->second;
}

int check_decoder(const AcaiDecoder *d) {
    ACAI_CHECK_ARG(d && d->layers, "decoder: null descriptor");
    ACAI_CHECK_ARG(d->B > 0 && d->L > 0 && d->E == d->H * d->dh && d->dhp >= d->dh && d->dhp <= 64 && (d->dhp & (d->dhp - 1)) == 0 &&
                       d->dhp * (d->dtype == ACAI_BF16 ? 2 : 4) >= 16,
                   "decoder: bad dims B=%d L=%d E=%d H=%d dh=%d dhp=%d", d->B, d->L, d->E, d->H, d->dh, d->dhp);
    ACAI_CHECK_ARG(d->dtype == ACAI_F32 || d->dtype == ACAI_BF16, "decoder: bad dtype");
    if (d->flags & ACAI_DEC_CROSS_FP8) {
        ACAI_CHECK_ARG(d->dtype == ACAI_BF16 && d->cross_group == 1, "decoder: an FP8 cross K/V needs the bf16 decoder and cross_group 1");
        for (int l = 0; l < d->L; ++l)
            ACAI_CHECK_ARG(d->layers[l].k_cross_scale && d->layers[l].v_cross_scale, "decoder: FP8 cross K/V of layer %d without scales", l);
    }
    ACAI_CHECK_ARG(d->self_chunk > 0 && d->cross_chunk > 0 && d->self_nsplit > 0 && d->cross_nsplit > 0 &&
                       (long)d->self_chunk * d->self_nsplit >= d->Tmax,
                   "decoder: attention split does not cover the cache");
    ACAI_CHECK_ARG(d->cross_off && d->cross_len && d->step && d->x && d->xn && d->qkv && d->attn && d->proj && d->hid && d->partial,
                   "decoder: null buffer");
    return 0;
}

template <typename TW>
int decode_core(const AcaiDecoder *d, const int64_t *tokens, hipStream_t st, bool do_embed = true, bool do_unembed = true,
                const AcaiBeam *beam = nullptr, const AcaiSlots *slots = nullptr, const AcaiSpec *spec = nullptr) {
    const int B = d->B, E = d->E, H = d->H, F = d->F;
    const int rnd = (d->flags & ACAI_GEMM_ROUND_BF16) ? ACAI_GEMM_ROUND_BF16 : 0;
    const float sc = 1.4426950408889634f / sqrtf((float)d->dh);
    int rc;
    if (do_embed && (rc = launch_embed(d, tokens, st))) return rc;

    // Fused path (bf16, MFMA skinny GEMM): the residual stream is kept PRE-LayerNorm (z) and every consumer applies the
    // LayerNorm on load, so a layer is 6 GEMV + 2 attention (+2 combine) launches instead of 17.
    SkinnyArgs probe{};
    probe.x = d->x; probe.W = d->layers[0].self_in_w; probe.K = E; probe.ldw = E; probe.ldx = E;
    const bool fused = sizeof(TW) == 2 && d->stats && rnd && skinny_mfma_ok(probe) && (F % 256 == 0) && F <= SKM_MAXK;
    bool hid_bf16 = false, hid_in_bf16 = false;
    // The per-row attention kernel, when it finishes its output inside its own launch, stores the (bf16-valued) rows as bf16 and the out /
    // cross-out GEMV takes the bf16-activation chain form at K = 1024: half the bytes every workgroup of the GEMV stages.  attn_bf16 says
    // what the last attend() left in d->attn.  ACAI_ATTN_BF16=0 keeps fp32 rows (A/B aid).
    static const bool no_chain = getenv("ACAI_SKINNY_CHAIN") && atoi(getenv("ACAI_SKINNY_CHAIN")) == 0;
    static const bool no_attn_bf16 = getenv("ACAI_ATTN_BF16") && atoi(getenv("ACAI_ATTN_BF16")) == 0;
    const bool attn_bf16_ok = fused && E == 1024 && !no_chain && !no_attn_bf16;
    bool attn_bf16 = false;
    // every GEMV of the step: y = x . W^T + bias (+ res); kvl: append the self K/V; lnw / lnb: LayerNorm (eps) of x on load, its row
    // statistics published to stats_out; rlnw / rlnb / rstats: LayerNorm of res from published statistics; ln2w / ln2b: a second
    // LayerNorm (eps 1e-6) after the first (unembed).  The LayerNorm operands are only passed on the fused path.
    auto skinny = [&](const float *x, int ldx, const void *W, const float *bias, const float *res, float *y, int ldy, int N, int K,
                      int flags, const AcaiDecLayer *kvl, const float *lnw = nullptr, const float *lnb = nullptr, float *stats_out = nullptr,
                      const float *rlnw = nullptr, const float *rlnb = nullptr, const float *rstats = nullptr, float eps = 1e-5f,
                      const float *ln2w = nullptr, const float *ln2b = nullptr) -> int {
        SkinnyArgs s{};
        s.x = x; s.W = W; s.bias = bias; s.residual = res; s.y = y;
        s.ldx = ldx; s.ldw = K; s.ldr = E; s.ldy = ldy; s.B = B; s.N = N; s.K = K; s.flags = flags;
        s.ln_w = lnw; s.ln_b = lnb; s.ln_eps = eps; s.stats_out = stats_out; s.rln_w = rlnw; s.rln_b = rlnb; s.rstats = rstats;
        s.ln2_w = ln2w; s.ln2_b = ln2b; s.ln2_eps = 1e-6f;
        s.y_bf16 = hid_bf16 && (flags & ACAI_GEMM_ROUND_BF16);
        s.x_bf16 = hid_in_bf16 && (flags & ACAI_GEMM_ROUND_BF16);
        if (kvl) {
            s.k_cache = kvl->k_self; s.v_cache = kvl->v_self; s.step = d->step;
            s.E = E; s.H = H; s.dh = d->dh; s.dhp = d->dhp; s.Tmax = d->Tmax;
        }
        return launch_skinny<TW>(s, st);
    };
    auto unembed = [&](const float *x, const float *lnw, const float *lnb, float eps, const float *ln2w, const float *ln2b) -> int {
        return skinny(x, E, d->unembed_w, d->unembed_b, nullptr, d->logits, d->V, d->V, E, rnd, nullptr, lnw, lnb, nullptr, nullptr, nullptr,
                      nullptr, eps, ln2w, ln2b);
    };
    // FP8 memory cache (ACAI_DEC_CROSS_FP8): the cross attention reads e4m3 rows of dhp8 = max(dhp, 16) elements and their scales
    const bool cross_f8 = (d->flags & ACAI_DEC_CROSS_FP8) != 0;
    auto attend = [&](const float *q, int ldq, const void *kc, const void *vc, bool cross, const AcaiDecLayer *ly = nullptr) -> int {
        DAttnArgs a{};
        a.q = q; a.kc = kc; a.vc = vc; a.ldq = ldq; a.H = H; a.dh = d->dh; a.dhp = d->dhp; a.Tmax = d->Tmax;
        a.partial = d->partial; a.scale_log2e = sc;
        const bool f8 = cross && cross_f8;
        if (cross) {
            a.seq_off = d->cross_off; a.seq_len = d->cross_len; a.chunk = d->cross_chunk; a.nsplit = d->cross_nsplit;
            if (f8) {
                a.dhp = d->dhp < 16 ? 16 : d->dhp;
                a.k_scale = ly->k_cross_scale; a.v_scale = ly->v_cross_scale;
            }
        } else {
            a.step = d->step; a.chunk = d->self_chunk; a.nsplit = d->self_nsplit;
            if (beam) {   // beam step: keys through the ancestor table (decode_attn_kernel's ANC instantiation)
                a.anc = beam->anc; a.anc_pitch = beam->pitch; a.anc_bstride = (long long)beam->rows * beam->pitch;
            }
            if (slots) {   // slot step: per-row lengths over the ring (decode_attn_kernel's SLOT instantiation)
                a.seq_len = slots->t; a.slot_first = slots->first;
            }
            if (spec) {   // verify step: keys through the image's table, t + j of them for row j (decode_attn_kernel's SPEC instantiation)
                a.seq_len = spec->t; a.spec_tab = spec->tab; a.anc_pitch = spec->pitch; a.anc_bstride = spec->D + 1;
            }
        }
        auto per_row = [&]() { return f8 ? launch_dattn_fp8(a, B, st) : launch_dattn<TW>(a, B, spec && !cross, st); };
        // rollout groups (bf16, d_h padded to 64): one K/V stream per image through the matrix-core kernel; otherwise the rows simply alias
        // the stored K/V through the per-row kernel (ACAI_DECODE_GROUP_KERNEL=0 forces that form: A/B aid)
        static const bool no_group = getenv("ACAI_DECODE_GROUP_KERNEL") && atoi(getenv("ACAI_DECODE_GROUP_KERNEL")) == 0;
        // (a verify step keeps the per-row kernel: the matrix-core form orders a row's sums differently from the greedy step's)
        const int group = (!f8 && !no_group && !spec && sizeof(TW) == 2 && d->dhp == 64 && cross && d->cross_group > 1 && B % d->cross_group == 0) ? d->cross_group : 1;
        // the splits are merged by the launch itself (one split, or tickets at a validated residency), else by a separate combine launch
        // behind the per-row kernel
        const bool merge = a.nsplit > 1 && d->tickets && (group > 1 || dattn_merge_in_launch(f8 ? ACAI_FP8_E4M3 : DT<TW>::id, a.dhp));
        attn_bf16 = false;
        if (a.nsplit == 1 || merge) {
            a.out = d->attn; a.ldo = E; a.round_out = rnd ? 1 : 0;
            attn_bf16 = attn_bf16_ok && group == 1 && !f8;   // (the matrix-core and FP8 kernels and the combine launch keep fp32 rows)
            a.out_bf16 = attn_bf16 ? 1 : 0;
            if (merge) a.tickets = d->tickets;
            return group > 1 ? launch_dattn_group(a, B, group, st) : per_row();
        }
        if ((rc = per_row())) return rc;
        return launch_attn_combine(d->partial, d->attn, E, B, H, d->dh, a.dhp, a.nsplit, rnd ? 1 : 0, st);
    };

    if (fused) {
        float *st0 = d->stats, *st1 = d->stats + 2 * B, *st2 = d->stats + 4 * B;
        float *zin = d->x, *z1 = d->proj, *z2 = d->xn;
        const float *lnw = nullptr, *lnb = nullptr;  // LayerNorm still to be applied to zin (norm3 of the previous layer)
        for (int l = 0; l < d->L; ++l) {
            const AcaiDecLayer *ly = d->layers + l;
            if ((rc = skinny(zin, E, ly->self_in_w, ly->self_in_b, nullptr, d->qkv, 3 * E, 3 * E, E, rnd, ly, lnw, lnb, st0))) return rc;
            if ((rc = attend(d->qkv, 3 * E, ly->k_self, ly->v_self, false))) return rc;
            hid_in_bf16 = attn_bf16;
            if ((rc = skinny(d->attn, E, ly->self_out_w, ly->self_out_b, zin, z1, E, E, E, rnd, nullptr, nullptr, nullptr, nullptr, lnw, lnb, st0))) return rc;
            hid_in_bf16 = false;
            if ((rc = skinny(z1, E, ly->cross_q_w, ly->cross_q_b, nullptr, d->qkv, 3 * E, E, E, rnd, nullptr, ly->n1_w, ly->n1_b, st1))) return rc;
            if ((rc = attend(d->qkv, 3 * E, ly->k_cross, ly->v_cross, true, ly))) return rc;
            hid_in_bf16 = attn_bf16;
            if ((rc = skinny(d->attn, E, ly->cross_out_w, ly->cross_out_b, z1, z2, E, E, E, rnd, nullptr, nullptr, nullptr, nullptr, ly->n1_w, ly->n1_b, st1))) return rc;
            hid_in_bf16 = false;
            hid_bf16 = true;   // linear1 -> GELU output is bf16 under autocast anyway: store it as such (half the x bytes of linear2)
            if ((rc = skinny(z2, E, ly->lin1_w, ly->lin1_b, nullptr, d->hid, F, F, E, rnd | ACAI_GEMM_GELU, nullptr, ly->n2_w, ly->n2_b, st2))) return rc;
            hid_bf16 = false;
            hid_in_bf16 = true;
            if ((rc = skinny(d->hid, F, ly->lin2_w, ly->lin2_b, z2, zin, E, E, F, rnd, nullptr, nullptr, nullptr, nullptr, ly->n2_w, ly->n2_b, st2))) return rc;
            hid_in_bf16 = false;
            lnw = ly->n3_w;
            lnb = ly->n3_b;
        }
        // x = norm3(z3) of the last layer, then the stack's final norm (eps 1e-6): both fused into the unembed GEMV's load when the chain
        // kernel takes it (E = 1024) - no stand-alone LayerNorm launch is left in a token step
        if (do_unembed && d->fn_w && E == 1024 && !no_chain && lnw) return unembed(zin, lnw, lnb, 1e-5f, d->fn_w, d->fn_b);
        if ((rc = acai_layernorm_fwd(zin, lnw, lnb, 1e-5f, d->proj, nullptr, B, E, st))) return rc;
        if (do_unembed && d->fn_w) return unembed(d->proj, d->fn_w, d->fn_b, 1e-6f, nullptr, nullptr);
        if (d->fn_w) {
            if ((rc = acai_layernorm_fwd(d->proj, d->fn_w, d->fn_b, 1e-6f, d->xn, nullptr, B, E, st))) return rc;
        } else {
            hipError_t e = hipMemcpyAsync(d->xn, d->proj, sizeof(float) * (size_t)B * E, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) return acai_set_err((int)e, "hipMemcpyAsync: %s", hipGetErrorString(e));
        }
    } else {
    for (int l = 0; l < d->L; ++l) {
        const AcaiDecLayer *ly = d->layers + l;
        // self attention (K:193-208)
        if ((rc = skinny(d->x, E, ly->self_in_w, ly->self_in_b, nullptr, d->qkv, 3 * E, 3 * E, E, rnd, ly))) return rc;
        if ((rc = attend(d->qkv, 3 * E, ly->k_self, ly->v_self, false))) return rc;
        if ((rc = skinny(d->attn, E, ly->self_out_w, ly->self_out_b, d->x, d->proj, E, E, E, rnd, nullptr))) return rc;
        if ((rc = acai_layernorm_fwd(d->proj, ly->n1_w, ly->n1_b, 1e-5f, d->x, nullptr, B, E, st))) return rc;
        // cross attention (K:212-220)
        if ((rc = skinny(d->x, E, ly->cross_q_w, ly->cross_q_b, nullptr, d->qkv, 3 * E, E, E, rnd, nullptr))) return rc;
        if ((rc = attend(d->qkv, 3 * E, ly->k_cross, ly->v_cross, true, ly))) return rc;
        if ((rc = skinny(d->attn, E, ly->cross_out_w, ly->cross_out_b, d->x, d->proj, E, E, E, rnd, nullptr))) return rc;
        if ((rc = acai_layernorm_fwd(d->proj, ly->n2_w, ly->n2_b, 1e-5f, d->x, nullptr, B, E, st))) return rc;
        // feed forward (K:222)
        if ((rc = skinny(d->x, E, ly->lin1_w, ly->lin1_b, nullptr, d->hid, F, F, E, rnd | ACAI_GEMM_GELU, nullptr))) return rc;
        if ((rc = skinny(d->hid, F, ly->lin2_w, ly->lin2_b, d->x, d->proj, E, E, F, rnd, nullptr))) return rc;
        if ((rc = acai_layernorm_fwd(d->proj, ly->n3_w, ly->n3_b, 1e-5f, d->x, nullptr, B, E, st))) return rc;
    }
    if (d->fn_w) {
        if ((rc = acai_layernorm_fwd(d->x, d->fn_w, d->fn_b, 1e-6f, d->xn, nullptr, B, E, st))) return rc;
    } else {
        hipError_t e = hipMemcpyAsync(d->xn, d->x, sizeof(float) * (size_t)B * E, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return acai_set_err((int)e, "hipMemcpyAsync: %s", hipGetErrorString(e));
    }
    }
    return do_unembed ? unembed(d->xn, nullptr, nullptr, 1e-5f, nullptr, nullptr) : 0;
}

// decode_core in the descriptor's weight dtype
int decode(const AcaiDecoder *d, const int64_t *tokens, hipStream_t st, bool do_embed = true, bool do_unembed = true,
           const AcaiBeam *beam = nullptr, const AcaiSlots *slots = nullptr, const AcaiSpec *spec = nullptr) {
    return d->dtype == ACAI_BF16 ? decode_core<bf16_t>(d, tokens, st, do_embed, do_unembed, beam, slots, spec)
                                 : decode_core<float>(d, tokens, st, do_embed, do_unembed, beam, slots, spec);
}

}  // namespace

extern "C" int acai_decode_hidden(const AcaiDecoder *d, const float *x_in, void *stream) {
    int rc = check_decoder(d);
    if (rc) return rc;
    ACAI_CHECK_ARG(x_in, "acai_decode_hidden: null input");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(d->x, x_in, sizeof(float) * (size_t)d->B * d->E, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return acai_set_err((int)e, "hipMemcpyAsync: %s", hipGetErrorString(e));
    rc = decode(d, nullptr, st, false, false);
    if (rc) return rc;
    if ((rc = launch_advance_cache(d, st))) return rc;
    x_valid_set(d, false);
    return 0;
}

// x = vocab_embedding[seqs[:, t-1]] + pos_embedding[t] for the armed state (t = step[0]): run once after arming; every later step's input is
// written by the previous step's argmax / sampling kernel.
extern "C" int acai_decode_embed(const AcaiDecoder *d, void *stream) {
    int rc = check_decoder(d);
    if (rc) return rc;
    ACAI_CHECK_ARG(d->emb && d->pos && d->seqs && d->max_len > 1, "acai_decode_embed: decoder has no embedding / sequence state");
    if ((rc = launch_embed(d, nullptr, (hipStream_t)stream))) return rc;
    x_valid_set(d, true);
    return 0;
}

// The descriptor and the embedding / unembed operands of every entry point that produces logits.
static int check_unembed(const AcaiDecoder *d, const char *fn) {
    int rc = check_decoder(d);
    if (rc) return rc;
    ACAI_CHECK_ARG(d->emb && d->pos && d->unembed_w && d->logits, "%s: decoder has no embedding / unembed", fn);
    return 0;
}

// x holds this step's input: `arm` is the entry point that writes it, once the `state` state is set up
static int check_x_valid(const AcaiDecoder *d, const char *fn, const char *arm, const char *state) {
    ACAI_CHECK_ARG(x_valid_get(d), "%s: x does not hold this step's input embedding - call %s after setting up the %s state and after every "
                                   "acai_decode_logits / acai_decode_hidden", fn, arm, state);
    return 0;
}

// Prologue of the chained greedy / sampling / beam steps: the operands, the sequence state and, for a chained step, that x holds this
// step's input (written by the previous step's selection kernel, or by acai_decode_embed after arming).
static int check_step(const AcaiDecoder *d, const char *fn, bool chained) {
    int rc = check_unembed(d, fn);
    if (rc) return rc;
    ACAI_CHECK_ARG(d->seqs && d->logprobs && d->finished && d->max_len > 1, "%s: null sequence state", fn);
    return chained ? check_x_valid(d, fn, "acai_decode_embed", "sequence") : 0;
}

// The draw of a sampling step; a slot step (slot != 0) also takes the uniforms' pitch and the slots' rows of it (declared in
// decode_internal.h: acai_debug_decode_select in decode_select.hip applies the same checks)
int check_draw(const AcaiDecoder *d, const char *fn, const float *uniforms, int top_k, float temperature, int slot, int ld_uniforms,
               const int32_t *urow) {
    ACAI_CHECK_ARG(uniforms, "%s: null uniforms", fn);
    ACAI_CHECK_ARG(!slot || urow, "%s: null urow", fn);
    ACAI_CHECK_ARG(!slot || ld_uniforms >= d->max_len, "%s: ld_uniforms %d is below max_len %d", fn, ld_uniforms, d->max_len);
    ACAI_CHECK_ARG(top_k >= 1 && top_k <= 64, "%s: top_k %d outside [1, 64]", fn, top_k);
    ACAI_CHECK_ARG(temperature > 0.f, "%s: temperature must be > 0 (got %g)", fn, (double)temperature);
    ACAI_CHECK_ARG(d->V <= 512, "%s: vocabulary %d above 512", fn, d->V);
    return 0;
}

extern "C" int acai_decode_step(const AcaiDecoder *d, void *stream) {
    // the step's input x was written by the previous step's argmax (or by acai_decode_embed after arming) when E allows 16-byte rows
    const bool chained = d && d->E % 4 == 0;
    int rc = check_step(d, "acai_decode_step", chained);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = decode(d, nullptr, st, !chained);
    if (rc) return rc;
    return launch_argmax_logprob(d, chained, st);
}

extern "C" int acai_decode_sample_step(const AcaiDecoder *d, const float *uniforms, int top_k, float temperature, void *stream) {
    const bool chained = d && d->E % 4 == 0;
    int rc = check_step(d, "acai_decode_sample_step", chained);
    if (rc) return rc;
    if ((rc = check_draw(d, "acai_decode_sample_step", uniforms, top_k, temperature))) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = decode(d, nullptr, st, !chained);
    if (rc) return rc;
    return launch_sample_logprob(d, uniforms, top_k, temperature, chained, st);
}

extern "C" int acai_decode_beam_step(const AcaiDecoder *d, const AcaiBeam *bs, void *stream) {
    int rc = check_step(d, "acai_decode_beam_step", true);
    if (rc) return rc;
    ACAI_CHECK_ARG(bs && bs->anc && bs->tok && bs->lp && bs->cum && bs->len, "acai_decode_beam_step: null beam state");
    ACAI_CHECK_ARG(bs->K >= 1 && bs->K <= BEAM_MAX && d->B % bs->K == 0 && bs->rows >= d->B && bs->pitch >= d->max_len && d->V <= 512 &&
                       d->E % 4 == 0 && d->self_chunk <= 16384,
                   "acai_decode_beam_step: needs 1 <= K <= 16 dividing B, rows >= B, pitch >= max_len, vocabulary <= 512, E %% 4 == 0, "
                   "self_chunk <= 16384 (K=%d B=%d rows=%d pitch=%d V=%d E=%d)", bs->K, d->B, bs->rows, bs->pitch, d->V, d->E);
    hipStream_t st = (hipStream_t)stream;
    rc = decode(d, nullptr, st, false, true, bs);
    if (rc) return rc;
    return launch_beam_select(d, bs, st);
}

static int check_slots(const AcaiDecoder *d, const AcaiSlots *sl, const char *fn) {
    int rc = check_unembed(d, fn);
    if (rc) return rc;
    ACAI_CHECK_ARG(d->seqs && d->logprobs && d->finished && d->max_len > 1 && d->max_len <= d->Tmax, "%s: null sequence state or max_len "
                   "outside [2, Tmax] (max_len=%d Tmax=%d)", fn, d->max_len, d->Tmax);
    ACAI_CHECK_ARG(sl && sl->t && sl->first && sl->cap && sl->rows >= d->B, "%s: null slot state or rows < B", fn);
    ACAI_CHECK_ARG(d->cross_group == 1 && d->E % 4 == 0, "%s: needs cross_group == 1 and E %% 4 == 0 (cross_group=%d E=%d)", fn,
                   d->cross_group, d->E);
    return 0;
}

extern "C" int acai_decode_slot_arm(const AcaiDecoder *d, const AcaiSlots *sl, const int32_t *rows, int n, void *stream) {
    int rc = check_slots(d, sl, "acai_decode_slot_arm");
    if (rc) return rc;
    ACAI_CHECK_ARG(n >= 0 && (n == 0 || rows), "acai_decode_slot_arm: bad row list (n=%d)", n);
    if (n > 0 && (rc = launch_slot_arm(d, sl, rows, n, (hipStream_t)stream))) return rc;
    x_valid_set(d, true);   // every armed row's x holds its first input; the caller keeps every other row finished or chained
    return 0;
}

extern "C" int acai_decode_slot_step(const AcaiDecoder *d, const AcaiSlots *sl, void *stream) {
    int rc = check_slots(d, sl, "acai_decode_slot_step");
    if (rc) return rc;
    if ((rc = check_x_valid(d, "acai_decode_slot_step", "acai_decode_slot_arm", "slot"))) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = decode(d, nullptr, st, false, true, nullptr, sl);
    if (rc) return rc;
    return launch_slot_argmax(d, sl, st);
}

extern "C" int acai_decode_slot_sample_step(const AcaiDecoder *d, const AcaiSlots *sl, const float *uniforms, int ld_uniforms,
                                            const int32_t *urow, int top_k, float temperature, void *stream) {
    int rc = check_slots(d, sl, "acai_decode_slot_sample_step");
    if (rc) return rc;
    if ((rc = check_draw(d, "acai_decode_slot_sample_step", uniforms, top_k, temperature, 1, ld_uniforms, urow))) return rc;
    if ((rc = check_x_valid(d, "acai_decode_slot_sample_step", "acai_decode_slot_arm", "slot"))) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = decode(d, nullptr, st, false, true, nullptr, sl);
    if (rc) return rc;
    return launch_slot_sample(d, sl, uniforms, ld_uniforms, urow, top_k, temperature, st);
}

// Prologue of the speculative entry points: the operands, the sequence state, the row layout (R = D + 1 rows per image sharing its cross
// K/V) and the speculative state.
static int check_spec(const AcaiDecoder *d, const AcaiSpec *sp, const char *fn) {
    int rc = check_unembed(d, fn);
    if (rc) return rc;
    ACAI_CHECK_ARG(d->seqs && d->logprobs && d->finished && d->max_len > 1 && d->max_len <= d->Tmax, "%s: null sequence state or max_len "
                   "outside [2, Tmax] (max_len=%d Tmax=%d)", fn, d->max_len, d->Tmax);
    ACAI_CHECK_ARG(sp && sp->t && sp->cap && sp->steps && sp->tab && sp->next, "%s: null speculative state", fn);
    ACAI_CHECK_ARG(sp->D >= 1 && sp->D <= 7, "%s: draft length %d outside [1, 7]", fn, sp->D);
    ACAI_CHECK_ARG(d->B % (sp->D + 1) == 0 && d->cross_group == sp->D + 1, "%s: needs B %% (D + 1) == 0 and cross_group == D + 1 (B=%d D=%d "
                   "cross_group=%d)", fn, d->B, sp->D, d->cross_group);
    ACAI_CHECK_ARG(!(d->flags & ACAI_DEC_CROSS_FP8), "%s: an FP8 cross K/V is not supported", fn);
    ACAI_CHECK_ARG(sp->rows >= d->B / (sp->D + 1) && sp->pitch >= d->max_len && sp->pitch <= d->Tmax, "%s: needs rows >= B / (D + 1) and "
                   "max_len <= pitch <= Tmax (rows=%d pitch=%d)", fn, sp->rows, sp->pitch);
    ACAI_CHECK_ARG(sp->drafts || (sp->ngram >= 1 && sp->ngram <= 8), "%s: without a drafts table ngram must be in [1, 8] (got %d)", fn, sp->ngram);
    ACAI_CHECK_ARG(d->self_chunk <= 16384, "%s: self_chunk %d above 16384", fn, d->self_chunk);
    return 0;
}

extern "C" int acai_decode_spec_arm(const AcaiDecoder *d, const AcaiSpec *sp, void *stream) {
    int rc = check_spec(d, sp, "acai_decode_spec_arm");
    if (rc) return rc;
    rc = launch_spec_accept(d, sp, 1, (hipStream_t)stream);
    if (rc) return rc;
    x_valid_set(d, true);
    return 0;
}

extern "C" int acai_decode_spec_step(const AcaiDecoder *d, const AcaiSpec *sp, void *stream) {
    int rc = check_spec(d, sp, "acai_decode_spec_step");
    if (rc) return rc;
    if ((rc = check_x_valid(d, "acai_decode_spec_step", "acai_decode_spec_arm", "speculative"))) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = decode(d, nullptr, st, false, true, nullptr, nullptr, sp);
    if (rc) return rc;
    return launch_spec_accept(d, sp, 0, st);
}

static int check_prompt(const AcaiDecoder *d, const AcaiPrompt *pr, int rows, const char *fn) {
    ACAI_CHECK_ARG(pr && pr->tok && pr->len, "%s: null prompt tables", fn);
    ACAI_CHECK_ARG(pr->pitch >= d->max_len && pr->rows >= rows, "%s: needs prompt pitch >= max_len and rows >= %d (pitch=%d max_len=%d rows=%d)",
                   fn, rows, pr->pitch, d->max_len, pr->rows);
    return 0;
}

extern "C" int acai_decode_prompt_step(const AcaiDecoder *d, const AcaiPrompt *prompt, void *stream) {
    const bool chained = d && d->E % 4 == 0;
    int rc = check_step(d, "acai_decode_prompt_step", chained);
    if (rc) return rc;
    if ((rc = check_prompt(d, prompt, d->B, "acai_decode_prompt_step"))) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = decode(d, nullptr, st, !chained);
    if (rc) return rc;
    return launch_prompt_logprob(d, prompt, chained, st);
}

extern "C" int acai_decode_spec_prompt_arm(const AcaiDecoder *d, const AcaiSpec *sp, const AcaiPrompt *prompt, void *stream) {
    int rc = check_spec(d, sp, "acai_decode_spec_prompt_arm");
    if (rc) return rc;
    if ((rc = check_prompt(d, prompt, d->B / (sp->D + 1), "acai_decode_spec_prompt_arm"))) return rc;
    rc = launch_spec_prompt_accept(d, sp, prompt, 1, (hipStream_t)stream);
    if (rc) return rc;
    x_valid_set(d, true);
    return 0;
}

extern "C" int acai_decode_spec_prompt_step(const AcaiDecoder *d, const AcaiSpec *sp, const AcaiPrompt *prompt, void *stream) {
    int rc = check_spec(d, sp, "acai_decode_spec_prompt_step");
    if (rc) return rc;
    if ((rc = check_prompt(d, prompt, d->B / (sp->D + 1), "acai_decode_spec_prompt_step"))) return rc;
    if ((rc = check_x_valid(d, "acai_decode_spec_prompt_step", "acai_decode_spec_prompt_arm", "speculative"))) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = decode(d, nullptr, st, false, true, nullptr, nullptr, sp);
    if (rc) return rc;
    return launch_spec_prompt_accept(d, sp, prompt, 0, st);
}

// Prologue of the two prompt-prefill entry points: the descriptor and the common depth C of the prompts.
static int check_prefill(const AcaiDecoder *d, int C, const char *fn) {
    int rc = check_decoder(d);
    if (rc) return rc;
    ACAI_CHECK_ARG(d->max_len > 1 && d->max_len <= d->Tmax, "%s: max_len outside [2, Tmax] (max_len=%d Tmax=%d)", fn, d->max_len, d->Tmax);
    ACAI_CHECK_ARG(C >= 1 && C <= d->max_len - 1, "%s: prefill depth C = %d outside [1, max_len - 1 = %d]", fn, C, d->max_len - 1);
    return 0;
}

extern "C" int acai_decode_prefill_self_kv(const AcaiDecoder *d, int layer, const void *qkv, int ld, int C, void *stream) {
    int rc = check_prefill(d, C, "acai_decode_prefill_self_kv");
    if (rc) return rc;
    ACAI_CHECK_ARG(qkv, "acai_decode_prefill_self_kv: null qkv");
    ACAI_CHECK_ARG(layer >= 0 && layer < d->L, "acai_decode_prefill_self_kv: layer %d outside [0, L = %d)", layer, d->L);
    ACAI_CHECK_ARG(ld >= 3 * d->E, "acai_decode_prefill_self_kv: ld = %d below 3E = %d", ld, 3 * d->E);
    ACAI_CHECK_ARG(d->layers[layer].k_self && d->layers[layer].v_self, "acai_decode_prefill_self_kv: null self K/V cache of layer %d", layer);
    return launch_prefill_self_kv(d, layer, qkv, ld, C, (hipStream_t)stream);
}

extern "C" int acai_decode_prefill_arm(const AcaiDecoder *d, const AcaiPrompt *prompt, const float *logits, int C, void *stream) {
    int rc = check_prefill(d, C, "acai_decode_prefill_arm");
    if (rc) return rc;
    ACAI_CHECK_ARG(logits, "acai_decode_prefill_arm: null logits");
    ACAI_CHECK_ARG(d->emb && d->pos && d->seqs && d->logprobs && d->finished, "acai_decode_prefill_arm: decoder has no embedding / sequence state");
    if ((rc = check_prompt(d, prompt, d->B, "acai_decode_prefill_arm"))) return rc;
    ACAI_CHECK_ARG(d->V <= 512, "acai_decode_prefill_arm: vocabulary %d above 512", d->V);
    if ((rc = launch_prefill_arm(d, prompt, logits, C, (hipStream_t)stream))) return rc;
    x_valid_set(d, true);   // x holds the input of step C + 1
    return 0;
}

// Prologue of the grammar-constrained steps, after the counterpart's own checks.
static int check_grammar(const AcaiDecoder *d, const AcaiGrammar *g, const char *fn) {
    ACAI_CHECK_ARG(g && g->next && g->resync && g->state, "%s: null grammar tables or state", fn);
    ACAI_CHECK_ARG(g->states >= 1 && g->states <= 32767, "%s: states %d outside [1, 32767]", fn, g->states);
    ACAI_CHECK_ARG(g->start >= 0 && g->start < g->states, "%s: start %d outside [0, states = %d)", fn, g->start, g->states);
    ACAI_CHECK_ARG(g->rows >= d->B, "%s: grammar rows %d below B = %d", fn, g->rows, d->B);
    ACAI_CHECK_ARG(d->V <= 512, "%s: vocabulary %d above 512", fn, d->V);
    return 0;
}

extern "C" int acai_decode_grammar_step(const AcaiDecoder *d, const AcaiGrammar *g, void *stream) {
    const bool chained = d && d->E % 4 == 0;
    int rc = check_step(d, "acai_decode_grammar_step", chained);
    if (rc) return rc;
    if ((rc = check_grammar(d, g, "acai_decode_grammar_step"))) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = decode(d, nullptr, st, !chained);
    if (rc) return rc;
    return launch_grammar_argmax(d, g, chained, st);
}

extern "C" int acai_decode_grammar_sample_step(const AcaiDecoder *d, const AcaiGrammar *g, const float *uniforms, int top_k, float temperature,
                                               void *stream) {
    const bool chained = d && d->E % 4 == 0;
    int rc = check_step(d, "acai_decode_grammar_sample_step", chained);
    if (rc) return rc;
    if ((rc = check_grammar(d, g, "acai_decode_grammar_sample_step"))) return rc;
    if ((rc = check_draw(d, "acai_decode_grammar_sample_step", uniforms, top_k, temperature))) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = decode(d, nullptr, st, !chained);
    if (rc) return rc;
    return launch_grammar_sample(d, g, uniforms, top_k, temperature, chained, st);
}

extern "C" int acai_decode_slot_grammar_step(const AcaiDecoder *d, const AcaiSlots *sl, const AcaiGrammar *g, void *stream) {
    int rc = check_slots(d, sl, "acai_decode_slot_grammar_step");
    if (rc) return rc;
    if ((rc = check_grammar(d, g, "acai_decode_slot_grammar_step"))) return rc;
    if ((rc = check_x_valid(d, "acai_decode_slot_grammar_step", "acai_decode_slot_arm", "slot"))) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = decode(d, nullptr, st, false, true, nullptr, sl);
    if (rc) return rc;
    return launch_slot_grammar_argmax(d, sl, g, st);
}

extern "C" int acai_decode_slot_grammar_sample_step(const AcaiDecoder *d, const AcaiSlots *sl, const AcaiGrammar *g, const float *uniforms,
                                                    int ld_uniforms, const int32_t *urow, int top_k, float temperature, void *stream) {
    int rc = check_slots(d, sl, "acai_decode_slot_grammar_sample_step");
    if (rc) return rc;
    if ((rc = check_grammar(d, g, "acai_decode_slot_grammar_sample_step"))) return rc;
    if ((rc = check_draw(d, "acai_decode_slot_grammar_sample_step", uniforms, top_k, temperature, 1, ld_uniforms, urow))) return rc;
    if ((rc = check_x_valid(d, "acai_decode_slot_grammar_sample_step", "acai_decode_slot_arm", "slot"))) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = decode(d, nullptr, st, false, true, nullptr, sl);
    if (rc) return rc;
    return launch_slot_grammar_sample(d, sl, g, uniforms, ld_uniforms, urow, top_k, temperature, st);
}

// Prologue of the loop-guard steps, after the counterpart's own checks (declared in decode_internal.h: acai_debug_decode_loop_select in
// decode_select.hip applies the same checks).
int check_loop(const AcaiDecoder *d, const AcaiLoop *loop, const char *fn) {
    ACAI_CHECK_ARG(loop && loop->run && loop->stop && loop->period && loop->start, "%s: null loop counters or report", fn);
    ACAI_CHECK_ARG(loop->rows >= d->B, "%s: loop rows %d below B = %d", fn, loop->rows, d->B);
    ACAI_CHECK_ARG(loop->max_period >= 1 && loop->max_period <= 64, "%s: max_period %d outside [1, 64]", fn, loop->max_period);
    ACAI_CHECK_ARG(loop->min_repeats >= 2, "%s: min_repeats %d below 2", fn, loop->min_repeats);
    ACAI_CHECK_ARG(loop->min_tokens >= 1, "%s: min_tokens %d below 1", fn, loop->min_tokens);
    return 0;
}

extern "C" int acai_decode_loop_step(const AcaiDecoder *d, const AcaiLoop *loop, void *stream) {
    const bool chained = d && d->E % 4 == 0;
    int rc = check_step(d, "acai_decode_loop_step", chained);
    if (rc) return rc;
    if ((rc = check_loop(d, loop, "acai_decode_loop_step"))) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = decode(d, nullptr, st, !chained);
    if (rc) return rc;
    return launch_loop_argmax(d, loop, chained, st);
}

extern "C" int acai_decode_slot_loop_step(const AcaiDecoder *d, const AcaiSlots *sl, const AcaiLoop *loop, void *stream) {
    int rc = check_slots(d, sl, "acai_decode_slot_loop_step");
    if (rc) return rc;
    if ((rc = check_loop(d, loop, "acai_decode_slot_loop_step"))) return rc;
    if ((rc = check_x_valid(d, "acai_decode_slot_loop_step", "acai_decode_slot_arm", "slot"))) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = decode(d, nullptr, st, false, true, nullptr, sl);
    if (rc) return rc;
    return launch_slot_loop_argmax(d, sl, loop, st);
}

extern "C" int acai_decode_logits(const AcaiDecoder *d, const int64_t *tokens, int time_step, void *stream) {
    int rc = check_unembed(d, "acai_decode_logits");
    if (rc) return rc;
    ACAI_CHECK_ARG(tokens && time_step >= 0 && time_step < d->Tmax, "acai_decode_logits: bad tokens / time_step %d", time_step);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = launch_set_step(d, time_step, st)) || (rc = decode(d, tokens, st))) return rc;
    if ((rc = launch_advance_cache(d, st))) return rc;
    x_valid_set(d, false);
    return 0;
}

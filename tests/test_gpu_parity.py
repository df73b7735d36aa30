"""Model-level parity on the GPU: the mirror modules (HIP path through the C ABI) against
  (1) the committed golden vectors produced by the imported reference (tests/golden/*.pt), and
  (2) the CPU oracle on seeded inputs at sizes it finishes in seconds.
Bars: fp32 path - bit-exact greedy token ids, logits within 1e-3;
      bf16 (autocast plumbing) path - token ids equal to the reference's bf16-autocast run on these fixtures,
      logits within bf16 resolution of the oracle's autocast restatement (same rounding points)."""
import os

import pytest
import torch
from torch.amp import autocast

from conftest import VOCAB, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from acai_omr_amd import _lib
    _lib.lib()
    return "cuda"


def md(a, b):
    return float((a.detach().float().cpu() - b.detach().float().cpu()).abs().max())


def build_vitomr(cfg, sd, dev, cache_dtype, max_batch=8):
    from acai_omr_amd.models.models import FineTuneOMREncoder, OMRDecoder, TeacherForcedViTOMR
    enc = FineTuneOMREncoder(cfg["P"], cfg["pe_h"], cfg["pe_w"], cfg["ft_depth"], num_layers=cfg["enc_layers"], hidden_dim=cfg["enc_dim"],
                             num_heads=cfg["enc_heads"], mlp_dim=cfg["enc_mlp"])
    dec = OMRDecoder(cfg["max_len"], VOCAB, num_layers=cfg["dec_layers"], hidden_dim=cfg["dec_dim"], num_heads=cfg["dec_heads"], mlp_dim=cfg["dec_mlp"])
    m = TeacherForcedViTOMR(enc, None, dec, transition_head_dim=cfg["head_dim"])
    m.load_state_dict(sd)
    if cache_dtype is not None:
        cached = m.decoder.to_cached_version(max_batch, cache_dtype)
        cached.load_state_dict(m.decoder.state_dict())
        m.decoder = cached
    return m.to(dev).eval()


@pytest.mark.parametrize("name", ["vitomr_small", "vitomr_dh64", "vitomr_dh64b", "vitomr_odd"])
def test_fp32_encoder_head_greedy_vs_reference_golden(dev, name):
    fx = load_golden(name)
    cfg, ref = fx["cfg"], fx["ref_fp32"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.float)
    with torch.no_grad():
        lat, mask = m.encoder(fx["imgs"])
        assert torch.equal(mask.cpu(), ref["latent_mask"])
        valid = ~ref["latent_mask"]
        assert md(lat.cpu()[valid], ref["latent"][valid]) < 1e-4
        if cfg["enc_heads"] % 2 == 0:
            assert md(lat, ref["latent"]) < 1e-4          # padded rows = final norm bias (eval fast path)
        mem = m.transition_head(lat)
        assert md(mem.cpu()[valid], ref["memory"][valid]) < 1e-4
        seqs, lps, smask = m.cached_greedy_generate(mem, mask, max_len=cfg["gen_len"])
    assert torch.equal(seqs.cpu(), ref["seqs"])            # bit-exact token ids
    assert torch.equal(smask.cpu(), ref["seq_mask"])
    assert md(lps, ref["log_probs"]) < 1e-3
    # per-step logits through OMRDecoder.cached_generate, fed with the reference's own tokens
    with torch.no_grad():
        m.decoder.prepare_caches(mem)
        T = ref["step_logits"].shape[1]
        full = torch.full((len(fx["imgs"]), cfg["gen_len"]), 1, dtype=torch.long)
        full[:, :ref["seqs"].shape[1]] = ref["seqs"]
        for t in range(1, T + 1):
            lg = m.decoder.cached_generate(full[:, t - 1:t].to(dev), t, mask)
            assert md(lg.squeeze(1), ref["step_logits"][:, t - 1]) < 1e-3, t


@pytest.mark.parametrize("name", ["vitomr_small", "vitomr_dh64", "vitomr_dh64b", "vitomr_odd"])
def test_bf16_inference_entry_point_vs_reference_and_oracle(dev, name):
    from acai_omr_amd.inference.vitomr_inference import inference
    from oracle import vitomr_oracle as O
    fx = load_golden(name)
    cfg, ref, sd = fx["cfg"], fx["ref_bf16"], fx["state_dict"]
    m = build_vitomr(cfg, sd, dev, torch.bfloat16)
    seqs, lps, smask = inference(m, fx["imgs"], dev, max_inference_len=cfg["gen_len"])
    oseqs, olps, omask = O.vitomr_inference(fx["imgs"], sd, cfg["enc_heads"], cfg["dec_heads"], cfg["P"], cfg["gen_len"])
    assert torch.equal(seqs.cpu(), oseqs) and torch.equal(smask.cpu(), omask)     # HIP == oracle, token for token
    assert torch.equal(seqs.cpu(), ref["seqs"]) and torch.equal(smask.cpu(), ref["seq_mask"])  # == reference under autocast
    assert md(lps, olps) < 0.07 and md(lps, ref["log_probs"]) < 0.13
    # API-level path (padded tensors + masks, as the reference's inference() is written) gives the same tokens
    with torch.no_grad():
        lat, mask = m.encoder(fx["imgs"])
        with autocast(device_type="cuda", dtype=torch.bfloat16):
            mem = m.transition_head(lat)
            assert mem.dtype == torch.bfloat16
            s2, l2, m2 = m.cached_greedy_generate(mem, mask, max_len=cfg["gen_len"])
    assert torch.equal(s2, seqs) and torch.equal(m2, smask)


def test_omr_encoder_interpolation_and_errors(dev):
    from acai_omr_amd.models.models import Encoder, OMREncoder
    fx = load_golden("omr_encoder_interp")
    enc = OMREncoder(4, 6, 10, num_layers=2, hidden_dim=32, num_heads=2, mlp_dim=64)
    enc.load_state_dict(fx["state_dict"])
    enc = enc.to(dev).eval()
    with torch.no_grad():
        lat, mask = enc(fx["imgs"])
    assert torch.equal(mask.cpu(), fx["mask"])
    assert md(lat, fx["latent"]) < 1e-4
    base = Encoder(4, 6, 10, num_layers=1, hidden_dim=32, num_heads=2, mlp_dim=64).to(dev).eval()
    with pytest.raises(ValueError) as e:
        with torch.no_grad():
            base([torch.rand(1, 28, 44)])
    assert str(e.value) == fx["too_large_msg"]
    # reference KAT tests/test_mae.py:8-24 (identity projection, ones PE)
    from torch import nn
    enc2 = Encoder(2, 60, 200, hidden_dim=4, num_heads=1).to(dev).eval()
    with torch.no_grad():
        enc2.projection.weight.copy_(torch.eye(4))
        enc2.projection.bias.zero_()
        enc2.pos_embedding = nn.Parameter(torch.ones(50, 50, 4, device=dev))
        enc2.pe_max_height, enc2.pe_max_width = 50, 50
        emb, mask = enc2.batchify([torch.ones(1, 4, 4), torch.ones(1, 4, 8)])
    exp = torch.cat([torch.cat([torch.ones(1, 4, 4) + 1, torch.zeros(1, 4, 4)], 1), torch.ones(1, 8, 4) + 1])
    assert torch.equal(emb.cpu(), exp)
    assert torch.equal(mask.cpu(), torch.stack([torch.arange(8) >= 4, torch.arange(8) >= 8]))


def test_teacher_forced_forward_eval_vs_golden(dev):
    """TeacherForcedViTOMR.forward in eval / no_grad (forward_eval, models.py:837-838) against the reference's logits."""
    for name in ("tf_small", "tf_dh64"):
        fx = load_golden(name)
        cfg = fx["cfg"]
        m = build_vitomr(cfg, fx["state_dict"], dev, None)
        with torch.no_grad():
            pred, tgt = m(list(zip(fx["imgs"], fx["lmx"])))
        assert torch.equal(tgt.cpu(), fx["target"])
        valid = fx["target"] != 1
        assert md(pred.cpu()[valid], fx["pred"][valid]) < 1e-3


# ---- tests written like the reference's tests/test_kv_caching.py: cached path == stock torch modules ------------------
def test_cached_mha_like_reference(dev):
    from torch import nn
    from acai_omr_amd.models.kv_caching import CachedMultiheadAttention, KVCache
    torch.manual_seed(0)
    head_dim, num_heads = 6, 2
    E = head_dim * num_heads
    uncached = nn.MultiheadAttention(E, num_heads, dropout=0.1, batch_first=True).eval()
    cached = CachedMultiheadAttention(E, num_heads, dropout=0.1, batch_first=True)
    cached.load_state_dict(uncached.state_dict())
    cached = cached.to(dev).eval()
    B, T = 2, 3
    cache = KVCache(B, T, num_heads, head_dim, dtype=torch.float)
    full = torch.empty(B, T, E)
    out = torch.empty(B, T, E)
    for t in range(T):
        tok = torch.rand(B, 1, E)
        full[:, t] = tok.squeeze(1)
        qkv = torch.nn.functional.linear(tok, uncached.in_proj_weight, uncached.in_proj_bias)
        q, k, v = (x.view(B, num_heads, 1, head_dim).to(dev) for x in qkv.chunk(3, dim=-1))
        K, V = cache.update(k, v)
        out[:, t] = cached.cached_forward(q, K, V).squeeze(1).cpu()
    causal = torch.triu(torch.ones(T, T), diagonal=1).bool()
    with torch.no_grad():
        ref = uncached(full, full, full, attn_mask=causal)[0]
    assert torch.allclose(out, ref, atol=2e-5)
    with pytest.raises(AssertionError):
        cache.update(k, v)  # overflow
    cache.reset()
    assert cache.size == 0


def test_cached_transformer_decoder_like_reference(dev):
    from torch import nn
    from acai_omr_amd.models.kv_caching import CachedTransformerDecoder, CachedTransformerDecoderLayer
    torch.manual_seed(1)
    E, H = 12, 2
    kw = dict(d_model=E, nhead=H, dim_feedforward=48, dropout=0.1, activation="gelu", batch_first=True)
    uncached = nn.TransformerDecoder(nn.TransformerDecoderLayer(**kw), num_layers=3, norm=nn.LayerNorm(E, eps=1e-6)).eval()
    B, Tmax, S = 4, 200, 8
    cached = CachedTransformerDecoder(CachedTransformerDecoderLayer(**kw), num_layers=3, max_batch_size=B, max_decoder_seq_len=Tmax,
                                      cache_dtype=torch.float, norm=nn.LayerNorm(E, eps=1e-6))
    cached.load_state_dict(uncached.state_dict())
    cached = cached.to(dev).eval()
    for bs, masks in ((4, None), (4, {1: 3, 2: 6, 3: 6}), (3, {0: 3, 2: 6})):
        latent = torch.rand(bs, S, E)
        mask = None
        if masks:
            mask = torch.full([bs, S], False)
            for b, s in masks.items():
                mask[b, s:] = True
        cached.prepare_caches(latent.to(dev))
        full = torch.empty(bs, 3, E)
        out = torch.empty(bs, 3, E)
        for t in range(3):
            tok = torch.rand(bs, 1, E)
            full[:, t] = tok.squeeze(1)
            out[:, t] = cached.cached_generate(tok.to(dev), memory_key_padding_mask=None if mask is None else mask.to(dev)).squeeze(1).cpu()
        causal = torch.triu(torch.ones(3, 3), diagonal=1).bool()
        with torch.no_grad():
            ref = uncached(full, memory=latent, tgt_mask=causal, memory_key_padding_mask=mask)
        assert torch.allclose(out, ref, atol=2e-5, rtol=1e-5)
    # layer-level API path (one launch per op) agrees with the fused step
    layer, cache = cached.layers[0], cached.self_attn_caches[0]
    cache.reset()
    mc = cached.cross_attn_caches[0]
    latent = torch.rand(2, S, E).to(dev)
    mc.cache_memory_keys_and_vals(latent, layer)
    tok = torch.rand(2, 1, E)
    y = layer.cached_forward(tok.to(dev), cache, mc.get_cached_keys_and_vals())
    with torch.no_grad():
        ref = uncached.layers[0](tok, latent.cpu())
    assert torch.allclose(y.cpu(), ref, atol=2e-5)


def test_omr_decoder_with_caching_like_reference(dev):
    from acai_omr_amd.models.models import OMRDecoder
    torch.manual_seed(2)
    kw = dict(max_lmx_seq_len=15, lmx_vocab_path=VOCAB, num_layers=5, hidden_dim=24, num_heads=4, mlp_dim=48)
    uncached = OMRDecoder(**kw).to(dev).eval()
    B = 8
    cached = OMRDecoder(**kw, use_caching=True, max_batch_size=B, cache_dtype=torch.float)
    cached.load_state_dict(uncached.state_dict())
    cached = cached.to(dev).eval()
    S = 20
    latent = torch.rand(B, S, 24).to(dev)
    mask = torch.full([B, S], False)
    mask[0, 16:] = True
    mask[2, 13:] = True
    mask[3, 14:] = True
    mask = mask.to(dev)
    T = 10
    full = torch.empty(B, T, dtype=torch.long)
    out = torch.empty(B, T, cached.vocab_size)
    cached.prepare_caches(latent)
    for t in range(T):
        tok = torch.randint(0, cached.vocab_size, [B, 1])
        full[:, t] = tok.squeeze(1)
        out[:, t] = cached.cached_generate(tok.to(dev), t, latent_attention_mask=mask).squeeze(1).cpu()
    with torch.no_grad():
        ref = uncached.generate(full.to(dev), latent, latent_attention_mask=mask).cpu()   # uncached teacher-forced path (HIP as well)
    assert torch.allclose(out, ref, atol=1e-4, rtol=1e-4)
    # against the oracle too (independent CPU math)
    from oracle import vitomr_oracle as O
    sd = {"decoder." + k: v.cpu() for k, v in uncached.state_dict().items()}
    lens_s = (~mask).sum(1).tolist()
    mem = torch.cat([latent[b, :l].cpu() for b, l in enumerate(lens_s)])
    o = O.decoder_forward_tf(full.reshape(-1), mem, [T] * B, lens_s, sd, 4, "fp32").reshape(B, T, -1)
    assert torch.allclose(out, o, atol=1e-4, rtol=1e-4)
    # overflow: 16 steps into a 15-long decoder
    cached.prepare_caches(latent)
    with pytest.raises(RuntimeError):
        for t in range(16):
            cached.cached_generate(torch.randint(0, cached.vocab_size, [B, 1]).to(dev), t, latent_attention_mask=mask)
    with pytest.raises(RuntimeError):
        uncached.prepare_caches(latent)


def test_greedy_early_exit_and_masking(dev):
    """Rows that emit <eos> keep generating junk that is masked afterwards (models.py:585-596); the loop stops once every
    row has finished.  Force <eos> by biasing the unembed."""
    fx = load_golden("vitomr_small")
    cfg = fx["cfg"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.float)
    with torch.no_grad():
        m.decoder.unembed.bias[2] += 100.0
        lat, mask = m.encoder(fx["imgs"])
        mem = m.transition_head(lat)
        seqs, lps, smask = m.cached_greedy_generate(mem, mask, max_len=20)
    assert seqs.shape == (3, 2) and seqs[:, 1].tolist() == [2, 2, 2] and bool(smask.all())
    assert m.create_inference_mask(torch.tensor([[0, 2, 10, 2], [0, 20, 20, 2]])).int().tolist() == [[1, 1, 0, 0], [1, 1, 1, 1]]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_full_size_decoder_ragged_batch_vs_oracle(dev, prec):
    """The full-size LMX decoder (12 layers, d=1024, 16 heads, mlp 4096, V=227: the fused bf16 step with LayerNorm-on-load GEMVs,
    K=4096 GEMV, split cross-attention with in-launch merge) on a ragged batch of memories, against the CPU oracle on the same
    seeded weights: greedy token ids and log-probs over a few steps."""
    from acai_omr_amd.models.models import OMRDecoder, ViTOMR
    from oracle import vitomr_oracle as O
    torch.manual_seed(3)
    dec = OMRDecoder(64, VOCAB, num_layers=12)
    with torch.no_grad():
        for n, p in dec.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
        dec.unembed.weight.mul_(6.0)
    cdt = torch.bfloat16 if prec == "bf16" else torch.float
    cached = dec.to_cached_version(4, cdt)
    cached.load_state_dict(dec.state_dict())
    model = ViTOMR(None, None, cached.to(dev).eval())
    lens = [700, 1300, 64]
    g = torch.Generator().manual_seed(4)
    mem = torch.randn(sum(lens), 1024, generator=g)
    if prec == "bf16":
        mem = O.rbf16(mem)
    steps = 7
    sd = {"decoder." + k: v for k, v in dec.state_dict().items()}
    oseqs, olps, omask, ologits = O.greedy_generate(mem, lens, sd, 16, prec, steps, return_logits=True)
    with torch.no_grad():
        md_ = mem.to(dev)
        seqs, lps, mask = model._greedy_packed(None if prec == "bf16" else md_, md_.to(torch.bfloat16) if prec == "bf16" else None, lens, steps)
    top2 = ologits.topk(2, dim=-1).values
    margin = (top2[..., 0] - top2[..., 1])  # (B, steps-1): the oracle's own top-2 margin per generated token
    if prec == "fp32":
        assert torch.equal(seqs.cpu(), oseqs)
        assert md(lps, olps) < 1e-3
    else:
        same = seqs.cpu()[:, 1:oseqs.shape[1]] == oseqs[:, 1:]
        # a token may only differ where the oracle itself was within bf16 resolution of a tie, and everything after it may differ
        for b in range(len(lens)):
            bad = (~same[b]).nonzero()
            if len(bad):
                first = int(bad[0])
                assert float(margin[b, first]) <= 0.13, (b, first, float(margin[b, first]))
        assert same.float().mean() > 0.8


def test_streamed_inference_events_match_batch_inference(dev):
    """streamed_inference (vitomr_inference.py:51-70 / models.py:625-647): event order, STEP payloads every flush_interval tokens,
    final sequence identical to inference(); single image only."""
    from acai_omr_amd.config import InferenceEvent
    from acai_omr_amd.inference.vitomr_inference import inference, streamed_inference
    fx = load_golden("vitomr_dh64")
    cfg = fx["cfg"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.bfloat16)
    img = fx["imgs"][1]
    seqs, lps, mask = inference(m, img, dev, max_inference_len=cfg["gen_len"])
    events = list(streamed_inference(img, m, dev, max_inference_len=cfg["gen_len"], flush_interval=3))
    kinds = [e["type"] for e in events]
    assert kinds[0] == InferenceEvent.ENCODING_START.value and kinds[1] == InferenceEvent.ENCODING_FINISH.value
    assert kinds[-1] == InferenceEvent.INFERENCE_FINISH.value and set(kinds[2:-1]) <= {InferenceEvent.STEP.value}
    fin = events[-1]["payload"]
    assert torch.equal(fin["sequence"], seqs) and torch.equal(fin["mask"], mask)
    steps = [e["payload"]["tokens"] for e in events if e["type"] == InferenceEvent.STEP.value]
    assert len(steps) >= 2 and all(t.shape == (1, 3) and t.dtype == torch.int for t in steps)
    streamed = torch.cat(steps, dim=1).long()
    assert torch.equal(streamed[0], seqs[0, 1:1 + streamed.shape[1]])
    with pytest.raises(ValueError):
        with torch.no_grad():
            lat, msk = m.encoder(fx["imgs"])
            list(m.streamed_cached_greedy_generate(m.transition_head(lat), msk))


@pytest.mark.parametrize("name", ["vitomr_small", "vitomr_dh64"])
@pytest.mark.parametrize("cache_dtype", [torch.float, torch.bfloat16])
def test_grpo_rollout_policy_sampling(dev, cache_dtype, name):
    """GRPOViTOMR.cached_forward_rollout_policy (models.py:988-1049) on the graph-replayed sampling step: every drawn token and log-prob
    equals the oracle's restatement of the step (top-k, temperature softmax, inverse-CDF draw, un-tempered log-softmax) applied to the
    per-step logits of the already reference-checked cached_generate path with the same uniforms; top_k = 1 degenerates to the greedy
    decode; rollouts that share one image's cross K/V (group_size) equal the materialised-copies form; draws follow the softmax."""
    import oracle.vitomr_oracle as O
    from acai_omr_amd import engine as EG
    from acai_omr_amd.models.models import GRPOViTOMR, OMREncoder
    fx = load_golden(name)
    cfg = fx["cfg"]
    base = build_vitomr(cfg, fx["state_dict"], dev, cache_dtype, max_batch=32)
    g = GRPOViTOMR(base.encoder, base.transition_head, base.decoder, base.state_dict()).to(dev).eval()
    assert isinstance(g.encoder, OMREncoder) and not any(p.requires_grad for p in g.encoder.parameters())
    assert all(p.requires_grad for p in g.decoder.parameters())
    bf = cache_dtype == torch.bfloat16
    G, T = 3, cfg["gen_len"]
    with torch.no_grad():
        lat0, mask0 = base.encoder(fx["imgs"])
        lat, mask = g.encoder(fx["imgs"])
        assert md(lat, lat0) < 1e-5 and torch.equal(mask, mask0)       # frozen/fine-tune stacks merged into one encoder stack
        mem = g.transition_head(lat)
        mem_x, mask_x = g.expand_img_latent_for_rollout(mem, mask, G)
        R = mem_x.shape[0]
        u = torch.rand(R, T, generator=torch.Generator().manual_seed(7))
        from torch.amp import autocast
        with autocast(device_type="cuda", dtype=torch.bfloat16, enabled=bf):
            r_flat = g.cached_forward_rollout_policy(mem_x, mask_x, max_actions=T, top_k=50, temperature=1.2, uniforms=u)
            r_grp = g.cached_forward_rollout_policy(mem_x, mask_x, max_actions=T, top_k=50, temperature=1.2, uniforms=u, group_size=G)
        # Grouped rollouts: rows of an image share its stored K/V; for bf16 / d_h = 64 the matrix-core group kernel also replaces the per-row
        # kernel, so logits may differ from the copies form by a bf16 ulp and a draw may legitimately fall on the other side of a CDF step.
        # Each form is therefore checked against the oracle on ITS OWN per-step logits (below); here: same shape, mostly the same draws.
        assert r_flat[0].shape[0] == r_grp[0].shape[0]
        n = min(r_flat[0].shape[1], r_grp[0].shape[1])
        assert float((r_flat[0][:, 1] == r_grp[0][:, 1]).float().mean()) >= 0.5 and n >= 2
        blocks = g.decoder.decoder_blocks
        mem32, lens = EG.unpad_rows(mem, mask)
        with autocast(device_type="cuda", dtype=torch.bfloat16, enabled=bf):
            blocks.prepare_caches_packed(mem32, None, lens, group_size=G)
            eng = blocks.engine(mem32.device)
            ro_g, lp_g, mk_g = (t.cpu() for t in r_grp)
            for t in range(1, ro_g.shape[1]):
                lg = eng.logits_step(ro_g[:, t - 1].to(dev), t)
                tok, lp = O.rollout_sample_step(lg.float().cpu(), u[:, t], 50, 1.2, round_lp=bf)
                live = mk_g[:, t]
                assert torch.equal(tok[live], ro_g[live, t]), t
                assert md(lp[live], lp_g[live, t]) < (2e-2 if bf else 1e-5), t
        rollouts, lps, rmask = (t.cpu() for t in r_flat)
        assert rollouts.shape[0] == R and rollouts.dtype == torch.int64 and torch.equal(rollouts[:, 0], torch.zeros(R, dtype=torch.long))
        assert bool((rollouts[~rmask] == 1).all()) and bool((lps[~rmask] == 0).all())
        # replay the drawn tokens through cached_generate and restate every draw with the oracle
        with autocast(device_type="cuda", dtype=torch.bfloat16, enabled=bf):
            g.decoder.prepare_caches(mem_x)
            checked = 0
            for t in range(1, rollouts.shape[1]):
                lg = g.decoder.cached_generate(rollouts[:, t - 1:t].to(dev), t, mask_x).squeeze(1)
                tok, lp = O.rollout_sample_step(lg.float().cpu(), u[:, t], 50, 1.2, round_lp=bf)
                live = rmask[:, t]
                assert torch.equal(tok[live], rollouts[live, t]), t
                assert md(lp[live], lps[live, t]) < (2e-2 if bf else 1e-5), t
                checked += int(live.sum())
        assert checked > R
        # more rows than one matrix-core tile holds (16): 20 rollouts of every image, grouped (two tiles per image) against materialised copies
        if bf:
            mem20, mask20 = g.expand_img_latent_for_rollout(mem[:1], mask[:1], 20)
            u20 = torch.rand(20, T, generator=torch.Generator().manual_seed(8))
            with autocast(device_type="cuda", dtype=torch.bfloat16):
                f20 = g.cached_forward_rollout_policy(mem20, mask20, max_actions=T, top_k=50, temperature=1.2, uniforms=u20)
                g20 = g.cached_forward_rollout_policy(mem20, mask20, max_actions=T, top_k=50, temperature=1.2, uniforms=u20, group_size=20)
            assert f20[0].shape[0] == g20[0].shape[0] == 20 and float((f20[0][:, 1] == g20[0][:, 1]).float().mean()) >= 0.5
            blocks.prepare_caches_packed(mem32[:lens[0]], None, lens[:1], group_size=20)
            eng = blocks.engine(mem32.device)
            for t in range(1, g20[0].shape[1]):
                lg = eng.logits_step(g20[0][:, t - 1], t)
                tok, _ = O.rollout_sample_step(lg.float().cpu(), u20[:, t], 50, 1.2, round_lp=True)
                live = g20[2][:, t].cpu()
                assert torch.equal(tok[live], g20[0].cpu()[live, t]), t
        # top_k = 1: the greedy decode, log-prob log_softmax over one kept logit = 0
        with autocast(device_type="cuda", dtype=torch.bfloat16, enabled=bf):
            seqs, _, smask = g.cached_greedy_generate(mem, mask, max_len=T)
            r1, lp1, m1 = g.cached_forward_rollout_policy(mem, mask, max_actions=T, top_k=1, temperature=0.7)
        assert torch.equal(r1, seqs) and torch.equal(m1, smask) and float(lp1.abs().max()) == 0.0
        # the draw follows softmax(top_k / temperature): 32 rollouts of image 0, first step, a few hundred draws
        if not bf:
            torch.manual_seed(0)
            m1x, k1x = g.expand_img_latent_for_rollout(mem[:1], mask[:1], 32)
            counts = torch.zeros(len(VOCAB_LIST := open(VOCAB).read().split()), dtype=torch.float64)
            for _ in range(12):
                ro, _, _ = g.cached_forward_rollout_policy(m1x, k1x, max_actions=2, top_k=5, temperature=1.0, group_size=32)
                counts += torch.bincount(ro[:, 1].cpu(), minlength=counts.numel()).double()
            g.decoder.prepare_caches(mem[:1])
            lg = g.decoder.cached_generate(torch.zeros(1, 1, dtype=torch.long, device=dev), 1, mask[:1]).squeeze(1).float().cpu()[0]
            top = torch.topk(lg, 5)
            probs = torch.zeros_like(counts)
            probs[top.indices] = torch.softmax(top.values.double(), 0)
            assert float((counts / counts.sum() - probs).abs().max()) < 0.12 and float(counts[probs == 0].sum()) == 0


def test_full_size_encoder_and_head_vs_oracle(dev):
    """The FULL-SIZE encoder (768 x 12 heads x 12 layers, 60 x 200 PE grid) and transition head on a ragged pair of systems, fp32 as
    `inference()` runs them (vitomr_inference.py:63,81), against the CPU oracle: the fixtures use reduced widths."""
    import oracle.vitomr_oracle as O
    from acai_omr_amd.config import ENCODER_FINE_TUNE_DEPTH, MAX_LMX_SEQ_LEN, NUM_DECODER_LAYERS, PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH
    from acai_omr_amd.models.models import FineTuneOMREncoder, OMRDecoder, TeacherForcedViTOMR
    torch.manual_seed(1)
    enc = FineTuneOMREncoder(PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH, ENCODER_FINE_TUNE_DEPTH)
    dec = OMRDecoder(MAX_LMX_SEQ_LEN, VOCAB, num_layers=NUM_DECODER_LAYERS)
    m = TeacherForcedViTOMR(enc, None, dec)
    g = torch.Generator().manual_seed(2)
    imgs = [torch.rand(1, 256, 1024, generator=g), torch.rand(1, 128, 640, generator=g)]
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    torch.set_num_threads(8)
    lat_o, lens = O.encoder_forward(imgs, sd, "encoder.", PATCH_SIZE, 12, "omr_ft", "fp32")
    mem_o = O.transition_head(lat_o, sd, "fp32")
    m = m.to(dev).eval()
    with torch.no_grad():
        lat, mask = m.encoder([im.to(dev) for im in imgs])
        mem = m.transition_head(lat)
    assert (~mask).sum(1).tolist() == lens
    o = 0
    for b, n in enumerate(lens):
        assert md(lat[b, :n], lat_o[o:o + n]) < 1e-3, b
        assert md(mem[b, :n], mem_o[o:o + n]) < 1e-3, b
        o += n


def test_full_length_decode_to_the_cache_limit_vs_oracle(dev):
    """Full-size decoder, fp32, greedy to the LAST position of the 1536-token self-attention cache (1535 graph-replayed steps, cache
    appends up to T_max - 1, positional rows up to 1535): token ids against the CPU oracle; a difference is only tolerated where the
    oracle's own top-2 margin is below fp32 accumulation noise, and one more step must be refused as the reference refuses it."""
    from acai_omr_amd.models.models import OMRDecoder, ViTOMR
    from oracle import vitomr_oracle as O
    torch.manual_seed(11)
    T = 1536
    dec = OMRDecoder(T, VOCAB, num_layers=12)
    with torch.no_grad():
        for n, p in dec.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
        dec.unembed.weight.mul_(6.0)
        dec.unembed.bias[2] = -1.0e4      # never <eos>: the loop must run to the cache limit
    cached = dec.to_cached_version(2, torch.float)
    cached.load_state_dict(dec.state_dict())
    model = ViTOMR(None, None, cached.to(dev).eval())
    lens = [96, 40]
    mem = torch.randn(sum(lens), 1024, generator=torch.Generator().manual_seed(12))
    sd = {"decoder." + k: v for k, v in dec.state_dict().items()}
    torch.set_num_threads(16)
    oseqs, olps, omask, ologits = O.greedy_generate(mem, lens, sd, 16, "fp32", T, return_logits=True)
    with torch.no_grad():
        seqs, lps, mask = model._greedy_packed(mem.to(dev), None, lens, T)
    assert seqs.shape == (2, T) and bool(mask.all())
    same = seqs.cpu() == oseqs
    top2 = ologits.topk(2, dim=-1).values
    margin = top2[..., 0] - top2[..., 1]
    for b in range(2):
        bad = (~same[b]).nonzero()
        if len(bad):
            first = int(bad[0])
            assert float(margin[b, first - 1]) < 2e-3, (b, first, float(margin[b, first - 1]))
    assert float(same.float().mean()) > 0.5
    eq = same.all(dim=1)
    assert md(lps[eq], olps[eq]) < 2e-3
    with pytest.raises(RuntimeError):
        model._greedy_packed(mem.to(dev), None, lens, T + 1)


def test_decode_is_deterministic_run_to_run(dev):
    """Two graph-replayed greedy decodes of the same ragged batch give bit-identical ids and log-probs: the in-launch split merge (whichever
    workgroup arrives last merges) and the device-side loop state leave no run-to-run freedom (tools/soak_decode.py is the long form)."""
    from acai_omr_amd.models.models import OMRDecoder, ViTOMR
    torch.manual_seed(21)
    dec = OMRDecoder(128, VOCAB, num_layers=4)
    cached = dec.to_cached_version(4, torch.bfloat16)
    cached.load_state_dict(dec.state_dict())
    model = ViTOMR(None, None, cached.to(dev).eval())
    lens = [2100, 1300, 3000]
    mem = torch.randn(sum(lens), 1024, generator=torch.Generator().manual_seed(22)).to(dev).to(torch.bfloat16)
    outs = []
    with torch.no_grad():
        for _ in range(3):
            seqs, lps, mask = model._greedy_packed(None, mem, lens, 96)
            outs.append((seqs.clone(), lps.clone()))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])


def test_decode_split_merge_runs_in_launch_on_this_toolchain(dev):
    """The headline decode step merges its attention splits inside the attention launches (decode_attn.hip, last-arriver hand-off) only at the
    workgroup residency it was validated at; otherwise it silently takes a separate combine launch (12 more launches per step: 0.712 against
    0.689 ms - round 4 shipped that way for a while because the check compared the occupancy API's answer with the wrong number).  On this
    pool's toolchain the validated path must be the one in use; a red test here after a ROCm upgrade means: re-run the determinism test and
    tools/soak_decode.py at the new residency (ACAI_DATTN_MERGE=1), then update dattn_merge_validated()."""
    from acai_omr_amd import _lib
    if os.environ.get("ACAI_DATTN_MERGE") is not None:
        pytest.skip("path forced by ACAI_DATTN_MERGE")
    assert _lib.lib().acai_decode_merge_in_launch(_lib.ACAI_BF16, 64) == 1
    assert _lib.lib().acai_decode_merge_in_launch(_lib.ACAI_BF16, 3) < 0      # argument check (dhp must be a power of two)


def test_full_size_batch_independence_of_decode(dev):
    """Size-independent property at the BASELINE configuration (8 sequences, 4096-patch memories, full-size decoder): a sequence decoded inside
    the batch of 8 gets the tokens and log-probs it gets when decoded alone (fp32 path: different cross-attention split counts and GEMV batch
    tiles may only move results by rounding noise)."""
    from acai_omr_amd.models.models import OMRDecoder, ViTOMR
    torch.manual_seed(13)
    dec = OMRDecoder(96, VOCAB, num_layers=12)
    with torch.no_grad():
        for n, p in dec.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
        dec.unembed.weight.mul_(6.0)
    cached = dec.to_cached_version(8, torch.float)
    cached.load_state_dict(dec.state_dict())
    model = ViTOMR(None, None, cached.to(dev).eval())
    S, steps = 4096, 40
    g = torch.Generator().manual_seed(14)
    mem = torch.randn(8 * S, 1024, generator=g).to(dev)
    with torch.no_grad():
        seqs, lps, mask = model._greedy_packed(mem, None, [S] * 8, steps)
        for b in (0, 5):
            s1, l1, m1 = model._greedy_packed(mem[b * S:(b + 1) * S].contiguous(), None, [S], steps)
            n = s1.shape[1]
            assert seqs.shape[1] >= n and torch.equal(s1[0], seqs[b, :n])   # the batch result is clipped to the longest row, hence >= n
            assert (l1[0] - lps[b, :n]).abs().max() < 1e-4


def test_full_size_batch_independence_of_mae(dev):
    """The same property for the full-size MAE on 512 x 2048 images (BASELINE configuration 2): an image's predictions, loss mask and targets
    do not depend on what else is in the ragged batch (same masking noise)."""
    from acai_omr_amd.config import MASK_RATIO, PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH
    from acai_omr_amd.models.models import MAE
    torch.manual_seed(15)
    mae = MAE(MASK_RATIO, PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH).to(dev).eval()
    g = torch.Generator().manual_seed(16)
    imgs = [torch.rand(1, 512, 2048, generator=g).to(dev), torch.rand(1, 256, 1024, generator=g).to(dev), torch.rand(1, 512, 2048, generator=g).to(dev)]
    noises = [torch.rand((im.shape[-2] // PATCH_SIZE) * (im.shape[-1] // PATCH_SIZE), generator=g) for im in imgs]
    with torch.no_grad():
        pred, lm, tgt = mae([(im, im) for im in imgs], noises=noises)
        for b in (0, 1):
            p1, lm1, t1 = mae([(imgs[b], imgs[b])], noises=[noises[b]])
            n = p1.shape[1]
            assert torch.equal(lm1[0], lm[b, :n]) and torch.equal(t1[0], tgt[b, :n])
            assert (p1[0] - pred[b, :n]).abs().max() < 2e-4


def test_chained_steps_after_a_stepwise_call_reembed_their_input(dev):
    """acai_decode_step takes its input from dec->x (written by the previous step's argmax kernel); the stepwise entry point
    (OMRDecoder.cached_generate -> acai_decode_logits) overwrites dec->x.  Mixing them must not decode from a stale input: the engine re-embeds
    from the device-side sequence state.  Greedy decode of the first tokens == decode where one step is taken through cached_generate."""
    fx = load_golden("vitomr_small")
    cfg = fx["cfg"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.float)
    with torch.no_grad():
        lat, mask = m.encoder(fx["imgs"])
        mem = m.transition_head(lat)
        ref, _, _ = m.cached_greedy_generate(mem, mask, max_len=cfg["gen_len"])
        # same decode, driven by hand: arm, 3 chained steps, one stepwise call (which overwrites dec->x), then chained steps again
        blocks = m.decoder.decoder_blocks
        from acai_omr_amd import engine as EG
        packed, lens = EG.unpad_rows(mem, mask)
        blocks.prepare_caches_packed(packed, None, lens)
        eng = blocks.engine(packed.device)
        with torch.cuda.stream(eng.stream):
            eng.arm(eng.B)
            eng.launch_steps(3, use_graph=False)
            torch.cuda.synchronize()
            eng.ws["x"].fill_(123.0)          # what a stepwise call leaves behind: someone else's input
            eng._x_valid = False
            eng.launch_steps(cfg["gen_len"] - 1 - 3, use_graph=False)
            torch.cuda.synchronize()
        got = eng.seqs[:eng.B, :cfg["gen_len"]].clone()
    n = ref.shape[1]
    live = m.create_inference_mask(got)[:, :n]
    assert torch.equal(got[:, :n].masked_fill(~live, m.decoder.pad_idx).cpu(), ref.cpu())


def test_c_abi_refuses_a_chained_step_on_a_stale_input(dev):
    """the chained-decode contract ("x must hold step t's embedding") lived in engine.py only; a C-ABI caller that mixed
    acai_decode_logits (which overwrites x) with acai_decode_step got a step on stale input and rc 0.  The library now keeps the marker itself:
    step after logits -> argument error with a message that names the remedy; after acai_decode_embed the step runs."""
    import ctypes

    from acai_omr_amd import _lib, ops
    from acai_omr_amd import engine as EG
    fx = load_golden("vitomr_small")
    cfg = fx["cfg"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.float)
    L = _lib.lib()
    with torch.no_grad():
        lat, mask = m.encoder(fx["imgs"])
        mem = m.transition_head(lat)
        blocks = m.decoder.decoder_blocks
        packed, lens = EG.unpad_rows(mem, mask)
        blocks.prepare_caches_packed(packed, None, lens)
        eng = blocks.engine(packed.device)
        with torch.cuda.stream(eng.stream):
            eng.arm(eng.B)                       # acai_decode_embed: marker set
            st = ops._st()
            assert L.acai_decode_step(ctypes.byref(eng._desc), st) == 0
            tok = torch.full((eng.B,), 5, dtype=torch.int64, device=dev)
            assert L.acai_decode_logits(ctypes.byref(eng._desc), tok.data_ptr(), 2, st) == 0     # overwrites x: marker cleared
            rc = L.acai_decode_step(ctypes.byref(eng._desc), st)
            assert rc != 0 and b"acai_decode_embed" in L.acai_last_error()
            assert L.acai_decode_hidden(ctypes.byref(eng._desc), eng.ws["x"].data_ptr(), st) == 0
            assert L.acai_decode_step(ctypes.byref(eng._desc), st) != 0
            assert L.acai_decode_embed(ctypes.byref(eng._desc), st) == 0
            assert L.acai_decode_step(ctypes.byref(eng._desc), st) == 0
            torch.cuda.synchronize()


def test_in_launch_merge_is_selected_only_at_its_validated_residency(dev):
    """the split partials are merged inside the attention launch only while decode_attn_kernel's residency is the one the
    hand-off was validated at (two workgroups per CU); ACAI_DATTN_MERGE forces either path.  Both paths give the same tokens."""
    import os
    import subprocess
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import torch, sys; sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests'); from test_gpu_parity import load_golden, build_vitomr\n"
            "fx = load_golden('vitomr_dh64b'); cfg = fx['cfg']; m = build_vitomr(cfg, fx['state_dict'], torch.device('cuda:0'), torch.bfloat16)\n"
            "from acai_omr_amd.inference.vitomr_inference import inference\n"
            "seqs, lps, mask = inference(m, fx['imgs'], 'cuda', max_inference_len=cfg['gen_len']); print('TOK', seqs.cpu().tolist())\n") % (ROOT, ROOT)
    outs = []
    for force in ("0", "1", None):
        env = dict(os.environ)
        env.pop("ACAI_DATTN_MERGE", None)
        if force is not None:
            env["ACAI_DATTN_MERGE"] = force
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-1500:]
        outs.append([ln for ln in r.stdout.splitlines() if ln.startswith("TOK")][0])
    assert outs[0] == outs[1] == outs[2]

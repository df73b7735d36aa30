"""Beam-search decoding on the GPU (acai_decode_beam_step through DecodeEngine.beam / ViTOMR.cached_beam_generate / inference) against
greedy decoding and the float64 beam reference (tests/beam_reference.py, which reorders its self caches physically instead of reading
them through an ancestor table).

Bars:
  * beam width 1 is greedy bit for bit (seqs, log_probs, mask), fp32 and bf16, fixtures and a full-width fused-chain decoder;
  * fp32, K in {2, 4, 5}: token ids / masks / lengths equal to the reference, cum within 1e-4 relative, provided that every step's
    reference margin between the K-th and (K+1)-th candidate exceeds 1e-3 (asserted: a seed without it fails);
  * bf16 full width, K = 4 (grouped matrix-core cross attention, fused chain): ids equal to the reference run with the device's bf16
    rounding points, for seeds whose minimum reference margin exceeds 0.04 (asserted and printed).  Measured on one MI355X: the logits of
    a step differ from the bf16 reference by single bf16 ulps (0.0625 / 0.125 at the |logit| of 8..32 the scaled unembed gives), so
    per-token log-probs differ by up to 0.109 and cum by up to 0.128 (seeds 9 / 15, margins 0.049 / 0.049).  The error is mostly common
    to the candidates a decision compares (they share their prefix), which is why the ids still agree; the per-token and cum bars are
    two bf16 ulps at |x| in [16, 32): 0.25;
  * exact ties (all logits equal to a chosen bias): slots, tie-breaks, frozen finished rows, len^alpha and the final choice equal the
    reference exactly."""

import pytest
import torch
from torch.amp import autocast

from beam_reference import beam_generate
from conftest import load_golden
from decode_support import build_vitomr, _decoder, dev, _same, _vit

pytestmark = pytest.mark.gpu


def _padded(mem, lens, dev):
    """packed (M, E) -> (B, Smax, E) and the padding mask (True = padding) as the encoder makes them."""
    B, Sm = len(lens), max(lens)
    out = torch.zeros(B, Sm, mem.shape[1], dtype=mem.dtype)
    mask = torch.ones(B, Sm, dtype=torch.bool)
    o = 0
    for b, l in enumerate(lens):
        out[b, :l] = mem[o:o + l]
        mask[b, :l] = False
        o += l
    return out.to(dev), mask.to(dev)


def _sd64(dec):
    return {"decoder." + k: v.detach().double() for k, v in dec.state_dict().items()}


# ---- 1. beam width 1 is greedy, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vitomr_small", "vitomr_dh64", "vitomr_odd"])
@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
def test_width_one_is_greedy_bitwise(dev, name, cdt):
    fx = load_golden(name)
    cfg, ref = fx["cfg"], fx["ref_fp32"]
    m = build_vitomr(cfg, fx["state_dict"], dev, cdt, max_batch=8)
    with torch.no_grad():
        lat, mask = m.encoder(fx["imgs"])
        with autocast(device_type="cuda", dtype=torch.bfloat16, enabled=cdt == torch.bfloat16):
            mem = m.transition_head(lat)
            g = m.cached_greedy_generate(mem, mask, max_len=cfg["gen_len"])
            b = m.cached_beam_generate(mem, mask, beam_width=1, max_len=cfg["gen_len"])
    _same(g, b)
    if cdt == torch.float32:
        assert torch.equal(b[0].cpu(), ref["seqs"]) and torch.equal(b[2].cpu(), ref["seq_mask"])


def test_width_one_is_greedy_bitwise_full_width_fused(dev):
    """L = 2, E = 1024, H = 16 on a ragged bf16 memory: the fused bf16 chain, several cross splits."""
    lens, T = [4096, 1300, 64], 24
    dec = _decoder(32)
    m = _vit(dec, 4, torch.bfloat16, dev)
    mem, mask = _padded(torch.randn(sum(lens), 1024, generator=torch.Generator().manual_seed(11)).to(torch.bfloat16), lens, dev)
    with torch.no_grad():
        g = m.cached_greedy_generate(mem, mask, max_len=T)
        b = m.cached_beam_generate(mem, mask, beam_width=1, max_len=T)
    _same(g, b)


# ---- 2. fp32, K in {2, 4, 5}, ragged memories, against the float64 reference -------------------------------------------------------------
@pytest.mark.parametrize("seed", [4, 5])
def test_fp32_beam_vs_float64_reference(dev, seed):
    lens, E, H, T = [300, 77, 150], 256, 4, 12
    dec = _decoder(16, E=E, H=H, Fd=512, seed=seed, scale=8.0)
    mem = torch.randn(sum(lens), E, generator=torch.Generator().manual_seed(seed + 100))
    m = _vit(dec, 16, torch.float32, dev)
    pm, mask = _padded(mem, lens, dev)
    sd = _sd64(dec)
    for K in (2, 4, 5):
        ref = beam_generate(mem.double(), lens, sd, H, "fp32", K, T)
        margin = min(ref["margins"])
        print(f"seed {seed} K {K}: reference min margin {margin:.4g}, {ref['steps']} steps, {int(ref['slot_fin'].sum())} finished slots")
        assert margin > 1e-3, f"seed {seed} K {K}: decisions not separated enough for an fp32 comparison (margin {margin})"
        with torch.no_grad():
            seqs, lps, smask = m.cached_beam_generate(pm, mask, beam_width=K, max_len=T)
        eng = m.decoder.decoder_blocks.engine(dev)
        assert torch.equal(seqs.cpu(), ref["seqs"]) and torch.equal(smask.cpu(), ref["mask"])
        assert float((lps.cpu().double() - ref["log_probs"]).abs().max()) < 1e-4
        # every slot: the same set of hypotheses per image (the order of two kept hypotheses may differ where their scores are closer than
        # the fp32 error), each with the reference's length and cum
        stok, slp, scum, slen = (x.cpu() for x in eng.beam_slots(T))
        for i in range(len(lens)):
            dv = {tuple(stok[i * K + k].tolist()): (int(slen[i * K + k]), float(scum[i * K + k])) for k in range(K)}
            rf = {tuple(ref["slot_seqs"][i * K + k].tolist()): (int(ref["slot_len"][i * K + k]), float(ref["slot_cum"][i * K + k])) for k in range(K)}
            assert dv.keys() == rf.keys()
            for h, (ln, c) in rf.items():
                assert dv[h][0] == ln and abs(dv[h][1] - c) <= 1e-4 * max(1.0, abs(c)), (h, dv[h], c)


# ---- 3. bf16, full width, K = 4 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [9, 15])
def test_bf16_full_width_beam_vs_reference(dev, seed):
    lens, E, H, T, K = [1500, 1000, 77], 1024, 16, 8, 4
    dec = _decoder(16, seed=seed, scale=16.0)
    mem = torch.randn(sum(lens), E, generator=torch.Generator().manual_seed(seed + 100)).to(torch.bfloat16)
    ref = beam_generate(mem.double(), lens, _sd64(dec), H, "bf16", K, T)
    margin = min(ref["margins"])
    m = _vit(dec, 16, torch.bfloat16, dev)
    pm, mask = _padded(mem, lens, dev)
    with torch.no_grad():
        seqs, lps, smask = m.cached_beam_generate(pm, mask, beam_width=K, max_len=T)
    eng = m.decoder.decoder_blocks.engine(dev)
    scum = eng.beam_slots(T)[2].cpu().double()
    err = float((lps.cpu().double() - ref["log_probs"]).abs().max()) if torch.equal(seqs.cpu(), ref["seqs"]) else float("nan")
    print(f"seed {seed}: reference min margin {margin:.4g}; max|lp dev - lp ref| {err:.3g}; max|cum dev - cum ref| "
          f"{float((scum - ref['slot_cum']).abs().max()):.3g}")
    assert margin > 0.04, f"seed {seed}: reference margin {margin} below the bar"
    assert torch.equal(seqs.cpu(), ref["seqs"]) and torch.equal(smask.cpu(), ref["mask"])
    assert err <= 0.25 and float((scum - ref["slot_cum"]).abs().max()) <= 0.25


# ---- 4. exact ties and finished beams ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_exact_ties_and_finished_beams(dev, cdt, alpha):
    """unembed.weight = 0: the logits are the bias at every row and step.  Tokens 10 and 20 tie at the top, <eos> is third, 30 and 40 tie
    fourth: step 1 puts <eos> in slot 2; from step 2 the finished row (score lp(eos)) outranks every live extension and sits in slot 0,
    reproducing itself, while the live slots hold exactly tied hypotheses (ties to the lower parent, then the lower rank).  alpha = 0 picks
    the short finished hypothesis, alpha = 1 the lowest of the tied long ones."""
    fx = load_golden("vitomr_small")
    cfg = fx["cfg"]
    m = build_vitomr(cfg, fx["state_dict"], dev, cdt, max_batch=16)
    eos = m.decoder.eos_idx
    bias = torch.full((m.decoder.vocab_size,), -4.0)
    bias[10] = bias[20] = 2.0
    bias[eos] = 1.5
    bias[30] = bias[40] = 1.0
    with torch.no_grad():
        m.decoder.unembed.weight.zero_()
        m.decoder.unembed.bias.copy_(bias.to(dev))
    K, T = 4, 8
    ref_fx = fx["ref_fp32"]
    valid = ~ref_fx["latent_mask"]
    lens = valid.sum(1).tolist()
    mem = ref_fx["memory"][valid]
    sd = {k: v.detach().double().cpu() for k, v in m.decoder.state_dict().items()}
    sd = {"decoder." + k: v for k, v in sd.items()}
    prec = "bf16" if cdt == torch.bfloat16 else "fp32"
    ref = beam_generate(mem.double(), lens, sd, cfg["dec_heads"], prec, K, T, alpha=alpha, eos_idx=eos)
    with torch.no_grad():
        seqs, lps, smask = m.cached_beam_generate(ref_fx["memory"].to(dev), ref_fx["latent_mask"].to(dev), beam_width=K, max_len=T,
                                                  length_penalty=alpha)
    eng = m.decoder.decoder_blocks.engine(dev)
    stok, slp, scum, slen = (x.cpu() for x in eng.beam_slots(T))
    assert torch.equal(stok, ref["slot_seqs"]) and torch.equal(slen.long(), ref["slot_len"])
    assert torch.equal(scum == float("-inf"), ref["slot_cum"] == float("-inf"))
    assert float((scum.double() - ref["slot_cum"]).abs().max()) < 1e-5
    assert torch.equal(seqs.cpu(), ref["seqs"]) and torch.equal(smask.cpu(), ref["mask"])
    # the scenario the docstring describes
    n = len(lens)
    assert bool((ref["slot_seqs"].view(n, K, T)[:, 0, 1] == eos).all()) and bool((ref["slot_len"].view(n, K)[:, 0] == 1).all())
    assert bool((ref["best"] == (0 if alpha == 0.0 else 1)).all())
    assert float((slp.double() - ref["slot_lps"]).abs().max()) <= (2 ** -7 if cdt == torch.bfloat16 else 1e-5)


# ---- 5. overshoot and state isolation ----------------------------------------------------------------------------------------------------
def test_poll_and_graph_forms_agree_and_other_modes_unaffected(dev):
    from acai_omr_amd import engine as EG
    fx = load_golden("vitomr_dh64b")
    cfg = fx["cfg"]
    T = cfg["gen_len"]

    def setup():
        m = build_vitomr(cfg, fx["state_dict"], dev, torch.bfloat16, max_batch=16)
        with torch.no_grad():
            lat, mask = m.encoder(fx["imgs"])
            with autocast(device_type="cuda", dtype=torch.bfloat16):
                mem = m.transition_head(lat)
        mem32, lens = EG.unpad_rows(mem, mask)
        return m, m.decoder.decoder_blocks, mem32, lens

    u = torch.rand(len(fx["imgs"]) * 2, T, generator=torch.Generator().manual_seed(3)).to(dev)

    def greedy(blocks, mem32, lens):
        blocks.prepare_caches_packed(mem32, None, lens)
        return tuple(x.clone() for x in blocks.engine(dev).greedy(T)[:2])

    def sample(blocks, mem32, lens):
        blocks.prepare_caches_packed(mem32, None, lens, group_size=2)
        return tuple(x.clone() for x in blocks.engine(dev).sample(T, 5, 1.3, uniforms=u)[:2])

    def beam(blocks, mem32, lens, **kw):
        blocks.prepare_caches_packed(mem32, None, lens, group_size=4)
        return blocks.engine(dev).beam(T, 4, 1.0, **kw)

    _, fb, fm, fl = setup()
    g0, s0 = greedy(fb, fm, fl), sample(fb, fm, fl)
    _, blocks, mem32, lens = setup()
    g1, s1 = greedy(blocks, mem32, lens), sample(blocks, mem32, lens)
    b16 = beam(blocks, mem32, lens, poll=16)
    b1 = beam(blocks, mem32, lens, poll=1)
    bng = beam(blocks, mem32, lens, poll=5, use_graph=False)
    g2, s2 = greedy(blocks, mem32, lens), sample(blocks, mem32, lens)
    b2 = beam(blocks, mem32, lens)
    for x in (b1, bng, b2):
        _same(b16, x)
    for x in (g1, g2):
        _same(g0, x)
    for x in (s1, s2):
        _same(s0, x)


# ---- 6. entry point and errors -----------------------------------------------------------------------------------------------------------
def test_inference_entry_point_and_errors(dev):
    from acai_omr_amd.inference.vitomr_inference import inference
    fx = load_golden("vitomr_dh64b")
    cfg = fx["cfg"]
    T = cfg["gen_len"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.bfloat16, max_batch=16)
    out4 = inference(m, fx["imgs"], "cuda", max_inference_len=T, beam_width=4)
    out1 = inference(m, fx["imgs"], "cuda", max_inference_len=T)
    with torch.no_grad():
        lat, mask = m.encoder(fx["imgs"])
        with autocast(device_type="cuda", dtype=torch.bfloat16):
            mem = m.transition_head(lat)
            b4 = m.cached_beam_generate(mem, mask, beam_width=4, max_len=T)
            g = m.cached_greedy_generate(mem, mask, max_len=T)
        for K in (0, 17):
            with pytest.raises(ValueError):
                m.cached_beam_generate(mem, mask, beam_width=K, max_len=T)
        with pytest.raises(ValueError):
            m.cached_beam_generate(mem, mask, beam_width=6, max_len=T)   # 3 images x 6 > max batch 16
        with pytest.raises(RuntimeError):
            m.cached_beam_generate(mem, mask, beam_width=2, max_len=cfg["max_len"] + 1)
    _same(out4, b4)
    _same(out1, g)
    assert torch.equal(out1[0].cpu(), fx["ref_bf16"]["seqs"])
    un = build_vitomr(cfg, fx["state_dict"], dev, None, max_batch=8)
    with torch.no_grad():
        lat, mask = un.encoder(fx["imgs"])
        with pytest.raises(RuntimeError, match="uncached"):
            un.cached_beam_generate(un.transition_head(lat), mask, beam_width=2, max_len=T)

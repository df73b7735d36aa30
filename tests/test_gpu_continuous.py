"""Continuous-batching greedy decode on the GPU (acai_decode_slot_step / acai_decode_slot_arm through DecodeEngine.continuous,
ViTOMR.cached_continuous_generate, continuous_inference and iter_continuous_inference).

Bars:
  * fixtures, fp32: ids and masks equal the reference's, log-probs within 1e-4, at slots 1, 2, N and with the images repeated 3x in a
    shuffled order through 2 slots at max_len = Tmax = 24 (many refills, the ring index wraps at least twice);
  * fixtures, bf16: continuous_inference equals inference() and the reference's ids, log-probs within the bars of
    test_bf16_inference_entry_point_vs_reference_and_oracle;
  * full width (E = 1024, 16 heads), 16 ragged memories, per-image caps around the 8-step graph and 16-step poll boundaries: every image
    equals _greedy_packed of that image alone at its cap (fp32: ids equal, log-probs within 1e-4; bf16: ids equal up to a decision whose
    reference margin is within two bf16 ulps (0.25, printed; at most 2 of 16 images), per-token log-probs within 0.25);
  * graph / eager and poll 1 / 16 forms, slots > N and N = 1 are bitwise equal;
  * a slot-mode run leaves greedy, beam and sampling decoding bitwise as on a fresh model, and a greedy run leaves slot mode as fresh;
  * errors, and the C ABI's argument checks."""
import ctypes
import random

import pytest
import torch
from torch.amp import autocast

from conftest import load_golden
from decode_support import build_vitomr, _decoder, dev, _md, _memory, _same, _vit

pytestmark = pytest.mark.gpu

FIXTURES = ["vitomr_small", "vitomr_dh64", "vitomr_dh64b", "vitomr_odd"]


# ---- 1. fixtures, fp32 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_fp32_fixtures_vs_reference(dev, name):
    fx = load_golden(name)
    cfg, ref = fx["cfg"], fx["ref_fp32"]
    N, T = len(fx["imgs"]), cfg["gen_len"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.float32, max_batch=8)
    mem, mask = _memory(m, fx["imgs"], False)
    for slots in sorted({1, 2, N, N + 3}):   # N + 3: idle slots from the start
        with torch.no_grad():
            seqs, lps, smask = m.cached_continuous_generate(mem, mask, max_len=T, slots=slots)
        assert torch.equal(seqs.cpu(), ref["seqs"]) and torch.equal(smask.cpu(), ref["seq_mask"]), slots
        assert _md(lps, ref["log_probs"]) < 1e-4, slots
    for i in range(N):   # N = 1
        with torch.no_grad():
            seqs, lps, smask = m.cached_continuous_generate(mem[i:i + 1], mask[i:i + 1], max_len=T, slots=1)
        n = seqs.shape[1]
        assert torch.equal(seqs[0].cpu(), ref["seqs"][i, :n]) and torch.equal(smask[0].cpu(), ref["seq_mask"][i, :n])
        assert not bool(ref["seq_mask"][i, n:].any()) and _md(lps[0], ref["log_probs"][i, :n]) < 1e-4
    # the images 3x in a shuffled order through 2 slots up to the cache length: many refills, the ring wraps
    order = [i for i in range(N) for _ in range(3)]
    random.Random(1).shuffle(order)
    Tmax = cfg["max_len"]
    with torch.no_grad():
        seqs, lps, smask = m.cached_continuous_generate(mem[order], mask[order], max_len=Tmax, slots=2)
    eng = m.decoder.decoder_blocks.engine(dev)
    wraps = eng.slot_steps // Tmax
    print(f"{name}: {len(order)} images through 2 slots, {eng.slot_steps} steps, ring wrapped {wraps}x")
    assert wraps >= 2
    assert int(eng.step[1]) == eng.slot_steps % Tmax
    rs, rl, rm = ref["seqs"], ref["log_probs"], ref["seq_mask"]
    for k, i in enumerate(order):   # a prefix of each row is the reference's row (greedy decoding is causal)
        assert torch.equal(seqs[k, :T].cpu(), rs[i]) and torch.equal(smask[k, :T].cpu(), rm[i])
        assert _md(lps[k, :T], rl[i]) < 1e-4
        g = m.cached_greedy_generate(mem[i:i + 1], mask[i:i + 1], max_len=Tmax)
        n = g[0].shape[1]
        assert torch.equal(seqs[k, :n], g[0][0]) and torch.equal(smask[k, :n], g[2][0]) and not bool(smask[k, n:].any())


# ---- 2. fixtures, bf16 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_bf16_continuous_inference_vs_inference_and_reference(dev, name):
    from acai_omr_amd.inference.vitomr_inference import continuous_inference, inference, iter_continuous_inference
    fx = load_golden(name)
    cfg, ref = fx["cfg"], fx["ref_bf16"]
    T = cfg["gen_len"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.bfloat16, max_batch=8)
    seqs, lps, smask = continuous_inference(m, fx["imgs"], "cuda", max_inference_len=T, slots=2)
    g = inference(m, fx["imgs"], "cuda", max_inference_len=T)
    assert torch.equal(seqs, g[0]) and torch.equal(smask, g[2])
    assert torch.equal(seqs.cpu(), ref["seqs"]) and torch.equal(smask.cpu(), ref["seq_mask"])
    assert _md(lps, ref["log_probs"]) < 0.13 and _md(lps, g[1]) < 0.07
    got = list(iter_continuous_inference(m, fx["imgs"], "cuda", max_inference_len=T, slots=2))
    assert sorted(i for i, *_ in got) == list(range(len(fx["imgs"])))
    for i, s, l, k in got:
        one = inference(m, [fx["imgs"][i]], "cuda", max_inference_len=T)
        assert torch.equal(s, one[0]) and torch.equal(k, one[2]) and _md(l, one[1]) < 0.07


# ---- 3. full width, ragged memories, caps around the graph / poll boundaries ------------------------------------------------------------
LENS = [256, 4096, 700, 1300, 3000, 512, 2048, 999, 4096, 300, 1500, 2600, 777, 3500, 1024, 2222]
CAPS = [2, 8, 9, 16, 17, 96, 33, 50, 64, 5, 12, 24, 70, 96, 40, 3]


def _full_width(cdt, dev, seed=5):
    dec = _decoder(128, seed=seed, scale=16.0)
    m = _vit(dec, 8, cdt, dev)
    mem = torch.randn(sum(LENS), 1024, generator=torch.Generator().manual_seed(seed + 100))
    return m, (mem.to(torch.bfloat16) if cdt == torch.bfloat16 else mem).to(dev)


def _alone(m, mem, cdt):
    """_greedy_packed of each image alone at its cap."""
    out, o = [], 0
    bf = cdt == torch.bfloat16
    for l, c in zip(LENS, CAPS):
        x = mem[o:o + l]
        with torch.no_grad():
            out.append(m._greedy_packed(None if bf else x, x if bf else None, [l], c))
        o += l
    return out


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
def test_full_width_each_image_as_alone(dev, cdt):
    m, mem = _full_width(cdt, dev)
    bf = cdt == torch.bfloat16
    ref = _alone(m, mem, cdt)
    margins = []   # bf16: per image, the reference's margin between its token at index t and the runner-up (stepwise fp32 logits)
    if bf:
        o = 0
        blocks = m.decoder.decoder_blocks
        eng = blocks.engine(dev)
        for (rs, _, rk), l in zip(ref, LENS):
            blocks.prepare_caches_packed(None, mem[o:o + l], [l])
            mg = [float("inf")]
            with torch.no_grad():
                for t in range(1, int(rk.sum())):
                    top = torch.topk(eng.logits_step(rs[:, t - 1], t).view(-1), 2).values
                    mg.append(float(top[0] - top[1]))
            margins.append(mg)
            o += l
        flat = [x for mg in margins for x in mg[1:]]
        print(f"bf16 full width: minimum reference margin {min(flat):.4g}, {sum(x == 0 for x in flat)} exact ties, "
              f"{sum(x <= 0.25 for x in flat)} within 0.25")
    for slots in (4, 8):
        with torch.no_grad():
            seqs, lps, smask = m._continuous_packed(None if bf else mem, mem if bf else None, LENS, CAPS, slots)
        diverged = []
        for i, (rs, rl, rk) in enumerate(ref):
            n = rs.shape[1]
            if not bf:
                assert torch.equal(seqs[i, :n], rs[0]) and torch.equal(smask[i, :n], rk[0]), (slots, i)
                assert not bool(smask[i, n:].any())
                assert _md(lps[i, :n], rl[0]) < 1e-4, (slots, i)
                continue
            # bf16: the logits are bf16-rounded (ulp 0.125 at the |logit| of 16..32 this decoder gives) and the slot run's cross split
            # differs from the image-alone run's, so a near-tie may go the other way; ids must agree up to the first decision whose
            # reference margin is within two ulps, and everything before it must agree
            p = n if torch.equal(seqs[i, :n], rs[0]) else int((seqs[i, :n] != rs[0]).nonzero()[0])
            if p < n:
                diverged.append((i, p, margins[i][p]))
                assert margins[i][p] <= 0.25, (slots, i, p, margins[i][p])
            else:
                assert torch.equal(smask[i, :n], rk[0]) and not bool(smask[i, n:].any()), (slots, i)
            assert _md(lps[i, :p], rl[0, :p]) < 0.25, (slots, i)
        if bf:
            print(f"slots {slots}: images diverging at a near-tie (image, index, reference margin): {diverged}")
            assert len(diverged) <= 2


# ---- 4. forms agree ----------------------------------------------------------------------------------------------------------------------
def test_forms_agree_bitwise(dev):
    m, mem = _full_width(torch.bfloat16, dev, seed=7)
    base = m._continuous_packed(None, mem, LENS, CAPS, 4)
    for kw in (dict(use_graph=False), dict(poll=1), dict(poll=1, use_graph=False), dict(poll=5)):
        _same(base, m._continuous_packed(None, mem, LENS, CAPS, 4, **kw))
    # slots > N (idle slots from the start) and N = 1
    o = [0]
    for l in LENS:
        o.append(o[-1] + l)
    for lens, caps, slots, x in ((LENS[:3], CAPS[3:6], 8, mem[:o[3]]), (LENS[5:6], CAPS[5:6], 1, mem[o[5]:o[6]]),
                                 (LENS[5:6], CAPS[5:6], 4, mem[o[5]:o[6]])):
        base = m._continuous_packed(None, x, lens, caps, slots)
        _same(base, m._continuous_packed(None, x, lens, caps, slots, poll=1, use_graph=False))
        assert base[0].shape[0] == len(lens) and bool((base[0][:, 0] == m.decoder.bos_idx).all())


# ---- 5. isolation ------------------------------------------------------------------------------------------------------------------------
def test_slot_mode_leaves_other_modes_alone(dev):
    from acai_omr_amd import engine as EG
    from acai_omr_amd.inference.vitomr_inference import inference
    fx = load_golden("vitomr_dh64b")
    cfg = fx["cfg"]
    T = cfg["gen_len"]
    u = torch.rand(len(fx["imgs"]) * 2, T, generator=torch.Generator().manual_seed(3)).to(dev)

    def setup():
        m = build_vitomr(cfg, fx["state_dict"], dev, torch.bfloat16, max_batch=16)
        mem, mask = _memory(m, fx["imgs"], True)
        return m, mem, mask

    def others(m, mem, mask):
        g = inference(m, fx["imgs"], "cuda", max_inference_len=T)
        with torch.no_grad(), autocast(device_type="cuda", dtype=torch.bfloat16):
            b = m.cached_beam_generate(mem, mask, beam_width=4, max_len=T)
        blocks = m.decoder.decoder_blocks
        mem32, lens = EG.unpad_rows(mem, mask)
        blocks.prepare_caches_packed(mem32, None, lens, group_size=2)
        s = tuple(x.clone() for x in blocks.engine(dev).sample(T, 5, 1.3, uniforms=u)[:2])
        return g + b + s

    def slot(m, mem, mask):
        with torch.no_grad():
            return m.cached_continuous_generate(mem, mask, max_len=[T, T - 3, 5], slots=2)

    m0, mem0, mask0 = setup()
    fresh_others = others(m0, mem0, mask0)
    m1, mem1, mask1 = setup()
    fresh_slot = slot(m1, mem1, mask1)
    _same(fresh_others, others(m1, mem1, mask1))       # slot mode, then greedy / beam / sampling
    _same(fresh_slot, slot(m1, mem1, mask1))           # greedy / beam / sampling, then slot mode
    m2, mem2, mask2 = setup()
    others(m2, mem2, mask2)
    _same(fresh_slot, slot(m2, mem2, mask2))


# ---- 6. errors and the C ABI -------------------------------------------------------------------------------------------------------------
def test_errors_and_c_abi_checks(dev):
    from acai_omr_amd import _lib
    fx = load_golden("vitomr_dh64b")
    cfg = fx["cfg"]
    T = cfg["gen_len"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.float32, max_batch=8)
    mem, mask = _memory(m, fx["imgs"], False)
    with torch.no_grad():
        for s in (0, 9):
            with pytest.raises(ValueError, match="slots must be in"):
                m.cached_continuous_generate(mem, mask, max_len=T, slots=s)
        with pytest.raises(ValueError, match="per-image caps"):
            m.cached_continuous_generate(mem, mask, max_len=[T, T])
        with pytest.raises(RuntimeError, match=f"{cfg['max_len'] + 1} decoding steps is too long for max sequence length of {cfg['max_len']}"):
            m.cached_continuous_generate(mem, mask, max_len=cfg["max_len"] + 1)
        with pytest.raises(RuntimeError, match=f"{cfg['max_len'] + 1} decoding steps is too long"):
            m.cached_continuous_generate(mem, mask, max_len=[T, cfg["max_len"] + 1, T])
        m.cached_continuous_generate(mem, mask, max_len=T, slots=2)
        # the engine's descriptors as the last run left them: an un-embedded x and cross_group != 1 are argument errors
        eng = m.decoder.decoder_blocks.engine(dev)
        L = _lib.lib()
        st = torch.cuda.current_stream().cuda_stream
        eng.logits_step(torch.zeros(eng.B, dtype=torch.int64, device=dev), 1)   # overwrites x
        assert L.acai_decode_slot_step(ctypes.byref(eng._desc), ctypes.byref(eng._slot_desc), st) != 0
        assert b"x does not hold" in L.acai_last_error()
        assert L.acai_decode_slot_arm(ctypes.byref(eng._desc), ctypes.byref(eng._slot_desc), None, 0, st) == 0
        eng._desc.cross_group = 2
        try:
            assert L.acai_decode_slot_step(ctypes.byref(eng._desc), ctypes.byref(eng._slot_desc), st) != 0
            assert b"cross_group" in L.acai_last_error()
        finally:
            eng._desc.cross_group = 1
        torch.cuda.synchronize()
    un = build_vitomr(cfg, fx["state_dict"], dev, None, max_batch=8)
    with torch.no_grad():
        lat, mask = un.encoder(fx["imgs"])
        with pytest.raises(RuntimeError, match="uncached"):
            un.cached_continuous_generate(un.transition_head(lat), mask, max_len=T)

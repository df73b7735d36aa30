"""Speculative greedy decoding on the GPU (acai_decode_spec_step / acai_decode_spec_arm through DecodeEngine.speculative,
ViTOMR.cached_speculative_generate and inference(speculative=D)).

Bars (the criterion is exact: speculative greedy decoding must BE greedy decoding):
  * fixtures, bf16 and fp32, D in {1, 2, 4, 7}, one image and the ragged batch, n-gram / oracle / adversarial drafts, graph and eager launch,
    poll 1 and 16: seqs, log-probs and mask torch.equal to cached_greedy_generate's;
  * step counts: oracle drafts ceil((T - 1) / (D + 1)), adversarial drafts T - 1, a half-corrupted table strictly between, n-gram drafts the
    count the plain-Python restatement (tests/speculative_reference.py) takes on the same token stream;
  * <eos> inside an accepted run, and a max_len that cuts one, end the sequence at that index;
  * the proposals read back after every step equal the restatement's;
  * a speculative run leaves greedy, beam, sampling and slot decoding bitwise as on a fresh model, and the reverse;
  * errors, the C ABI's argument checks, and inference(speculative=4) == inference()."""
import ctypes
import math

import pytest
import torch
from torch.amp import autocast

import speculative_reference as SR
from conftest import load_golden
from decode_support import build_vitomr, dev, _memory, _same

pytestmark = pytest.mark.gpu

FIXTURES = ["vitomr_small", "vitomr_dh64", "vitomr_dh64b", "vitomr_odd"]
DS = [1, 2, 4, 7]


def _tables(greedy, max_len, V):
    """Draft tables (B, max_len) from a greedy result: oracle (the output itself, none past each row's end), adversarial (every token
    changed) and half (indices 2, 3 of every four changed)."""
    seqs, _, mask = greedy
    B, n = seqs.shape
    oracle = torch.full((B, max_len), -1, dtype=torch.int64, device=seqs.device)
    oracle[:, :n] = torch.where(mask, seqs, torch.full_like(seqs, -1))
    wrong = torch.where(oracle >= 0, (oracle + 1) % V, torch.full_like(oracle, 7))
    bad = (torch.arange(max_len, device=seqs.device) % 4 >= 2).unsqueeze(0)
    return {"oracle": oracle, "adversarial": wrong, "half": torch.where(bad, wrong, oracle)}


def _spec(m, mem, mask, max_len, D, drafts=None, ngram=3, poll=16, use_graph=True, on_chunk=None):
    """_speculative_packed with the launch form exposed -> (seqs, log_probs, mask), steps per image (list)."""
    from acai_omr_amd import engine as EG
    mem32, lens = EG.unpad_rows(mem, mask)
    blocks = m.decoder._cached_blocks()
    blocks.prepare_caches_packed(mem32, None, lens, group_size=D + 1, per_row_cross=True)
    eng = blocks.engine(mem.device)
    seqs, lps, steps = eng.speculative(max_len, D, ngram=ngram, drafts=drafts, poll=poll, use_graph=use_graph, on_chunk=on_chunk)
    return m.mask_and_clip_seqs(seqs.clone(), lps.clone()), steps.tolist()


def _restated_steps(row, T, max_len, D, ngram, eos):
    """Steps the restatement takes with n-gram drafts when the greedy stream is `row` (T tokens)."""
    toks = row[:T].tolist()
    nxt = lambda prefix: toks[len(prefix)]   # noqa: E731
    seq, steps, log = SR.speculative_decode(nxt, toks[0], eos, T, D, SR.ngram_source(ngram))
    assert seq == toks
    return steps, log


# ---- 1. equality with greedy and step counts, every fixture / precision / D / draft source / launch form -------------------------------
@pytest.mark.parametrize("cdt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", FIXTURES)
def test_equals_greedy_and_step_counts(dev, name, cdt):
    fx = load_golden(name)
    cfg = fx["cfg"]
    T = cfg["gen_len"]
    bf = cdt == torch.bfloat16
    m = build_vitomr(cfg, fx["state_dict"], dev, cdt, max_batch=24)
    V, eos = m.decoder.vocab_size, m.decoder.eos_idx
    mem_all, mask_all = _memory(m, fx["imgs"], bf)
    last = len(fx["imgs"]) - 1
    for label, sl in (("one image", slice(last, last + 1)), ("ragged batch", slice(0, None))):
        mem, mask = mem_all[sl], mask_all[sl]
        with torch.no_grad(), autocast(device_type="cuda", dtype=torch.bfloat16, enabled=bf):
            g = m.cached_greedy_generate(mem, mask, max_len=T)
            Tn = g[2].sum(dim=1).tolist()   # tokens per image, <bos> included
            tabs = _tables(g, T, V)
            for D in DS:
                want = {"oracle": [math.ceil((t - 1) / (D + 1)) for t in Tn], "adversarial": [t - 1 for t in Tn],
                        "ngram": [_restated_steps(g[0][i].cpu(), Tn[i], T, D, 3, eos)[0] for i in range(len(Tn))]}
                for src in ("ngram", "oracle", "adversarial", "half"):
                    for form in (dict(), dict(use_graph=False), dict(poll=1), dict(poll=1, use_graph=False)):
                        s, steps = _spec(m, mem, mask, T, D, drafts=tabs.get(src), **form)
                        where = (name, label, D, src, form)
                        assert torch.equal(s[0], g[0]) and torch.equal(s[2], g[2]), where
                        assert torch.equal(s[1], g[1]), (where, float((s[1] - g[1]).abs().max()))
                        if src == "half":
                            assert all(lo < st < hi for lo, st, hi in zip(want["oracle"], steps, want["adversarial"])), (where, steps)
                        else:
                            assert steps == want[src], (where, steps, want[src])
                # the public entry point
                _same(g, m.cached_speculative_generate(mem, mask, max_len=T, draft_len=D))
                _same(g, m.cached_speculative_generate(mem, mask, max_len=T, draft_len=D, drafts=tabs["oracle"]))
                print(f"{name} {label} {'bf16' if bf else 'fp32'} D={D}: T = {Tn}, steps with n-gram drafts {want['ngram']}")


# ---- 1b. full width (E = 1024, 16 heads, d_h 64: the fused MFMA GEMV chain and the split cross attention of the flagship decoder) ------
@pytest.mark.parametrize("cdt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_full_width_equals_greedy(dev, cdt):
    from acai_omr_amd.models.models import OMRDecoder, ViTOMR
    from conftest import VOCAB
    torch.manual_seed(5)
    T = 64
    dec = OMRDecoder(T, VOCAB, num_layers=2, hidden_dim=1024, num_heads=16, mlp_dim=4096)
    with torch.no_grad():
        for n, p in dec.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
        dec.unembed.weight.mul_(16.0)
    c = dec.to_cached_version(24, cdt)
    c.load_state_dict(dec.state_dict())
    m = ViTOMR(None, None, c.to(dev).eval())
    bf = cdt == torch.bfloat16
    V = m.decoder.vocab_size
    for lens in ([1024], [4096], [700, 4096, 1300]):
        mem = torch.randn(sum(lens), 1024, generator=torch.Generator().manual_seed(100 + len(lens)))
        mem = (mem.to(torch.bfloat16) if bf else mem).to(dev)
        args = (None if bf else mem, mem if bf else None, lens)
        with torch.no_grad():
            g = m._greedy_packed(*args, T)
            Tn = g[2].sum(dim=1).tolist()
            tabs = _tables(g, T, V)
            for D in ((1, 4, 7) if len(lens) == 1 else (2, 7)):
                for src in ("ngram", "oracle", "adversarial", "half"):
                    s = m._speculative_packed(*args, T, D, drafts=tabs.get(src))
                    where = (lens, D, src)
                    assert torch.equal(s[0], g[0]) and torch.equal(s[2], g[2]), where
                    assert torch.equal(s[1], g[1]), (where, float((s[1] - g[1]).abs().max()))
                    steps = m.decoder.decoder_blocks.engine(dev).spec_steps[:len(lens)].tolist()
                    if src == "oracle":
                        assert steps == [math.ceil((t - 1) / (D + 1)) for t in Tn], (where, steps)
                    if src == "adversarial":
                        assert steps == [t - 1 for t in Tn], (where, steps)
                _same(g, m._speculative_packed(*args, T, D, poll=1, use_graph=False))


# ---- 2. sequence ends inside an accepted run ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_eos_and_max_len_inside_an_accepted_run(dev, cdt):
    fx = load_golden("vitomr_dh64b")
    cfg = fx["cfg"]
    bf = cdt == torch.bfloat16
    m = build_vitomr(cfg, fx["state_dict"], dev, cdt, max_batch=24)
    V = m.decoder.vocab_size
    mem, mask = _memory(m, fx["imgs"], bf)
    Tfull = cfg["gen_len"]
    with torch.no_grad(), autocast(device_type="cuda", dtype=torch.bfloat16, enabled=bf):
        g0 = m.cached_greedy_generate(mem, mask, max_len=Tfull)
        # a max_len that cuts an accepted run: (max_len - 1) % (D + 1) != 0
        for D, T in ((4, 7), (7, 6), (2, 8), (7, 12), (1, 2), (4, 2)):
            g = m.cached_greedy_generate(mem, mask, max_len=T)
            assert g[0].shape[1] == T
            for src, tab in _tables(g, T, V).items():
                s, steps = _spec(m, mem, mask, T, D, drafts=tab)
                _same(g, s)
                if src == "oracle":
                    assert steps == [math.ceil((T - 1) / (D + 1))] * 3
            _same(g, _spec(m, mem, mask, T, D)[0])
        # <eos> inside an accepted run: the token image 0 emits at index 6 becomes <eos> (images 1 and 2 emit it elsewhere or never), on a
        # fresh model - captured decode graphs hold the <eos> id they were captured with
        m = build_vitomr(cfg, fx["state_dict"], dev, cdt, max_batch=24)
        old = m.decoder.eos_idx
        m.decoder.eos_idx = int(g0[0][0, 6])
        try:
            g = m.cached_greedy_generate(mem, mask, max_len=Tfull)
            Tn = g[2].sum(dim=1).tolist()
            assert Tn[0] == 7 and max(Tn) > 7, Tn
            for D in DS:
                for src, tab in _tables(g, Tfull, V).items():
                    s, steps = _spec(m, mem, mask, Tfull, D, drafts=tab)
                    _same(g, s)
                    if src == "oracle":
                        assert steps == [math.ceil((t - 1) / (D + 1)) for t in Tn], (D, steps, Tn)
                for form in (dict(), dict(poll=1, use_graph=False)):
                    _same(g, _spec(m, mem, mask, Tfull, D, **form)[0])
                _same(tuple(x[:1, :7] for x in g), _spec(m, mem[:1], mask[:1], Tfull, D)[0])
        finally:
            m.decoder.eos_idx = old


# ---- 3. the drafter: proposals read back after every step ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vitomr_small", "vitomr_dh64b", "vitomr_odd"])
def test_ngram_proposals_equal_the_restatement(dev, name):
    fx = load_golden(name)
    cfg = fx["cfg"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.float32, max_batch=24)
    mem, mask = _memory(m, fx["imgs"], False)
    T = cfg["max_len"]   # the longest run the cache allows: the toy decoders repeat themselves
    eng = m.decoder.decoder_blocks.engine(dev)
    with torch.no_grad():
        g = m.cached_greedy_generate(mem, mask, max_len=T)
        Tn = g[2].sum(dim=1).tolist()
        for D, ngram in ((4, 3), (7, 1), (2, 8)):
            seen = []
            s, steps = _spec(m, mem, mask, T, D, ngram=ngram, poll=1, use_graph=False,
                             on_chunk=lambda done: seen.append((eng.spec_t[:len(Tn)].tolist(), eng.spec_next[:len(Tn)].tolist(), eng.finished[:len(Tn)].tolist())))
            _same(g, s)
            accepted = 0
            for i, t_i in enumerate(Tn):
                want_steps, log = _restated_steps(g[0][i].cpu(), t_i, T, D, ngram, m.decoder.eos_idx)
                assert steps[i] == want_steps, (name, D, ngram, i)
                for k in range(want_steps - 1):   # after step k + 1 the image waits with the drafts of step k + 2
                    t, nxt, fin = (x[i] for x in seen[k])
                    assert not fin and t == log[k + 1][0] and nxt[1:D + 1] == log[k + 1][1] and nxt[0] == int(g[0][i, t - 1]), (name, D, ngram, i, k)
                assert seen[want_steps - 1][2][i] == 1
                accepted += (t_i - 1) - want_steps
            print(f"{name} D={D} ngram={ngram}: steps {steps} for {Tn} tokens, {accepted} draft tokens accepted")
            if name != "vitomr_dh64b":
                assert accepted > 0   # the sequences repeat: drafts are accepted


# ---- 4. isolation --------------------------------------------------------------------------------------------------------------------
def test_speculative_mode_leaves_other_modes_alone(dev):
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
            c = m.cached_continuous_generate(mem, mask, max_len=[T, T - 3, 5], slots=2)
        blocks = m.decoder.decoder_blocks
        mem32, lens = EG.unpad_rows(mem, mask)
        blocks.prepare_caches_packed(mem32, None, lens, group_size=2)
        s = tuple(x.clone() for x in blocks.engine(dev).sample(T, 5, 1.3, uniforms=u)[:2])
        return g + b + c + s

    def spec(m, mem, mask):
        with torch.no_grad(), autocast(device_type="cuda", dtype=torch.bfloat16):
            return m.cached_speculative_generate(mem, mask, max_len=T, draft_len=4) + \
                m.cached_speculative_generate(mem[:2], mask[:2], max_len=T - 2, draft_len=7, ngram=2)

    m0, mem0, mask0 = setup()
    fresh_others = others(m0, mem0, mask0)
    m1, mem1, mask1 = setup()
    fresh_spec = spec(m1, mem1, mask1)
    _same(fresh_others, others(m1, mem1, mask1))       # speculative, then greedy / beam / slot / sampling
    _same(fresh_spec, spec(m1, mem1, mask1))           # greedy / beam / slot / sampling, then speculative
    m2, mem2, mask2 = setup()
    others(m2, mem2, mask2)
    _same(fresh_spec, spec(m2, mem2, mask2))


# ---- 5. errors, the C ABI, inference ---------------------------------------------------------------------------------------------------
def test_errors_and_c_abi_checks(dev):
    from acai_omr_amd import _lib
    from acai_omr_amd import engine as EG
    fx = load_golden("vitomr_dh64b")
    cfg = fx["cfg"]
    T = cfg["gen_len"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.float32, max_batch=8)
    mem, mask = _memory(m, fx["imgs"], False)
    with torch.no_grad():
        for D in (0, 8):
            with pytest.raises(ValueError, match="draft_len must be in"):
                m.cached_speculative_generate(mem, mask, max_len=T, draft_len=D)
        with pytest.raises(ValueError, match="exceed the cache's max batch size"):
            m.cached_speculative_generate(mem, mask, max_len=T, draft_len=2)          # 3 x 3 rows > 8
        with pytest.raises(ValueError, match="ngram must be in"):
            m.cached_speculative_generate(mem[:1], mask[:1], max_len=T, draft_len=2, ngram=0)
        with pytest.raises(ValueError, match="drafts must be"):
            m.cached_speculative_generate(mem[:1], mask[:1], max_len=T, draft_len=2, drafts=torch.zeros(1, T + 1, dtype=torch.int64))
        with pytest.raises(RuntimeError, match="too long for max sequence length"):
            m.cached_speculative_generate(mem[:1], mask[:1], max_len=cfg["max_len"] + 1, draft_len=2)
        # the memories prepared for another mode (plain greedy rows, a beam / rollout group): not combinable
        blocks = m.decoder.decoder_blocks
        eng = blocks.engine(dev)
        mem32, lens = EG.unpad_rows(mem, mask)
        for kw in (dict(), dict(group_size=2), dict(group_size=4)):
            blocks.prepare_caches_packed(mem32[:lens[0]], None, lens[:1], **kw)
            with pytest.raises(ValueError, match="per_row_cross=True"):
                eng.speculative(T, 1)
        m.cached_speculative_generate(mem[:2], mask[:2], max_len=T, draft_len=3)
        # the engine's descriptors as the last run left them
        L = _lib.lib()
        st = torch.cuda.current_stream().cuda_stream
        d, sp = ctypes.byref(eng._desc), ctypes.byref(eng._spec_desc)
        eng.logits_step(torch.zeros(eng.B, dtype=torch.int64, device=dev), 1)   # overwrites x
        assert L.acai_decode_spec_step(d, sp, st) != 0 and b"x does not hold" in L.acai_last_error()
        for field, bad, msg in (("D", 0, b"outside [1, 7]"), ("D", 8, b"outside [1, 7]"), ("D", 1, b"cross_group"), ("ngram", 0, b"ngram"),
                                ("pitch", 1, b"pitch"), ("rows", 1, b"rows"), ("t", None, b"null")):
            keep = getattr(eng._spec_desc, field)
            setattr(eng._spec_desc, field, bad)
            try:
                assert L.acai_decode_spec_arm(d, sp, st) != 0 and msg in L.acai_last_error(), (field, L.acai_last_error())
            finally:
                setattr(eng._spec_desc, field, keep)
        assert L.acai_decode_spec_arm(d, sp, st) == 0
        keep = eng._desc.cross_group
        eng._desc.cross_group = 1
        try:
            assert L.acai_decode_spec_step(d, sp, st) != 0 and b"cross_group" in L.acai_last_error()
        finally:
            eng._desc.cross_group = keep
        torch.cuda.synchronize()
    f8 = build_vitomr(cfg, fx["state_dict"], dev, torch.bfloat16, max_batch=8, memory_cache_dtype=torch.float8_e4m3fn)
    with torch.no_grad(), pytest.raises(ValueError, match="FP8"):
        f8.cached_speculative_generate(mem[:1].to(torch.bfloat16), mask[:1], max_len=T, draft_len=2)


@pytest.mark.parametrize("name", FIXTURES)
def test_inference_entry_point(dev, name):
    from acai_omr_amd.inference.vitomr_inference import inference
    fx = load_golden(name)
    cfg = fx["cfg"]
    T = cfg["gen_len"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.bfloat16, max_batch=15)
    g = inference(m, fx["imgs"], "cuda", max_inference_len=T)
    _same(g, inference(m, fx["imgs"], "cuda", max_inference_len=T, speculative=4))
    _same(inference(m, fx["imgs"][0], "cuda", max_inference_len=T), inference(m, fx["imgs"][0], "cuda", max_inference_len=T, speculative=7))
    _same(g, inference(m, fx["imgs"], "cuda", max_inference_len=T, speculative=0))
    with pytest.raises(ValueError, match="beam"):
        inference(m, fx["imgs"], "cuda", max_inference_len=T, speculative=2, beam_width=2)
    with pytest.raises(ValueError, match="max batch size"):
        inference(m, fx["imgs"], "cuda", max_inference_len=T, speculative=7)

"""Speculative greedy decoding without a GPU: the plain-Python restatement (tests/speculative_reference.py) reproduces plain greedy for every
draft source, its step counts are the ones the design states, and the host-side argument checks raise as documented."""
import ctypes
import math
import os
import random
import re

import pytest
import torch

import spec_accept_cases as SC
import speculative_reference as SR
from conftest import ROOT, VOCAB

BOS, EOS, V = 0, 1, 11


def _toy(seed, period=None, eos_at=None):
    """A deterministic next_token(prefix): a hash of the last two tokens (never <eos>), or a periodic pattern; <eos> once the prefix has
    eos_at tokens."""
    def nxt(prefix):
        if eos_at is not None and len(prefix) == eos_at:
            return EOS
        if period is not None:
            return 2 + (len(prefix) % period + seed) % (V - 2)
        h = (prefix[-1] * 31 + (prefix[-2] if len(prefix) > 1 else 7) * 17 + seed * 13 + (len(prefix) // 9)) % (V - 2)
        return 2 + h
    return nxt


def _oracle_table(greedy, max_len):
    return list(greedy) + [SR.NONE] * (max_len - len(greedy))


def _adversarial_table(greedy, max_len):
    return [2 + (tok - 2 + 1) % (V - 2) if tok >= 2 else 2 for tok in greedy] + [3] * (max_len - len(greedy))   # every token changed


CASES = [(seed, period, eos_at, max_len) for seed in (0, 3) for period in (None, 3, 5) for eos_at in (None, 2, 7, 12, 13) for max_len in (2, 3, 9, 14, 24)]


@pytest.mark.parametrize("D", range(1, 8))
def test_restatement_reproduces_greedy_for_every_draft_source(D):
    for seed, period, eos_at, max_len in CASES:
        nxt = _toy(seed, period, eos_at)
        greedy = SR.greedy_decode(nxt, BOS, EOS, max_len)
        T = len(greedy)
        rnd = random.Random(seed * 100 + D)
        half = [tok if rnd.random() < 0.5 else 2 + (tok - 1) % (V - 2) for tok in _oracle_table(greedy, max_len)]
        sources = {"none": SR.no_drafts, "oracle": SR.table_proposals(_oracle_table(greedy, max_len)),
                   "adversarial": SR.table_proposals(_adversarial_table(greedy, max_len)), "half": SR.table_proposals(half),
                   "ngram1": SR.ngram_source(1), "ngram3": SR.ngram_source(3), "ngram8": SR.ngram_source(8)}
        for name, src in sources.items():
            seq, steps, log = SR.speculative_decode(nxt, BOS, EOS, max_len, D, src)
            assert seq == greedy, (name, D, seed, period, eos_at, max_len)
            assert sum(len(w) for _, _, w in log) == T - 1
            if name in ("none", "adversarial"):
                assert steps == T - 1
            if name == "oracle":
                assert steps == math.ceil((T - 1) / (D + 1))
            assert math.ceil((T - 1) / (D + 1)) <= steps <= T - 1


def test_no_accepted_draft_takes_max_len_minus_one_steps():
    for D in (1, 4, 7):
        seq, steps, _ = SR.speculative_decode(_toy(1), BOS, EOS, 24, D, SR.no_drafts)
        assert len(seq) == 24 and steps == 23


def test_ngram_drafter_rule():
    P = SR.ngram_proposals
    assert P([0], 3, 3) == [-1, -1, -1]                       # nothing earlier
    assert P([0, 5, 6, 7, 5, 6], 3, 3) == [7, 5, 6]          # suffix (5, 6) occurred at 1..2: what followed
    assert P([0, 5, 6, 7, 5, 6], 5, 3) == [7, 5, 6, -1, -1]  # only as far as the sequence goes
    assert P([0, 5, 6, 5, 7, 5], 2, 3) == [7, 5]             # most recent earlier occurrence of (5): index 3
    assert P([0, 5, 6, 9, 6], 2, 3) == [9, 6]                # m = 3, 2 fail, m = 1 matches
    assert P([0, 5, 5, 5], 2, 3) == [5, -1]                  # overlapping occurrence: e = 3
    assert P([0, 4, 5, 6], 2, 3) == [-1, -1]
    # a periodic sequence is drafted perfectly once one period is seen
    nxt = _toy(0, period=4)
    seq, steps, log = SR.speculative_decode(nxt, BOS, EOS, 40, 4, SR.ngram_source(3))
    assert seq == SR.greedy_decode(nxt, BOS, EOS, 40) and steps < 20
    assert all(len(w) == 5 for _, _, w in log[8:-1])


def test_struct_and_symbols_match_header():
    from acai_omr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "acai_omr_hip.h")).read()
    body = hdr[hdr.rindex("typedef struct {", 0, hdr.index("} AcaiSpec;")):hdr.index("} AcaiSpec;")]
    names = re.findall(r"\b([A-Za-z_]+)\s*;", body)
    assert [f for f, _ in _lib.AcaiSpec._fields_] == names == ["D", "ngram", "pitch", "rows", "t", "cap", "steps", "tab", "next", "drafts"]
    assert ctypes.sizeof(_lib.AcaiSpec) == 4 * 4 + 6 * 8
    for fn in ("acai_decode_spec_step", "acai_decode_spec_arm", "acai_debug_decode_spec_accept"):
        assert fn in _lib.exported_symbols() and re.search(r"\b" + fn + r"\s*\(", hdr)


# ---- one step as a state transition (speculative_reference.spec_step) against the chained restatements -----------------------------------
STEP_CASES = [(seed, period, eos_at, max_len) for seed in (0, 3) for period in (None, 3, 5)
              for eos_at, max_len in ((None, 24), (2, 9), (7, 14), (13, 24), (12, 3), (None, 2))]


def _chain(cfg, D, st, nxts, **src):
    """Iterates spec_step from the armed state st on logits planted from the toy streams.  -> (final state, per image log as
    speculative_decode's, per image [(index, float64 log-prob)])."""
    st = SR.spec_step(st, None, cfg, D, arm=True, **src)
    n_img = len(nxts)
    logs, lps = [[] for _ in nxts], [[] for _ in nxts]
    for _ in range(cfg.max_len):
        if int(st.finished[cfg.B]) == 0:
            break
        nx = SR.spec_step(st, SC.toy_logits(cfg, D, st, nxts), cfg, D, arm=False, **src)
        for i in range(n_img):
            if nx.written[i] is not None:
                t = int(st.t[i])
                drafts = [int(v) if int(v) >= 0 else SR.NONE for v in st.next[i, 1:D + 1]]
                logs[i].append((t, drafts, [int(v) for v in nx.seqs[i, t:t + nx.written[i]]]))
                lps[i] += [float(v) for v in nx.logprobs[i, t:t + nx.written[i]]]
        st = nx
    assert int(st.finished[cfg.B]) == 0
    return st, logs, lps


def _armed(cfg, D, caps, pitch):
    st = SR.new_spec_state(cfg, D, pitch)
    st.cap[:] = torch.tensor(caps)
    return st


@pytest.mark.parametrize("D", range(1, 8))
def test_spec_step_iterated_is_speculative_decode(D):
    """Every image of one state is one toy case with its own cap; every draft source; sequence, step count and per-step log."""
    T = 24
    nxts = [_toy(seed, period, eos_at) for seed, period, eos_at, _ in STEP_CASES]
    caps = [c[3] for c in STEP_CASES]
    greedy = [SR.greedy_decode(nxt, BOS, EOS, cap) for nxt, cap in zip(nxts, caps)]
    cfg = SC.make_cfg(V, len(nxts) * (D + 1), T, T, E=4, eos=EOS, pad=0, bos=BOS)
    rnd = random.Random(D)
    tables = {"none": [[SR.NONE] * T for _ in greedy], "oracle": [_oracle_table(g, T) for g in greedy],
              "adversarial": [_adversarial_table(g, T) for g in greedy],
              "half": [[tok if rnd.random() < 0.5 else 2 + (tok - 1) % (V - 2) for tok in _oracle_table(g, T)] for g in greedy]}
    runs = [(name, dict(drafts=torch.tensor(tb)), [SR.table_proposals(row) for row in tb]) for name, tb in tables.items()]
    runs += [(f"ngram{n}", dict(ngram=n), [SR.ngram_source(n)] * len(nxts)) for n in (1, 3, 8)]
    for name, src, sources in runs:
        st, logs, _ = _chain(cfg, D, _armed(cfg, D, caps, T), nxts, **src)
        for i, (nxt, cap) in enumerate(zip(nxts, caps)):
            seq, steps, log = SR.speculative_decode(nxt, BOS, EOS, cap, D, sources[i])
            assert seq == greedy[i] and [int(v) for v in st.seqs[i, :len(seq)]] == seq, (name, D, STEP_CASES[i])
            assert int(st.steps[i]) == steps and logs[i] == log, (name, D, STEP_CASES[i], logs[i], log)
            assert int(st.finished[i]) == 1 and int(st.t[i]) == len(seq)


@pytest.mark.parametrize("D", range(1, 8))
def test_spec_step_iterated_is_prompted_decoding(D):
    """The prompt source with both fall-backs: speculative_prompt_decode's sequence, steps and log, and prompt_decode run token by token
    (tokens and float64 log-probs of the same prefix-determined logits)."""
    import prompt_reference as PR
    T = 20
    nxt = _toy(1)
    prompts = [[], [5], [4, 9, 3], [6, 2, 7, 7, 3, 10, 4], [3, 8, 8, EOS], list(range(2, 11)) * 2 + [5], [9] * 12]
    assert len(prompts[5]) == T - 1
    cfg = SC.make_cfg(V, len(prompts) * (D + 1), T, T, E=4, eos=EOS, pad=0, bos=BOS)
    tok = torch.full((len(prompts), T + 3), -7, dtype=torch.int64)
    for i, p in enumerate(prompts):
        tok[i, 1:len(p) + 1] = torch.tensor(p, dtype=torch.int64)
    prompt = dict(tok=tok, len=torch.tensor([len(p) for p in prompts]))
    streams = [PR.prompted(nxt, p) for p in prompts]
    full = [SR.greedy_decode(s, BOS, EOS, T) for s in streams]
    table = [_oracle_table(g, T) for g in full]
    for name, src, fallbacks in (("ngram3", dict(ngram=3), [SR.ngram_source(3)] * len(prompts)),
                                 ("table", dict(drafts=torch.tensor(table)), [SR.table_proposals(row) for row in table])):
        st, logs, lps = _chain(cfg, D, _armed(cfg, D, [T] * len(prompts), T), [nxt] * len(prompts), prompt=prompt, **src)
        for i, p in enumerate(prompts):
            seq, steps, log = PR.speculative_prompt_decode(nxt, BOS, EOS, T, D, p, fallbacks[i])
            assert [int(v) for v in st.seqs[i, :len(seq)]] == seq == full[i] and int(st.steps[i]) == steps and logs[i] == log, (name, D, i)
            pseq, plps, _ = PR.prompt_decode(lambda s: SC.prefix_logits(s, nxt(s), V).double().tolist(), BOS, EOS, T, p)
            assert pseq == seq and len(lps[i]) == len(plps) - 1
            assert max(abs(a - b) for a, b in zip(lps[i], plps[1:])) < 1e-12, (name, D, i)


def test_accept_cases_write_what_they_are_named_for():
    """The images of the accept-rule test (spec_accept_cases.accept_images): the reference writes exactly the number of tokens each is built
    for, and the planted arg-max leads every row by at least 1.0."""
    for D in range(1, 8):
        for Vc in (3, 65, 512):
            imgs = SC.accept_images(D, Vc, 24)
            names = {im.name for im in imgs}
            assert {"n0", f"n{D}", "none_first", "eos_g0", "eos_after_last", "cap_at_end", "t_is_cap_minus_1", "tie_lower_is_draft",
                    "tie_higher_is_draft", "argmax_at_0"} <= names
            assert D < 2 or {"wrong_then_right", "eos_accepted", "cap_inside"} <= names
            assert D < 3 or "none_middle" in names
            assert Vc < 65 or {"argmax_at_63", "argmax_at_64", f"argmax_at_{Vc - 1}"} <= names
            cfg = SC.make_cfg(Vc, len(imgs) * (D + 1), 24, 28, E=4)
            lg = SC.plant_logits(cfg, D, imgs, D, Vc)
            SC.check_margins(lg, imgs, D)
            n = SR.spec_step(SC.build_state(cfg, D, 26, imgs), lg, cfg, D, arm=False, ngram=3)
            assert n.written == [im.expect for im in imgs], (D, Vc, [(im.name, w, im.expect) for im, w in zip(imgs, n.written) if w != im.expect])
            for i, im in enumerate(imgs):
                t = len(im.prefix)
                assert [int(v) for v in n.seqs[i, t:t + im.expect]] == im.greedy[:im.expect], im.name
                ends = im.name.startswith(("eos", "cap", "t_is"))
                assert int(n.finished[i]) == int(ends), im.name


def test_drafter_cases_discriminate():
    """The long histories (spec_accept_cases: every builder asserts its own property): reached through one verify step, the reference drafts
    what ngram_proposals gives on the finished history, and a drafter that looks at 64 candidate ends only differs on every far case."""
    count = 0
    for ngram in (1, 3, 8):
        for D in (1, 4, 7):
            cases = [(name, h, 0, None) for name, h in SC.single_occurrence_histories(ngram, D)]
            cases += [(name, h, acc, cap) for name, h, ng, acc, cap in SC.special_histories(D) if ng == ngram]
            assert {f"t{t}_{e}" for t in (130, 150, 199) for e in ("e_t-1", "e_t-64", "e_t-65", "e_m")} <= {c[0] for c in cases}
            assert {"t150_e_t-129", "t199_e_t-129", "t66_e_t-1"} <= {c[0] for c in cases}
            imgs = [SC.history_image(h, D, acc, cap) for _, h, acc, cap in cases]
            cfg = SC.make_cfg(512, len(imgs) * (D + 1), 200, 208, E=4)
            n = SR.spec_step(SC.build_state(cfg, D, 200, imgs), SC.plant_logits(cfg, D, imgs, ngram, D), cfg, D, arm=False, ngram=ngram)
            for i, (name, h, acc, cap) in enumerate(cases):
                t = len(h)
                assert int(n.t[i]) == t and [int(v) for v in n.seqs[i, :t]] == h and n.written[i] == 1 + acc, name
                want = [v if t + j < (cap or 200) else SR.NONE for j, v in enumerate(SR.ngram_proposals(h, D, ngram), start=1)]
                assert [int(v) for v in n.next[i, 1:D + 1]] == want, name
                count += 1
    assert count > 120


def _cpu_vit(max_batch, memory_cache_dtype=None):
    from acai_omr_amd.models.models import OMRDecoder, ViTOMR
    dec = OMRDecoder(16, VOCAB, num_layers=1, hidden_dim=32, num_heads=2, mlp_dim=64)
    return ViTOMR(None, None, dec.to_cached_version(max_batch, torch.bfloat16, memory_cache_dtype).eval())


def test_host_argument_checks_raise_without_a_gpu():
    m = _cpu_vit(8)
    lat = torch.zeros(2, 4, 32)
    for D in (0, 8, -1):
        with pytest.raises(ValueError, match="draft_len"):
            m.cached_speculative_generate(lat, None, max_len=8, draft_len=D)
    with pytest.raises(ValueError, match="max batch size"):
        m.cached_speculative_generate(lat, None, max_len=8, draft_len=4)      # 2 x 5 rows > 8
    with pytest.raises(ValueError, match="max batch size"):
        _cpu_vit(4).cached_speculative_generate(lat[:1], None, max_len=8, draft_len=4)
    with pytest.raises(ValueError, match="FP8"):
        _cpu_vit(8, torch.float8_e4m3fn).cached_speculative_generate(lat[:1], None, max_len=8, draft_len=2)
    from acai_omr_amd.inference.vitomr_inference import inference
    with pytest.raises(ValueError, match="beam"):
        inference(m, [torch.zeros(1, 32, 32)], "cpu", speculative=2, beam_width=2)
    import inspect
    sig = inspect.signature(inference)
    assert sig.parameters["speculative"].default == 0

"""Prompted decoding without a GPU: the plain-Python restatement (tests/prompt_reference.py) - tokens and log-probs at forced and free
indices, a prompt-final <eos>, P = 0, P = max_len - 1, ragged batches, the speculative prompt step's verify-step count - and the argument
validation of the public entry points, the C ABI declaration and the ctypes mirror."""
import ctypes
import math
import os
import re

import pytest
import torch

import prompt_reference as PR
import speculative_reference as SR
from conftest import ROOT, VOCAB

BOS, EOS, V = 0, 1, 11


def _logits(seed):
    """step_logits(seq): deterministic logits from the last two tokens and the index, never preferring <bos>; <eos> wins at some indices."""
    def f(seq):
        g = torch.Generator().manual_seed(seed * 7919 + seq[-1] * 131 + (seq[-2] if len(seq) > 1 else 5) * 17 + len(seq))
        lg = (torch.randn(V, generator=g, dtype=torch.float64) * 3).tolist()
        lg[BOS] = -50.0
        return lg
    return f


def _greedy_token(step_logits):
    return lambda prefix: PR.argmax_first(step_logits(list(prefix)))


def test_log_prob_is_log_softmax_and_exact_for_the_argmax():
    lg = _logits(3)([BOS, 4, 7])
    ref = torch.log_softmax(torch.tensor(lg, dtype=torch.float64), 0)
    for k in range(V):
        assert abs(PR.log_prob(lg, k) - float(ref[k])) < 1e-12
    a = PR.argmax_first(lg)
    m = max(lg)
    assert PR.log_prob(lg, a) == -math.log(sum(math.exp(v - m) for v in lg))   # first term exactly 0: the greedy step's value
    assert PR.argmax_first([1.0, 5.0, 5.0, 2.0]) == 1                           # first index on ties


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_forced_and_free_indices(seed):
    f = _logits(seed)
    max_len = 20
    g_seq, g_lp, _ = PR.prompt_decode(f, BOS, EOS, max_len, [])            # P = 0 is plain greedy
    assert g_seq == SR.greedy_decode(_greedy_token(f), BOS, EOS, max_len)
    L = len(g_seq) - 1
    # the model's own output as the prompt, every split: the same tokens and log-probs, bit for bit
    for P in sorted({0, 1, 2, L // 2, L - 1, L}):
        if 0 <= P <= L:
            seq, lp, forced = PR.prompt_decode(f, BOS, EOS, max_len, g_seq[1:1 + P])
            assert seq == g_seq and lp == g_lp and forced == [False] + [True] * P + [False] * (L - P), P
    # tokens the model would not choose
    prompt = [2 + (seed + 3 * i) % (V - 2) for i in range(6)]
    seq, lp, forced = PR.prompt_decode(f, BOS, EOS, max_len, prompt)
    assert seq[1:7] == prompt and forced[1:7] == [True] * 6 and not any(forced[7:])
    differs = 0
    for t in range(1, len(seq)):
        lg = f(seq[:t])
        want = torch.log_softmax(torch.tensor(lg, dtype=torch.float64), 0)[seq[t]]
        assert abs(lp[t] - float(want)) < 1e-12
        if t <= 6:
            differs += seq[t] != PR.argmax_first(lg)
        else:
            assert seq[t] == PR.argmax_first(lg)                                # free indices: greedy on the forced context
    assert differs >= 3


def test_prompt_final_eos_and_full_length_prompt():
    f = _logits(5)
    max_len = 12
    seq, lp, forced = PR.prompt_decode(f, BOS, EOS, max_len, [4, 6, EOS])
    assert seq == [BOS, 4, 6, EOS] and forced == [False, True, True, True] and len(lp) == 4     # the row ends there
    full = [2 + i % (V - 2) for i in range(max_len - 1)]
    seq, lp, forced = PR.prompt_decode(f, BOS, EOS, max_len, full)                                # P = max_len - 1: nothing is free
    assert seq == [BOS] + full and all(forced[1:]) and len(seq) == max_len
    with pytest.raises(AssertionError):
        PR.prompt_decode(f, BOS, EOS, max_len, full + [3])


def test_ragged_batch_and_the_unfinished_count():
    fs = [_logits(s) for s in (0, 1, 2, 3)]
    step = lambda i, seq: fs[i](seq)   # noqa: E731
    max_len = 14
    prompts = [[], [5, 3, EOS], [2 + i % 5 for i in range(max_len - 1)], [7, 7]]
    rows, counts = PR.batch_decode(step, BOS, EOS, max_len, prompts)
    for i, (seq, lp) in enumerate(rows):
        alone, alone_lp, _ = PR.prompt_decode(fs[i], BOS, EOS, max_len, prompts[i])
        assert PR.clip(seq, EOS) == alone and lp[:len(alone)] == alone_lp                         # a row does not depend on its neighbours
    assert len(counts) == max_len - 1 and counts[-1] >= 1        # the full-length prompt holds the batch to the last step ...
    assert all(c >= 1 for c in counts[:-1])                      # ... and counts as unfinished while it is inside its prompt
    # all rows end with their prompts: the batch exits right after the longest one
    rows, counts = PR.batch_decode(step, BOS, EOS, max_len, [[5, EOS], [4, 4, 4, EOS], [EOS]])
    assert counts == [2, 1, 1, 0] and [PR.clip(s, EOS) for s, _ in rows] == [[BOS, 5, EOS], [BOS, 4, 4, 4, EOS], [BOS, EOS]]
    # an <eos> the model generates right after the prompt
    rows, counts = PR.batch_decode(lambda i, seq: [0.0, 9.0 if len(seq) == 4 else -9.0] + [1.0] * (V - 2), BOS, EOS, max_len, [[3, 3, 3]])
    assert counts == [1, 1, 1, 0] and rows[0][0] == [BOS, 3, 3, 3, EOS]


@pytest.mark.parametrize("D", range(1, 8))
def test_speculative_prompt_steps_and_tokens(D):
    max_len = 40
    for seed in (0, 4):
        f = _logits(seed)
        nxt = _greedy_token(f)
        for P in (0, 1, D, D + 1, D + 2, 2 * (D + 1) - 1, 2 * (D + 1), 17, max_len - 1):
            prompt = [2 + (seed + 5 * i) % (V - 2) for i in range(P)]
            want, _, _ = PR.prompt_decode(f, BOS, EOS, max_len, prompt)
            seq, steps, log = PR.speculative_prompt_decode(nxt, BOS, EOS, max_len, D, prompt)
            assert seq == want, (D, P)
            # the prompt and the first free token: ceil((P + 1) / (D + 1)) steps, the last of them crossing the prompt's end
            n_first = min(PR.verify_steps(P, D), len(log))
            written = sum(len(w) for _, _, w in log[:n_first])
            assert written == min(P + 1, len(want) - 1), (D, P, log[:n_first])
            if P + 1 <= len(want) - 1 and P > 0:
                t, drafts, w = log[n_first - 1]
                assert t + len(w) - 1 == P + 1                               # it ends on the first free token ...
                if P % (D + 1):
                    assert t <= P and len(w) == P - t + 2                    # ... and crosses the prompt's end unless a step ended on it
                    assert drafts[:P - t + 1] == prompt[t - 1:]
                assert all(d == PR.NONE for d in drafts[max(P - t + 1, 0):]) # no draft past the prompt
                assert sum(len(x) for _, _, x in log[:n_first - 1]) < P + 1  # and it took every one of those steps
            # without other drafts every later step emits one token
            assert steps == n_first + max(0, len(want) - 1 - written)
            # with the n-gram drafter after the prompt the tokens stay the same
            seq2, steps2, _ = PR.speculative_prompt_decode(nxt, BOS, EOS, max_len, D, prompt, SR.ngram_source(3))
            assert seq2 == want and steps2 <= steps
        # a prompt-final <eos> inside an accepted run ends the sequence there
        prompt = [3, 4, 5, EOS]
        seq, steps, log = PR.speculative_prompt_decode(nxt, BOS, EOS, max_len, D, prompt)
        assert seq == [BOS] + prompt and steps == math.ceil(4 / (D + 1))


def test_verify_step_formula():
    assert [PR.verify_steps(P, 7) for P in (0, 6, 7, 8, 14, 15, 512)] == [1, 1, 1, 2, 2, 2, 65]
    assert [PR.verify_steps(P, 3) for P in (0, 2, 3, 4, 512)] == [1, 1, 1, 2, 129]
    assert PR.verify_steps(512, 1) == 257


def test_struct_and_symbols_match_header():
    from acai_omr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "acai_omr_hip.h")).read()
    body = hdr[hdr.rindex("typedef struct {", 0, hdr.index("} AcaiPrompt;")):hdr.index("} AcaiPrompt;")]
    names = re.findall(r"\b([A-Za-z_]+)\s*;", body)
    assert [f for f, _ in _lib.AcaiPrompt._fields_] == names == ["tok", "len", "pitch", "rows"]
    assert ctypes.sizeof(_lib.AcaiPrompt) == 2 * 8 + 2 * 4
    for fn in ("acai_decode_prompt_step", "acai_decode_spec_prompt_arm", "acai_decode_spec_prompt_step"):
        assert fn in _lib.exported_symbols() and re.search(r"\b" + fn + r"\s*\(", hdr)


def _cpu_vit(max_batch):
    from acai_omr_amd.models.models import OMRDecoder, ViTOMR
    dec = OMRDecoder(16, VOCAB, num_layers=1, hidden_dim=32, num_heads=2, mlp_dim=64)
    return ViTOMR(None, None, dec.to_cached_version(max_batch, torch.bfloat16).eval())


def test_prefix_validation_raises_without_a_gpu():
    from acai_omr_amd.inference import vitomr_inference as VI
    m = _cpu_vit(8)
    dec = m.decoder
    Vn, bos, pad, eos = dec.vocab_size, dec.bos_idx, dec.pad_idx, dec.eos_idx
    ok = next(i for i in range(Vn) if i not in (bos, pad, eos))
    chk = m._check_prefix
    assert chk(None, 2, 16) is None
    out = chk([[ok, ok], torch.tensor([], dtype=torch.int64), torch.tensor([ok, eos], dtype=torch.int32)], 3, 16)
    assert [o.tolist() for o in out] == [[ok, ok], [], [ok, eos]] and all(o.dtype == torch.int64 for o in out)
    assert [o.tolist() for o in chk(torch.tensor([ok, ok, ok]), 1, 16)] == [[ok, ok, ok]]          # one 1-D tensor: one image
    assert [o.tolist() for o in chk([[ok] * 15], 1, 16)] == [[ok] * 15]                           # P = max_len - 1 is allowed
    for bad, n, msg in (([[ok]], 2, "entries for 2 images"), ([[ok], [Vn]], 2, "outside"), ([[-1]], 1, "outside"),
                        ([[ok, bos]], 1, "<bos> or <pad>"), ([[pad]], 1, "<bos> or <pad>"), ([[ok, eos, ok]], 1, "<eos> before its end"),
                        ([[ok] * 16], 1, "more than max_len - 1"), ([[0.5, 1.5]], 1, "integer"), ([[[ok]]], 1, "1-D")):
        with pytest.raises(ValueError, match=msg):
            chk(bad, n, 16)
    lat = torch.zeros(2, 4, 32)
    # the entry points validate before anything reaches the device, and the unsupported combinations say so
    with pytest.raises(ValueError, match="entries for 2 images"):
        m.cached_greedy_generate(lat, None, max_len=8, prefix=[[ok]])
    with pytest.raises(ValueError, match="<eos> before its end"):
        m.cached_speculative_generate(lat, None, max_len=8, draft_len=2, prefix=[[eos, ok], []])
    with pytest.raises(ValueError, match="more than max_len - 1"):
        next(m.streamed_cached_greedy_generate(lat[:1], None, max_len=4, prefix=[[ok] * 4]))
    for call in (lambda: m.cached_beam_generate(lat, None, beam_width=2, max_len=8, prefix=[[ok], []]),
                 lambda: m.cached_continuous_generate(lat, None, max_len=8, prefix=[[ok], []]),
                 lambda: VI.inference(m, None, "cuda", max_inference_len=8, beam_width=2, prefix=[[ok]]),
                 lambda: VI.continuous_inference(m, [], "cuda", prefix=[[ok]]),
                 lambda: VI.iter_continuous_inference(m, [], "cuda", prefix=[[ok]])):
        with pytest.raises(ValueError, match="out of scope here"):
            call()
    from acai_omr_amd.models.models import GRPOViTOMR
    with pytest.raises(ValueError, match="out of scope here"):
        GRPOViTOMR.cached_forward_rollout_policy(m, lat, None, prefix=[[ok], []])

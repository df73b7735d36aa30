"""CPU checks of the float64 beam-search reference (tests/beam_reference.py) that the GPU beam tests compare against:
beam width 1 is the oracle's greedy decode, and every returned hypothesis's cumulative log-prob equals a teacher-forced re-scoring."""
import pytest
import torch

from beam_reference import beam_generate, rescore
from conftest import load_golden


def _case(name):
    fx = load_golden(name)
    cfg, ref = fx["cfg"], fx["ref_fp32"]
    sd = {k: v.double() for k, v in fx["state_dict"].items() if k.startswith("decoder.")}
    valid = ~ref["latent_mask"]
    lens = valid.sum(1).tolist()
    mem = ref["memory"][valid].double()
    return cfg, sd, mem, lens


@pytest.mark.parametrize("name", ["vitomr_small", "vitomr_dh64", "vitomr_odd"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_width_one_is_greedy(name, prec):
    from oracle import vitomr_oracle as O
    cfg, sd, mem, lens = _case(name)
    out = beam_generate(mem, lens, sd, cfg["dec_heads"], prec, 1, cfg["gen_len"])
    s, lp, m = O.greedy_generate(mem, lens, sd, cfg["dec_heads"], prec, cfg["gen_len"])
    assert torch.equal(out["seqs"], s) and torch.equal(out["mask"], m)
    assert float((out["log_probs"] - lp.double()).abs().max()) < 1e-6   # (the oracle keeps its log-probs in an fp32 tensor)
    # cum of a width-1 beam is the sum of its (unrounded) per-token log-probs
    assert torch.allclose(out["cum"], rescore(mem, lens, sd, cfg["dec_heads"], prec, out["seqs"]), rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("name,K,alpha", [("vitomr_small", 3, 1.0), ("vitomr_dh64", 4, 0.0), ("vitomr_odd", 5, 0.7)])
def test_cum_equals_teacher_forced_rescoring(name, K, alpha):
    cfg, sd, mem, lens = _case(name)
    out = beam_generate(mem, lens, sd, cfg["dec_heads"], "fp32", K, cfg["gen_len"], alpha=alpha)
    assert len(out["margins"]) == out["steps"]
    tot = rescore(mem, lens, sd, cfg["dec_heads"], "fp32", out["seqs"])
    assert torch.allclose(out["cum"], tot, rtol=1e-10, atol=1e-10), (out["cum"], tot)
    # every live slot's cum re-scores as well, and the slots of an image are ordered by cum
    n = len(lens)
    for i in range(n):
        c = out["slot_cum"][i * K:(i + 1) * K]
        assert bool((c[:-1] >= c[1:]).all())


"""Clipping by the global gradient norm inside the fused AdamW step, as far as it can be checked without a device: the float64 restatement
of tests/clip_reference.py against torch's own clip + AdamW in fp32, the C ABI declarations, and that the new optimizer arguments stay out
of what a checkpoint carries."""
import inspect
import os
import re

import pytest
import torch

import clip_reference as C
import row_reference as R
from test_gpu_row_kernels import P_BAR, V_BAR, within

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("max_norm", C.MAX_NORMS)
@pytest.mark.parametrize("case", R.ADAMW_CASES)
def test_restatement_matches_torch_clip_and_adamw(case, max_norm):
    """torch.nn.utils.clip_grad_norm_(foreach=False) + torch.optim.AdamW(foreach=False) in fp32 on the CPU stay inside the bars the GPU tests
    use (measured: at most 0.32 of them, the norm within 1.5e-7 relative), so the restatement states what torch computes."""
    params, grads, hyper = R.adamw_case(case)
    theirs = [torch.nn.Parameter(p.clone()) for p in params]
    ot = torch.optim.AdamW(R.adamw_groups(theirs, hyper), foreach=False)
    p64, m64, v64, steps, norms, coefs = C.clipped_adamw_run(params, grads, hyper, max_norm)
    worst = 0.0
    for it, gs in enumerate(grads):
        for b, g in zip(theirs, gs):
            b.grad = None if g is None else g.clone()
        total = torch.nn.utils.clip_grad_norm_(theirs, max_norm=max_norm, foreach=False)
        assert abs(float(total) - norms[it]) <= 2 * C.ULP32 * norms[it], (case, max_norm, it)
        ot.step()
    for i, b in enumerate(theirs):
        tag = (case, max_norm, R.ADAMW_SIZES[i])
        st = ot.state[b]
        assert float(st["step"]) == steps[i], tag
        for got, ref, bar in ((b, p64[i], P_BAR), (st["exp_avg"], m64[i], P_BAR), (st["exp_avg_sq"], v64[i], V_BAR)):
            w = within(got, ref, **bar)
            worst = max(worst, w)
            assert w <= 1.0, (tag, w)
    print(f"{case} max_norm={max_norm}: torch fp32 uses {worst:.2f} of the bars; norms {norms[0]:.1f} / {norms[2]:.1f}, coefficients {coefs[0]:.3g} / {coefs[2]:.3g}")
    if case != "zero_grad":     # 1.0 always clips, 300 only the louder third step, 1e4 never
        assert [c < 1.0 for c in coefs] == {1.0: [True] * 6, 300.0: [False, False, True, False, False, False], 1e4: [False] * 6}[max_norm]
    else:
        assert norms == [0.0] * 6 and coefs == [1.0] * 6


def test_coefficient_formulas_agree():
    for n in (0.0, 0.5, 1.0, 285.3, 2870.0):
        for mx in C.MAX_NORMS:
            assert abs(float(C.clip_coef_fp32(torch.tensor(n), mx)) - C.clip_coef(n, mx)) <= 4 * C.ULP32
    assert C.clip_coef(5.0, 0.0) == C.clip_coef(5.0, -1.0) == C.clip_coef(5.0, float("inf")) == 1.0


def test_new_symbols_are_declared():
    from acai_omr_amd import _lib
    hdr = open(os.path.join(HERE, "..", "include", "acai_omr_hip.h")).read()
    for name in ("acai_grad_norm", "acai_adamw_step_clipped"):
        assert re.search(r"\bint " + name + r"\s*\(", hdr) and name in _lib._SIGNATURES, name
    m = re.search(r"int acai_grad_norm\(([^;]*)\);", hdr)
    params = [p.strip().split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")]
    assert params == ["tensors", "chunk_tensor", "chunk_off", "tensor_chunk0", "n_tensors", "n_chunks", "chunk_elems", "grad_scale", "max_norm",
                      "workspace", "tensor_norm", "result", "stream"]
    assert len(_lib._SIGNATURES["acai_grad_norm"][1]) == len(params)
    m = re.search(r"int acai_adamw_step_clipped\(([^;]*)\);", hdr)
    params = [p.strip().split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")]
    assert params == ["tensors", "groups", "chunk_tensor", "chunk_off", "n_chunks", "chunk_elems", "grad_scale", "result", "skip_nonfinite", "skipped",
                      "stream"]
    assert len(_lib._SIGNATURES["acai_adamw_step_clipped"][1]) == len(params)
    for word, value in (("TOTAL", _lib.GRAD_NORM_TOTAL), ("COEF", _lib.GRAD_NORM_COEF), ("FINITE", _lib.GRAD_NORM_FINITE), ("WORDS", _lib.GRAD_NORM_WORDS)):
        assert re.search(r"#define ACAI_GRAD_NORM_" + word + r" " + str(value) + r"\b", hdr), word


def test_clip_arguments_stay_out_of_checkpoints():
    """max_grad_norm / skip_nonfinite are not group hyper-parameters: state_dict() and param_groups look as they did, and as torch.optim.AdamW's
    own do for the keys FusedAdamW has."""
    from acai_omr_amd.optim import FusedAdamW
    def make(**kw):
        ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(5))]
        return FusedAdamW([dict(params=ps[:1], lr=1e-3), dict(params=ps[1:], weight_decay=0.0)], lr=2e-3, **kw)
    plain, clipped = make(), make(max_grad_norm=1.0, skip_nonfinite=False)
    assert clipped.defaults == plain.defaults and set(plain.defaults) == {"lr", "betas", "eps", "weight_decay"}
    assert [set(g) for g in clipped.param_groups] == [set(g) for g in plain.param_groups]
    assert set(clipped.state_dict()) == set(plain.state_dict()) == {"state", "param_groups"}
    assert [set(g) for g in clipped.state_dict()["param_groups"]] == [set(g) for g in plain.state_dict()["param_groups"]]
    assert clipped.grad_norm is None and clipped.clip_coef is None and clipped.skipped_steps is None and clipped.grad_norms() is None


def test_python_surface():
    from acai_omr_amd import ops
    from acai_omr_amd.optim import FusedAdamW
    from acai_omr_amd.train import grpo as G
    sig = inspect.signature(FusedAdamW.__init__).parameters
    assert sig["max_grad_norm"].default is None and sig["skip_nonfinite"].default is True
    assert list(sig)[:8] == ["self", "params", "lr", "betas", "eps", "weight_decay", "amsgrad", "maximize"]
    sig = inspect.signature(FusedAdamW.step).parameters
    assert list(sig) == ["self", "closure", "grad_scale", "max_grad_norm"] and sig["grad_scale"].default == 1.0
    sig = inspect.signature(G.grpo_update).parameters
    assert list(sig)[-2:] == ["grammar", "fused_clip"] and sig["fused_clip"].kind is inspect.Parameter.KEYWORD_ONLY and sig["fused_clip"].default is False
    sig = inspect.signature(ops.grad_norm).parameters
    assert sig["grad_scale"].kind is inspect.Parameter.KEYWORD_ONLY and sig["per_tensor"].default is False
    with pytest.raises(RuntimeError):       # no CPU fallback
        ops.grad_norm([torch.zeros(4)])
    with pytest.raises(ValueError):         # refused before anything runs
        G.grpo_update(None, None, torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1), [], None, None, "cpu", reward_fn=None, fused_clip=True)

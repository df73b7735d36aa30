"""The float64 reference of tests/test_gpu_decode_self_attn.py is itself right, its defects are loud, and the GPU bar has room (no GPU).

On every case the GPU file compares with float64:
  * the reference - which finds its keys through the step / length / table operands, as a kernel must - equals a per-key loop over the
    logical rows the builders started from, so the builders and the resolution agree;
  * the plain form equals torch's scaled_dot_product_attention in float64;
  * every defect that applies to the form moves the result by at least four times the GPU bar (2e-5) - a kernel that made the same mistake
    could not pass - where a result poisoned by NaN counts as moved without bound;
  * plain fp32 torch stays under a quarter of the bar: a correct kernel has room.
The rollout-group cases also hold the condition of the one-hot inputs: the reference is the selected V row to 1e-9.

`python tests/test_decode_attn_reference_cpu.py` prints the smallest effect of each defect per form."""
import pytest
import torch
import torch.nn.functional as F

import decode_attn_reference as R


def _self_cases(form):
    """Every self-form case of the GPU file at this (dtype, dh); the speculative ones at both values of chunk nsplit."""
    cs = R.self_cases(*form, 256)
    return cs + [(n + "_cover192", c) for n, c in R.spec_cases(*form, 192)]


def _check(name, case, effects=None):
    ref = R.reference(case)
    assert bool(torch.isfinite(ref).all()), name
    assert float((ref - R.naive(case)).abs().max()) < 1e-12, name
    assert R.moved(R.fp32_torch(case).double(), ref) < R.BAR / 4, (name, R.moved(R.fp32_torch(case).double(), ref))
    if case.form == "plain":
        q = case.q.double().view(-1, R.H, 1, case.dh)
        n = int(case.step[1]) + 1
        sd = F.scaled_dot_product_attention(q, case.kc[:, :, :n, :case.dh].double(), case.vc[:, :, :n, :case.dh].double())
        assert float((sd.reshape(ref.shape) - ref).abs().max()) < 1e-12, name
    defects, family = R.defects_for(case)
    for d in defects:
        eff = R.moved(R.reference(case, d), ref)
        assert eff >= 4 * R.BAR, (name, d, eff)
        if effects is not None:
            key = (family, d)
            effects[key] = min(effects.get(key, float("inf")), eff)


@pytest.mark.parametrize("form", R.FORMS, ids=R.form_id)
def test_self_form_reference(form):
    for name, case in _self_cases(form):
        _check(f"{R.form_id(form)} {name}", case)


@pytest.mark.parametrize("group", list(R.GROUP_MEMS))
def test_group_reference(group):
    for dh in (64, 48):
        for kind in ("mean", "onehot"):
            case = R.build_group(dh, group, kind)
            _check(f"group{group} dh{dh} {kind}", case)
            ref = R.reference(case)
            if kind == "onehot":
                assert float((ref - R.one_hot_targets(case)).abs().max()) < 1e-9
            else:
                mean = torch.stack([v.double().mean(1).reshape(-1) for _, _, v in case.logical])
                assert float((ref - mean).abs().max()) < 1e-12


def test_builders_keep_their_promises():
    """NaN wherever no key lives, zero pad columns, tables in range."""
    for form in (("bf16", 12), ("fp32", 64)):
        dh = form[1]
        for name, c in _self_cases(form) + [("ring_identity", R.build_ring(*form, identity=True)),
                                            ("ancestor_identity", R.build_ancestor(*form, 65, 1, identity=True))]:
            used = torch.zeros(c.kc.shape[:3], dtype=torch.bool).reshape(-1)
            for b in range(c.q.shape[0]):
                for h in range(R.H):
                    used[R._key_rows(c, b, h, None)] = True
            for cache in (c.kc, c.vc):
                live = torch.isfinite(cache[..., :dh]).all(-1).reshape(-1)
                dead = torch.isnan(cache[..., :dh]).all(-1).reshape(-1)
                assert torch.equal(live, used) and torch.equal(dead, ~used), name
                assert bool((cache[..., dh:] == 0).all()), name
            rows = c.kc.shape[0]
            if c.form == "ancestor":
                assert int(c.table.min()) >= 0 and int(c.table.max()) < rows and c.pitch > R.TMAX, name
            if c.form == "ring":
                assert int(c.table.min()) >= 0 and int(c.table.max()) < R.TMAX, name
                assert all(f != 0 for f, n in zip(c.table.tolist(), c.lens) if n == R.TMAX) or "identity" in name
            if c.form == "spec":
                assert int(c.table.min()) >= 0 and int((c.table >> 3).max()) < R.TMAX and int((c.table & 7).max()) < c.stride, name


def test_ring_windows_cover_every_kind():
    for v in (0, 1):
        first = R.ring_firsts(R.LENGTHS, v)
        ends = [(f, f + n - 1) for f, n in zip(first, R.LENGTHS)]
        assert any(e < R.TMAX - 1 for _, e in ends) and any(e == R.TMAX - 1 and f < R.TMAX - 1 for f, e in ends)
        assert any(f == R.TMAX - 1 and e > f for f, e in ends) and any(f < R.TMAX - 1 and e >= R.TMAX for f, e in ends)


if __name__ == "__main__":
    eff = {}
    for form in R.FORMS:
        for name, case in _self_cases(form):
            _check(name, case, eff)
    for name, case in R.group_cases():
        _check(name, case, eff)
    for (fam, d), e in sorted(eff.items()):
        print(f"{fam:13s} {d:24s} smallest effect over the cases {e:.3g}   (bar {R.BAR:g})")

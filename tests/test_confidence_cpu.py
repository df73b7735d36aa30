"""Per-token confidence without a GPU: the references of tests/confidence_reference.py against rows worked by hand, and every argument
error of the public layer raised before the HIP library is touched."""
import math

import pytest
import torch

import confidence_reference as R
from conftest import VOCAB

INF = float("inf")


# ---- the reference against hand-worked rows --------------------------------------------------------------------------------------------
def test_order_breaks_ties_by_index():
    row = torch.tensor([1.0, 3.0, 3.0, -2.0, 3.0, 1.0], dtype=torch.float64)
    assert R.order(row).tolist() == [1, 2, 4, 0, 5, 3]
    assert [R.rank_of(row, c) for c in range(6)] == [3, 0, 1, 5, 2, 4]
    lp, ent, rank, ids, tlp = R.token_confidence(row[None].repeat(6, 1), torch.arange(6), 3)
    assert rank.tolist() == [3, 0, 1, 5, 2, 4]
    assert ids.tolist() == [[1, 2, 4]] * 6
    # by hand: sum exp = 3 e^3 + 2 e + e^-2
    lse = math.log(3 * math.exp(3) + 2 * math.exp(1) + math.exp(-2))
    assert float((lp - (row - lse)).abs().max()) < 1e-14
    assert float((tlp - (3.0 - lse)).abs().max()) < 1e-14
    p = torch.exp(row - lse)
    assert abs(float(ent[0]) + float((p * (row - lse)).sum())) < 1e-14


@pytest.mark.parametrize("V", [1, 5, 230])
def test_constant_row(V):
    """Every token ties: entropy log V, every log-probability -log V, rank = chosen, top-k 0 .. K-1; whatever the temperature."""
    K = min(V, 8)
    logits = torch.full((V, V), -7.25, dtype=torch.float64)
    for tau in (1.0, 0.5, 2.0):
        lp, ent, rank, ids, tlp = R.token_confidence(logits, torch.arange(V), K, tau)
        assert rank.tolist() == list(range(V))
        assert ids.tolist() == [list(range(K))] * V
        assert float((ent - math.log(V)).abs().max()) < 1e-13
        assert float((lp + math.log(V)).abs().max()) < 1e-13 and float((tlp + math.log(V)).abs().max()) < 1e-13


def test_minus_inf_entries_come_last_by_index_and_add_no_entropy():
    row = torch.tensor([-INF, 0.0, -INF, math.log(3.0), -INF], dtype=torch.float64)   # p = (0, 1/4, 0, 3/4, 0)
    lp, ent, rank, ids, tlp = R.token_confidence(row[None].repeat(5, 1), torch.arange(5), 5)
    assert ids[0].tolist() == [3, 1, 0, 2, 4]
    assert rank.tolist() == [2, 1, 3, 0, 4]
    want = torch.tensor([-INF, math.log(0.25), -INF, math.log(0.75), -INF], dtype=torch.float64)
    assert bool((lp[[0, 2, 4]] == -INF).all()) and float((lp[[1, 3]] - want[[1, 3]]).abs().max()) < 1e-15
    assert tlp[0, 2:].tolist() == [-INF] * 3
    h = -(0.25 * math.log(0.25) + 0.75 * math.log(0.75))
    assert float((ent - h).abs().max()) < 1e-15 and bool(torch.isfinite(ent).all())


def test_temperature_scales_the_logits_not_the_order():
    row = torch.tensor([[0.0, 2.0, 1.0, 2.0]], dtype=torch.float64)
    a = R.token_confidence(row, torch.tensor([2]), 4, 1.0)
    b = R.token_confidence(row, torch.tensor([2]), 4, 2.0)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and a[3].tolist() == [[1, 3, 2, 0]]
    want = torch.log_softmax(row / 2.0, -1)
    assert float((b[0] - want[0, 2]).abs()) < 1e-15 and float(b[1]) > float(a[1])   # flatter: more entropy
    f32 = R.token_confidence_f32(row, torch.tensor([2]), 4, 2.0)
    assert f32[0].dtype == torch.float32 and torch.equal(f32[3], b[3])


def test_weighted_sum_and_weights():
    maps = [torch.tensor([[0.5, 0.5], [1.0, 0.0], [0.25, 0.75]], dtype=torch.float64), torch.zeros(0, 3, dtype=torch.float64)]
    w = [torch.tensor([2.0, 0.0, 4.0], dtype=torch.float64), torch.zeros(0, dtype=torch.float64)]
    heat = R.weighted_sum(maps, w)
    assert heat[0].tolist() == [2.0, 4.0] and heat[1].tolist() == [0.0, 0.0, 0.0]
    lp, ent = torch.tensor([math.log(0.5), 0.0], dtype=torch.float64), torch.tensor([0.3, 0.0], dtype=torch.float64)
    assert R.weight_of("entropy", lp, ent) is ent
    assert float((R.weight_of("surprisal", lp, ent) - torch.tensor([math.log(2.0), 0.0], dtype=torch.float64)).abs().max()) < 1e-15
    assert float((R.weight_of("error", lp, ent) - torch.tensor([0.5, 0.0], dtype=torch.float64)).abs().max()) < 1e-15
    with pytest.raises(ValueError):
        R.weight_of("margin", lp, ent)


# ---- TokenConfidence -------------------------------------------------------------------------------------------------------------------
def test_token_confidence_properties():
    from acai_omr_amd.models.models import TokenConfidence
    nan = float("nan")
    lp = torch.tensor([[nan, -1.0, -3.0, nan], [nan, nan, nan, nan]])
    tlp = torch.tensor([[[nan, nan], [-0.5, -1.0], [-0.25, -3.0], [nan, nan]], [[nan, nan]] * 4])
    ids = torch.full((2, 4, 2), -1)
    c = TokenConfidence(lp, lp.clone(), torch.full((2, 4), -1), ids, tlp)
    assert c.uncertainty is None and c.alignment is None
    m = c.margin
    assert m[0, 1:3].tolist() == [0.5, 2.75] and bool(torch.isnan(m[0, [0, 3]]).all()) and bool(torch.isnan(m[1]).all())
    mean = c.mean_log_prob
    assert float(mean[0]) == -2.0 and math.isnan(float(mean[1]))
    one = TokenConfidence(lp, lp.clone(), torch.full((2, 4), -1), ids[..., :1], tlp[..., :1])
    assert one.margin.shape == (2, 4) and bool(torch.isnan(one.margin).all())
    assert "TokenConfidence" in repr(c)


# ---- argument errors come before any GPU work ------------------------------------------------------------------------------------------
@pytest.fixture()
def cpu_model(monkeypatch):
    """A small decoder on the CPU whose HIP library cannot be loaded: reaching it is an AssertionError, not the ValueError asked for."""
    from acai_omr_amd import _lib
    from acai_omr_amd.models.models import OMRDecoder, ViTOMR

    def no_library():
        raise AssertionError("the HIP library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    dec = OMRDecoder(16, VOCAB, num_layers=2, hidden_dim=16, num_heads=2, mlp_dim=32)
    return ViTOMR(None, None, dec.eval())


def _args():
    return torch.zeros(1, 5, 16), None, torch.zeros(1, 4, dtype=torch.long)


BAD_TOP_K = [0, -1, 9, 2.0, "3", None, True]
BAD_TEMPERATURE = [0, 0.0, -1.0, float("nan"), float("inf"), "hot", None]


@pytest.mark.parametrize("top_k", BAD_TOP_K, ids=repr)
def test_bad_top_k_raises_value_error(cpu_model, top_k):
    from acai_omr_amd.inference.vitomr_inference import confident_inference
    with pytest.raises(ValueError, match="top_k"):
        cpu_model.token_confidence(*_args(), top_k=top_k)
    with pytest.raises(ValueError, match="top_k"):
        cpu_model.uncertainty_maps(*_args(), grids=[(1, 5)], top_k=top_k)
    with pytest.raises(ValueError, match="top_k"):
        confident_inference(cpu_model, [torch.zeros(1, 8, 8)], "cpu", top_k=top_k)


@pytest.mark.parametrize("temperature", BAD_TEMPERATURE, ids=repr)
def test_bad_temperature_raises_value_error(cpu_model, temperature):
    from acai_omr_amd.inference.vitomr_inference import confident_inference
    with pytest.raises(ValueError, match="temperature"):
        cpu_model.token_confidence(*_args(), temperature=temperature)
    with pytest.raises(ValueError, match="temperature"):
        cpu_model.uncertainty_maps(*_args(), grids=[(1, 5)], temperature=temperature)
    with pytest.raises(ValueError, match="temperature"):
        confident_inference(cpu_model, [torch.zeros(1, 8, 8)], "cpu", temperature=temperature)


@pytest.mark.parametrize("weight", ["margin", "", None, 3, torch.zeros(1, 3), torch.zeros(4), torch.zeros(1, 4, dtype=torch.bool)],
                         ids=lambda w: repr(w)[:30])
def test_bad_weight_raises_value_error(cpu_model, weight):
    with pytest.raises(ValueError, match="weight"):
        cpu_model.uncertainty_maps(*_args(), grids=[(1, 5)], weight=weight)


def test_bad_uncertainty_name_raises_value_error(cpu_model):
    from acai_omr_amd.inference.vitomr_inference import confident_inference
    for bad in ("margin", 3, torch.zeros(1, 4)):
        with pytest.raises(ValueError):
            confident_inference(cpu_model, [torch.zeros(1, 8, 8)], "cpu", uncertainty=bad)
    with pytest.raises(ValueError):
        confident_inference(cpu_model, [torch.zeros(1, 8, 8)], "cpu", uncertainty="entropy", layers=[])
    with pytest.raises(ValueError):
        confident_inference(cpu_model, [torch.zeros(1, 8, 8)], "cpu", beam_width=2, speculative=2)
    with pytest.raises(TypeError, match="confident_inference"):
        confident_inference(cpu_model, [torch.zeros(1, 8, 8)], "cpu", return_maps=True)


@pytest.mark.parametrize("grids", [None, [], [(1, 5), (1, 5)], [(0, 5)], [(5, 0)], [(2, 2)], [(1, 4)], [5], "x"], ids=repr)
def test_bad_grids_raise_value_error(cpu_model, grids):
    with pytest.raises(ValueError):
        cpu_model.uncertainty_maps(*_args(), grids=grids)


def test_bad_sequences_and_selection_raise_value_error(cpu_model):
    mem, mask, seqs = _args()
    with pytest.raises(ValueError):
        cpu_model.token_confidence(mem, mask, seqs.float())
    with pytest.raises(ValueError):
        cpu_model.token_confidence(mem, mask, seqs, seq_mask=torch.ones(1, 3, dtype=torch.bool))
    with pytest.raises(ValueError):
        cpu_model.uncertainty_maps(mem, mask, seqs, grids=[(1, 5)], layers=[2])
    with pytest.raises(ValueError):
        cpu_model.uncertainty_maps(mem, mask, seqs, grids=[(1, 5)], head_weights=[-1.0, 2.0])
    with pytest.raises(ValueError, match="patch_size"):
        cpu_model.uncertainty_maps(mem, mask, seqs, grids=[(1, 5)], return_alignment=True)   # (this model has no encoder)


def test_ops_refuse_cpu_tensors_and_bad_arguments_before_the_library(cpu_model):
    from acai_omr_amd import ops
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.token_confidence(torch.zeros(2, 5), torch.zeros(2, dtype=torch.long))
    z = torch.zeros(4)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.attn_map_weighted_sum(z, torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), z, 1)

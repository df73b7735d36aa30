"""Token-to-image alignment without a GPU: the references of tests/alignment_reference.py are tied to the pinned oracle and to brute force,
and every argument error of the public layer is raised before the HIP library is touched."""
import pytest
import torch

import alignment_reference as R
from conftest import VOCAB, load_golden


def _f64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


@pytest.fixture(scope="module")
def golden():
    from oracle import vitomr_oracle as O
    fx = load_golden("vitomr_small")
    sd = _f64(fx["state_dict"])
    ref = fx["ref_fp32"]
    mem, lens_s = O.unpad(ref["memory"].double(), ref["latent_mask"])
    return fx["cfg"], sd, mem, lens_s, ref["seqs"]


def _oracle_step_logits(cfg, sd, mem, lens_s, seqs):
    """decode_step fed with the fixture's own tokens: logits [B, T' - 1, V], entry t - 1 chooses index t."""
    from oracle import vitomr_oracle as O
    state = O.DecodeState(mem, lens_s, sd, cfg["dec_heads"], "fp32")
    return torch.stack([O.decode_step(state, seqs[:, t - 1], t) for t in range(1, seqs.shape[1])], 1)


def test_reference_with_offset_1_is_the_oracles_decode_step_by_step(golden):
    """quirk Q1: the cached decode embeds the token at index t-1 at position t; the teacher-forced restatement with position_offset=1 then
    gives the decode's logits at every step, and with offset 0 it does not."""
    cfg, sd, mem, lens_s, seqs = golden
    B, T = seqs.shape
    step = _oracle_step_logits(cfg, sd, mem, lens_s, seqs)
    tokens, lens_t = seqs[:, :T - 1].reshape(-1), [T - 1] * B
    L, H = cfg["dec_layers"], cfg["dec_heads"]
    w = torch.full((L, H), 1.0 / (L * H), dtype=torch.float64)
    maps1, logits1 = R.decoder_maps(sd, tokens, mem, (lens_t, lens_s), H, list(range(L)), w, 1)
    d1 = float((logits1.view(B, T - 1, -1) - step).abs().max())
    print(f"\noffset 1: max |logits - decode_step| = {d1:.3e}")
    assert d1 < 1e-9
    maps0, logits0 = R.decoder_maps(sd, tokens, mem, (lens_t, lens_s), H, list(range(L)), w, 0)
    d0 = float((logits0.view(B, T - 1, -1) - step).abs().max())
    dm = max(float((a - b).abs().max()) for a, b in zip(maps0, maps1))
    print(f"offset 0: max |logits - decode_step| = {d0:.3e}, max |map(0) - map(1)| = {dm:.3e}")
    assert d0 > 1e-2 and dm > 1e-4
    for m, s in zip(maps1, lens_s):
        assert m.shape == (T - 1, s) and float((m.sum(-1) - 1).abs().max()) < 1e-12


def test_probs_mean_rows_sum_to_the_weights_sum():
    g = torch.Generator().manual_seed(3)
    H, dh, lens_q, lens_k = 3, 8, [4, 1, 7], [5, 9, 1]
    q = torch.randn(sum(lens_q), H * dh, generator=g, dtype=torch.float64)
    k = torch.randn(sum(lens_k), H * dh + 5, generator=g, dtype=torch.float64)   # (columns past H*dh are ignored)
    w = torch.tensor([0.5, 0.0, 1.25], dtype=torch.float64)
    maps = R.probs_mean(q, k, lens_q, lens_k, H, dh, w)
    for m, lq, lk in zip(maps, lens_q, lens_k):
        assert m.shape == (lq, lk) and bool((m >= 0).all())
        assert float((m.sum(-1) - 1.75).abs().max()) < 1e-12
    one = R.probs_mean(q, k, lens_q, lens_k, H, dh, [0.0, 1.0, 0.0])[0]
    s = (q[:4, 8:16] @ k[:5, 8:16].t()) / 8 ** 0.5
    assert float((one - torch.softmax(s, -1)).abs().max()) < 1e-14


@pytest.mark.parametrize("h,w", [(1, 1), (5, 1), (1, 7), (4, 7), (3, 64)])
def test_locate_equals_a_brute_force_loop(h, w):
    g = torch.Generator().manual_seed(h * 100 + w)
    m = torch.rand(6, h * w, generator=g, dtype=torch.float64) ** 4
    m[1] = 0.0                                  # a dead row
    m[2, :] = 0.25                              # every patch ties: index 0 wins
    if h * w > 2:
        m[3, [h * w - 1, 1]] = 2.0              # an exact tie between two patches: the lower one wins
    patch, loc = R.locate(m, w)
    bp, bl = R.locate_loop(m, w)
    assert torch.equal(patch, bp)
    assert float((loc - bl).abs().max()) < 1e-12
    assert int(patch[1]) == 0 and float(loc[1].abs().max()) == 0.0
    assert int(patch[2]) == 0 and (h * w <= 2 or int(patch[3]) == 1)


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


BAD_LAYERS = [[], [2], [-3], [0, 0], [1, -1], 3, ["a"]]
BAD_WEIGHTS = [[1.0], [[1.0, 1.0]] * 3, [-1.0, 2.0], [float("nan"), 1.0], [float("inf"), 1.0], [0.0, 0.0], [[0.0, 0.0], [0.0, 0.0]], "ab",
               torch.ones(2, 2, 2)]


@pytest.mark.parametrize("layers", BAD_LAYERS, ids=repr)
def test_bad_layers_raise_value_error(cpu_model, layers):
    dec = cpu_model.decoder
    tokens, mem = torch.zeros(3, dtype=torch.long), torch.zeros(5, 16)
    with pytest.raises(ValueError):
        dec.cross_attention_maps_packed(tokens, [3], mem, None, [5], layers=layers)
    with pytest.raises(ValueError):
        cpu_model.cross_attention_maps(mem[None], None, torch.zeros(1, 4, dtype=torch.long), layers=layers)
    with pytest.raises(ValueError):
        cpu_model.locate_tokens(mem[None], None, torch.zeros(1, 4, dtype=torch.long), layers=layers, grids=[(1, 5)], patch_size=4)


@pytest.mark.parametrize("weights", BAD_WEIGHTS, ids=lambda w: repr(w)[:40])
def test_bad_head_weights_raise_value_error(cpu_model, weights):
    dec = cpu_model.decoder
    tokens, mem = torch.zeros(3, dtype=torch.long), torch.zeros(5, 16)
    with pytest.raises(ValueError):
        dec.cross_attention_maps_packed(tokens, [3], mem, None, [5], head_weights=weights)
    with pytest.raises(ValueError):
        cpu_model.cross_attention_maps(mem[None], None, torch.zeros(1, 4, dtype=torch.long), head_weights=weights)
    from acai_omr_amd.inference.vitomr_inference import aligned_inference
    with pytest.raises(ValueError):
        aligned_inference(cpu_model, [torch.zeros(1, 8, 8)], "cpu", head_weights=weights)


def test_selection_is_normalised_and_ordered(cpu_model):
    dec = cpu_model.decoder
    sel, w = dec._alignment_selection(None, None)
    assert sel == [0, 1] and torch.equal(w, torch.full((2, 2), 0.25, dtype=torch.float64))
    sel, w = dec._alignment_selection([-1, 0], [[1.0, 3.0], [4.0, 0.0]])      # rows follow `layers`: layer 1 first
    assert sel == [0, 1] and torch.allclose(w, torch.tensor([[0.5, 0.0], [0.125, 0.375]], dtype=torch.float64))
    sel, w = dec._alignment_selection((1,), torch.tensor([2.0, 6.0]))
    assert sel == [1] and torch.allclose(w, torch.tensor([[0.25, 0.75]], dtype=torch.float64))


@pytest.mark.parametrize("grids", [None, [], [(1, 5), (1, 5)], [(0, 5)], [(5, 0)], [(-1, -5)], [(2, 2)], [(1, 4)], [5], "x"], ids=repr)
def test_bad_grids_raise_value_error(cpu_model, grids):
    mem = torch.zeros(1, 5, 16)
    with pytest.raises(ValueError):
        cpu_model.locate_tokens(mem, None, torch.zeros(1, 4, dtype=torch.long), grids=grids, patch_size=4)


def test_grid_must_divide_the_masked_length(cpu_model):
    mem = torch.zeros(2, 6, 16)
    mask = torch.tensor([[False] * 6, [False] * 4 + [True] * 2])
    with pytest.raises(ValueError, match="does not cover"):
        cpu_model.locate_tokens(mem, mask, torch.zeros(2, 4, dtype=torch.long), grids=[(2, 3), (2, 3)], patch_size=4)
    with pytest.raises(ValueError, match="patch_size"):
        cpu_model.locate_tokens(mem, mask, torch.zeros(2, 4, dtype=torch.long), grids=[(2, 3), (2, 2)])


def test_alignment_lengths(cpu_model):
    dec = cpu_model.decoder
    e, p = dec.eos_idx, dec.pad_idx
    seqs = torch.tensor([[0, 5, 6, e, p], [0, 5, 6, 7, 8], [0, e, p, p, p], [0, 5, 6, 7, e]])
    assert cpu_model._alignment_lengths(seqs, None) == [4, 5, 2, 5]
    mask = torch.tensor([[1, 1, 1, 1, 0], [1, 1, 1, 0, 1], [1, 1, 0, 0, 0], [1, 1, 1, 1, 1]], dtype=torch.bool)
    assert cpu_model._alignment_lengths(seqs, mask) == [4, 3, 2, 5]
    with pytest.raises(ValueError):
        cpu_model._alignment_lengths(seqs.float(), None)

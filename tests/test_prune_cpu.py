"""Blank-patch pruning without a GPU: properties of the numpy restatement (tests/prune_reference.py), PruneConfig's validation, the host side
of the pruned `PackedPatches`, and the INPUT CONDITIONS the GPU tests (tests/test_gpu_prune.py) rest on."""
import numpy as np
import pytest
import torch

import prune_reference as R
from conftest import load_golden


def test_ink_counts_are_strict_and_float32():
    rows = np.array([[0.5, 0.49999997, 0.0, 1.0], [np.nan, -1.0, 0.5, 0.5]], dtype=np.float32)
    assert R.ink_counts(rows, 0.5).tolist() == [2, 1]          # 0.5 itself is not ink, a NaN is not ink
    assert R.ink_counts(rows, float("inf")).tolist() == [4, 3]   # everything finite is below +inf
    assert R.ink_counts(rows, float("-inf")).tolist() == [0, 0]


@pytest.mark.parametrize("halo", [0, 1, 2, 3])
def test_keep_rule_is_a_chebyshev_dilation(halo):
    g = np.random.default_rng(halo)
    h, w = 7, 11
    ink = (g.random(h * w) < 0.06).astype(np.int32) * 5
    keep = R.keep_mask(ink, h, w, 0, halo)
    inked = ink.reshape(h, w) > 0
    rr, cc = np.nonzero(inked)
    for r in range(h):
        for c in range(w):
            near = bool(len(rr)) and bool((np.maximum(np.abs(rr - r), np.abs(cc - c)) <= halo).any())
            assert keep[r, c] == near
    assert (keep >= inked).all()
    if halo:
        assert (keep >= R.keep_mask(ink, h, w, 0, halo - 1)).all()   # monotone in the halo
    assert R.keep_mask(ink, h, w, 5, halo).all()                     # max_ink = 5: nothing is inked -> the all-blank fallback keeps all


def test_kept_indices_do_not_leak_across_images():
    dims = [(2, 3), (1, 4), (3, 2)]
    ink = np.zeros(6 + 4 + 6, dtype=np.int32)
    ink[5] = 9        # the last patch of image 0: image 1's first patch is its neighbour in the stream, not in the grid
    ink[10] = 9       # the first patch of image 2
    kept = R.kept_indices(ink, dims, 0, 1)
    assert kept[0].tolist() == [1, 2, 4, 5]
    assert kept[1].tolist() == [0, 1, 2, 3]      # blank: keeps everything
    assert kept[2].tolist() == [0, 1, 2, 3]
    rows = np.arange(16 * 2).reshape(16, 2)
    out, packed, sel = R.compact(rows, kept, dims)
    assert packed.tolist() == [1, 2, 4, 5, 0, 1, 2, 3, 0, 1, 2, 3] and sel.tolist() == [1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13]
    assert (out == rows[sel]).all()


def test_pe_rows_inside_and_beyond_the_table():
    dims = [(2, 3), (3, 5), (1, 2), (5, 2)]
    kept = [np.array([0, 4], np.int32), np.array([0, 7, 14], np.int32), np.array([1], np.int32), np.array([3, 9], np.int32)]
    pe = R.pe_rows(kept, dims, (2, 4))    # images 1 and 3 exceed the 2 x 4 table: their grids are appended at rows 8 and 8 + 15
    assert [p.tolist() for p in pe] == [[0, 5], [8, 15, 22], [1], [8 + 15 + 3, 8 + 15 + 9]]


def test_expand_map_is_a_scatter_with_zeros():
    m = np.arange(1, 7, dtype=np.float32).reshape(2, 3)
    out = R.expand_map(m, np.array([1, 4, 5]), 7)
    assert out.shape == (2, 7) and (out[:, [1, 4, 5]] == m).all() and out[:, [0, 2, 3, 6]].sum() == 0


@pytest.mark.parametrize("kw", [dict(ink_level=float("nan")), dict(ink_level="0.5"), dict(ink_level=True), dict(max_ink=-1), dict(max_ink=1.5),
                                dict(max_ink=True), dict(halo=-1), dict(halo=4), dict(halo=1.0), dict(halo=False)])
def test_prune_config_refuses(kw):
    from acai_omr_amd.prune import PruneConfig
    with pytest.raises(ValueError):
        PruneConfig(**kw)


def test_prune_config_defaults_and_argument_forms():
    from acai_omr_amd.page import DetectConfig
    from acai_omr_amd.prune import PruneConfig, as_config
    cfg = PruneConfig()
    assert (cfg.ink_level, cfg.max_ink, cfg.halo) == (0.5, 0, 1) and cfg.ink_level == DetectConfig().ink_threshold
    assert as_config(None) is None and as_config(False) is None and as_config(True) == cfg and as_config(cfg) is cfg
    assert PruneConfig(ink_level=float("inf"), halo=3, max_ink=7).halo == 3
    with pytest.raises(TypeError):
        as_config(1)


def test_pruned_packed_patches_slice_on_the_host():
    """slice() of a pruned stream: kept rows, kept indices and positional rows of the chosen images, with the appended grids of the images in
    front of the slice taken off the positional rows that point behind the table."""
    from acai_omr_amd.utils import PackedPatches
    dims = [(2, 3), (3, 5), (1, 2), (5, 2)]
    kept = [np.array([0, 4], np.int32), np.array([0, 7, 14], np.int32), np.array([1], np.int32), np.array([3, 9], np.int32)]
    pe = R.pe_rows(kept, dims, (2, 4))
    n = sum(len(k) for k in kept)
    pk = PackedPatches(torch.arange(n * 4).view(n, 4), dims, 2, torch.from_numpy(np.concatenate(kept)), [len(k) for k in kept],
                       torch.from_numpy(np.concatenate(pe)), (2, 4))
    assert pk.pruned and pk.lens == [2, 3, 1, 2] and len(pk) == 4
    s = pk.slice(2, 4)
    assert s.pruned and s.dims == dims[2:] and s.kept_lens == [1, 2] and s.kept.tolist() == [1, 3, 9]
    assert torch.equal(s.patches, pk.patches[5:8])
    assert s.pe_index.tolist() == np.concatenate(R.pe_rows(kept[2:], dims[2:], (2, 4))).tolist()
    assert pk.slice(0, 2).pe_index.tolist() == np.concatenate(pe[:2]).tolist()
    plain = PackedPatches(torch.zeros(8, 4), [(2, 2), (2, 2)], 2)
    assert not plain.pruned and plain.lens == [4, 4] and plain.kept is None
    with pytest.raises(ValueError):
        PackedPatches(torch.zeros(2, 4), [(2, 2)], 2, kept=torch.zeros(2, dtype=torch.int32))


# ---- input conditions of the GPU tests ------------------------------------------------------------------------------------------------------
def _all_test_images():
    fx = load_golden(R.PARITY_FIXTURE)
    imgs = [t for seed in R.PARITY_SEEDS for t in R.parity_images(seed, fx["cfg"]["P"])]
    return imgs + R.model_images()


def test_synthetic_images_stay_clear_of_the_ink_level():
    """Paper in [0.8, 1), ink in [0, 0.35): nothing in [0.4, 0.6], so neither bf16 rounding (relative 2^-8) nor a resize's fp32 rounding can
    carry a pixel across the level 0.5."""
    for t in _all_test_images():
        a = t.numpy()
        assert a.dtype == np.float32 and a.min() >= 0.0 and a.max() < 1.0
        assert not ((a >= 0.4) & (a <= 0.6)).any()
        assert ((a < R.INK_HI) | (a >= R.PAPER_LO)).all() and (a < R.INK_HI).any()
        b = t.to(torch.bfloat16).float().numpy()
        assert ((a < 0.5) == (b < 0.5)).all()


def test_synthetic_images_kept_share():
    """25 % .. 75 % of the patches are kept at halo = 1, strictly fewer at halo = 0 - per set of images a GPU test encodes together."""
    fx = load_golden(R.PARITY_FIXTURE)
    sets = [(R.parity_images(seed, fx["cfg"]["P"]), fx["cfg"]["P"]) for seed in R.PARITY_SEEDS]
    sets.append((R.model_images(), 16))
    for imgs, P in sets:
        k1, total = R.kept_share(imgs, P, halo=1)
        k0, _ = R.kept_share(imgs, P, halo=0)
        print(f"kept {k0} (halo 0) / {k1} (halo 1) of {total}")
        assert 0.25 * total <= k1 <= 0.75 * total
        assert 0 < k0 < k1


@pytest.mark.parametrize("seed", R.PARITY_SEEDS)
def test_oracle_parity_seeds_have_a_top2_margin(seed):
    """The oracle's smallest top-2 logit margin over all decode steps on the pruned stream is at least 1e-2: ten times the 1e-3 step-logit
    bar of test_fp32_encoder_head_greedy_vs_reference_golden, so the token comparison of the GPU parity test is not decided by rounding."""
    fx = load_golden(R.PARITY_FIXTURE)
    res = R.oracle_pruned(fx, R.parity_images(seed, fx["cfg"]["P"]), return_logits=True)
    top = res["logits"].topk(2, dim=-1).values
    margin = float((top[..., 0] - top[..., 1]).min())
    print(f"seed {seed}: smallest top-2 margin {margin:.4f} over {res['logits'].shape[1]} steps, kept {res['lens']}")
    assert margin >= 1e-2
    dims = [(H // fx["cfg"]["P"], W // fx["cfg"]["P"]) for H, W in R.PARITY_SIZES]
    assert any(h > fx["cfg"]["pe_h"] or w > fx["cfg"]["pe_w"] for h, w in dims)      # one grid exceeds the positional table
    assert all(0 < k <= h * w for k, (h, w) in zip(res["lens"], dims)) and sum(res["lens"]) < sum(h * w for h, w in dims)

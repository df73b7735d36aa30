"""Blank-patch pruning on the GPU (acai_omr_amd/prune.py, csrc/prune.hip): the four kernels against the numpy restatement
(tests/prune_reference.py) with torch.equal at every launch edge, and the pruned stream through the encoder, every decode mode, the
alignment and confidence passes and page_inference.  The conditions on the inputs (ink well away from the level, the kept share, the
oracle's top-2 margins) are checked without a GPU in tests/test_prune_cpu.py."""
import numpy as np
import pytest
import torch
from torch.amp import autocast

import page_reference as PR
import prune_reference as R
from conftest import load_golden
from decode_support import _same, build_vitomr, dev  # noqa: F401

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
LEVEL = 0.5


def md(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- 1. patch_ink ----------------------------------------------------------------------------------------------------------------------------
def _ink_rows(M, L, dtype, seed):
    """Rows of values around the level, a sixth of them exactly the level (which is not ink), in `dtype`."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(M, L, generator=g)
    x[torch.rand(M, L, generator=g) < 1 / 6] = LEVEL
    if M:
        x[0, 0] = LEVEL
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("L", [16, 64, 256, 18])
def test_patch_ink(dev, dtype, L):
    """Every M of {1, 63, 64, 65, 1000}: contiguous rows (16-byte loads) and a view that starts one element into its buffer with an odd
    pitch (element by element), both equal to the restatement."""
    from acai_omr_amd import ops
    for M in (1, 63, 64, 65, 1000):
        x = _ink_rows(M, L, dtype, 17 * M + L)
        want = torch.from_numpy(R.ink_counts(x.float().numpy(), LEVEL))
        assert int((x.float() == LEVEL).sum()) > 0
        got = ops.patch_ink(x.to(dev), LEVEL)
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), (M, L)
        buf = torch.zeros(M * (L + 3) + 1, dtype=dtype, device=dev)
        view = buf[1:].view(M, L + 3)[:, :L]
        view.copy_(x)
        assert view.data_ptr() % 16 != 0
        assert torch.equal(ops.patch_ink(view, LEVEL).cpu(), want), (M, L, "view")
        if M == 65:     # a slice of a contiguous stream, as PackedPatches.slice hands out
            assert torch.equal(ops.patch_ink(x.to(dev)[3:], LEVEL).cpu(), want[3:])
    everything = ops.patch_ink(_ink_rows(5, L, dtype, 1).to(dev), float("inf"))
    assert everything.tolist() == [L] * 5


# ---- 2. patch_keep ----------------------------------------------------------------------------------------------------------------------------
KEEP_DIMS = [(1, 1), (1, 37), (41, 1), (3, 67), (1, 63), (1, 64), (5, 13), (15, 17), (16, 16), (1, 257), (33, 31), (32, 32), (25, 41), (17, 241),
             (6, 7), (4, 9), (2, 2)]
BLANK, FULL = 14, 15       # image (6, 7) holds no ink at all, image (4, 9) ink everywhere


def _keep_ink():
    """Sparse ink counts in 0 .. 6 over KEEP_DIMS; the last patch of every image and the first of the next are inked (a leak across images
    would keep patches the grid does not make neighbours)."""
    assert sorted(h * w for h, w in KEEP_DIMS[4:14]) == [63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
    g = np.random.default_rng(7)
    parts = []
    for i, (h, w) in enumerate(KEEP_DIMS):
        n = h * w
        a = np.where(g.random(n) < 0.04, g.integers(1, 7, n), 0).astype(np.int32)
        a[-1] = a[0] = 5
        if i == BLANK:
            a[:] = 0
        if i == FULL:
            a[:] = 4
        parts.append(a)
    return np.concatenate(parts)


@pytest.mark.parametrize("max_ink", [0, 3])
@pytest.mark.parametrize("halo", [0, 1, 2, 3])
def test_patch_keep(dev, halo, max_ink):
    from acai_omr_amd import ops
    ink = _keep_ink()
    table, rows, max_grid = ops.prune_table(KEEP_DIMS, (4, 8), dev)
    assert rows == ink.size and max_grid == 4097
    kept_local, count = ops.patch_keep(_t(ink, dev), table, max_grid, max_ink, halo)
    want = R.kept_indices(ink, KEEP_DIMS, max_ink, halo)
    assert count.dtype == torch.int32 and count.tolist() == [len(k) for k in want]
    got, o = kept_local.cpu(), 0
    for k, (h, w) in zip(want, KEEP_DIMS):
        assert torch.equal(got[o:o + len(k)], torch.from_numpy(k)), (h, w)
        o += h * w
    assert len(want[BLANK]) == 42 and len(want[FULL]) == 36
    if halo == 0 and max_ink == 0:
        assert sum(len(k) for k in want) < ink.size // 4      # the case really drops patches


# ---- 3. patch_compact (through prune_patches) and attn_map_expand -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("layout", ["contiguous", "view"])
def test_prune_patches_compacts_bitwise(dev, dtype, layout):
    from acai_omr_amd.prune import PruneConfig, prune_patches
    from acai_omr_amd.utils import PackedPatches
    P, pe_grid = 4, (6, 10)
    dims = [(6, 10), (7, 11), (1, 1), (3, 5), (12, 3), (2, 4)]       # (7, 11) and (12, 3) exceed the table: the interpolated branch
    M, L = sum(h * w for h, w in dims), P * P
    g = torch.Generator().manual_seed(3)
    x = (0.8 + 0.2 * torch.rand(M, L, generator=g)).clamp(max=0.99)
    x[torch.rand(M, L, generator=g) < 0.01] = 0.1
    x[60:60 + 77][5] = 0.2
    x = x.to(dtype)
    if layout == "view":
        buf = torch.zeros(M * (L + 1) + 1, dtype=dtype, device=dev)
        xd = buf[1:].view(M, L + 1)[:, :L]
        xd.copy_(x)
    else:
        xd = x.to(dev)
    for cfg in (PruneConfig(), PruneConfig(halo=0), PruneConfig(max_ink=1, halo=2)):
        out = prune_patches(PackedPatches(xd, dims, P), cfg, pe_grid)
        kept = R.kept_indices(R.ink_counts(x.float().numpy(), cfg.ink_level), dims, cfg.max_ink, cfg.halo)
        _, packed, sel = R.compact(x.float().numpy(), kept, dims)
        assert out.pruned and out.dims == dims and out.kept_lens == [len(k) for k in kept] and out.pe_grid == pe_grid
        assert out.patches.dtype == dtype and out.patches.is_contiguous()
        as_int = torch.int32 if dtype == F32 else torch.int16
        assert torch.equal(out.patches.cpu().view(as_int), x[torch.from_numpy(sel).long()].contiguous().view(as_int))
        assert out.kept.dtype == torch.int32 and torch.equal(out.kept.cpu(), torch.from_numpy(packed))
        o = 0
        for k in kept:
            assert bool((np.diff(out.kept.cpu().numpy()[o:o + len(k)]) > 0).all())
            o += len(k)
        assert torch.equal(out.pe_index.cpu(), torch.from_numpy(np.concatenate(R.pe_rows(kept, dims, pe_grid))))
        assert 0 < sum(out.kept_lens) < M
        # slices of the pruned stream are pruned streams of the slices
        for i0, i1 in ((0, 2), (2, 6), (1, 5)):
            s = out.slice(i0, i1)
            assert torch.equal(s.pe_index.cpu(), torch.from_numpy(np.concatenate(R.pe_rows(kept[i0:i1], dims[i0:i1], pe_grid))))
            assert torch.equal(s.kept.cpu(), torch.from_numpy(np.concatenate(kept[i0:i1]))) and s.patches.shape[0] == sum(s.kept_lens)


def test_attn_map_expand(dev):
    from acai_omr_amd import ops
    g = np.random.default_rng(5)
    lens_q, kept_lens, full = [1, 70, 3, 2], [5, 300, 1, 4], [9, 700, 1, 4]
    kept = [np.sort(g.choice(s, k, replace=False)).astype(np.int32) for k, s in zip(kept_lens, full)]
    maps = [g.random((t, k), dtype=np.float32) + 0.5 for t, k in zip(lens_q, kept_lens)]
    flat = _t(np.concatenate([m.reshape(-1) for m in maps]), dev)
    out, offs, off_dev = ops.attn_map_expand(flat, lens_q, kept_lens, full, _t(np.concatenate(kept), dev))
    assert offs == ops.attn_map_layout(lens_q, full)[0] and off_dev.tolist() == offs and out.numel() == sum(t * s for t, s in zip(lens_q, full))
    for o, t, s, m, k in zip(offs, lens_q, full, maps, kept):
        assert torch.equal(out[o:o + t * s].view(t, s).cpu(), torch.from_numpy(R.expand_map(m, k, s)))
    with pytest.raises(ValueError):
        ops.attn_map_expand(flat, lens_q, kept_lens, [9, 200, 1, 4], _t(np.concatenate(kept), dev))     # more kept than the grid holds


# ---- models -----------------------------------------------------------------------------------------------------------------------------------
def _packed(m, imgs, dev):
    """The fp32 patch stream inference() forms for images (the encoder runs outside autocast)."""
    from acai_omr_amd import ops
    from acai_omr_amd.utils import PackedPatches
    P = m.encoder.patch_size
    dims = [(t.shape[-2] // P, t.shape[-1] // P) for t in imgs]
    patches = torch.empty(sum(h * w for h, w in dims), P * P, dtype=F32, device=dev)
    r0 = 0
    for t in imgs:
        r0 += ops.patchify(t.to(dev).float().contiguous(), P, patches, r0)
    return PackedPatches(patches, dims, P)


def _restated_kept(imgs, P, halo=1, max_ink=0):
    rows = np.concatenate([R.patch_rows(t[0].numpy(), P) for t in imgs])
    dims = [(t.shape[-2] // P, t.shape[-1] // P) for t in imgs]
    return R.kept_indices(R.ink_counts(rows, LEVEL), dims, max_ink, halo), dims


@pytest.fixture(scope="module")
def model(dev):
    fx = load_golden(R.MODEL_FIXTURE)
    m = build_vitomr(fx["cfg"], fx["state_dict"], dev, BF, 9)       # 3 images x (2 drafts + 1) rows for speculative decoding
    imgs = R.model_images()
    pruned = m.encoder.prune_packed(_packed(m, imgs, dev))
    kept, dims = _restated_kept(imgs, 16)
    assert pruned.kept_lens == [len(k) for k in kept] and torch.equal(pruned.kept.cpu(), torch.from_numpy(np.concatenate(kept)))
    assert sum(pruned.kept_lens) < sum(h * w for h, w in dims)
    return fx, m, imgs, pruned, kept, dims


# ---- 4. identity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", [torch.float, BF], ids=["fp32", "bf16"])
def test_everything_inked_is_the_unpruned_call_bit_for_bit(dev, cache, monkeypatch):
    from acai_omr_amd import ops
    from acai_omr_amd.inference.vitomr_inference import inference
    from acai_omr_amd.prune import PruneConfig
    fx = load_golden(R.MODEL_FIXTURE)
    m = build_vitomr(fx["cfg"], fx["state_dict"], dev, cache, len(fx["imgs"]))
    calls = {n: 0 for n in ("patch_ink", "patch_keep", "patch_compact", "attn_map_expand")}
    for n in calls:
        def counted(*a, _n=n, _f=getattr(ops, n), **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, n, counted)
    T = fx["cfg"]["gen_len"]
    if cache == BF:
        run = lambda **kw: inference(m, fx["imgs"], "cuda", max_inference_len=T, **kw)   # noqa: E731
    else:
        # inference() decodes under autocast(bf16) whatever the cache; the fp32 path is the one test_fp32_encoder_head_greedy_vs_reference_golden
        # runs: encoder, head and greedy decode without autocast
        def run(**kw):
            with torch.no_grad():
                lat, _, lens = m.encoder.forward_packed(fx["imgs"], **kw)
                return m._greedy_packed(m.transition_head.forward_packed(lat), None, lens, T)
    want = run()
    assert not any(calls.values()), calls                         # prune=None issues none of the new launches
    got = run(prune=PruneConfig(ink_level=float("inf")))
    assert calls == {"patch_ink": 1, "patch_keep": 1, "patch_compact": 1, "attn_map_expand": 0}
    _same(got, want)
    _same(run(prune=False), want)


# ---- 5. oracle parity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.PARITY_SEEDS)
def test_fp32_pruned_stream_vs_oracle(dev, seed):
    """The oracle's fp32 pipeline run on the kept rows of its own embedding (prune_reference.oracle_pruned) against the HIP path: latent and
    memory within the 1e-4 bars of test_fp32_encoder_head_greedy_vs_reference_golden, tokens and mask equal, log-probs within 1e-3.  The
    third image's 7 x 11 grid exceeds the 6 x 10 positional table."""
    fx = load_golden(R.PARITY_FIXTURE)
    cfg = fx["cfg"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.float, 3)
    imgs = R.parity_images(seed, cfg["P"])
    ref = R.oracle_pruned(fx, imgs)
    with torch.no_grad():
        lat, _, lens, pruned = m.encoder.forward_packed(imgs, prune=True, return_pruned=True)
        assert lens == ref["lens"] and torch.equal(pruned.kept.cpu(), torch.from_numpy(np.concatenate(ref["kept"])))
        # the positional rows through the device index are the rows of the full gather
        sel = torch.from_numpy(R.compact(np.zeros((sum(h * w for h, w in pruned.dims), 1)), ref["kept"], pruned.dims)[2]).long().to(dev)
        assert torch.equal(m.encoder._pe_packed(pruned.dims, index=pruned.pe_index), m.encoder._pe_packed(pruned.dims)[sel])
        mem = m.transition_head.forward_packed(lat)
        seqs, lps, mask = m._greedy_packed(mem, None, lens, cfg["gen_len"])
    print(f"\nseed {seed}: latent {md(lat, ref['latent']):.2e} memory {md(mem, ref['memory']):.2e} log-probs {md(lps, ref['log_probs']):.2e}")
    assert md(lat, ref["latent"]) < 1e-4 and md(mem, ref["memory"]) < 1e-4
    assert torch.equal(seqs.cpu(), ref["seqs"]) and torch.equal(mask.cpu(), ref["seq_mask"])
    assert md(lps, ref["log_probs"]) < 1e-3


# ---- 6. decode modes on a pruned memory -----------------------------------------------------------------------------------------------------
def test_greedy_on_a_pruned_memory(dev, model):
    from acai_omr_amd.inference.vitomr_inference import inference
    fx, m, imgs, pruned, kept, dims = model
    T = fx["cfg"]["gen_len"]
    got = inference(m, imgs, "cuda", max_inference_len=T, prune=True)
    with torch.no_grad():
        lat, _, lens = m.encoder.forward_packed(pruned)
        assert lens == pruned.kept_lens and lat.shape[0] == sum(lens)
        with autocast(device_type="cuda", dtype=BF):
            mem = m.transition_head.forward_packed(lat)
            want = m._greedy_packed(None, mem, lens, T)
    _same(got, want)
    _same(inference(m, pruned, "cuda", max_inference_len=T), want)
    _same(inference(m, _packed(m, imgs, dev), "cuda", max_inference_len=T, prune=True), want)


@pytest.mark.parametrize("mode", ["beam", "speculative", "fp8", "continuous"])
def test_decode_modes_on_a_pruned_memory(dev, model, mode):
    """inference(prune=) in every decode mode against its own unpruned-API call on the explicitly pruned PackedPatches."""
    from acai_omr_amd.inference.vitomr_inference import continuous_inference, inference
    fx, m, imgs, pruned, kept, dims = model
    T = fx["cfg"]["gen_len"]
    if mode == "fp8":
        m = build_vitomr(fx["cfg"], fx["state_dict"], dev, BF, 3, memory_cache_dtype=torch.float8_e4m3fn)
    if mode == "continuous":
        _same(continuous_inference(m, imgs, "cuda", max_inference_len=T, slots=2, prune=True),
              continuous_inference(m, pruned, "cuda", max_inference_len=T, slots=2))
        _same(continuous_inference(m, _packed(m, imgs, dev), "cuda", max_inference_len=T, slots=2, prune=True),
              continuous_inference(m, pruned, "cuda", max_inference_len=T, slots=2))
        return
    kw = {"beam": dict(beam_width=2), "speculative": dict(speculative=2), "fp8": {}}[mode]
    _same(inference(m, imgs, "cuda", max_inference_len=T, prune=True, **kw), inference(m, pruned, "cuda", max_inference_len=T, **kw))


# ---- 7. alignment and heat maps ----------------------------------------------------------------------------------------------------------------
def test_alignment_speaks_of_the_full_grid(dev, model):
    from acai_omr_amd.inference.vitomr_inference import aligned_inference, confident_inference, diagnosed_inference
    fx, m, imgs, pruned, kept, dims = model
    T = fx["cfg"]["gen_len"]
    seqs, lps, mask, al = aligned_inference(m, imgs, "cuda", max_inference_len=T, return_maps=True, prune=True)
    with torch.no_grad():
        lat, _, lens = m.encoder.forward_packed(pruned)
        with autocast(device_type="cuda", dtype=BF):
            mem = m.transition_head.forward_packed(lat)
            plain = m._align_packed(None, mem, lens, seqs, mask, None, None, True)      # the maps over the kept patches
    assert al.grids == dims
    Ls = m._alignment_lengths(seqs, mask)
    for i, ((h, w), k) in enumerate(zip(dims, kept)):
        full = al.maps[i].cpu()
        assert full.shape == (Ls[i] - 1, h * w) and plain[i].shape == (Ls[i] - 1, len(k))
        assert torch.equal(full[:, torch.from_numpy(k).long()], plain[i].cpu())          # kept columns: bitwise
        dropped = np.setdiff1d(np.arange(h * w), k)
        assert len(dropped) and bool((full[:, torch.from_numpy(dropped).long()] == 0).all())
        p = al.patch[i, 1:Ls[i]].cpu().numpy()
        assert np.isin(p, k).all()                                                      # an index into the FULL grid, at a kept patch
        c = al.center_px[i, 1:Ls[i]].cpu()
        assert bool((c[:, 0] >= 0).all()) and bool((c[:, 0] <= 16 * w).all()) and bool((c[:, 1] <= 16 * h).all())
    _same(aligned_inference(m, pruned, "cuda", max_inference_len=T)[:3], (seqs, lps, mask))
    *_, conf = confident_inference(m, imgs, "cuda", max_inference_len=T, uncertainty="entropy", prune=True)
    for (h, w), k, heat in zip(dims, kept, conf.uncertainty):
        assert heat.shape == (h, w)
        flat = heat.reshape(-1).cpu()
        assert bool((flat[torch.from_numpy(np.setdiff1d(np.arange(h * w), k)).long()] == 0).all()) and float(flat.sum()) > 0
    assert conf.alignment.grids == dims
    targets = [seqs[i][mask[i]].cpu() for i in range(len(imgs))]
    *_, dconf, ea = diagnosed_inference(m, imgs, targets, "cuda", max_inference_len=T, prune=True)
    assert [tuple(u.shape) for u in dconf.uncertainty] == dims and all(float(u.abs().sum()) == 0 for u in dconf.uncertainty)   # no errors: all zero
    with pytest.raises(ValueError):
        m._check_grids(dims, pruned.kept_lens)        # the kept counts are not what the grids cover


# ---- 8. page_inference ------------------------------------------------------------------------------------------------------------------------
TRUTH = [(14, 37, 191, 74), (14, 107, 191, 123), (14, 167, 191, 204)]


@pytest.mark.parametrize("cfg", [True, "halo0"])
def test_page_inference_pruned(dev, cfg):
    from acai_omr_amd import page as pg
    from acai_omr_amd.inference.vitomr_inference import continuous_inference, page_inference
    from acai_omr_amd.prune import PruneConfig
    from acai_omr_amd.utils import DynamicResize
    fx = load_golden(R.MODEL_FIXTURE)
    m = build_vitomr(fx["cfg"], fx["state_dict"], dev, BF, 2)      # a cache of 2 rows: 3 systems = two encode chunks of the pruned stream
    tr = DynamicResize(16, 32, 4, 8, True)
    page = torch.from_numpy(PR.synthetic_page()[0]).float() / 255.0
    prune = True if cfg is True else PruneConfig(halo=0)
    pc = PruneConfig() if cfg is True else prune
    res = page_inference(m, page, "cuda", tr, boxes=TRUTH, max_inference_len=12, prune=prune)
    packed = pg.split_pages(pg.ingest_pages([page], None, device=tr.device), [TRUTH], tr)
    pruned = m.encoder.prune_packed(packed, pc)
    want = continuous_inference(m, pruned, "cuda", max_inference_len=12)
    assert torch.equal(res.seqs, want[0]) and torch.equal(res.log_probs, want[1]) and torch.equal(res.seq_mask, want[2])
    assert res.patches_total == [h * w for h, w in packed.dims] and res.patches_kept == pruned.kept_lens
    assert all(k <= t for k, t in zip(res.patches_kept, res.patches_total))
    kept = R.kept_indices(R.ink_counts(packed.patches.float().cpu().numpy(), pc.ink_level), packed.dims, pc.max_ink, pc.halo)
    assert torch.equal(pruned.kept.cpu(), torch.from_numpy(np.concatenate(kept)))
    print(f"\npage: kept {res.patches_kept} of {res.patches_total}")
    plain = page_inference(m, page, "cuda", tr, boxes=TRUTH, max_inference_len=12)
    assert plain.patches_kept == plain.patches_total == res.patches_total


# ---- 9. errors -----------------------------------------------------------------------------------------------------------------------------
def test_prune_refusals(dev, model):
    from acai_omr_amd import ops
    from acai_omr_amd.inference.vitomr_inference import inference
    from acai_omr_amd.models.models import MAE
    from acai_omr_amd.prune import PruneConfig, prune_patches
    fx, m, imgs, pruned, kept, dims = model
    with pytest.raises(ValueError):
        PruneConfig(halo=4)
    with pytest.raises(TypeError):
        inference(m, imgs, "cuda", max_inference_len=4, prune="yes")
    with pytest.raises(ValueError):
        inference(m, pruned, "cuda", max_inference_len=4, prune=True)          # already pruned
    with pytest.raises(ValueError):
        prune_patches(pruned)
    table, rows, max_grid = ops.prune_table(dims, (4, 8), dev)
    ink = torch.zeros(rows, dtype=torch.int32, device=dev)
    for bad in (dict(halo=4), dict(halo=-1), dict(max_ink=-1)):
        with pytest.raises(ValueError):
            ops.patch_keep(ink, table, max_grid, **bad)
    with pytest.raises(ValueError):
        ops.prune_table([(1025, 1024)], (4, 8), dev)                            # a grid beyond 2^20 patches
    with pytest.raises(ValueError):
        prune_patches(pruned.slice(0, 1))
    # training mode (gradients enabled, parameters that take them): encoding a pruned stream is out of scope
    assert any(p.requires_grad for p in m.encoder.parameters())
    with torch.enable_grad():
        with pytest.raises(ValueError):
            m.encoder.forward_packed(imgs, prune=True)
        with pytest.raises(ValueError):
            m.encoder.forward_packed(pruned)
        with pytest.raises(ValueError):
            m.encoder.embed_packed(imgs, prune=PruneConfig())
    mae = MAE(0.75, 16, 4, 8, encoder_hidden_dim=32, decoder_hidden_dim=32, encoder_kwargs=dict(num_layers=1, num_heads=2, mlp_dim=64),
              decoder_kwargs=dict(num_layers=1, num_heads=2, mlp_dim=64)).to(dev)
    with pytest.raises(ValueError):
        mae(imgs, prune=True)
    with pytest.raises(ValueError):
        mae.forward_packed(imgs, prune=PruneConfig())
    with torch.no_grad(), pytest.raises(ValueError):
        mae.encoder.forward_packed([t.to(dev) for t in imgs], prune=True)

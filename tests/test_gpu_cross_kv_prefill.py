"""acai_cross_kv_prefill (the memory cache every decode mode reads) against a float64 reference, on every GEMM kernel its dispatch
(epi 1 in csrc/gemm_plan.h) can pick: K/V = mem . Wkv^T + bkv, scattered head-major, ragged per sequence and padded from dh to dhp.

Every case checks the values at the addressed elements, that every other element of both buffers (pad lanes d in [dh, dhp), the gaps
between the sequences' regions, a guard before the first and after the last region) still holds the sentinel it was filled with, and
runs with and without the bias.  Tolerances (inputs scaled as in test_gpu_kernels._check_gemm_nt: mem ~ N(0,1), Wkv ~ N(0,1)/sqrt(E),
bkv ~ N(0,1)):
  fp32  |out - ref| < 2e-5 * max(1, sqrt(E)/8)                    the project's fp32 GEMM tolerance
  bf16  |out - ref| <= 2^-8 |ref| + 1e-4 sqrt(E) + 1e-4           one bf16 ulp (twice the half-ulp of the final rounding) plus the
                                                                  project's fp32-accumulation term; reference on the bf16-rounded operands

Which kernel a shape reaches is not derived here: the comments next to the shapes say why a shape was chosen, and each test asserts the
kernel its calls ran (acai_gemm_last_plan; the rule itself is csrc/gemm_plan.h, tested without a GPU in test_gemm_plan_cpu.py).  N = 2E,
K = E; a K-tile is 64 bf16 / 32 fp32 elements, a 16-byte chunk 8 / 4.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = 776.0     # exact in bf16 (seven significant bits; 777 would round to it); no K/V value of these inputs comes near it
GUARD = 96       # elements before the first and after the last region


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from acai_omr_amd import _lib
    _lib.lib()  # fails loudly if the HIP library is not built
    return torch.device("cuda:0")


def _ragged(M, g, lo=2, hi=150):
    """Ragged lengths that sum to M, in shuffled order: one of 1, one above 256 where M > 300, the rest drawn from [lo, hi]."""
    lens = [1]
    if M > 300:
        lens.append(257 + int(torch.randint(0, 40, (1,), generator=g)))
    rest = M - sum(lens)
    while rest > 0:
        l = min(rest, int(torch.randint(lo, hi + 1, (1,), generator=g)))
        lens.append(l)
        rest -= l
    return [lens[i] for i in torch.randperm(len(lens), generator=g).tolist()]


def _layout(lens, H, dhp, g, single_off=None):
    """seq_off and the buffer size: the sequences' regions (H * len * dhp elements) laid out in a shuffled order, so that seq_off is
    neither ascending nor descending in b, an odd number of unused elements after each, GUARD elements at either end."""
    B = len(lens)
    if B == 1:
        return [single_off], single_off + H * lens[0] * dhp + GUARD
    while True:
        order = torch.randperm(B, generator=g).tolist()
        off, o = [0] * B, GUARD
        for b in order:
            off[b] = o
            o += H * lens[b] * dhp + 1 + 2 * int(torch.randint(0, 20, (1,), generator=g))
        if B < 3 or (off != sorted(off) and off != sorted(off, reverse=True)):
            return off, o + GUARD


def _positions(row_seq, row_pos, seq_off, seq_len, H, dh, dhp):
    """int64 [M, H, dh]: the cache element of (memory row r, head h, lane d) = seq_off[b] + (h * seq_len[b] + s) * dhp + d."""
    b = row_seq.long()
    h = torch.arange(H, device=b.device).view(1, H, 1)
    d = torch.arange(dh, device=b.device).view(1, 1, dh)
    return seq_off[b].view(-1, 1, 1) + (h * seq_len[b].long().view(-1, 1, 1) + row_pos.long().view(-1, 1, 1)) * dhp + d


def _scatter_ref(kv, pos, total):
    """float64 [total] with kv [M, E] (column h*dh + d) at pos [M, H, dh], and the mask of the addressed elements."""
    flat = pos.reshape(-1)
    assert int(flat.min()) >= GUARD and int(flat.max()) < total - GUARD, "test layout: a position outside the buffer's interior"
    mask = torch.zeros(total, dtype=torch.bool, device=kv.device)
    mask[flat] = True
    assert int(mask.sum()) == flat.numel(), "test layout: two (row, head, lane) triples share an element"
    ref = torch.zeros(total, dtype=torch.float64, device=kv.device)
    ref[flat] = kv.reshape(-1)
    return ref, mask


_cases = {}


def _case(dev, H, dh, dhp, E, M, dtype, lens=None, view="contig", on_device=False, single_off=None, lo=2, hi=150):
    """Inputs on the GPU and float64 references (with and without the bias) of one shape; built once and shared by the tests that use the
    shape (the pinned variants), never modified.  on_device: the float64 reference runs as a torch matmul on the GPU (the batch-size cases)."""
    key = (H, dh, dhp, E, M, dtype, tuple(lens) if lens else None, view, single_off)
    if key in _cases:
        return _cases[key]
    assert E == H * dh and dhp >= dh
    g = torch.Generator().manual_seed(1000 * E + M + (7 if dtype == "bf16" else 0))
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    mem = torch.randn(M, E, generator=g)
    w_in = torch.randn(3 * E, E, generator=g) / math.sqrt(E)     # the cross-attention in-projection; Wkv is its row slice [E:], as in the engine
    b_in = torch.randn(3 * E, generator=g)
    if dtype == "bf16":
        mem, w_in = mem.to(tdt).float(), w_in.to(tdt).float()     # the reference sees the bf16-rounded operands
    if lens is None:
        lens = [M] if single_off is not None else _ragged(M, g, lo, hi)
    assert sum(lens) == M and (single_off is not None or 1 in lens) and (M <= 300 or single_off is not None or max(lens) > 256)
    seq_off, total = _layout(lens, H, dhp, g, single_off)
    # memory rows in shuffled order: row r holds position row_pos[r] of sequence row_seq[r]
    perm = torch.randperm(M, generator=g)
    row_seq = torch.cat([torch.full((l,), b, dtype=torch.int32) for b, l in enumerate(lens)])[perm]
    row_pos = torch.cat([torch.arange(l, dtype=torch.int32) for l in lens])[perm]
    seq_off_t, seq_len_t = torch.tensor(seq_off, dtype=torch.int64), torch.tensor(lens, dtype=torch.int32)

    rdev = dev if on_device else torch.device("cpu")
    pos = _positions(row_seq.to(rdev), row_pos.to(rdev), seq_off_t.to(rdev), seq_len_t.to(rdev), H, dh, dhp)
    base = mem.to(rdev).double() @ w_in[E:].to(rdev).double().t()
    c = {"H": H, "dh": dh, "dhp": dhp, "E": E, "M": M, "dtype": dtype, "tdt": tdt, "total": total, "rdev": rdev}
    for name, kv in (("nobias", base), ("bias", base + b_in[E:].to(rdev).double())):
        k_ref, mask = _scatter_ref(kv[:, :E], pos, total)
        v_ref, _ = _scatter_ref(kv[:, E:], pos, total)
        c[name] = (k_ref, v_ref)
    c["mask"] = mask
    del base, pos

    md = mem.to(dev).to(tdt)
    if view == "odd_stride":       # a column view of a wider buffer: row stride 77 elements, first element 5 elements in -> !fast
        wide = torch.zeros(M, E + 13, dtype=tdt, device=dev)
        wide[:, 5:5 + E] = md
        md = wide[:, 5:5 + E]
        assert md.stride(0) % 4 != 0
    elif view == "aligned_view":   # row stride E + 24 (a multiple of 8), first element 8 elements in (16 / 32 bytes) -> fast
        wide = torch.zeros(M, E + 24, dtype=tdt, device=dev)
        wide[:, 8:8 + E] = md
        md = wide[:, 8:8 + E]
        assert md.stride(0) % 8 == 0 and md.data_ptr() % 16 == 0
    else:
        assert view == "contig"
    c["mem"] = md
    c["wkv"] = w_in.to(dev).to(tdt)[E:]
    c["bkv"] = b_in.to(dev)[E:]
    assert c["wkv"].stride(0) == E and c["wkv"].data_ptr() == c["wkv"]._base.data_ptr() + E * E * c["wkv"].element_size()
    c["row_seq"], c["row_pos"], c["seq_off"], c["seq_len"] = row_seq.to(dev), row_pos.to(dev), seq_off_t.to(dev), seq_len_t.to(dev)
    if not on_device:
        _cases[key] = c
    return c


def _run(dev, c, bias, round_bf16=False):
    from acai_omr_amd import ops
    k = torch.full((c["total"],), SENT, dtype=c["tdt"], device=dev)
    v = torch.full((c["total"],), SENT, dtype=c["tdt"], device=dev)
    ops.cross_kv_prefill(c["mem"], c["wkv"], c["bkv"] if bias else None, c["row_seq"], c["row_pos"], c["seq_off"], c["seq_len"], k, v,
                         c["H"], c["dh"], c["dhp"], round_bf16=round_bf16)
    torch.cuda.synchronize()
    return k, v


def _check_one(out, ref, mask, E, dtype, what):
    o = out.to(ref.device)
    ibits = torch.int16 if o.dtype == torch.bfloat16 else torch.int32
    sent = torch.full((1,), SENT, dtype=o.dtype, device=o.device).view(ibits)
    stray = int((o.view(ibits)[~mask] != sent).sum())
    err = (o.double()[mask] - ref[mask]).abs()
    if dtype == "fp32":
        bound = torch.full_like(err, 2e-5 * max(1.0, math.sqrt(E) / 8))
    else:
        bound = 2.0 ** -8 * ref[mask].abs() + 1e-4 * math.sqrt(E) + 1e-4
    print(f"{what}: max |out - ref| {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}, "
          f"unaddressed elements changed {stray} of {int((~mask).sum())}")
    assert stray == 0, f"{what}: {stray} elements outside the addressed set were written"
    if dtype == "fp32":
        assert bool((err < bound).all()), f"{what}: max error {float(err.max()):.3e} against {float(bound[0]):.3e}"
    else:
        assert bool((err <= bound).all()), f"{what}: max error / bound {float((err / bound).max()):.3f}"


def _check(dev, c, what, ran=None):
    """ran: the kernel each call must have launched (_lib.gemm_last_kernels)"""
    from acai_omr_amd import _lib
    for name in ("bias", "nobias"):
        k, v = _run(dev, c, name == "bias")
        assert ran is None or _lib.gemm_last_kernels() == [ran], (what, name, _lib.gemm_last_kernels())
        k_ref, v_ref = c[name]
        # (K against the K reference in k_out and V against the V reference in v_out: data in the wrong buffer fails both)
        _check_one(k, k_ref, c["mask"], c["E"], c["dtype"], f"{what} {name} K")
        _check_one(v, v_ref, c["mask"], c["E"], c["dtype"], f"{what} {name} V")


# ---- the register-staged kernel (gemm_nt_kernel), auto dispatch ------------------------------------------------------------------------
GENERIC = [
    # E = 10: K % EPC != 0 (10 % 8, 10 % 4) -> !fast -> gemm_nt_kernel<FAST = false> for both types.  One 128 x 128 tile, 20 of its columns.
    (2, 5, 8, 10, 11, [3, 1, 7]),
    # E = 48: 48 % 8 == 0 and contiguous, aligned operands -> fast; 48 % 64 != 0 (bf16), 48 % 32 != 0 (fp32) -> gemm_nt_kernel<FAST = true>
    # with a partial last K-tile.  N = 96: the K/V boundary (column 48) lies inside the 32-lane column block [32, 64), heads of 12 columns
    # straddle the blocks' edges, pad lanes [12, 16).  M = 50: one row tile.
    (4, 12, 16, 48, 50, [20, 1, 29]),
    # M = 257: three 128-row tiles, the last with one row; sequence 0 (129 rows) is longer than a tile.
    (4, 12, 16, 48, 257, [129, 1, 127]),
]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("H,dh,dhp,E,M,lens", GENERIC, ids=lambda p: "-".join(map(str, p)) if isinstance(p, list) else str(p))
def test_generic_kernels(dev, H, dh, dhp, E, M, lens, dtype):
    _check(dev, _case(dev, H, dh, dhp, E, M, dtype, lens=lens), f"E={E} M={M} {dtype}", ran=f"gemm_nt_kernel<fast={int(E % 8 == 0)}>")


# E = 64, M = 130 (two row tiles, the second with 2 rows; H = 1, one 64-lane head): a whole number of K-tiles in both types, one small
# problem -> the 128 x 128 two-stage LDS-DMA kernel for contiguous operands and for an aligned view; a row stride of 77 elements allows no
# 16-byte chunks -> the register-staged kernel with guarded loads.
# With H = 1 the position h * len + s does not depend on how heads and positions interleave, so the same shape also runs as four heads of 16.
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("view", ["contig", "odd_stride", "aligned_view"])
@pytest.mark.parametrize("H,dh", [(1, 64), (4, 16)])
def test_two_stage_tile_and_memory_views(dev, H, dh, view, dtype):
    _check(dev, _case(dev, H, dh, dh, 64, 130, dtype, lens=[64, 1, 65], view=view), f"E=64 H={H} M=130 {view} {dtype}",
           ran="gemm_nt_kernel<fast=0>" if view == "odd_stride" else "gemm_nt_glds_kernel<wm=2>")


# ---- the LDS-DMA kernels, each pinned --------------------------------------------------------------------------------------------------
# M is the smallest count of the form 256 n + 5 with at least eight 256 x 256 tiles (then at least eight 256 x 128 tiles too), so that a
# pinned 4 / 5 / 6 is not sent back to variant 1; the last 256-row tile holds 5 rows.  K-tiles bf16 / fp32 = E/64 / E/32.
# The scatter epilogue has no persistent 256 x 256 ring: 6 runs the 256 x 256 kernel of 5 (its epilogue takes the wave's block as two
# 64-row halves).
PINNED_KERNEL = {1: "gemm_nt_glds_kernel<wm=2>", 2: "gemm_nt_glds_kernel<wm=4>", 3: "gemm_nt_glds3_kernel", 4: "gemm_nt_pers_kernel",
                 5: "gemm_nt_256_kernel", 6: "gemm_nt_256_kernel"}
PINNED = [
    # N = 256: cdiv(N,256) = 1 -> cdiv(M,256) >= 8 -> M > 1792.  2 / 4 K-tiles.
    (128, 8, 16, 16, 1797),
    # N = 384: cdiv(N,256) = 2 -> cdiv(M,256) >= 4 -> M > 768.  3 / 6 K-tiles.  Heads of 48 columns: their edges are not on the 32-column
    # blocks; pad lanes [48, 64); the K/V boundary (column 192) is in the middle of the 128-column tile [128, 256) and of the 256-column tile [0, 256).
    (192, 4, 48, 64, 773),
    (192, 6, 32, 32, 773),
    # N = 640: cdiv(N,256) = 3 -> cdiv(M,256) >= 3 -> M > 512.  5 / 10 K-tiles.
    (320, 5, 64, 64, 517),
]


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("E,H,dh,dhp,M", PINNED)
def test_lds_dma_kernels_pinned(dev, E, H, dh, dhp, M, dtype, variant):
    from acai_omr_amd import _lib
    c = _case(dev, H, dh, dhp, E, M, dtype)
    _lib.check(_lib.lib().acai_gemm_set_variant(variant), "acai_gemm_set_variant")
    try:
        _check(dev, c, f"variant {variant} E={E} H={H} M={M} {dtype}", ran=PINNED_KERNEL[variant])
    finally:
        _lib.lib().acai_gemm_set_variant(0)


# ---- auto dispatch at batch size: what a rollout batch of 64 images by a few hundred memory tokens runs --------------------------------
# bf16, E = 512: N = 1024, M = 16400 is 65 x 8 = 520 tiles of 256 x 128 - the smallest row count of a rollout batch past the 512 tiles from
#   which the auto rule leaves the 128 x 128 kernel; 8 K-tiles -> the persistent three-stage ring.
# fp32, E = 1024: N = 2048, M = 8000 is 32 x 16 = 512 such tiles; 32 K-tiles of 32 floats -> the three-stage kernel.
@pytest.mark.parametrize("dtype,E,H,dh,M", [("bf16", 512, 8, 64, 16400), ("fp32", 1024, 16, 64, 8000)])
def test_auto_dispatch_at_batch_size(dev, dtype, E, H, dh, M):
    _check(dev, _case(dev, H, dh, dh, E, M, dtype, on_device=True, lo=100, hi=400), f"auto E={E} M={M} {dtype}",
           ran="gemm_nt_pers_kernel" if dtype == "bf16" else "gemm_nt_glds3_kernel")


# ---- the slot refill's call shape (engine._slot_refill): one sequence, row_seq all zero, a one-element seq_off that is not zero ----------
# (4, 12, 16, 48, 50) -> gemm_nt_kernel<FAST = true>, (1, 64, 64, 64, 130) -> variant 1, as derived above
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("H,dh,dhp,E,M", [(4, 12, 16, 48, 50), (1, 64, 64, 64, 130)])
def test_single_sequence_at_an_offset(dev, H, dh, dhp, E, M, dtype):
    c = _case(dev, H, dh, dhp, E, M, dtype, single_off=GUARD + 1237)
    assert int(c["row_seq"].abs().max()) == 0 and c["seq_off"].numel() == 1 and int(c["seq_off"][0]) > 0
    _check(dev, c, f"single sequence E={E} M={M} {dtype}")


# ---- flags ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,dh,dhp,E,M,lens", [GENERIC[1], (1, 64, 64, 64, 130, [64, 1, 65])], ids=["generic", "lds_dma"])
def test_round_flag_is_a_no_op_for_a_bf16_cache(dev, H, dh, dhp, E, M, lens):
    """The bf16 store rounds anyway: ACAI_GEMM_ROUND_BF16 (what the engine passes for a bf16 cache) must not change one bit."""
    c = _case(dev, H, dh, dhp, E, M, "bf16", lens=lens)
    k0, v0 = _run(dev, c, True)
    k1, v1 = _run(dev, c, True, round_bf16=True)
    assert torch.equal(k0.view(torch.int16), k1.view(torch.int16)) and torch.equal(v0.view(torch.int16), v1.view(torch.int16))


def test_round_flag_with_an_fp32_cache_is_refused(dev):
    """fp32 output is not rounded by the scatter epilogue: the flag is an error there (through the Python wrapper, on real operands)."""
    c = _case(dev, 4, 12, 16, 48, 50, "fp32", lens=[20, 1, 29])
    with pytest.raises(RuntimeError, match="ACAI_GEMM_ROUND_BF16"):
        _run(dev, c, True, round_bf16=True)

"""lane_xor_add / lane_xor_max (csrc/common.h) against the __shfl_xor butterfly stage they replace in decode attention, bit for bit.

acai_debug_lane_xor runs both on the same 64 lanes: row 0 of the result is the stage made on the DPP network (quad permutes for offsets
1 and 2, a rotation of the 16-lane row by 8, v_permlane16_swap / v_permlane32_swap for 16 and 32), row 1 the stage made with the shuffle.
Decode attention's results must not move by a bit when it swaps one for the other, so equality here is equality of bit patterns.

Offset 4 has no exact DPP form on gfx950.  The key loop uses row_half_mirror (lane i reads lane 7 - i of its group of 8) for it, which is
the lane i ^ 4 stage ONLY where the four lanes of every quad hold the same value - true of a score sum after its stages 1 and 2, not of
anything else (the wave merge keeps __shfl_xor at offset 4).  The offset-4 test therefore feeds quad-uniform rows, and a second test shows
that the restriction is real: on rows that are not quad-uniform the mirror form gives something else."""
import pytest
import torch

from decode_support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

OFFSETS = [1, 2, 8, 16, 32]


def _rows():
    """[rows][64] float32: random, mixed magnitudes, signed zeros, infinities (inf - inf among the sums), denormals, and a lane-index row."""
    g = torch.Generator().manual_seed(64)
    f32 = torch.float32
    tiny, big = torch.finfo(f32).tiny, torch.finfo(f32).max
    rows = [torch.randn(8, 64, generator=g),
            torch.randn(8, 64, generator=g) * torch.exp2(torch.randint(-40, 40, (8, 64), generator=g).float()),      # mixed magnitudes
            torch.randn(4, 64, generator=g) * tiny * 0.01,                                                           # denormals
            torch.randn(4, 64, generator=g) * tiny,                                                                  # around the denormal edge
            torch.where(torch.rand(4, 64, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0)),                # signed zeros
            torch.randn(4, 64, generator=g) * big * 0.6,                                                             # sums that overflow
            torch.arange(64, dtype=f32).repeat(1, 1)]
    sp = torch.randn(8, 64, generator=g)
    pick = torch.randint(0, 6, (8, 64), generator=g)
    for i, val in enumerate((float("inf"), float("-inf"), 0.0, -0.0, tiny * 0.5)):
        sp = torch.where(pick == i, torch.tensor(val), sp)
    rows.append(sp)
    x = torch.cat(rows).to(f32).contiguous()
    assert bool((x.abs() < tiny).logical_and(x != 0).any()) and bool(torch.isinf(x).any())
    return x


def _probe(dev, x, offset, op):
    from acai_omr_amd import _lib
    xin = x.to(dev)
    out = torch.full((2,) + tuple(x.shape), 7.0, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().acai_debug_lane_xor(xin.data_ptr(), x.shape[0], offset, op, out.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "acai_debug_lane_xor")
    torch.cuda.synchronize()
    return out.cpu()


def _stage(x, offset, op):
    """The stage on the CPU: lane i combines with lane i ^ offset."""
    partner = x[:, torch.arange(64) ^ offset]
    return torch.maximum(x, partner) if op else x + partner


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("op", [0, 1], ids=["add", "max"])
@pytest.mark.parametrize("offset", OFFSETS)
def test_lane_xor_stage_equals_the_shuffle_stage_bit_for_bit(dev, offset, op):  # noqa: F811
    x = _rows()
    got = _probe(dev, x, offset, op)
    assert torch.equal(_bits(got[0]), _bits(got[1])), (offset, op, (_bits(got[0]) != _bits(got[1])).nonzero()[:8].tolist())
    # and the shuffle stage is the stage: lane i with lane i ^ offset (on the eight rows of ordinary values: no statement here about how
    # the host adds denormals or orders a pair of zeros)
    assert torch.equal(_bits(got[1][:8]), _bits(_stage(x[:8], offset, op)))


@pytest.mark.parametrize("op", [0, 1], ids=["add", "max"])
def test_offset_4_mirror_form_equals_the_shuffle_on_quad_uniform_rows(dev, op):  # noqa: F811
    """row_half_mirror is the offset-4 stage only for quad-uniform input (see the module docstring): every quad holds one value."""
    x = _rows()[:, ::4].repeat_interleave(4, dim=1).contiguous()
    got = _probe(dev, x, 4, op)
    assert torch.equal(_bits(got[0]), _bits(got[1]))


def test_offset_4_mirror_form_is_not_a_general_stage(dev):  # noqa: F811
    """Lane index as the value: lane i ^ 4 would give i + (i ^ 4), the mirror gives i + (i - i % 8 + 7 - i % 8)."""
    x = torch.arange(64, dtype=torch.float32).reshape(1, 64)
    got = _probe(dev, x, 4, 0)
    lane = torch.arange(64)
    assert torch.equal(got[1][0], (lane + (lane ^ 4)).float())
    assert torch.equal(got[0][0], (lane + (lane - lane % 8 + 7 - lane % 8)).float())
    assert not torch.equal(got[0], got[1])

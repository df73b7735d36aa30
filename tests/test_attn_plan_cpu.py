"""The attention selection rule (csrc/attn_plan.h) through acai_attn_plan: a pure host function, called here without a GPU.

TABLE holds the plan of every case of tests/attn_probe.py in each dtype / prescaled combination the edge tests run it in, of the shapes the
source comments name, and of each override value on a shape that it changes.  Its expected values were recorded from the dispatch code as it
stood before the rule became a function of its own (launch<>, launch_bwd<> and the launchers of the kernel files compiled verbatim into a
host program whose launches were logged), so a row that changes means the selection changed: retuning a threshold shows here, and in the
GPU tests that assert the kernels they name.  A recorded launch is what that code handed to the kernel: the kernel, its template form, grid,
block, dynamic LDS bytes and the host-set fields of the argument block (tail, tail256, nqb / nblk)."""
import ctypes

import pytest

import attn_probe as P
from acai_omr_amd import _lib
from acai_omr_amd._lib import (ATTN_K_FWD as K_FWD, ATTN_K_FWD64 as K_FWD64, ATTN_K_FWD64W as K_FWD64W, ATTN_K_FWD64_TAIL as K_FWD64_TAIL,
                               ATTN_K_BWD_DQ as K_BWD_DQ, ATTN_K_BWD_DKV as K_BWD_DKV, ATTN_K_BWD_DQ2 as K_BWD_DQ2, ATTN_K_BWD_DKV2 as K_BWD_DKV2,
                               ATTN_K_BWD64W_DQ as K_BWD64W_DQ, ATTN_K_BWD64W_DKV as K_BWD64W_DKV, ATTN_K_BWD1P as K_BWD1P,
                               ATTN_OV_TWO_BLOCK as OV_TWO_BLOCK, ATTN_OV_FWD64 as OV_FWD64, ATTN_OV_BWD64_WIDE as OV_BWD64_WIDE,
                               ATTN_OV_BWD_1P as OV_BWD_1P, ATTN_OV_XCD_ORDER as OV_XCD_ORDER)

DEFAULTS = tuple(r[0] for r in _lib.ATTN_OV_RANGE)


def _q(backward, es, H, dh, lens_q, lens_k, causal=0, accum=0, drop=0, pre=0, ws=0, ov=None, aligned=1, ld=None):
    """A query as the entry points state it for packed, 16-byte aligned operands (what the edge tests pass): lens_k None = self-attention
    over the queries' own offsets; ws: a workspace as large as anyone may want is lent."""
    lk = lens_k or lens_q
    ld = ld or H * dh
    q = _lib.AcaiAttnQuery(backward=backward, elem_size=es, B=len(lens_q), H=H, dh=dh, max_q=max(lens_q), max_k=max(lk) if backward else 0,
                           total_q=sum(lens_q), total_k=sum(lk) if backward else 0, causal=causal, accum_dkv=accum, dropout=drop, q_prescaled=pre,
                           ldq=ld, ldk=ld, ldv=ld, ldo=ld, lddo=ld, lddq=ld, lddk=ld, lddv=ld, aligned=aligned, cu_k_is_cu_q=int(lens_k is None),
                           workspace_bytes=(1 << 40) if ws else 0)
    for i, v in enumerate(DEFAULTS):
        q.ov[i] = (ov or {}).get(i, v)
    return q


def _recorded(l):
    """An AcaiAttnLaunch as TABLE records one: (kernel, (elem, dhp, fast, drop, pre, nq, waves), grid, block, LDS bytes, tail, tail256, nblk).
    Only the instantiated kernels have a form, and only the forward one has `nq`; the rest of the tuple is zero, as recorded."""
    form = (0,) * 7
    if l.kernel in (K_FWD, K_BWD_DQ, K_BWD_DKV):
        form = (l.elem_size, l.dhp, l.fast, l.drop, l.pre, l.nq if l.kernel == K_FWD else 0, 0)
    elif l.kernel == K_FWD64:
        form = (0,) * 6 + (l.waves,)
    return (l.kernel, form, (l.grid_x, l.grid_y, l.grid_z), l.block, l.lds_bytes, l.tail, l.tail256, l.nblk)


def _plan(q):
    out, n, refusal = (_lib.AcaiAttnLaunch * 4)(), ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.check(_lib.lib().acai_attn_plan(ctypes.byref(q), out, ctypes.byref(n), ctypes.byref(refusal)), "acai_attn_plan")
    assert 0 <= n.value <= 4 and (n.value == 0) == (refusal.value != 0)
    return [out[i] for i in range(n.value)], refusal.value


# (query, [launch as _recorded gives it, ...], what acai_attn_varlen_bwd_workspace_bytes answered for the shape)
TABLE = [
    # attn_probe.FWD_GENERIC, every dtype / prescaled combination of the edge tests
    (_q(0, 4, 2, 16, [65, 64], None, causal=1), [(K_FWD, (4, 32, 1, 0, 0, 1, 0), (1, 2, 2), 256, 0, 0, 0, 0)], 0),
    (_q(0, 4, 2, 16, [65, 64], None, causal=1, pre=1), [(K_FWD, (4, 32, 1, 0, 1, 1, 0), (1, 2, 2), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 2, 16, [65, 64], None, causal=1), [(K_FWD, (2, 32, 1, 0, 0, 1, 0), (1, 2, 2), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 2, 16, [65, 64], None, causal=1, pre=1), [(K_FWD, (2, 32, 1, 0, 1, 1, 0), (1, 2, 2), 256, 0, 0, 0, 0)], 0),
    (_q(0, 4, 3, 32, [130, 1, 77], None), [(K_FWD, (4, 32, 1, 0, 0, 1, 0), (2, 3, 3), 256, 0, 0, 0, 0)], 0),
    (_q(0, 4, 3, 32, [130, 1, 77], None, pre=1), [(K_FWD, (4, 32, 1, 0, 1, 1, 0), (2, 3, 3), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 3, 32, [130, 1, 77], None), [(K_FWD, (2, 32, 1, 0, 0, 1, 0), (2, 3, 3), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 3, 32, [130, 1, 77], None, pre=1), [(K_FWD, (2, 32, 1, 0, 1, 1, 0), (2, 3, 3), 256, 0, 0, 0, 0)], 0),
    (_q(0, 4, 4, 12, [7, 12], [20, 13]), [(K_FWD, (4, 32, 1, 0, 0, 1, 0), (1, 4, 2), 256, 0, 0, 0, 0)], 0),
    (_q(0, 4, 4, 12, [7, 12], [20, 13], pre=1), [(K_FWD, (4, 32, 1, 0, 1, 1, 0), (1, 4, 2), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 4, 12, [7, 12], [20, 13]), [(K_FWD, (2, 32, 0, 0, 0, 1, 0), (1, 4, 2), 256, 0, 0, 0, 0)], 0),
    (_q(0, 4, 4, 16, [7, 12], [20, 13]), [(K_FWD, (4, 32, 1, 0, 0, 1, 0), (1, 4, 2), 256, 0, 0, 0, 0)], 0),
    (_q(0, 4, 4, 16, [7, 12], [20, 13], pre=1), [(K_FWD, (4, 32, 1, 0, 1, 1, 0), (1, 4, 2), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 4, 16, [7, 12], [20, 13]), [(K_FWD, (2, 32, 1, 0, 0, 1, 0), (1, 4, 2), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 4, 16, [7, 12], [20, 13], pre=1), [(K_FWD, (2, 32, 1, 0, 1, 1, 0), (1, 4, 2), 256, 0, 0, 0, 0)], 0),
    (_q(0, 4, 2, 64, [300], None, causal=1), [(K_FWD, (4, 64, 1, 0, 0, 1, 0), (3, 2, 1), 256, 0, 0, 0, 0)], 0),
    (_q(0, 4, 2, 64, [300], None, causal=1, pre=1), [(K_FWD, (4, 64, 1, 0, 1, 1, 0), (3, 2, 1), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 2, 64, [300], None, causal=1), [(K_FWD, (2, 64, 1, 0, 0, 1, 0), (3, 2, 1), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 2, 64, [300], None, causal=1, pre=1), [(K_FWD, (2, 64, 1, 0, 1, 1, 0), (3, 2, 1), 256, 0, 0, 0, 0)], 0),
    (_q(0, 4, 2, 8, [130, 1, 77], None), [(K_FWD, (4, 32, 1, 0, 0, 1, 0), (2, 2, 3), 256, 0, 0, 0, 0)], 0),
    (_q(0, 4, 2, 8, [130, 1, 77], None, pre=1), [(K_FWD, (4, 32, 1, 0, 1, 1, 0), (2, 2, 3), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 2, 8, [130, 1, 77], None), [(K_FWD, (2, 32, 1, 0, 0, 1, 0), (2, 2, 3), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 2, 8, [130, 1, 77], None, pre=1), [(K_FWD, (2, 32, 1, 0, 1, 1, 0), (2, 2, 3), 256, 0, 0, 0, 0)], 0),
    # attn_probe.FWD_TWO_BLOCK
    (_q(0, 2, 3, 32, [513, 640, 1], None, pre=1), [(K_FWD, (2, 32, 1, 0, 1, 2, 0), (3, 3, 3), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 2, 32, [600, 513], [1000, 577], pre=1), [(K_FWD, (2, 32, 1, 0, 1, 2, 0), (3, 2, 2), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 2, 24, [520], [64], pre=1), [(K_FWD, (2, 32, 1, 0, 1, 2, 0), (3, 2, 1), 256, 0, 0, 0, 0)], 0),
    # attn_probe.FWD_64
    (_q(0, 2, 2, 64, [513, 130], [1100, 64], pre=1), [(K_FWD64W, (0, 0, 0, 0, 0, 0, 0), (12, 1, 1), 256, 0, 32, 0, -3), (K_FWD64_TAIL, (0, 0, 0, 0, 0, 0, 0), (1, 2, 2), 512, 0, 32, 0, 0)], 0),
    (_q(0, 2, 1, 64, [40, 129, 192], [40, 65, 191], pre=1), [(K_FWD64W, (0, 0, 0, 0, 0, 0, 0), (3, 1, 1), 256, 0, 32, 0, -1), (K_FWD64_TAIL, (0, 0, 0, 0, 0, 0, 0), (1, 1, 3), 512, 0, 32, 0, 0)], 0),
    (_q(0, 2, 1, 64, [256], [1], pre=1), [(K_FWD64W, (0, 0, 0, 0, 0, 0, 0), (1, 1, 1), 256, 0, 0, 0, 1)], 0),
    (_q(0, 2, 2, 64, [288, 289, 20], [700, 64, 1], pre=1), [(K_FWD64W, (0, 0, 0, 0, 0, 0, 0), (12, 1, 1), 256, 0, 32, 0, -2), (K_FWD64_TAIL, (0, 0, 0, 0, 0, 0, 0), (1, 2, 3), 512, 0, 32, 0, 0)], 0),
    (_q(0, 2, 1, 64, [513] * 3, [1100] * 3, pre=1), [(K_FWD64W, (0, 0, 0, 0, 0, 0, 0), (6, 1, 1), 256, 0, 32, 0, -2), (K_FWD64_TAIL, (0, 0, 0, 0, 0, 0, 0), (1, 1, 3), 512, 0, 32, 0, 0)], 0),
    # attn_probe.FWD_64 on the four-wave and eight-wave attn_fwd64_kernel
    (_q(0, 2, 2, 64, [513, 130], [1100, 64], pre=1, ov={OV_FWD64: 1}), [(K_FWD64, (0, 0, 0, 0, 0, 0, 4), (5, 2, 2), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 2, 64, [513, 130], [1100, 64], pre=1, ov={OV_FWD64: 2}), [(K_FWD64, (0, 0, 0, 0, 0, 0, 8), (3, 2, 2), 512, 0, 0, 0, 0)], 0),
    (_q(0, 2, 1, 64, [40, 129, 192], [40, 65, 191], pre=1, ov={OV_FWD64: 1}), [(K_FWD64, (0, 0, 0, 0, 0, 0, 4), (2, 1, 3), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 1, 64, [40, 129, 192], [40, 65, 191], pre=1, ov={OV_FWD64: 2}), [(K_FWD64, (0, 0, 0, 0, 0, 0, 8), (1, 1, 3), 512, 0, 0, 0, 0)], 0),
    (_q(0, 2, 1, 64, [256], [1], pre=1, ov={OV_FWD64: 1}), [(K_FWD64, (0, 0, 0, 0, 0, 0, 4), (2, 1, 1), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 1, 64, [256], [1], pre=1, ov={OV_FWD64: 2}), [(K_FWD64, (0, 0, 0, 0, 0, 0, 8), (1, 1, 1), 512, 0, 0, 0, 0)], 0),
    (_q(0, 2, 2, 64, [288, 289, 20], [700, 64, 1], pre=1, ov={OV_FWD64: 1}), [(K_FWD64, (0, 0, 0, 0, 0, 0, 4), (3, 2, 3), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 2, 64, [288, 289, 20], [700, 64, 1], pre=1, ov={OV_FWD64: 2}), [(K_FWD64, (0, 0, 0, 0, 0, 0, 8), (2, 2, 3), 512, 0, 0, 0, 0)], 0),
    (_q(0, 2, 1, 64, [513] * 3, [1100] * 3, pre=1, ov={OV_FWD64: 1}), [(K_FWD64, (0, 0, 0, 0, 0, 0, 4), (5, 1, 3), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 1, 64, [513] * 3, [1100] * 3, pre=1, ov={OV_FWD64: 2}), [(K_FWD64, (0, 0, 0, 0, 0, 0, 8), (3, 1, 3), 512, 0, 0, 0, 0)], 0),
    # attn_probe.BWD_GENERIC, every dtype / prescaled combination
    (_q(1, 4, 2, 16, [65, 64], None, causal=1, ws=1), [(K_BWD_DQ, (4, 32, 1, 0, 0, 0, 0), (1, 2, 2), 256, 36864, 0, 0, 0), (K_BWD_DKV, (4, 32, 1, 0, 0, 0, 0), (1, 2, 2), 256, 37888, 0, 0, 0)], 0),
    (_q(1, 4, 2, 16, [65, 64], None, causal=1, pre=1, ws=1), [(K_BWD_DQ, (4, 32, 1, 0, 1, 0, 0), (1, 2, 2), 256, 36864, 0, 0, 0), (K_BWD_DKV, (4, 32, 1, 0, 1, 0, 0), (1, 2, 2), 256, 37888, 0, 0, 0)], 0),
    (_q(1, 2, 2, 16, [65, 64], None, causal=1, ws=1), [(K_BWD_DQ, (2, 32, 1, 0, 0, 0, 0), (1, 2, 2), 256, 16384, 0, 0, 0), (K_BWD_DKV, (2, 32, 1, 0, 0, 0, 0), (1, 2, 2), 256, 17408, 0, 0, 0)], 0),
    (_q(1, 2, 2, 16, [65, 64], None, causal=1, pre=1, ws=1), [(K_BWD_DQ, (2, 32, 1, 0, 1, 0, 0), (1, 2, 2), 256, 16384, 0, 0, 0), (K_BWD_DKV, (2, 32, 1, 0, 1, 0, 0), (1, 2, 2), 256, 17408, 0, 0, 0)], 0),
    (_q(1, 4, 2, 32, [333, 128], None, ws=1), [(K_BWD_DQ, (4, 32, 1, 0, 0, 0, 0), (3, 2, 2), 256, 36864, 0, 0, 0), (K_BWD_DKV, (4, 32, 1, 0, 0, 0, 0), (3, 2, 2), 256, 37888, 0, 0, 0)], 0),
    (_q(1, 4, 2, 32, [333, 128], None, pre=1, ws=1), [(K_BWD_DQ, (4, 32, 1, 0, 1, 0, 0), (3, 2, 2), 256, 36864, 0, 0, 0), (K_BWD_DKV, (4, 32, 1, 0, 1, 0, 0), (3, 2, 2), 256, 37888, 0, 0, 0)], 0),
    (_q(1, 2, 2, 32, [333, 128], None, ws=1), [(K_BWD_DQ, (2, 32, 1, 0, 0, 0, 0), (3, 2, 2), 256, 16384, 0, 0, 0), (K_BWD_DKV, (2, 32, 1, 0, 0, 0, 0), (3, 2, 2), 256, 17408, 0, 0, 0)], 0),
    (_q(1, 2, 2, 32, [333, 128], None, pre=1, ws=1), [(K_BWD_DQ, (2, 32, 1, 0, 1, 0, 0), (3, 2, 2), 256, 16384, 0, 0, 0), (K_BWD_DKV, (2, 32, 1, 0, 1, 0, 0), (3, 2, 2), 256, 17408, 0, 0, 0)], 0),
    (_q(1, 4, 1, 64, [256], [400], ws=1), [(K_BWD_DQ, (4, 64, 1, 0, 0, 0, 0), (2, 1, 1), 256, 69632, 0, 0, 0), (K_BWD_DKV, (4, 64, 1, 0, 0, 0, 0), (4, 1, 1), 256, 70656, 0, 0, 0)], 0),
    (_q(1, 4, 1, 64, [256], [400], pre=1, ws=1), [(K_BWD_DQ, (4, 64, 1, 0, 1, 0, 0), (2, 1, 1), 256, 69632, 0, 0, 0), (K_BWD_DKV, (4, 64, 1, 0, 1, 0, 0), (4, 1, 1), 256, 70656, 0, 0, 0)], 0),
    (_q(1, 2, 1, 64, [256], [400], ws=1), [(K_BWD_DQ, (2, 64, 1, 0, 0, 0, 0), (2, 1, 1), 256, 32768, 0, 0, 0), (K_BWD_DKV, (2, 64, 1, 0, 0, 0, 0), (4, 1, 1), 256, 33792, 0, 0, 0)], 0),
    (_q(1, 2, 1, 64, [256], [400], pre=1, ws=1), [(K_BWD64W_DQ, (0, 0, 0, 0, 0, 0, 0), (1, 1, 1), 256, 0, 0, 0, 1), (K_BWD_DKV, (2, 64, 1, 0, 1, 0, 0), (4, 1, 1), 256, 33792, 0, 0, 0)], 0),
    (_q(1, 4, 4, 12, [7, 12], [20, 13], ws=1), [(K_BWD_DQ, (4, 32, 1, 0, 0, 0, 0), (1, 4, 2), 256, 36864, 0, 0, 0), (K_BWD_DKV, (4, 32, 1, 0, 0, 0, 0), (1, 4, 2), 256, 37888, 0, 0, 0)], 0),
    (_q(1, 4, 4, 12, [7, 12], [20, 13], pre=1, ws=1), [(K_BWD_DQ, (4, 32, 1, 0, 1, 0, 0), (1, 4, 2), 256, 36864, 0, 0, 0), (K_BWD_DKV, (4, 32, 1, 0, 1, 0, 0), (1, 4, 2), 256, 37888, 0, 0, 0)], 0),
    (_q(1, 2, 4, 12, [7, 12], [20, 13], ws=1), [(K_BWD_DQ, (2, 32, 0, 0, 0, 0, 0), (1, 4, 2), 256, 16384, 0, 0, 0), (K_BWD_DKV, (2, 32, 0, 0, 0, 0, 0), (1, 4, 2), 256, 17408, 0, 0, 0)], 0),
    (_q(1, 4, 2, 8, [130, 77], None, ws=1), [(K_BWD_DQ, (4, 32, 1, 0, 0, 0, 0), (2, 2, 2), 256, 36864, 0, 0, 0), (K_BWD_DKV, (4, 32, 1, 0, 0, 0, 0), (2, 2, 2), 256, 37888, 0, 0, 0)], 0),
    (_q(1, 4, 2, 8, [130, 77], None, pre=1, ws=1), [(K_BWD_DQ, (4, 32, 1, 0, 1, 0, 0), (2, 2, 2), 256, 36864, 0, 0, 0), (K_BWD_DKV, (4, 32, 1, 0, 1, 0, 0), (2, 2, 2), 256, 37888, 0, 0, 0)], 0),
    (_q(1, 2, 2, 8, [130, 77], None, ws=1), [(K_BWD_DQ, (2, 32, 1, 0, 0, 0, 0), (2, 2, 2), 256, 16384, 0, 0, 0), (K_BWD_DKV, (2, 32, 1, 0, 0, 0, 0), (2, 2, 2), 256, 17408, 0, 0, 0)], 0),
    (_q(1, 2, 2, 8, [130, 77], None, pre=1, ws=1), [(K_BWD_DQ, (2, 32, 1, 0, 1, 0, 0), (2, 2, 2), 256, 16384, 0, 0, 0), (K_BWD_DKV, (2, 32, 1, 0, 1, 0, 0), (2, 2, 2), 256, 17408, 0, 0, 0)], 0),
    # attn_probe.BWD_TWO_BLOCK, no workspace lent
    (_q(1, 2, 2, 32, [513, 700], None, pre=1), [(K_BWD_DQ2, (0, 0, 0, 0, 0, 0, 0), (3, 2, 2), 256, 16384, 0, 0, 0), (K_BWD_DKV2, (0, 0, 0, 0, 0, 0, 0), (3, 2, 2), 256, 17408, 0, 0, 0)], 326912),
    (_q(1, 2, 2, 32, [600, 513], [1000, 577], pre=1), [(K_BWD_DQ2, (0, 0, 0, 0, 0, 0, 0), (3, 2, 2), 256, 16384, 0, 0, 0), (K_BWD_DKV2, (0, 0, 0, 0, 0, 0, 0), (4, 2, 2), 256, 17408, 0, 0, 0)], 301312),
    (_q(1, 2, 1, 24, [1025], [512], pre=1), [(K_BWD_DQ2, (0, 0, 0, 0, 0, 0, 0), (5, 1, 1), 256, 16384, 0, 0, 0), (K_BWD_DKV2, (0, 0, 0, 0, 0, 0, 0), (2, 1, 1), 256, 17408, 0, 0, 0)], 0),
    # attn_probe.BWD_TWO_BLOCK + BWD_ONE_PASS_EQUAL, a workspace lent
    (_q(1, 2, 2, 32, [513, 700], None, pre=1, ws=1), [(K_BWD1P, (0, 0, 0, 0, 0, 0, 0), (8, 1, 1), 256, 153088, 0, 0, 2)], 326912),
    (_q(1, 2, 2, 32, [600, 513], [1000, 577], pre=1, ws=1), [(K_BWD1P, (0, 0, 0, 0, 0, 0, 0), (8, 1, 1), 256, 153088, 0, 0, 2)], 301312),
    (_q(1, 2, 1, 24, [1025], [512], pre=1, ws=1), [(K_BWD_DQ2, (0, 0, 0, 0, 0, 0, 0), (5, 1, 1), 256, 16384, 0, 0, 0), (K_BWD_DKV2, (0, 0, 0, 0, 0, 0, 0), (2, 1, 1), 256, 17408, 0, 0, 0)], 0),
    (_q(1, 2, 2, 32, [1024] * 2, None, pre=1, ws=1), [(K_BWD1P, (0, 0, 0, 0, 0, 0, 0), (8, 1, 1), 256, 153088, 0, 1, 2)], 540672),
    (_q(1, 2, 2, 32, [600] * 2, [1536] * 2, pre=1, ws=1), [(K_BWD1P, (0, 0, 0, 0, 0, 0, 0), (12, 1, 1), 256, 153088, 0, 1, 3)], 323584),
    # attn_probe.BWD_64
    (_q(1, 2, 2, 64, [513, 700], None, pre=1, ws=1), [(K_BWD64W_DQ, (0, 0, 0, 0, 0, 0, 0), (8, 1, 1), 256, 0, 0, 0, -2), (K_BWD_DQ, (2, 64, 1, 0, 1, 0, 0), (2, 2, 2), 256, 32768, 0, 1, 0), (K_BWD_DKV, (2, 64, 1, 0, 1, 0, 0), (6, 2, 2), 256, 33792, 0, 0, 0)], 0),
    (_q(1, 2, 2, 64, [600, 256, 40], [1000, 577, 300], pre=1, ws=1), [(K_BWD64W_DQ, (0, 0, 0, 0, 0, 0, 0), (12, 1, 1), 256, 0, 0, 0, -2), (K_BWD_DQ, (2, 64, 1, 0, 1, 0, 0), (2, 2, 3), 256, 32768, 0, 1, 0), (K_BWD_DKV, (2, 64, 1, 0, 1, 0, 0), (8, 2, 3), 256, 33792, 0, 0, 0)], 0),
    (_q(1, 2, 2, 64, [768], [129], pre=1, ws=1), [(K_BWD64W_DQ, (0, 0, 0, 0, 0, 0, 0), (6, 1, 1), 256, 0, 0, 0, 3), (K_BWD_DKV, (2, 64, 1, 0, 1, 0, 0), (2, 2, 1), 256, 33792, 0, 0, 0)], 0),
    # attn_probe.BWD_64 with the wide dK / dV form forced on
    (_q(1, 2, 2, 64, [513, 700], None, pre=1, ws=1, ov={OV_BWD64_WIDE: 3}), [(K_BWD64W_DQ, (0, 0, 0, 0, 0, 0, 0), (8, 1, 1), 256, 0, 0, 0, -2), (K_BWD_DQ, (2, 64, 1, 0, 1, 0, 0), (2, 2, 2), 256, 32768, 0, 1, 0), (K_BWD64W_DKV, (0, 0, 0, 0, 0, 0, 0), (8, 1, 1), 256, 0, 0, 0, -2), (K_BWD_DKV, (2, 64, 1, 0, 1, 0, 0), (2, 2, 2), 256, 33792, 0, 2, 0)], 0),
    (_q(1, 2, 2, 64, [600, 256, 40], [1000, 577, 300], pre=1, ws=1, ov={OV_BWD64_WIDE: 3}), [(K_BWD64W_DQ, (0, 0, 0, 0, 0, 0, 0), (12, 1, 1), 256, 0, 0, 0, -2), (K_BWD_DQ, (2, 64, 1, 0, 1, 0, 0), (2, 2, 3), 256, 32768, 0, 1, 0), (K_BWD64W_DKV, (0, 0, 0, 0, 0, 0, 0), (18, 1, 1), 256, 0, 0, 0, -3), (K_BWD_DKV, (2, 64, 1, 0, 1, 0, 0), (2, 2, 3), 256, 33792, 0, 2, 0)], 0),
    (_q(1, 2, 2, 64, [768], [129], pre=1, ws=1, ov={OV_BWD64_WIDE: 3}), [(K_BWD64W_DQ, (0, 0, 0, 0, 0, 0, 0), (6, 1, 1), 256, 0, 0, 0, 3), (K_BWD_DKV, (2, 64, 1, 0, 1, 0, 0), (2, 2, 1), 256, 33792, 0, 0, 0)], 0),
    # attn_probe.BWD_ACCUMULATE
    (_q(1, 2, 2, 64, [300], [513], accum=1, pre=1, ws=1), [(K_BWD64W_DQ, (0, 0, 0, 0, 0, 0, 0), (2, 1, 1), 256, 0, 0, 0, 1), (K_BWD_DQ, (2, 64, 1, 0, 1, 0, 0), (1, 2, 1), 256, 32768, 0, 1, 0), (K_BWD_DKV, (2, 64, 1, 0, 1, 0, 0), (5, 2, 1), 256, 33792, 0, 0, 0)], 0),
    # the encoder: 16 x 12 heads x 4096 x 4096, d_h 64
    (_q(0, 2, 12, 64, [4096] * 16, None, pre=1), [(K_FWD64W, (0, 0, 0, 0, 0, 0, 0), (3072, 1, 1), 256, 0, 0, 0, 16)], 0),
    (_q(1, 2, 12, 64, [4096] * 16, None, pre=1, ws=1), [(K_BWD64W_DQ, (0, 0, 0, 0, 0, 0, 0), (3072, 1, 1), 256, 0, 0, 0, 16), (K_BWD64W_DKV, (0, 0, 0, 0, 0, 0, 0), (3072, 1, 1), 256, 0, 0, 0, 16)], 0),
    # the decoder's cross attention: 513 x 4096, 16 x 16 heads
    (_q(0, 2, 16, 64, [513] * 16, [4096] * 16, pre=1), [(K_FWD64W, (0, 0, 0, 0, 0, 0, 0), (512, 1, 1), 256, 0, 32, 0, -2), (K_FWD64_TAIL, (0, 0, 0, 0, 0, 0, 0), (1, 16, 16), 512, 0, 32, 0, 0)], 0),
    (_q(1, 2, 16, 64, [513] * 16, [4096] * 16, pre=1, ws=1), [(K_BWD64W_DQ, (0, 0, 0, 0, 0, 0, 0), (512, 1, 1), 256, 0, 0, 0, 2), (K_BWD_DQ, (2, 64, 1, 0, 1, 0, 0), (1, 16, 16), 256, 32768, 0, 1, 0), (K_BWD_DKV, (2, 64, 1, 0, 1, 0, 0), (32, 16, 16), 256, 33792, 0, 0, 0)], 0),
    # the MAE decoder: 16 heads, d_h 32, 1024 x 1024, with and without a workspace
    (_q(0, 2, 16, 32, [1024] * 32, None, pre=1), [(K_FWD, (2, 32, 1, 0, 1, 2, 0), (4, 16, 32), 256, 0, 0, 0, 0)], 0),
    (_q(1, 2, 16, 32, [1024] * 32, None, pre=1, ws=1), [(K_BWD1P, (0, 0, 0, 0, 0, 0, 0), (1024, 1, 1), 256, 153088, 0, 1, 2)], 67239936),
    (_q(1, 2, 16, 32, [1024] * 32, None, pre=1), [(K_BWD_DQ2, (0, 0, 0, 0, 0, 0, 0), (4, 16, 32), 256, 16384, 0, 0, 0), (K_BWD_DKV2, (0, 0, 0, 0, 0, 0, 0), (4, 16, 32), 256, 17408, 0, 0, 0)], 67239936),
    # ACAI_ATTN_OV_TWO_BLOCK = 0, forward and backward
    (_q(0, 2, 16, 32, [1024] * 32, None, pre=1, ov={OV_TWO_BLOCK: 0}), [(K_FWD, (2, 32, 1, 0, 1, 1, 0), (8, 16, 32), 256, 0, 0, 0, 0)], 0),
    (_q(1, 2, 16, 32, [1024] * 32, None, pre=1, ov={OV_TWO_BLOCK: 0}), [(K_BWD_DQ, (2, 32, 1, 0, 1, 0, 0), (8, 16, 32), 256, 16384, 0, 0, 0), (K_BWD_DKV, (2, 32, 1, 0, 1, 0, 0), (8, 16, 32), 256, 17408, 0, 0, 0)], 67239936),
    # ACAI_ATTN_OV_FWD64 = four-wave, eight-wave, generic kernel
    (_q(0, 2, 12, 64, [4096] * 16, None, pre=1, ov={OV_FWD64: 1}), [(K_FWD64, (0, 0, 0, 0, 0, 0, 4), (32, 12, 16), 256, 0, 0, 0, 0)], 0),
    (_q(0, 2, 12, 64, [4096] * 16, None, pre=1, ov={OV_FWD64: 2}), [(K_FWD64, (0, 0, 0, 0, 0, 0, 8), (16, 12, 16), 512, 0, 0, 0, 0)], 0),
    (_q(0, 2, 12, 64, [4096] * 16, None, pre=1, ov={OV_FWD64: 3}), [(K_FWD, (2, 64, 1, 0, 1, 1, 0), (32, 12, 16), 256, 0, 0, 0, 0)], 0),
    # ACAI_ATTN_OV_BWD64_WIDE = 0 .. 3 on the decoder's cross attention (auto = 1 there)
    (_q(1, 2, 16, 64, [513] * 16, [4096] * 16, pre=1, ws=1, ov={OV_BWD64_WIDE: 0}), [(K_BWD_DQ, (2, 64, 1, 0, 1, 0, 0), (5, 16, 16), 256, 32768, 0, 0, 0), (K_BWD_DKV, (2, 64, 1, 0, 1, 0, 0), (32, 16, 16), 256, 33792, 0, 0, 0)], 0),
    (_q(1, 2, 16, 64, [513] * 16, [4096] * 16, pre=1, ws=1, ov={OV_BWD64_WIDE: 1}), [(K_BWD64W_DQ, (0, 0, 0, 0, 0, 0, 0), (512, 1, 1), 256, 0, 0, 0, 2), (K_BWD_DQ, (2, 64, 1, 0, 1, 0, 0), (1, 16, 16), 256, 32768, 0, 1, 0), (K_BWD_DKV, (2, 64, 1, 0, 1, 0, 0), (32, 16, 16), 256, 33792, 0, 0, 0)], 0),
    (_q(1, 2, 16, 64, [513] * 16, [4096] * 16, pre=1, ws=1, ov={OV_BWD64_WIDE: 2}), [(K_BWD_DQ, (2, 64, 1, 0, 1, 0, 0), (5, 16, 16), 256, 32768, 0, 0, 0), (K_BWD64W_DKV, (0, 0, 0, 0, 0, 0, 0), (4096, 1, 1), 256, 0, 0, 0, -16), (K_BWD_DKV, (2, 64, 1, 0, 1, 0, 0), (2, 16, 16), 256, 33792, 0, 2, 0)], 0),
    (_q(1, 2, 16, 64, [513] * 16, [4096] * 16, pre=1, ws=1, ov={OV_BWD64_WIDE: 3}), [(K_BWD64W_DQ, (0, 0, 0, 0, 0, 0, 0), (512, 1, 1), 256, 0, 0, 0, 2), (K_BWD_DQ, (2, 64, 1, 0, 1, 0, 0), (1, 16, 16), 256, 32768, 0, 1, 0), (K_BWD64W_DKV, (0, 0, 0, 0, 0, 0, 0), (4096, 1, 1), 256, 0, 0, 0, -16), (K_BWD_DKV, (2, 64, 1, 0, 1, 0, 0), (2, 16, 16), 256, 33792, 0, 2, 0)], 0),
    # ... and 1 on the encoder (auto = 3 there)
    (_q(1, 2, 12, 64, [4096] * 16, None, pre=1, ws=1, ov={OV_BWD64_WIDE: 1}), [(K_BWD64W_DQ, (0, 0, 0, 0, 0, 0, 0), (3072, 1, 1), 256, 0, 0, 0, 16), (K_BWD_DKV, (2, 64, 1, 0, 1, 0, 0), (32, 12, 16), 256, 33792, 0, 0, 0)], 0),
    # ACAI_ATTN_OV_BWD_1P = 0
    (_q(1, 2, 16, 32, [1024] * 32, None, pre=1, ws=1, ov={OV_BWD_1P: 0}), [(K_BWD_DQ2, (0, 0, 0, 0, 0, 0, 0), (4, 16, 32), 256, 16384, 0, 0, 0), (K_BWD_DKV2, (0, 0, 0, 0, 0, 0, 0), (4, 16, 32), 256, 17408, 0, 0, 0)], 0),
    # ACAI_ATTN_OV_XCD_ORDER = 0 on an equal-length batch, 1 on a ragged one
    (_q(0, 2, 12, 64, [4096] * 16, None, pre=1, ov={OV_XCD_ORDER: 0}), [(K_FWD64W, (0, 0, 0, 0, 0, 0, 0), (3072, 1, 1), 256, 0, 0, 0, -16)], 0),
    (_q(1, 2, 12, 64, [4096] * 16, None, pre=1, ws=1, ov={OV_XCD_ORDER: 0}), [(K_BWD64W_DQ, (0, 0, 0, 0, 0, 0, 0), (3072, 1, 1), 256, 0, 0, 0, -16), (K_BWD64W_DKV, (0, 0, 0, 0, 0, 0, 0), (3072, 1, 1), 256, 0, 0, 0, -16)], 0),
    (_q(0, 2, 2, 64, [513, 130], [1100, 64], pre=1, ov={OV_XCD_ORDER: 1}), [(K_FWD64W, (0, 0, 0, 0, 0, 0, 0), (12, 1, 1), 256, 0, 32, 0, 3), (K_FWD64_TAIL, (0, 0, 0, 0, 0, 0, 0), (1, 2, 2), 512, 0, 32, 0, 0)], 0),
    (_q(1, 2, 2, 64, [513, 700], None, pre=1, ws=1, ov={OV_XCD_ORDER: 1}), [(K_BWD64W_DQ, (0, 0, 0, 0, 0, 0, 0), (8, 1, 1), 256, 0, 0, 0, 2), (K_BWD_DQ, (2, 64, 1, 0, 1, 0, 0), (2, 2, 2), 256, 32768, 0, 1, 0), (K_BWD_DKV, (2, 64, 1, 0, 1, 0, 0), (6, 2, 2), 256, 33792, 0, 0, 0)], 0),
]


def _id(row):
    q = row[0]
    ov = "".join(f"-ov{i}={q.ov[i]}" for i in range(len(DEFAULTS)) if q.ov[i] != DEFAULTS[i])
    return (f"{'bwd' if q.backward else 'fwd'}-{'bf16' if q.elem_size == 2 else 'fp32'}-B{q.B}-H{q.H}-dh{q.dh}-q{q.max_q}of{q.total_q}-k{q.max_k}of{q.total_k}"
            f"{'-causal' if q.causal else ''}{'-accum' if q.accum_dkv else ''}{'-pre' if q.q_prescaled else ''}{'-self' if q.cu_k_is_cu_q else ''}"
            f"{'-ws' if q.workspace_bytes else ''}{ov}")


@pytest.mark.parametrize("row", TABLE, ids=_id)
def test_plan_equals_the_recorded_dispatch(row):
    q, expected, _ = row
    plan, refusal = _plan(q)
    assert refusal == 0 and [_recorded(l) for l in plan] == expected
    for l in plan:   # what the recording did not hold follows from what it did
        assert l.rows >= 1 and l.block in (256, 512)
        if l.kernel == K_BWD1P:
            assert l.equal_len == l.tail256 and l.nblk == q.max_k // 512 + l.partial_blocks and l.grid_x == l.nblk * q.H * q.B
        elif l.kernel in (K_FWD64W, K_BWD64W_DQ, K_BWD64W_DKV):
            assert l.grid_x == abs(l.nblk) * q.H * q.B and (l.grid_y, l.grid_z) == (1, 1)


def test_table_holds_every_probe_case_in_every_combination_the_edge_tests_run():
    have = {(q.backward, q.elem_size, q.H, q.dh, q.B, q.max_q, q.total_q, q.max_k, q.total_k, q.causal, q.q_prescaled) for q, _, _ in TABLE}
    for backward, cases in ((0, P.FWD_CASES), (1, P.BWD_CASES)):
        for H, dh, lq, lk, causal in cases:
            generic = (H, dh, lq, lk, causal) in (P.BWD_GENERIC if backward else P.FWD_GENERIC)
            for es in (4, 2) if generic else (2,):
                for pre in (0, 1) if generic else (1,):
                    if pre and dh % (16 // es):
                        continue
                    k = lk or lq
                    assert (backward, es, H, dh, len(lq), max(lq), sum(lq), max(k) if backward else 0, sum(k) if backward else 0, int(causal), pre) in have


def test_workspace_bytes_equal_what_the_plan_implies():
    L = _lib.lib()
    for q, _, recorded in (r for r in TABLE if r[0].backward):
        flags = q.causal | (q.accum_dkv << 1)
        args = (q.B, q.H, q.dh, q.max_q, q.max_k, q.total_q, q.total_k, flags, _lib.ACAI_BF16 if q.elem_size == 2 else _lib.ACAI_F32, 0.1 if q.dropout else 0.0, q.q_prescaled)
        lent = _lib.AcaiAttnQuery.from_buffer_copy(q)
        lent.workspace_bytes = 1 << 40
        with_ws, _ = _plan(lent)
        implied = (q.total_q + 64) * q.H * 32 * 4 if with_ws[0].kernel == K_BWD1P else 0
        # (the entry asks with the process-wide overrides, the rows with their own)
        saved = []
        for i in range(len(DEFAULTS)):
            v = ctypes.c_int(0)
            _lib.check(L.acai_attn_get_override(i, ctypes.byref(v)), "acai_attn_get_override")
            saved.append(v.value)
            _lib.check(L.acai_attn_set_override(i, q.ov[i]), "acai_attn_set_override")
        try:
            got = L.acai_attn_varlen_bwd_workspace_bytes(*args)
        finally:
            for i, v in enumerate(saved):
                _lib.check(L.acai_attn_set_override(i, v), "acai_attn_set_override")
        assert got == implied == recorded, (_id((q,)), got, implied, recorded)
        one_byte_short = _lib.AcaiAttnQuery.from_buffer_copy(q)
        one_byte_short.workspace_bytes = max(implied - 1, 0)
        assert all(l.kernel != K_BWD1P for l in _plan(one_byte_short)[0])


def test_overrides_are_copied_into_the_query_and_restored():
    """Setting and restoring every override leaves the plan of a default query as it was, and the setter refuses values outside its range
    (so a test that pins a form cannot pin one that does not exist)."""
    from acai_omr_amd import ops
    L = _lib.lib()
    before = [[_recorded(l) for l in _plan(q)[0]] for q, _, _ in TABLE]
    for which, (default, lo, hi) in enumerate(_lib.ATTN_OV_RANGE):
        for value in range(lo, hi + 1):
            with ops.attn_override(which, value):
                v = ctypes.c_int(99)
                _lib.check(L.acai_attn_get_override(which, ctypes.byref(v)), "acai_attn_get_override")
                assert v.value == value
            _lib.check(L.acai_attn_get_override(which, ctypes.byref(v)), "acai_attn_get_override")
            assert v.value == default
        for bad in (lo - 1, hi + 1):
            assert L.acai_attn_set_override(which, bad) != 0
    assert L.acai_attn_set_override(len(DEFAULTS), 0) != 0 and L.acai_attn_set_override(-1, 0) != 0
    assert [[_recorded(l) for l in _plan(q)[0]] for q, _, _ in TABLE] == before


def test_plan_returns_the_two_refusals():
    bf, f32 = 2, 4
    # prescaled q without aligned operands: a misaligned base, a row stride or a head size that is no multiple of a 16-byte chunk
    for q in (_q(0, bf, 2, 32, [100], None, pre=1, aligned=0), _q(0, bf, 2, 32, [100], None, pre=1, ld=68), _q(0, bf, 2, 12, [100], None, pre=1),
              _q(1, f32, 2, 32, [100], None, pre=1, aligned=0), _q(1, bf, 2, 32, [100], None, pre=1, ld=68),
              _q(1, bf, 2, 64, [600], None, pre=1, ld=1 << 22)):   # ... or rows past the 32-bit buffer resources of the backward staging
        assert _plan(q) == ([], _lib.ATTN_REFUSE_PRESCALED)
    # accumulating dk / dv without bf16 and aligned operands
    for q in (_q(1, f32, 2, 32, [100], None, accum=1), _q(1, bf, 2, 32, [100], None, accum=1, aligned=0), _q(1, bf, 2, 12, [100], None, accum=1)):
        assert _plan(q) == ([], _lib.ATTN_REFUSE_ACCUM)
    assert _plan(_q(1, bf, 2, 32, [100], None, accum=1))[1] == 0 and _plan(_q(0, bf, 2, 12, [100], None))[1] == 0


def test_plan_refuses_a_malformed_query():
    out, n = (_lib.AcaiAttnLaunch * 4)(), ctypes.c_int(0)
    for bad in (_q(0, 3, 2, 32, [100], None), _q(0, 2, 2, 65, [100], None), _q(0, 2, 0, 32, [100], None), _q(1, 2, 2, 32, [100], [0]),
                _q(0, 2, 2, 32, [100], None, ov={OV_FWD64: 4}), _q(1, 2, 2, 32, [100], None, ov={OV_BWD64_WIDE: -2})):
        assert _lib.lib().acai_attn_plan(ctypes.byref(bad), out, ctypes.byref(n), None) != 0

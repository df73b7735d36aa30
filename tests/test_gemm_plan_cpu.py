"""The GEMM selection rule (csrc/gemm_plan.h) through acai_gemm_plan: a pure host function, called here without a GPU.

TABLE holds the plan of the shapes the source comments and the GPU tests name.  Its expected values were recorded from the selection code
as it stood before the rule became a function of its own (that code compiled verbatim into a host program whose launches were logged), so
a row that changes means the selection changed: retuning a threshold shows here, and in the GPU tests that assert the kernel they name."""
import ctypes
import random

import pytest

from acai_omr_amd import _lib
from acai_omr_amd._lib import (GEMM_K_REG as K_REG, GEMM_K_GLDS as K_GLDS, GEMM_K_GLDS3 as K_GLDS3, GEMM_K_PERS as K_PERS, GEMM_K_256 as K_256,
                               GEMM_K_PERS256 as K_PERS256, GEMM_K_PP as K_PP, GEMM_K_TN_GLDS as K_TN_GLDS, GEMM_K_TN_RING as K_TN_RING,
                               GEMM_K_TN_PP as K_TN_PP)

F32, BF16 = _lib.ACAI_F32, _lib.ACAI_BF16
FIELDS = ("kernel", "wm", "fast", "pp_mode", "grid", "block", "ksplit", "vec_epi", "row0", "rows", "k0", "k", "colsum")


def _q(es, M, N, K, epi=0, trans_a=0, trans_w=0, lda=None, ldw=None, ldc=None, out_dtype=None, flags=None, aux_mode=0, has_residual=0,
       scale_cols=0, want_colsum=0, variant=0, n_cu=256, aligned=1):
    """A query as the entry points state it: contiguous, 16-byte aligned operands; bf16 -> bf16 with the autocast rounding, fp32 -> fp32."""
    out_dtype = (BF16 if es == 2 else F32) if out_dtype is None else out_dtype
    flags = (_lib.GEMM_ROUND_BF16 if out_dtype == BF16 else 0) if flags is None else flags
    ldc = N if ldc is None else ldc
    return _lib.AcaiGemmQuery(elem_size=es, epi=epi, trans_a=trans_a, trans_w=trans_w, M=M, N=N, K=K, lda=lda or (M if trans_a else K),
                              ldw=ldw or (N if trans_w else K), ldc=ldc, ldr=ldc, ldaux=ldc, a_aligned=aligned, w_aligned=aligned, c_aligned=aligned,
                              r_aligned=aligned, aux_aligned=aligned, out_dtype=out_dtype, flags=flags, aux_mode=aux_mode, has_residual=has_residual,
                              scale_cols=scale_cols, want_colsum=want_colsum, variant=variant, n_cu=n_cu)


def _plan(q):
    out, n = (_lib.AcaiGemmLaunch * 2)(), ctypes.c_int(-1)
    _lib.check(_lib.lib().acai_gemm_plan(ctypes.byref(q), out, ctypes.byref(n)), "acai_gemm_plan")
    assert 1 <= n.value <= 2
    return [tuple(getattr(out[i], f) for f in FIELDS) for i in range(n.value)]


# (query, [launch as FIELDS, ...])
TABLE = [
    # teacher-forced stream, bf16
    (_q(2, 8208, 1024, 1024), [(K_PP, 0, 0, 1, 132, 512, 0, 1, 0, 8208, 0, 1024, 0)]),
    (_q(2, 8192, 1024, 1024), [(K_GLDS, 2, 0, 0, 512, 256, 0, 1, 0, 8192, 0, 1024, 0)]),
    (_q(2, 8208, 2048, 1024), [(K_PP, 0, 0, 1, 256, 512, 0, 1, 0, 8192, 0, 1024, 0), (K_GLDS, 2, 0, 0, 16, 256, 0, 1, 8192, 16, 0, 1024, 0)]),
    (_q(2, 8192, 2048, 1024), [(K_PP, 0, 0, 1, 256, 512, 0, 1, 0, 8192, 0, 1024, 0)]),
    (_q(2, 8208, 3072, 1024), [(K_PP, 0, 0, 1, 256, 512, 0, 1, 0, 8208, 0, 1024, 0)]),
    (_q(2, 8192, 3072, 1024), [(K_GLDS, 2, 0, 0, 1536, 256, 0, 1, 0, 8192, 0, 1024, 0)]),
    (_q(2, 8208, 4096, 1024), [(K_PP, 0, 0, 1, 256, 512, 0, 1, 0, 8192, 0, 1024, 0), (K_GLDS, 2, 0, 0, 32, 256, 0, 1, 8192, 16, 0, 1024, 0)]),
    (_q(2, 8192, 4096, 1024), [(K_PP, 0, 0, 1, 256, 512, 0, 1, 0, 8192, 0, 1024, 0)]),
    (_q(2, 8208, 1024, 4096), [(K_PP, 0, 0, 1, 132, 512, 0, 1, 0, 8208, 0, 4096, 0)]),
    (_q(2, 8192, 1024, 4096), [(K_GLDS, 2, 0, 0, 512, 256, 0, 1, 0, 8192, 0, 4096, 0)]),
    (_q(2, 8208, 2048, 4096), [(K_PP, 0, 0, 1, 256, 512, 0, 1, 0, 8192, 0, 4096, 0), (K_GLDS, 2, 0, 0, 16, 256, 0, 1, 8192, 16, 0, 4096, 0)]),
    (_q(2, 8192, 2048, 4096), [(K_PP, 0, 0, 1, 256, 512, 0, 1, 0, 8192, 0, 4096, 0)]),
    (_q(2, 8208, 3072, 4096), [(K_PP, 0, 0, 1, 256, 512, 0, 1, 0, 8208, 0, 4096, 0)]),
    (_q(2, 8192, 3072, 4096), [(K_GLDS, 2, 0, 0, 1536, 256, 0, 1, 0, 8192, 0, 4096, 0)]),
    (_q(2, 8208, 4096, 4096), [(K_PP, 0, 0, 1, 256, 512, 0, 1, 0, 8192, 0, 4096, 0), (K_GLDS, 2, 0, 0, 32, 256, 0, 1, 8192, 16, 0, 4096, 0)]),
    (_q(2, 8192, 4096, 4096), [(K_PP, 0, 0, 1, 256, 512, 0, 1, 0, 8192, 0, 4096, 0)]),
    (_q(2, 16416, 1024, 4096), [(K_PP, 0, 0, 1, 256, 512, 0, 1, 0, 16384, 0, 4096, 0), (K_GLDS, 2, 0, 0, 8, 256, 0, 1, 16384, 32, 0, 4096, 0)]),
    # MAE shapes
    (_q(2, 131072, 3072, 512), [(K_PP, 0, 0, 1, 256, 512, 0, 1, 0, 131072, 0, 512, 0)]),
    (_q(2, 32768, 768, 3072), [(K_PP, 0, 0, 1, 256, 512, 0, 1, 0, 32768, 0, 3072, 0)]),
    # the same in fp32 (a K-tile is 32 floats)
    (_q(4, 8208, 1024, 1024), [(K_GLDS, 2, 0, 0, 520, 256, 0, 1, 0, 8208, 0, 1024, 0)]),
    (_q(4, 8192, 1024, 1024), [(K_GLDS, 2, 0, 0, 512, 256, 0, 1, 0, 8192, 0, 1024, 0)]),
    (_q(4, 8208, 2048, 1024), [(K_GLDS3, 0, 0, 0, 528, 512, 0, 1, 0, 8208, 0, 1024, 0)]),
    (_q(4, 8192, 2048, 1024), [(K_GLDS3, 0, 0, 0, 512, 512, 0, 1, 0, 8192, 0, 1024, 0)]),
    (_q(4, 8208, 3072, 1024), [(K_GLDS3, 0, 0, 0, 792, 512, 0, 1, 0, 8208, 0, 1024, 0)]),
    (_q(4, 8192, 3072, 1024), [(K_GLDS3, 0, 0, 0, 768, 512, 0, 1, 0, 8192, 0, 1024, 0)]),
    (_q(4, 8208, 4096, 1024), [(K_GLDS3, 0, 0, 0, 1056, 512, 0, 1, 0, 8208, 0, 1024, 0)]),
    (_q(4, 8192, 4096, 1024), [(K_GLDS3, 0, 0, 0, 1024, 512, 0, 1, 0, 8192, 0, 1024, 0)]),
    (_q(4, 8208, 1024, 4096), [(K_GLDS, 2, 0, 0, 520, 256, 0, 1, 0, 8208, 0, 4096, 0)]),
    (_q(4, 8192, 1024, 4096), [(K_GLDS, 2, 0, 0, 512, 256, 0, 1, 0, 8192, 0, 4096, 0)]),
    (_q(4, 8208, 2048, 4096), [(K_GLDS3, 0, 0, 0, 528, 512, 0, 1, 0, 8208, 0, 4096, 0)]),
    (_q(4, 8192, 2048, 4096), [(K_GLDS3, 0, 0, 0, 512, 512, 0, 1, 0, 8192, 0, 4096, 0)]),
    (_q(4, 8208, 3072, 4096), [(K_GLDS3, 0, 0, 0, 792, 512, 0, 1, 0, 8208, 0, 4096, 0)]),
    (_q(4, 8192, 3072, 4096), [(K_GLDS3, 0, 0, 0, 768, 512, 0, 1, 0, 8192, 0, 4096, 0)]),
    (_q(4, 8208, 4096, 4096), [(K_GLDS3, 0, 0, 0, 1056, 512, 0, 1, 0, 8208, 0, 4096, 0)]),
    (_q(4, 8192, 4096, 4096), [(K_GLDS3, 0, 0, 0, 1024, 512, 0, 1, 0, 8192, 0, 4096, 0)]),
    (_q(4, 16416, 1024, 4096), [(K_GLDS3, 0, 0, 0, 520, 512, 0, 1, 0, 16416, 0, 4096, 0)]),
    # MAE shapes
    (_q(4, 131072, 3072, 512), [(K_PERS, 0, 0, 0, 256, 512, 0, 1, 0, 131072, 0, 512, 0)]),
    (_q(4, 32768, 768, 3072), [(K_GLDS3, 0, 0, 0, 768, 512, 0, 1, 0, 32768, 0, 3072, 0)]),
    # cross K/V prefill (epi 1: N = 2E, K = E), each LDS-DMA kernel pinned
    (_q(2, 1797, 256, 128, epi=1, variant=1), [(K_GLDS, 2, 0, 0, 30, 256, 0, 0, 0, 1797, 0, 128, 0)]),
    (_q(2, 1797, 256, 128, epi=1, variant=2), [(K_GLDS, 4, 0, 0, 16, 512, 0, 0, 0, 1797, 0, 128, 0)]),
    (_q(2, 1797, 256, 128, epi=1, variant=3), [(K_GLDS3, 0, 0, 0, 16, 512, 0, 0, 0, 1797, 0, 128, 0)]),
    (_q(2, 1797, 256, 128, epi=1, variant=4), [(K_PERS, 0, 0, 0, 16, 512, 0, 0, 0, 1797, 0, 128, 0)]),
    (_q(2, 1797, 256, 128, epi=1, variant=5), [(K_256, 0, 0, 0, 8, 512, 0, 0, 0, 1797, 0, 128, 0)]),
    (_q(2, 1797, 256, 128, epi=1, variant=6), [(K_256, 0, 0, 0, 8, 512, 0, 0, 0, 1797, 0, 128, 0)]),
    (_q(2, 773, 384, 192, epi=1, variant=1), [(K_GLDS, 2, 0, 0, 21, 256, 0, 0, 0, 773, 0, 192, 0)]),
    (_q(2, 773, 384, 192, epi=1, variant=2), [(K_GLDS, 4, 0, 0, 12, 512, 0, 0, 0, 773, 0, 192, 0)]),
    (_q(2, 773, 384, 192, epi=1, variant=3), [(K_GLDS3, 0, 0, 0, 12, 512, 0, 0, 0, 773, 0, 192, 0)]),
    (_q(2, 773, 384, 192, epi=1, variant=4), [(K_PERS, 0, 0, 0, 12, 512, 0, 0, 0, 773, 0, 192, 0)]),
    (_q(2, 773, 384, 192, epi=1, variant=5), [(K_256, 0, 0, 0, 8, 512, 0, 0, 0, 773, 0, 192, 0)]),
    (_q(2, 773, 384, 192, epi=1, variant=6), [(K_256, 0, 0, 0, 8, 512, 0, 0, 0, 773, 0, 192, 0)]),
    (_q(2, 517, 640, 320, epi=1, variant=1), [(K_GLDS, 2, 0, 0, 25, 256, 0, 0, 0, 517, 0, 320, 0)]),
    (_q(2, 517, 640, 320, epi=1, variant=2), [(K_GLDS, 4, 0, 0, 15, 512, 0, 0, 0, 517, 0, 320, 0)]),
    (_q(2, 517, 640, 320, epi=1, variant=3), [(K_GLDS3, 0, 0, 0, 15, 512, 0, 0, 0, 517, 0, 320, 0)]),
    (_q(2, 517, 640, 320, epi=1, variant=4), [(K_PERS, 0, 0, 0, 15, 512, 0, 0, 0, 517, 0, 320, 0)]),
    (_q(2, 517, 640, 320, epi=1, variant=5), [(K_256, 0, 0, 0, 9, 512, 0, 0, 0, 517, 0, 320, 0)]),
    (_q(2, 517, 640, 320, epi=1, variant=6), [(K_256, 0, 0, 0, 9, 512, 0, 0, 0, 517, 0, 320, 0)]),
    (_q(2, 16400, 1024, 512, epi=1), [(K_PERS, 0, 0, 0, 256, 512, 0, 0, 0, 16400, 0, 512, 0)]),
    (_q(4, 1797, 256, 128, epi=1, variant=1), [(K_GLDS, 2, 0, 0, 30, 256, 0, 0, 0, 1797, 0, 128, 0)]),
    (_q(4, 1797, 256, 128, epi=1, variant=2), [(K_GLDS, 4, 0, 0, 16, 512, 0, 0, 0, 1797, 0, 128, 0)]),
    (_q(4, 1797, 256, 128, epi=1, variant=3), [(K_GLDS3, 0, 0, 0, 16, 512, 0, 0, 0, 1797, 0, 128, 0)]),
    (_q(4, 1797, 256, 128, epi=1, variant=4), [(K_PERS, 0, 0, 0, 16, 512, 0, 0, 0, 1797, 0, 128, 0)]),
    (_q(4, 1797, 256, 128, epi=1, variant=5), [(K_256, 0, 0, 0, 8, 512, 0, 0, 0, 1797, 0, 128, 0)]),
    (_q(4, 1797, 256, 128, epi=1, variant=6), [(K_256, 0, 0, 0, 8, 512, 0, 0, 0, 1797, 0, 128, 0)]),
    (_q(4, 773, 384, 192, epi=1, variant=1), [(K_GLDS, 2, 0, 0, 21, 256, 0, 0, 0, 773, 0, 192, 0)]),
    (_q(4, 773, 384, 192, epi=1, variant=2), [(K_GLDS, 4, 0, 0, 12, 512, 0, 0, 0, 773, 0, 192, 0)]),
    (_q(4, 773, 384, 192, epi=1, variant=3), [(K_GLDS3, 0, 0, 0, 12, 512, 0, 0, 0, 773, 0, 192, 0)]),
    (_q(4, 773, 384, 192, epi=1, variant=4), [(K_PERS, 0, 0, 0, 12, 512, 0, 0, 0, 773, 0, 192, 0)]),
    (_q(4, 773, 384, 192, epi=1, variant=5), [(K_256, 0, 0, 0, 8, 512, 0, 0, 0, 773, 0, 192, 0)]),
    (_q(4, 773, 384, 192, epi=1, variant=6), [(K_256, 0, 0, 0, 8, 512, 0, 0, 0, 773, 0, 192, 0)]),
    (_q(4, 517, 640, 320, epi=1, variant=1), [(K_GLDS, 2, 0, 0, 25, 256, 0, 0, 0, 517, 0, 320, 0)]),
    (_q(4, 517, 640, 320, epi=1, variant=2), [(K_GLDS, 4, 0, 0, 15, 512, 0, 0, 0, 517, 0, 320, 0)]),
    (_q(4, 517, 640, 320, epi=1, variant=3), [(K_GLDS3, 0, 0, 0, 15, 512, 0, 0, 0, 517, 0, 320, 0)]),
    (_q(4, 517, 640, 320, epi=1, variant=4), [(K_PERS, 0, 0, 0, 15, 512, 0, 0, 0, 517, 0, 320, 0)]),
    (_q(4, 517, 640, 320, epi=1, variant=5), [(K_256, 0, 0, 0, 9, 512, 0, 0, 0, 517, 0, 320, 0)]),
    (_q(4, 517, 640, 320, epi=1, variant=6), [(K_256, 0, 0, 0, 9, 512, 0, 0, 0, 517, 0, 320, 0)]),
    # weight gradients (dW = dY^T X: M x N from K tokens), bf16
    (_q(2, 136, 264, 4096, trans_a=1, trans_w=1, out_dtype=F32), [(K_TN_RING, 0, 0, 0, 24, 512, 8, 1, 0, 136, 0, 4096, 0)]),
    # ... and in fp32
    (_q(4, 136, 264, 4096, trans_a=1, trans_w=1, out_dtype=F32), [(K_REG, 0, 1, 0, 192, 256, 32, 1, 0, 136, 0, 4096, 0)]),
    (_q(2, 768, 2304, 8256, trans_a=1, trans_w=1, out_dtype=F32), [(K_TN_RING, 0, 0, 0, 216, 512, 4, 1, 0, 768, 0, 8256, 0)]),
    (_q(2, 512, 8, 640, trans_a=1, trans_w=1, out_dtype=F32), [(K_TN_GLDS, 0, 0, 0, 8, 256, 2, 1, 0, 512, 0, 640, 0)]),
    (_q(2, 40, 1000, 192, trans_a=1, trans_w=1, out_dtype=F32), [(K_TN_GLDS, 0, 0, 0, 8, 256, 1, 1, 0, 40, 0, 192, 0)]),
    (_q(2, 1024, 1024, 8208, trans_a=1, trans_w=1, out_dtype=F32), [(K_TN_RING, 0, 0, 0, 256, 512, 8, 1, 0, 1024, 0, 8208, 0)]),
    (_q(2, 264, 136, 100, trans_a=1, trans_w=1, out_dtype=F32), [(K_TN_GLDS, 0, 0, 0, 6, 256, 1, 1, 0, 264, 0, 64, 0), (K_REG, 0, 1, 0, 6, 256, 1, 1, 0, 264, 64, 36, 0)]),
    # ... and in fp32
    (_q(4, 264, 136, 100, trans_a=1, trans_w=1, out_dtype=F32), [(K_REG, 0, 1, 0, 6, 256, 1, 1, 0, 264, 0, 100, 0)]),
    (_q(2, 3072, 512, 16384, trans_a=1, trans_w=1, out_dtype=F32), [(K_TN_PP, 0, 0, 0, 240, 512, 10, 1, 0, 3072, 0, 16384, 0)]),
    (_q(2, 520, 264, 8232, trans_a=1, trans_w=1, out_dtype=F32), [(K_TN_RING, 0, 0, 0, 144, 512, 16, 1, 0, 520, 0, 8232, 0)]),
    (_q(2, 768, 2304, 4096, trans_a=1, trans_w=1, out_dtype=F32), [(K_TN_RING, 0, 0, 0, 216, 512, 4, 1, 0, 768, 0, 4096, 0)]),
    (_q(2, 512, 512, 32768, trans_a=1, trans_w=1, out_dtype=F32), [(K_TN_RING, 0, 0, 0, 256, 512, 32, 1, 0, 512, 0, 32768, 0)]),
    (_q(2, 4096, 1024, 8208, trans_a=1, trans_w=1, out_dtype=F32), [(K_TN_PP, 0, 0, 0, 256, 512, 4, 1, 0, 4096, 0, 8208, 0)]),
    (_q(2, 1024, 4096, 8271, trans_a=1, trans_w=1, out_dtype=F32), [(K_TN_PP, 0, 0, 0, 256, 512, 4, 1, 0, 1024, 0, 8271, 0)]),
    (_q(2, 2048, 1024, 1025, trans_a=1, trans_w=1, out_dtype=F32), [(K_TN_RING, 0, 0, 0, 128, 512, 2, 1, 0, 2048, 0, 1025, 0)]),
    # pinned variants on a test shape: 6, 7, 8 (the plain epilogue has no deferred form), and 7 in fp32, which has neither ring
    (_q(2, 8232, 2072, 192, variant=6), [(K_PERS256, 0, 0, 0, 256, 512, 0, 1, 0, 8232, 0, 192, 0)]),
    (_q(2, 8232, 2072, 192, variant=7), [(K_PP, 0, 0, 1, 256, 512, 0, 1, 0, 8232, 0, 192, 0)]),
    (_q(2, 8232, 2072, 192, variant=8), [(K_PP, 0, 0, 1, 256, 512, 0, 1, 0, 8232, 0, 192, 0)]),
    (_q(4, 8232, 2072, 96, variant=7), [(K_256, 0, 0, 0, 297, 512, 0, 1, 0, 8232, 0, 96, 0)]),
    # small, and an unaligned leading dimension
    (_q(2, 37, 19, 10), [(K_REG, 0, 0, 0, 1, 256, 0, 0, 0, 37, 0, 10, 0)]),
    (_q(4, 37, 19, 10), [(K_REG, 0, 0, 0, 1, 256, 0, 0, 0, 37, 0, 10, 0)]),
    (_q(2, 8208, 1024, 1024, lda=1027), [(K_REG, 0, 0, 0, 520, 256, 0, 1, 0, 8208, 0, 1024, 0)]),
    # teacher-forced stream, bf16 at a second CU count
    (_q(2, 8208, 1024, 1024, n_cu=64), [(K_PP, 0, 0, 1, 64, 512, 0, 1, 0, 8192, 0, 1024, 0), (K_GLDS, 2, 0, 0, 8, 256, 0, 1, 8192, 16, 0, 1024, 0)]),
    (_q(2, 8192, 1024, 1024, n_cu=64), [(K_PP, 0, 0, 1, 64, 512, 0, 1, 0, 8192, 0, 1024, 0)]),
    (_q(2, 8208, 2048, 1024, n_cu=64), [(K_PP, 0, 0, 1, 64, 512, 0, 1, 0, 8192, 0, 1024, 0), (K_GLDS, 2, 0, 0, 16, 256, 0, 1, 8192, 16, 0, 1024, 0)]),
    (_q(2, 8192, 2048, 1024, n_cu=64), [(K_PP, 0, 0, 1, 64, 512, 0, 1, 0, 8192, 0, 1024, 0)]),
    (_q(2, 8208, 3072, 1024, n_cu=64), [(K_PP, 0, 0, 1, 64, 512, 0, 1, 0, 8192, 0, 1024, 0), (K_GLDS, 2, 0, 0, 24, 256, 0, 1, 8192, 16, 0, 1024, 0)]),
    (_q(2, 8192, 3072, 1024, n_cu=64), [(K_PP, 0, 0, 1, 64, 512, 0, 1, 0, 8192, 0, 1024, 0)]),
    (_q(2, 8208, 4096, 1024, n_cu=64), [(K_PP, 0, 0, 1, 64, 512, 0, 1, 0, 8192, 0, 1024, 0), (K_GLDS, 2, 0, 0, 32, 256, 0, 1, 8192, 16, 0, 1024, 0)]),
    (_q(2, 8192, 4096, 1024, n_cu=64), [(K_PP, 0, 0, 1, 64, 512, 0, 1, 0, 8192, 0, 1024, 0)]),
    (_q(2, 8208, 1024, 4096, n_cu=64), [(K_PP, 0, 0, 1, 64, 512, 0, 1, 0, 8192, 0, 4096, 0), (K_GLDS, 2, 0, 0, 8, 256, 0, 1, 8192, 16, 0, 4096, 0)]),
    (_q(2, 8192, 1024, 4096, n_cu=64), [(K_PP, 0, 0, 1, 64, 512, 0, 1, 0, 8192, 0, 4096, 0)]),
    (_q(2, 8208, 2048, 4096, n_cu=64), [(K_PP, 0, 0, 1, 64, 512, 0, 1, 0, 8192, 0, 4096, 0), (K_GLDS, 2, 0, 0, 16, 256, 0, 1, 8192, 16, 0, 4096, 0)]),
    (_q(2, 8192, 2048, 4096, n_cu=64), [(K_PP, 0, 0, 1, 64, 512, 0, 1, 0, 8192, 0, 4096, 0)]),
    (_q(2, 8208, 3072, 4096, n_cu=64), [(K_PP, 0, 0, 1, 64, 512, 0, 1, 0, 8192, 0, 4096, 0), (K_GLDS, 2, 0, 0, 24, 256, 0, 1, 8192, 16, 0, 4096, 0)]),
    (_q(2, 8192, 3072, 4096, n_cu=64), [(K_PP, 0, 0, 1, 64, 512, 0, 1, 0, 8192, 0, 4096, 0)]),
    (_q(2, 8208, 4096, 4096, n_cu=64), [(K_PP, 0, 0, 1, 64, 512, 0, 1, 0, 8192, 0, 4096, 0), (K_GLDS, 2, 0, 0, 32, 256, 0, 1, 8192, 16, 0, 4096, 0)]),
    (_q(2, 8192, 4096, 4096, n_cu=64), [(K_PP, 0, 0, 1, 64, 512, 0, 1, 0, 8192, 0, 4096, 0)]),
    (_q(2, 16416, 1024, 4096, n_cu=64), [(K_PP, 0, 0, 1, 64, 512, 0, 1, 0, 16384, 0, 4096, 0), (K_GLDS, 2, 0, 0, 8, 256, 0, 1, 16384, 32, 0, 4096, 0)]),
]


@pytest.mark.parametrize("i", range(len(TABLE)))
def test_plan_of_named_shape(i):
    q, want = TABLE[i]
    assert _plan(q) == want


def test_table_reaches_every_kernel():
    assert {l[0] for _, want in TABLE for l in want} == set(range(len(_lib.GEMM_KERNEL_NAMES)))


PP_FORMS = {1, 1 | 32, 1 | 2 | 4, 1 | 8, 0, 16, 1 | 2 | 128, 1 | 256}   # what pp_mode_ok accepts (gemm_plan.h), as GEMM_PP_* bits
# a pinned variant and the kernels its documented fall-back chain may end in (7 -> 6 -> 5; 4 / 5 / 6 / 7 -> 1 under 8 tiles); wm rides along
CHAIN = {1: {(K_GLDS, 2)}, 2: {(K_GLDS, 4)}, 3: {(K_GLDS3, 0)}, 4: {(K_PERS, 0), (K_GLDS, 2)}, 5: {(K_256, 0), (K_GLDS, 2)},
         6: {(K_PERS256, 0), (K_256, 0), (K_GLDS, 2)}, 7: {(K_PP, 0), (K_PERS256, 0), (K_256, 0), (K_GLDS, 2)}}
CHAIN[8] = CHAIN[7]
MODES = [  # out_dtype, flags, aux_mode, has_residual, scale_cols: the eight ping-pong forms, then three it has no instantiation for
    (BF16, 2, 0, 0, 0), (BF16, 2, 0, 0, 8), (BF16, 3, 1, 0, 0), (BF16, 2, 2, 0, 0), (F32, 0, 0, 0, 0), (F32, 2, 0, 1, 0), (BF16, 3, 3, 0, 0),
    (BF16, 2, 4, 0, 0), (BF16, 3, 0, 0, 0), (BF16, 2, 0, 1, 0), (F32, 1, 0, 1, 0)]


def _draw(rng):
    es = rng.choice((2, 4))
    dim = lambda: rng.choice((rng.randint(1, 300), 64 * rng.randint(1, 80), 64 * rng.randint(1, 80) + rng.choice((1, 8, 16, 40)),
                              256 * rng.randint(16, 600) + rng.choice((0, 5, 16, 32, 33))))
    M, N, K = dim(), min(dim(), 8192), min(dim(), 16384)
    kind = rng.choice(("nt", "nt", "nt", "dw", "trans", "epi1"))
    kw = dict(variant=rng.choice((0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8)), n_cu=rng.choice((256, 304, 64, 8)), aligned=rng.choice((1, 1, 1, 0)))
    pad = rng.choice((0, 0, 8, 3))
    if kind == "dw":
        M = min(M, 8192)
        kw.update(trans_a=1, trans_w=1, out_dtype=F32, lda=M + pad, ldw=N + pad, ldc=N + pad, want_colsum=rng.choice((0, 1)))
    elif kind == "trans":
        ta = rng.choice((0, 1))
        kw.update(trans_a=ta, trans_w=1 - ta, out_dtype=F32, lda=(M if ta else K) + pad, ldw=(K if ta else N) + pad, ldc=N + pad)
    elif kind == "epi1":
        kw.update(epi=1, lda=K + pad, ldw=K + pad)
    else:
        od, fl, am, res, sc = rng.choice(MODES)
        kw.update(out_dtype=od, flags=fl, aux_mode=am, has_residual=res, scale_cols=min(sc, N), lda=K + pad, ldw=K + pad, ldc=N + pad)
    return kind, _q(es, M, N, K, **kw)


def test_plan_properties_over_drawn_queries():
    rng = random.Random(20240607)
    seen = set()
    for _ in range(4000):
        kind, q = _draw(rng)
        plan = [dict(zip(FIELDS, l)) for l in _plan(q)]
        what = (kind, [(f, getattr(q, f)) for f, _ in q._fields_], plan)
        if kind == "dw":   # split-K weight gradient: every launch takes all output rows, the launches' token ranges tile [0, K)
            assert all(l["row0"] == 0 and l["rows"] == q.M for l in plan), what
            pos = 0
            for l in plan:
                assert l["k0"] == pos and l["k"] >= 1, what
                pos += l["k"]
            assert pos == q.K, what
            assert all(l["ksplit"] >= 1 for l in plan), what
            assert sum(l["colsum"] for l in plan) <= q.want_colsum and all(l["kernel"] == K_TN_PP for l in plan if l["colsum"]), what
        else:              # every launch takes the whole reduction, the launches' row ranges tile [0, M)
            pos = 0
            for l in plan:
                assert l["row0"] == pos and l["rows"] >= 1 and l["k0"] == 0 and l["k"] == q.K and l["ksplit"] == 0 and not l["colsum"], what
                pos += l["rows"]
            assert pos == q.M, what
        for l in plan:
            seen.add(l["kernel"])
            assert l["grid"] >= 1 and l["block"] in (256, 512), what
            persistent = l["kernel"] in (K_PERS, K_PERS256, K_PP)
            assert not persistent or l["grid"] <= q.n_cu, what
            if l["kernel"] == K_PP:
                assert (l["pp_mode"] & ~_lib.GEMM_PP_DEFER) in PP_FORMS and q.elem_size == 2 and q.epi == 0 and l["vec_epi"], what
                assert not (l["pp_mode"] & _lib.GEMM_PP_DEFER) or q.variant == 8, what
            else:
                assert l["pp_mode"] == 0, what
            if l["kernel"] in (K_PERS256, K_TN_GLDS, K_TN_RING, K_TN_PP):
                assert q.elem_size == 2 and q.epi == 0, what
            assert (l["kernel"] in (K_TN_GLDS, K_TN_RING, K_TN_PP)) <= (kind == "dw"), what
        if q.variant and kind != "dw":
            assert len(plan) == 1, what   # the remainder-row split belongs to the auto rule
            l = plan[0]
            if l["kernel"] != K_REG:      # (the register-staged kernel: operands the LDS-DMA kernels cannot take)
                assert (l["kernel"], l["wm"]) in CHAIN[q.variant], what
                t256 = -(-q.M // 256) * -(-q.N // 256)
                t4 = -(-q.M // 256) * -(-q.N // 128)
                if q.variant >= 4:
                    small = t4 < 8 if q.variant == 4 else t256 < 8
                    assert ((l["kernel"], l["wm"]) == (K_GLDS, 2)) == small, what
    assert seen == set(range(len(_lib.GEMM_KERNEL_NAMES)))   # the draw reaches every kernel


def test_plan_refuses_a_malformed_query():
    out, n = (_lib.AcaiGemmLaunch * 2)(), ctypes.c_int(0)
    for bad in (_q(3, 8, 8, 8), _q(2, 0, 8, 8), _q(2, 8, 8, 8, n_cu=0), _q(2, 8, 8, 8, variant=9), _q(2, 8, 8, 8, epi=1, trans_w=1)):
        assert _lib.lib().acai_gemm_plan(ctypes.byref(bad), out, ctypes.byref(n)) != 0

"""Half the activation bytes for the decode step's out / cross-out GEMVs: decode_attn_kernel stores its (bf16-valued) output rows as bf16 and
the GEMV takes skinny_chain_kernel<true, 0, 4>, the bf16-activation chain form at K = 1024.

  * The form through skinny_gemm_ex: bit-identical to the fp32-activation form on the same bf16-valued rows, and inside the float64 bars of
    tests/test_gpu_decode_forms.py.
  * The whole step (2-layer full-width decoder, greedy from the 8-step graph, one beam run, one slot run): ids, log-probs and last logits
    identical with ACAI_ATTN_BF16 on and off.

The switch is read once per process, so both sides of the on / off comparison come from fresh child processes (this file run as a script,
once per side).  The float64 checks run in the test process, which must have the switch at its default."""
import math
import os
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("ACAI_ATTN_BF16",)
BS = [1, 3, 8, 9, 16, 17]                      # a partial tile, the second build pass (> 8 rows), a second batch tile (> 16)
STEP_LENS = {200: [200, 131, 64, 177, 200, 96, 150, 8], 1100: [1100, 300, 1025, 64, 700, 1100, 513, 1024],
             2300: [2300, 200, 1100, 2049, 64, 1500, 2300, 1024]}   # ragged memories: one split; two; three splits at chunk 1024


# ---------------------------------------------------------------------------------------------------------------------------------------
# what both child processes compute (every tensor deterministic from seeds; results on the CPU)

def _step_models(dev):
    from decode_support import _decoder, _vit
    return _vit(_decoder(16, seed=5, scale=16.0), 16, torch.bfloat16, dev)


def _mem(lens, seed, dev):
    return torch.randn(sum(lens), 1024, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).to(dev)


def _compute(dev):
    out = {}
    m = _step_models(dev)
    eng = m.decoder.decoder_blocks.engine
    with torch.no_grad():
        for B in (1, 3, 8):
            for top, lens in STEP_LENS.items():
                lens = lens[:B]
                seqs, lps, mask = m._greedy_packed(None, _mem(lens, top + B, dev), lens, 13)   # 12 steps: the 8-step graph, then single steps
                e = eng(dev)
                assert e.cross_chunk == 1024 and e.cross_nsplit == -(-max(lens) // 1024)
                out[f"greedy_B{B}_S{top}"] = (seqs.cpu(), lps.cpu(), mask.cpu(), e.ws["logits"][:B].float().cpu().clone())
        lens = [1100, 200, 2300]
        out["beam"] = tuple(t.cpu() for t in m._beam_packed(None, _mem(lens, 77, dev), lens, 4, 9, 1.0))
        lens = [2300, 200, 1100, 64, 1500]
        out["slot"] = tuple(t.cpu() for t in m._continuous_packed(None, _mem(lens, 78, dev), lens, [9, 6, 12, 4, 8], 3))
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from acai_omr_amd import _lib
    _lib.lib()
    torch.save(_compute(torch.device("cuda:0")), sys.argv[1])
    sys.exit(0)


# ---------------------------------------------------------------------------------------------------------------------------------------
from decode_support import dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sides(dev):
    """(switches on, switches off): _compute() in two fresh child processes, started together."""
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for name, val in (("on", None), ("off", "0")):
            env = dict(os.environ)
            for s in SWITCHES:
                env.pop(s, None)
                if val is not None:
                    env[s] = val
            env["ACAI_CROSS_CHUNK"] = "1024"
            path = os.path.join(tmp, name + ".pt")
            procs.append((path, subprocess.Popen([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                                                 stderr=subprocess.STDOUT, text=True)))
        res = []
        for path, p in procs:
            log, _ = p.communicate(timeout=600)
            assert p.returncode == 0, log[-3000:]
            res.append(torch.load(path, weights_only=False))
    return res


def _defaults():
    assert all(os.environ.get(s) is None for s in SWITCHES), "the in-process checks are of the default forms: unset " + ", ".join(SWITCHES)


def _bitwise(on, off, keys):
    for k in keys:
        assert len(on[k]) == len(off[k]), k
        for i, (a, b) in enumerate(zip(on[k], off[k])):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (k, i, float((a.double() - b.double()).abs().max()))
            assert bool(torch.isfinite(a.double()).all()), (k, i)


# ---- 1. bf16 activations at K = 1024 ---------------------------------------------------------------------------------------------------
def _published(dev, z, w, b):
    """(mean, rstd) of z's rows as a LayerNorm-on-load launch publishes them (K = z's width, a multiple of 256), else float64 on the host."""
    from acai_omr_amd import ops
    from test_gpu_decode_forms import ln64
    B, N = z.shape
    if N % 256 == 0:
        stats = torch.full((B, 2), float("nan"), device=dev)
        ops.skinny_gemm_ex(z.to(dev), torch.zeros(64, N, dtype=torch.bfloat16, device=dev), ln=(w.to(dev), b.to(dev)), stats_out=stats)
        torch.cuda.synchronize()
        return stats
    _, m, r = ln64(z, w, b, 1e-5)
    return torch.stack([m, r], 1).float().to(dev)


@pytest.mark.parametrize("B", BS)
def test_bf16_k1024_form_equals_fp32_form_and_float64_bars(dev, B):
    """N = 227 (a tail row block, 4 rows per workgroup), 1024 (4), 3072 (16 rows; 1600 <= N < 2560 would take 8: N = 2048 rides along);
    ldx = K + 512; without a residual, and with the LayerNorm'd residual rebuilt from published statistics."""
    _defaults()
    from acai_omr_amd import ops
    from test_gpu_decode_forms import _gemv, _rows
    K, pad = 1024, 512
    for N in (227, 1024, 2048, 3072):
        g = torch.Generator().manual_seed(5000 + 17 * B + N)
        z = _rows(B, N, "edges", g)
        w, b = 1 + 0.2 * torch.randn(N, generator=g), 0.2 * torch.randn(N, generator=g)
        rln = dict(z=z, w=w, b=b, stats=_published(dev, z, w, b))
        xb = torch.randn(B, K + pad, generator=g).to(torch.bfloat16).to(dev)
        W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).to(dev)
        bias = (0.1 * torch.randn(N, generator=g)).to(dev)
        for res in (False, True):
            kw = dict(bias=bias, round_bf16=True)
            if res:
                kw.update(residual=z.to(dev), rln=(w.to(dev), b.to(dev)), rstats=rln["stats"])
            y16 = ops.skinny_gemm_ex(xb[:, :K], W, **kw)
            y32 = ops.skinny_gemm_ex(xb.float()[:, :K], W, **kw)
            torch.cuda.synchronize()
            assert xb[:, :K].stride(0) == K + pad and torch.equal(y16, y32), (B, N, res, float((y16 - y32).abs().max()))
            r = _gemv(dev, B, N, K=K, xbf=True, rnd=True, ldx_pad=pad, res=res, rln=rln if res else None, seed=4, form="chain<true,0,4>")
            print(f"chain<true,0,4> B={B} N={N} res={res}: max|dev-R_bf| {r['err']:.3g} gap {r['gap']:.3g}")


# ---- 2. the whole step -------------------------------------------------------------------------------------------------------------------
def test_whole_step_identical_with_switches_on_and_off(sides):
    on, off = sides
    keys = [f"greedy_B{B}_S{top}" for B in (1, 3, 8) for top in STEP_LENS] + ["beam", "slot"]
    _bitwise(on, off, keys)
    # the runs decode 12 tokens per row, and a row's logits depend on its own memory
    s8, lg8 = on["greedy_B8_S2300"][0], on["greedy_B8_S2300"][3]
    assert s8.shape == (8, 13) and not torch.equal(lg8[0], lg8[1])

"""Who fetches which piece of the chain GEMVs' activation image (skinny_chain_kernel): the K = 4096 bf16 form runs four waves with four K
slices each instead of sixteen with one.  That changes no bit of any result: the image in LDS, the per-slice MFMA chains and the order of
the final sum are what they were.  torch.equal everywhere, no tolerance.

  1. Every chain form through ops.skinny_gemm_ex, in the test process (switch at its default), against
       * the same call in a child process with ACAI_SKINNY_INGEST=0 (sixteen waves), and
       * where the generic skinny_mfma_kernel does the same arithmetic (no LayerNorm on load: its row sums are a butterfly, the chain's ride
         the DPP network), the same call with the weights in a strided view whose extent the chain's 32-bit buffer offsets refuse.
     LN = 2 (the unembedding's double LayerNorm) and the KV-append form are not reachable through skinny_gemm_ex: the whole step runs both.
  2. The whole step (2-layer full-width decoder: greedy from the 8-step graph for B = 1, 3, 8, one beam run, one slot run): ids, log-probs
     and last logits identical with ACAI_SKINNY_INGEST=0 and unset.

The switch is read once per process, so each side of a comparison across it comes from a fresh child process (this file run as a script)."""
import math
import os
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "ACAI_SKINNY_INGEST"
BS = [1, 3, 8, 9, 16, 17]                       # one row; a partial tile; the > 8 rows pass; a second batch tile
NS_K1024 = [20, 227, 1024, 1100, 3072, 4096]    # one workgroup; 57; 256; 275 workgroups with a ragged last one; 16 rows per workgroup: 192 and 256
NS_K4096 = [20, 1024, 1100]
STEP_LENS = [1100, 300, 1025, 64, 700, 1100, 513, 1024]
CHAIN_LIMIT = 0xFFF00000                        # the chain kernel takes N * ldw * 2 bytes of weights below this (launch_skinny)


# ---------------------------------------------------------------------------------------------------------------------------------------
# what the test process and both child processes compute (every tensor deterministic from seeds; results on the CPU)

def _operands(N, K, dev):
    g = torch.Generator().manual_seed(1000 * K + N)
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).to(dev)
    bias = (0.1 * torch.randn(N, generator=g)).to(dev)
    rw, rb = (1 + 0.2 * torch.randn(N, generator=g)).to(dev), (0.2 * torch.randn(N, generator=g)).to(dev)
    lw, lb = (1 + 0.2 * torch.randn(K, generator=g)).to(dev), (0.2 * torch.randn(K, generator=g)).to(dev)
    return W, bias, rw, rb, lw, lb


def _forms(dev, wview=None):
    """name -> tensor for every form / shape.  wview(W): the weights as the launch gets them (identity, or the view the chain refuses); with
    a view only the forms without a LayerNorm on load are computed."""
    from acai_omr_amd import ops
    out = {}
    for K, NS in ((1024, NS_K1024), (4096, NS_K4096)):
        for N in NS:
            W, bias, rw, rb, lw, lb = _operands(N, K, dev)
            Wl = W if wview is None else wview(W)
            for B in BS:
                g = torch.Generator().manual_seed(77 * B + N + K)
                pad = 512                                                   # ldx = K + 512: a row stride that is not the row length
                xb = torch.randn(B, K + pad, generator=g).to(torch.bfloat16).to(dev)[:, :K]
                xf = (torch.randn(B, K + pad, generator=g) + 3.0 * torch.randn(B, 1, generator=g)).to(dev)[:, :K]
                z = (torch.randn(B, N, generator=g) + 2.0 * torch.randn(B, 1, generator=g)).to(dev)
                zstats = torch.stack([z.mean(1), 1 / torch.sqrt(z.var(1, unbiased=False) + 1e-5)], 1).contiguous()
                tag = f"K{K}_N{N}_B{B}"
                # bf16 activations (out / cross-out at K = 1024, lin2 at K = 4096): bare, and with the LayerNorm'd residual from statistics
                out[tag + "_bf16"] = ops.skinny_gemm_ex(xb, Wl, bias=bias, round_bf16=True)
                out[tag + "_bf16_res_rln"] = ops.skinny_gemm_ex(xb, Wl, bias=bias, round_bf16=True, residual=z, rln=(rw, rb), rstats=zstats)
                if K != 1024:
                    continue
                # fp32 activations without a LayerNorm (LN = 0), plain residual
                out[tag + "_f32_res"] = ops.skinny_gemm_ex(xf, Wl, bias=bias, residual=z)
                if wview is not None:
                    continue
                # LN = 1: published statistics (qkv / cross-q), then GELU + bf16 out (lin1)
                stats = torch.full((B, 2), float("nan"), device=dev)
                out[tag + "_ln"] = ops.skinny_gemm_ex(xf, Wl, bias=bias, round_bf16=True, ln=(lw, lb), stats_out=stats)
                out[tag + "_ln_stats"] = stats
                out[tag + "_ln_gelu_bf16"] = ops.skinny_gemm_ex(xf, Wl, bias=bias, round_bf16=True, gelu=True, out_dtype=torch.bfloat16, ln=(lw, lb))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _step(dev):
    from decode_support import _decoder, _vit
    m = _vit(_decoder(16, seed=5, scale=16.0), 16, torch.bfloat16, dev)
    mem = lambda lens, seed: torch.randn(sum(lens), 1024, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).to(dev)
    out = {}
    with torch.no_grad():
        for B in (1, 3, 8):
            lens = STEP_LENS[:B]
            seqs, lps, mask = m._greedy_packed(None, mem(lens, 40 + B), lens, 13)   # 12 steps: the 8-step graph, then single steps
            e = m.decoder.decoder_blocks.engine(dev)
            out[f"greedy_B{B}"] = (seqs.cpu(), lps.cpu(), mask.cpu(), e.ws["logits"][:B].float().cpu().clone())
        lens = [1100, 200, 2300]
        out["beam"] = tuple(t.cpu() for t in m._beam_packed(None, mem(lens, 77), lens, 4, 9, 1.0))
        lens = [2300, 200, 1100, 64, 1500]
        out["slot"] = tuple(t.cpu() for t in m._continuous_packed(None, mem(lens, 78), lens, [9, 6, 12, 4, 8], 3))
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from acai_omr_amd import _lib
    _lib.lib()
    d = torch.device("cuda:0")
    torch.save({"forms": _forms(d), "step": _step(d)}, sys.argv[1])
    sys.exit(0)


# ---------------------------------------------------------------------------------------------------------------------------------------
from decode_support import dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sides(dev):
    """(switch unset, switch = 0): forms and whole step from two fresh child processes, started together."""
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for name, val in (("new", None), ("parent", "0")):
            env = dict(os.environ)
            env.pop(SWITCH, None)
            if val is not None:
                env[SWITCH] = val
            path = os.path.join(tmp, name + ".pt")
            procs.append((path, subprocess.Popen([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                                                 stderr=subprocess.STDOUT, text=True)))
        res = []
        for path, p in procs:
            log, _ = p.communicate(timeout=600)
            assert p.returncode == 0, log[-3000:]
            res.append(torch.load(path, weights_only=False))
    return res


@pytest.fixture(scope="module")
def here(dev):
    """The forms in the test process, switch at its default."""
    assert os.environ.get(SWITCH) is None, "the in-process checks are of the default forms: unset " + SWITCH
    return _forms(dev)


@pytest.fixture(scope="module")
def generic(dev):
    """The forms without a LayerNorm on load through skinny_mfma_kernel: the weights sit in a view of one large buffer whose row stride puts
    N * ldw * 2 past what the chain kernel's buffer offsets take."""
    big = torch.empty(CHAIN_LIMIT // 2 + 9 * 4096 + 8, dtype=torch.bfloat16, device=dev)

    def wview(W):
        N, K = W.shape
        ldw = (-(-(CHAIN_LIMIT // 2) // N) + 7) & ~7
        assert N * ldw * 2 >= CHAIN_LIMIT and (N - 1) * ldw + K <= big.numel()
        v = big.as_strided((N, K), (ldw, 1))
        v.copy_(W)
        return v
    out = _forms(dev, wview)
    del big
    torch.cuda.empty_cache()
    return out


def _equal(a, b, keys):
    assert keys
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, float((a[k].double() - b[k].double()).abs().max()))
        assert bool(torch.isfinite(a[k].double()).all()), k


# ---- 1. the forms ------------------------------------------------------------------------------------------------------------------------
def test_forms_equal_the_generic_kernel(here, generic):
    """bf16 K = 1024, bf16 K = 4096 (four waves) and fp32 LN = 0, every B and N."""
    assert len(generic) == len(BS) * (3 * len(NS_K1024) + 2 * len(NS_K4096))
    _equal(here, generic, sorted(generic))


def test_forms_equal_parent_behaviour(here, sides):
    """Every form, the LayerNorm-on-load ones and their published statistics included, against the child process with sixteen waves."""
    new, parent = sides
    assert len(here) == len(BS) * (6 * len(NS_K1024) + 2 * len(NS_K4096))
    assert sorted(here) == sorted(parent["forms"]) == sorted(new["forms"])
    _equal(here, parent["forms"], sorted(here))
    _equal(here, new["forms"], sorted(here))
    # the statistics are the rows' own: every row has another mean
    st = here["K1024_N1100_B17_ln_stats"]
    assert st.shape == (17, 2) and len(set(st[:, 0].tolist())) == 17


# ---- 2. the whole step -------------------------------------------------------------------------------------------------------------------
def test_whole_step_identical_with_the_switch_at_0_and_unset(sides):
    new, parent = sides
    keys = ["greedy_B1", "greedy_B3", "greedy_B8", "beam", "slot"]
    for k in keys:
        assert len(new["step"][k]) == len(parent["step"][k]), k
        for i, (a, b) in enumerate(zip(new["step"][k], parent["step"][k])):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (k, i, float((a.double() - b.double()).abs().max()))
            assert bool(torch.isfinite(a.double()).all()), (k, i)
    s8, lg8 = new["step"]["greedy_B8"][0], new["step"]["greedy_B8"][3]
    assert s8.shape == (8, 13) and not torch.equal(lg8[0], lg8[1])

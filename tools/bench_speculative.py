"""Speculative greedy decoding against plain greedy decoding on ONE image (the interactive case), bf16, bench.py's random-init weights, in
one process with the variants interleaved round by round.  Every variant is timed as a user runs it - DecodeEngine.greedy /
DecodeEngine.speculative from arming to the last poll, graphs captured beforehand - with a host clock around work that ends in a device
synchronise; the cross-K/V prefill is outside the window.

Per image size (default 256x1024 and 512x2048) and per draft length D:
  * the verify step's time (a run whose drafts are all wrong takes exactly max_len - 1 steps) against the greedy step's, and their ratio -
    the tokens per step at which speculative decoding breaks even;
  * tokens/s and mean tokens per step with `drafts` tables built from the greedy output with 0 / 25 / 50 / 75 / 100 % of the entries changed;
  * the same with the n-gram drafter on what these weights emit.  RANDOM-INIT WEIGHTS: that acceptance says nothing about a trained
    checkpoint on real scores.
Every speculative output is compared with the greedy output (torch.equal on tokens and log-probs) before it is timed.  Also reports the
n-gram drafter's tokens per step on the golden fixtures (toy weights).  One JSON line on stdout, the same written to --out.

  python tools/bench_speculative.py --rounds 5 --tokens 256 --out bench_outputs/speculative_bench.json
"""
import argparse
import json
import os
import sys
import time

import torch
from torch.amp import autocast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DS = (1, 2, 4, 7)
SHARES = (0, 25, 50, 75, 100)


def memory(vitomr, img):
    with torch.no_grad():
        lat32, _, lens = vitomr.encoder.forward_packed([img])
        with autocast(device_type="cuda", dtype=torch.bfloat16):
            return vitomr.transition_head.forward_packed(lat32), lens


def corrupt(greedy_row, share, V, seed):
    """The greedy tokens as a drafts table with exactly share % of the entries (index >= 1) changed."""
    tab = greedy_row.clone()
    n = tab.numel() - 1
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:round(n * share / 100)] + 1
    tab[idx.to(tab.device)] = (tab[idx.to(tab.device)] + 1) % V
    return tab.unsqueeze(0)


def stats(xs):
    s = sorted(xs)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


def bench_size(vitomr, dev, height, width, T, rounds):
    blocks = vitomr.decoder.decoder_blocks
    eng = blocks.engine(dev)
    V = vitomr.decoder.vocab_size
    img = torch.rand(1, height, width, generator=torch.Generator().manual_seed(1000)).to(dev)
    mem, lens = memory(vitomr, img)

    def run(D, drafts):
        """-> seconds, tokens written after <bos>, steps, (seqs, lps)"""
        blocks.prepare_caches_packed(None, mem, lens, group_size=D + 1, per_row_cross=D > 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            if D == 0:
                seqs, lps, steps = eng.greedy(T)
            else:
                seqs, lps, st = eng.speculative(T, D, drafts=drafts)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        seqs, lps = seqs.clone(), lps.clone()
        if D > 0:
            steps = int(st[0])
        mask = vitomr.create_inference_mask(seqs)
        return dt, int(mask.sum()) - 1, steps, (seqs.masked_fill(~mask, 0), lps.masked_fill(~mask, 0.0))

    _, n_tok, _, g = run(0, None)   # cold: code objects, graph capture
    variants = [("greedy", 0, None)]
    for D in DS:
        for sh in SHARES:
            variants.append((f"D{D}_changed{sh}", D, corrupt(g[0][0], sh, V, 17 * D + sh)))
        variants.append((f"D{D}_ngram", D, None))
    for name, D, drafts in variants[1:]:   # cold runs double as the equality check
        _, n, _, s = run(D, drafts)
        assert n == n_tok and torch.equal(s[0], g[0]) and torch.equal(s[1], g[1]), f"{name}: speculative output differs from greedy"
    times = {name: [] for name, _, _ in variants}
    steps_of = {}
    for _ in range(rounds):
        for name, D, drafts in variants:
            dt, n, steps, _ = run(D, drafts)
            times[name].append(dt)
            steps_of[name] = steps if D > 0 else n   # greedy: one token per step (its loop overshoots to the next poll)
    res = dict(patches=lens[0], tokens=n_tok, cross_chunk=eng.cross_chunk, cross_nsplit=eng.cross_nsplit, equal_to_greedy=True)
    gs = stats([n_tok / t for t in times["greedy"]])
    g_step_ms = stats([t / n_tok * 1e3 for t in times["greedy"]])
    res["greedy"] = dict(tokens_per_s=gs, ms_per_token=g_step_ms)
    for D in DS:
        r = {}
        full = f"D{D}_changed100"
        step_ms = stats([t / steps_of[full] * 1e3 for t in times[full]])
        r["verify_step_ms"] = step_ms
        r["step_cost_ratio"] = step_ms["median"] / g_step_ms["median"]   # = tokens per step at break-even
        for name in [f"D{D}_changed{sh}" for sh in SHARES] + [f"D{D}_ngram"]:
            tps = stats([n_tok / t for t in times[name]])
            r[name.split("_", 1)[1]] = dict(steps=steps_of[name], tokens_per_step=n_tok / steps_of[name], tokens_per_s=tps,
                                            speedup_vs_greedy=tps["median"] / gs["median"])
        res[f"D{D}"] = r
    return res


def fixtures_ngram(dev):
    """Tokens per step of the n-gram drafter (D = 4, ngram = 3) on the golden fixtures' toy decoders, up to their cache length."""
    from acai_omr_amd.models.models import FineTuneOMREncoder, OMRDecoder, TeacherForcedViTOMR
    out = {}
    for name in ("vitomr_small", "vitomr_dh64", "vitomr_dh64b", "vitomr_odd"):
        fx = torch.load(os.path.join(ROOT, "tests", "golden", name + ".pt"), map_location="cpu", weights_only=False)
        cfg = fx["cfg"]
        enc = FineTuneOMREncoder(cfg["P"], cfg["pe_h"], cfg["pe_w"], cfg["ft_depth"], num_layers=cfg["enc_layers"], hidden_dim=cfg["enc_dim"],
                                 num_heads=cfg["enc_heads"], mlp_dim=cfg["enc_mlp"])
        dec = OMRDecoder(cfg["max_len"], os.path.join(ROOT, "lmx_vocab.txt"), num_layers=cfg["dec_layers"], hidden_dim=cfg["dec_dim"],
                         num_heads=cfg["dec_heads"], mlp_dim=cfg["dec_mlp"])
        m = TeacherForcedViTOMR(enc, None, dec, transition_head_dim=cfg["head_dim"])
        m.load_state_dict(fx["state_dict"])
        c = m.decoder.to_cached_version(16, torch.bfloat16)
        c.load_state_dict(m.decoder.state_dict())
        m.decoder = c
        m = m.to(dev).eval()
        with torch.no_grad():
            lat, mask = m.encoder(fx["imgs"])
            with autocast(device_type="cuda", dtype=torch.bfloat16):
                mem = m.transition_head(lat)
                s = m.cached_speculative_generate(mem, mask, max_len=cfg["max_len"], draft_len=4, ngram=3)
        steps = m.decoder.decoder_blocks.engine(dev).spec_steps[:len(fx["imgs"])].tolist()
        toks = (s[2].sum(dim=1) - 1).tolist()
        out[name] = dict(tokens=toks, steps=steps, tokens_per_step=[t / st for t, st in zip(toks, steps)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256x1024,512x2048")
    ap.add_argument("--tokens", type=int, default=256, help="tokens decoded per run (max_len - 1)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    from acai_omr_amd.inference.vitomr_inference import set_up_omr_inference
    torch.manual_seed(0)   # bench.py's weights
    vitomr, _ = set_up_omr_inference(os.path.join(ROOT, "lmx_vocab.txt"), max_batch_size=8, cache_dtype=torch.bfloat16, device="cuda")
    vitomr = vitomr.eval()
    res = {}
    for size in a.sizes.split(","):
        h, w = (int(x) for x in size.split("x"))
        res[size] = bench_size(vitomr, dev, h, w, a.tokens + 1, a.rounds)
    out = dict(workload="one image, bf16, random-init weights (bench.py's): DecodeEngine.greedy against DecodeEngine.speculative, arming to last "
                        "poll, graphs captured beforehand; changedNN = drafts table = greedy output with NN % of the entries changed",
               note="n-gram acceptance is what random-init / toy weights emit; it says nothing about trained checkpoints on real scores",
               tokens_per_run=a.tokens, rounds=a.rounds, device=torch.cuda.get_device_name(dev), sizes=res, fixtures_ngram_D4=fixtures_ngram(dev))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

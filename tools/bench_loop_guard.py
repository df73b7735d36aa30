"""The loop guard, measured.  All of it in ONE process, the variants of a part alternated.

(a) The guarded greedy step against the unguarded one: bench.py's decode (8 images of 512x2048, bf16, random-init full-size model), 256
    steps.  The unguarded step is the parent commit's code - adding the LOOP feature left the existing instantiations of
    greedy_select_kernel instruction for instruction what they were - so both run from this library, alternated:
    `repeats` rounds of (greedy, guarded), each figure the median of 3 runs of `steps` steps (host clock from the call to
    DecodeEngine.greedy to its return, ending in a device synchronise).  The guard is one that cannot fire (min_tokens above the row), so
    both decode the same `steps` steps.  Reported: every repeat, the medians, the unguarded step's own repeat-to-repeat spread and the
    difference against it.
(c) A continuous-batching run of 64 images (the 8 benchmark images, 8 times) with caps spread over 100 .. 768 through 16 slots, with and
    without a guard (R = 3, M = 8, P = 64): decode steps, wall time (host clock around the whole call, median of 3 alternated runs) and
    the share of rows the guard stopped.  These are RANDOM weights: the share says nothing about trained checkpoints.
(d) acai_repeat_scan on 128 x 768 tokens against a torch restatement (unfold plus comparisons for the 64 periods), device events around
    windows of launches, median of 5 windows; the two are checked against each other first.
((b), bench.py's headline on this commit against the parent's, is two runs of bench.py itself.)

One JSON line on stdout, the same written to --out.

  python tools/bench_loop_guard.py --out profiles/loop_guard_bench.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def build(a):
    import torch
    from acai_omr_amd.inference.vitomr_inference import set_up_omr_inference
    torch.manual_seed(0)   # bench.py's weights
    vitomr, _ = set_up_omr_inference(os.path.join(ROOT, "lmx_vocab.txt"), max_batch_size=max(a.batch, a.slots), cache_dtype=torch.bfloat16, device="cuda")
    g = torch.Generator().manual_seed(1000)   # bench.py's rank-0 images
    imgs = [torch.rand(1, a.height, a.width, generator=g).to("cuda:0") for _ in range(a.batch)]
    return vitomr.eval(), imgs


def bench_step(a, vitomr, imgs):
    import torch
    from torch.amp import autocast
    from acai_omr_amd.loops import LoopGuard
    blocks = vitomr.decoder.decoder_blocks
    with torch.no_grad():
        lat32, _, lens = vitomr.encoder.forward_packed(imgs)
        with autocast(device_type="cuda", dtype=torch.bfloat16):
            mem = vitomr.transition_head.forward_packed(lat32)
        blocks.prepare_caches_packed(None, mem, lens)
    eng = blocks.engine(torch.device("cuda:0"))
    T = a.steps + 1
    variants = {"greedy": {}, "guarded": {"loop_guard": LoopGuard(2, T + 1)}}
    reps = {k: [] for k in variants}
    with torch.no_grad():
        for kw in variants.values():       # cold: code objects, graph capture
            eng.greedy(T, poll=T, **kw)
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for name, kw in variants.items():
                runs = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    _, _, done = eng.greedy(T, poll=T, **kw)
                    torch.cuda.synchronize()
                    runs.append((time.perf_counter() - t0) * 1e3)
                    assert done == a.steps
                reps[name].append(median(runs) / a.steps)
    out = {k: dict(ms_per_step=v, median=median(v), min=min(v), max=max(v)) for k, v in reps.items()}
    gm = out["greedy"]["median"]
    out.update(workload=f"{a.batch} images of {a.height}x{a.width}, bf16, {a.steps} greedy steps from replayed graphs, bench.py's random-init weights",
               repeats=a.repeats, greedy_spread_pct=(out["greedy"]["max"] - out["greedy"]["min"]) / gm * 100,
               guarded_vs_greedy_pct=(out["guarded"]["median"] / gm - 1) * 100)
    return out


def bench_continuous(a, vitomr, imgs):
    import torch
    from acai_omr_amd.inference.vitomr_inference import _encode_chunks
    from acai_omr_amd.loops import LoopGuard
    N = a.images
    caps = [100 + (i * 668) // (N - 1) for i in range(N)]
    caps = [caps[(i * 37) % N] for i in range(N)]   # spread over the queue, not sorted
    guard = LoopGuard(min_repeats=3, min_tokens=8, max_period=64)
    eng = vitomr.decoder.decoder_blocks.engine(torch.device("cuda:0"))
    res = {"plain": dict(ms=[]), "guarded": dict(ms=[])}
    with torch.no_grad():
        mem, lens = _encode_chunks(vitomr, [imgs[i % len(imgs)] for i in range(N)], "cuda")
        for rnd in range(4):   # round 0 is cold
            for name, kw in (("plain", {}), ("guarded", {"loop_guard": guard})):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = vitomr._continuous_packed(None, mem, lens, caps, a.slots, **kw)
                torch.cuda.synchronize()
                if rnd:
                    res[name]["ms"].append((time.perf_counter() - t0) * 1e3)
                res[name].update(steps=eng.slot_steps, tokens=int(got[2].sum()))
                if kw:
                    res[name].update(rows_stopped=int(got[3].looped.sum()), share_stopped=float(got[3].looped.float().mean()),
                                     periods=sorted(set(got[3].period.tolist()) - {0}))
    for v in res.values():
        v["ms_median"] = median(v["ms"])
    return dict(images=N, slots=a.slots, caps="100 .. 768", guard="R=3 M=8 P=64", note="random weights: the share of rows stopped says nothing "
                "about trained checkpoints", **res)


def torch_scan(tok, P, R, M):
    """(stop, period) by unfold plus comparisons: for every period the windows of need(p) equalities that all hold; 0, 0 where none."""
    import torch
    N, T = tok.shape
    best = torch.full((N,), T, dtype=torch.int64, device=tok.device)
    per = torch.zeros(N, dtype=torch.int64, device=tok.device)
    for p in range(P, 0, -1):   # descending: on a tie the smaller period overwrites
        need = max((R - 1) * p, M)
        if 1 + p + need > T:
            continue
        eq = tok[:, 1 + p:] == tok[:, 1:T - p]                  # eq[:, j]: index i = 1 + p + j against i - p >= 1
        hit = eq.unfold(1, need, 1).all(dim=-1)                 # window starting at j ends at index p + j + need
        first = torch.where(hit.any(dim=1), hit.int().argmax(dim=1) + p + need, torch.full_like(best, T))
        take = first <= best
        best, per = torch.where(take, first, best), torch.where(take, torch.full_like(per, p), per)
    none = best == T
    return torch.where(none, torch.zeros_like(best), best), torch.where(none, torch.zeros_like(per), per)


def bench_scan(N=128, T=768, P=64, R=3, M=8):
    import torch
    from acai_omr_amd import ops
    g = torch.Generator().manual_seed(5)
    tok = torch.randint(3, 6, (N, T), generator=g)
    tok[:, 0] = 0
    tok = tok.to("cuda:0")
    stop, period, _, _ = ops.repeat_scan(tok, P, R, M)
    ws, wp = torch_scan(tok, P, R, M)
    assert torch.equal(stop.long(), ws) and torch.equal(period.long(), wp), "the kernel and the torch restatement disagree"
    out = {}
    for name, fn, n in (("acai_repeat_scan", lambda: ops.repeat_scan(tok, P, R, M), 50), ("torch_unfold", lambda: torch_scan(tok, P, R, M), 5)):
        win = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            win.append(e0.elapsed_time(e1) / n * 1e3)
        out[name] = dict(us_per_call=median(win), us_min=min(win), us_max=max(win))
    return dict(rows=N, tokens_per_row=T, params=f"P={P} R={R} M={M}", rows_fired=int((period > 0).sum()),
                note="device events around windows of calls (the kernel's call includes its output allocation), median of 5 windows", **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    vitomr, imgs = build(a)
    out = dict(device=torch.cuda.get_device_name(0), scan=bench_scan(), step=bench_step(a, vitomr, imgs), continuous=bench_continuous(a, vitomr, imgs))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

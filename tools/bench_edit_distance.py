"""Time the token edit distance op (acai_edit_distance) from a replayed hipGraph on the two workloads that matter:
  grpo   R = 128 rollouts of random length <= 768 in groups of 8 against targets of 300-700 tokens (one GRPO minibatch's reward term);
  worst  R = 32 pairs of 1536 x 1536 unrelated random tokens (MAX_LMX_SEQ_LEN on both sides: nothing matches, no row is short).
Seeded inputs; the results are checked against the CPU reference of the tests (tests/edit_distance_reference.py), whose wall time on the same
pairs is reported for context, as is the launch's share of the recorded GRPO update epoch (profiles/grpo_bench_mi355x.json).  Writes one JSON
line to profiles/edit_distance_bench.json and prints it.

    python tools/bench_edit_distance.py [--launches 50] [--reps 5] [--out profiles/edit_distance_bench.json]
"""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def workload(name, rng):
    if name == "grpo":
        R, group, vocab = 128, 8, 227
        pred_len = rng.integers(1, 769, size=R)
        tgt_len = rng.integers(300, 701, size=R // group)
    else:
        R, group, vocab = 32, 1, 227
        pred_len = np.full(R, 1536)
        tgt_len = np.full(R, 1536)
    pred = rng.integers(0, vocab, size=(R, int(pred_len.max())))
    tgt = rng.integers(0, vocab, size=(R // group, int(tgt_len.max())))
    return pred, pred_len, tgt, tgt_len, group


def bench(name, launches, reps, rng):
    from acai_omr_amd import ops
    from edit_distance_reference import edit_distances
    pred, pred_len, tgt, tgt_len, group = workload(name, rng)
    R = pred.shape[0]
    cells = int(sum(int(pred_len[r]) * int(tgt_len[r // group]) for r in range(R)))
    t0 = time.perf_counter()
    want = edit_distances(pred, pred_len, tgt, tgt_len, group)
    cpu_s = time.perf_counter() - t0
    dev = "cuda"
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(tgt).to(dev)
    pl, tl = torch.from_numpy(pred_len).int().to(dev), torch.from_numpy(tgt_len).int().to(dev)
    out = torch.empty(R, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    times = []
    with torch.cuda.stream(s):
        ops.edit_distance(p, pl, t, tl, group=group, out=out)
        s.synchronize()
        assert out.cpu().tolist() == want, f"{name}: the device distances differ from the CPU reference"
        g = ops.Graph()
        g.begin()
        try:
            for _ in range(launches):
                ops.edit_distance(p, pl, t, tl, group=group, out=out)
        finally:
            g.end()
        g.launch()
        s.synchronize()
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.launch()
            e1.record()
            s.synchronize()
            times.append(e0.elapsed_time(e1) / launches * 1e3)
        assert out.cpu().tolist() == want
    us = float(np.median(times))
    return {"pairs": R, "group": group, "pred_len_max": int(pred_len.max()), "tgt_len_max": int(tgt_len.max()), "cells": cells,
            "us_per_launch": round(us, 2), "us_per_launch_min_max": [round(min(times), 2), round(max(times), 2)],
            "cell_updates_per_s": round(cells / (us * 1e-6), 0), "cpu_reference_ms": round(cpu_s * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50, help="launches per captured graph")
    ap.add_argument("--reps", type=int, default=5, help="timed graph replays (the median is reported)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_distance_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_edit_distance.py needs a GPU: a CPU run says nothing about the kernel")
    rng = np.random.default_rng(0)
    epoch_ms = json.load(open(os.path.join(ROOT, "profiles", "grpo_bench_mi355x.json")))["epoch_ms_grouped"]
    res = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], "date": datetime.date.today().isoformat(), "timing": f"hipGraph of {a.launches} launches, device events, median of {a.reps} replays",
           "grpo": bench("grpo", a.launches, a.reps, rng), "worst": bench("worst", a.launches, a.reps, rng), "update_epoch_ms": epoch_ms}
    res["grpo"]["share_of_update_epoch"] = round(res["grpo"]["us_per_launch"] * 1e-3 / epoch_ms, 6)
    res["worst"]["share_of_update_epoch"] = round(res["worst"]["us_per_launch"] * 1e-3 / epoch_ms, 6)
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

"""Time the edit alignment op (acai_edit_align) from a replayed hipGraph against the distance op (acai_edit_distance) on the same inputs, on
tools/bench_edit_distance.py's two workloads and seeds:
  grpo   R = 128 rollouts of random length <= 768 in groups of 8 against targets of 300-700 tokens;
  worst  R = 32 pairs of 1536 x 1536 unrelated random tokens.
Both ops are checked against the CPU references of the tests before anything is timed (tests/edit_alignment_reference.py, whose wall time on
the same pairs is reported, and tests/edit_distance_reference.py).  The two graphs are replayed ALTERNATELY in one process: one warm-up replay
each, then `reps` timed pairs of replays; the median and the min / max of the replays are reported, and the ratio of the medians.  With
--inference the script also times diagnosed_inference against confident_inference(uncertainty="error") on the 8 x 512x2048 shape of the other
extension benches (tools/bench_confidence.py's workload: random weights, 512 tokens per image; the targets are random rows of 452-513 tokens).  Writes one JSON line to
profiles/edit_alignment_bench.json and prints it.

    python tools/bench_edit_alignment.py [--launches 20] [--reps 7] [--inference] [--out profiles/edit_alignment_bench.json]
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

from bench_edit_distance import workload  # noqa: E402  (the same workloads, drawn from the same seed in the same order)


def _graph(ops, stream, launches, fn):
    g = ops.Graph()
    g.begin()
    try:
        for _ in range(launches):
            fn()
    finally:
        g.end()
    g.launch()   # warm-up replay
    stream.synchronize()
    return g


def _timed(stream, g, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.launch()
    e1.record()
    stream.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3


def bench(name, launches, reps, rng):
    from acai_omr_amd import ops
    from edit_alignment_reference import edit_alignments
    from edit_distance_reference import edit_distances
    pred, pred_len, tgt, tgt_len, group = workload(name, rng)
    R = pred.shape[0]
    cells = int(sum(int(pred_len[r]) * int(tgt_len[r // group]) for r in range(R)))
    t0 = time.perf_counter()
    want = edit_alignments(pred, pred_len, tgt, tgt_len, group)
    cpu_s = time.perf_counter() - t0
    want_dist = edit_distances(pred, pred_len, tgt, tgt_len, group)
    dev = "cuda"
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(tgt).to(dev)
    pl, tl = torch.from_numpy(pred_len).int().to(dev), torch.from_numpy(tgt_len).int().to(dev)
    dist = torch.empty(R, dtype=torch.int32, device=dev)
    ws_bytes = ops.edit_alignment_workspace_bytes(p.shape[1], t.shape[1], R)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()
    t_align, t_dist = [], []

    def same():
        return all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(out, want)) and dist.cpu().tolist() == want_dist

    with torch.cuda.stream(s):
        out = ops.edit_alignment(p, pl, t, tl, group=group, workspace=ws)
        ops.edit_distance(p, pl, t, tl, group=group, out=dist)
        s.synchronize()
        assert same(), f"{name}: the device results differ from the CPU references"
        g_align = _graph(ops, s, launches, lambda: ops.edit_alignment(p, pl, t, tl, group=group, out=out, workspace=ws))
        g_dist = _graph(ops, s, launches, lambda: ops.edit_distance(p, pl, t, tl, group=group, out=dist))
        for _ in range(reps):
            t_align.append(_timed(s, g_align, launches))
            t_dist.append(_timed(s, g_dist, launches))
        assert same()
    a, d = float(np.median(t_align)), float(np.median(t_dist))
    return {"pairs": R, "group": group, "pred_len_max": int(pred_len.max()), "tgt_len_max": int(tgt_len.max()), "cells": cells,
            "align_us_per_launch": round(a, 2), "align_us_min_max": [round(min(t_align), 2), round(max(t_align), 2)],
            "distance_us_per_launch": round(d, 2), "distance_us_min_max": [round(min(t_dist), 2), round(max(t_dist), 2)],
            "align_over_distance": round(a / d, 3), "align_cell_updates_per_s": round(cells / (a * 1e-6), 0),
            "workspace_bytes": ws_bytes, "direction_bytes_written": int(sum(
                (min(int(pred_len[r]), int(tgt_len[r // group])) * _dir_words(max(int(pred_len[r]), int(tgt_len[r // group]))) * 256) for r in range(R))),
            "cpu_reference_ms": round(cpu_s * 1e3, 1)}


def _dir_words(m):
    """Direction words a lane stores per DP row for a longer row of m tokens (csrc/seqalign.hip: align_strip_width / align_dir_words)."""
    w = (m + 63) // 64
    W = next(x for x in (1, 2, 4, 8, 12, 16, 24, 32, 48, 64) if w <= x)
    return (2 * W + 31) // 32


def bench_inference(reps, tokens=512):
    """diagnosed_inference against confident_inference(uncertainty="error") on 8 images of 512 x 2048 decoded to `tokens` tokens each (<eos>
    suppressed, bench.py's weights: tools/bench_confidence.py's workload), alternated; wall time around a device synchronise, in ms: the median
    and min / max of `reps` runs after one warm-up each.  The step that diagnosed_inference adds - the alignment launch and the weight
    tensor built from it (ViTOMR._error_weights) - is also timed alone on the decoded rows."""
    from acai_omr_amd.inference.vitomr_inference import confident_inference, diagnosed_inference, set_up_omr_inference
    torch.manual_seed(0)
    vitomr, _ = set_up_omr_inference(os.path.join(ROOT, "lmx_vocab.txt"), max_batch_size=8, cache_dtype=torch.bfloat16, device="cuda")
    vitomr = vitomr.eval()
    with torch.no_grad():
        vitomr.decoder.unembed.bias[vitomr.decoder.eos_idx] = -1e4   # <eos> suppressed: every row runs to the cap
    g = torch.Generator().manual_seed(1000)
    imgs = [torch.rand(1, 512, 2048, generator=g).to("cuda") for _ in range(8)]
    V = vitomr.decoder.vocab_size
    targets = [torch.randint(3, V, (int(n),), generator=g) for n in torch.randint(tokens - 60, tokens + 2, (8,), generator=g)]

    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    conf = lambda: confident_inference(vitomr, imgs, "cuda", max_inference_len=tokens + 1, uncertainty="error")   # noqa: E731
    diag = lambda: diagnosed_inference(vitomr, imgs, targets, "cuda", max_inference_len=tokens + 1)               # noqa: E731
    run(conf), run(diag)
    tc, td = [], []
    for _ in range(reps):
        tc.append(run(conf)[0])
        ms, out = run(diag)
        td.append(ms)
    seqs, mask = out[0], out[2]
    step = lambda: vitomr._error_weights(seqs, mask, targets, None)   # noqa: E731
    run(step)
    ts = [run(step)[0] for _ in range(max(reps, 5))]
    c, d = float(np.median(tc)), float(np.median(td))
    return {"images": 8, "image": [512, 2048], "decoded_lens": mask.sum(-1).tolist(), "target_lens": [int(t.shape[0]) for t in targets],
            "confident_error_ms": round(c, 2), "confident_error_ms_min_max": [round(min(tc), 2), round(max(tc), 2)],
            "diagnosed_ms": round(d, 2), "diagnosed_ms_min_max": [round(min(td), 2), round(max(td), 2)], "diagnosed_minus_confident_ms": round(d - c, 2),
            "align_and_weights_ms": round(float(np.median(ts)), 3), "align_and_weights_ms_min_max": [round(min(ts), 3), round(max(ts), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20, help="launches per captured graph")
    ap.add_argument("--reps", type=int, default=7, help="timed replays of each graph, alternated (the median is reported)")
    ap.add_argument("--inference", action="store_true", help="also time diagnosed_inference against confident_inference")
    ap.add_argument("--inference-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_alignment_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_edit_alignment.py needs a GPU: a CPU run says nothing about the kernel")
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0],
           "date": datetime.date.today().isoformat(),
           "timing": f"hipGraphs of {a.launches} launches, device events, the two ops alternated, median of {a.reps} replays after one warm-up replay",
           "grpo": bench("grpo", a.launches, a.reps, rng), "worst": bench("worst", a.launches, a.reps, rng)}
    if a.inference:
        res["inference"] = bench_inference(a.inference_reps)
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

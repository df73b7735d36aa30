"""Streamed continuous batching against the silent path it rides on, on one MI355X, in one process, warmed (random-init weights and
synthetic pages: bench.build_model with <eos> suppressed, so every row runs to its cap).  It measures
  (a) continuous_inference over --images images of 512 x 2048 with per-image caps spread over --cap-lo .. --cap-hi, --slots slots, polled
      at its default: the parent commit's path, which streaming leaves unchanged;
  (b) streamed_continuous_inference on the same inputs at each --flush interval, consuming every event - alternated with (a), one call
      of each per round, --repeats rounds after a warm-up of every path;
  first_step   the time from the call to the first STEP event (the encode is inside it) at each interval;
  flush_launch ops.slot_flush alone, back to back, on the engine's own slot state as the run left it: host clock around --calls calls
               that end in a synchronise, --reps windows.  Its KERNEL time comes from a trace of its own:
                   rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_stream.py --flush-only
  page         streamed_page_inference against page_inference on tools/bench_page.py's A4 page (ten systems, --page-len tokens each).
The bar, written with the result: at flush interval 16, median (b) - median (a) may not exceed (a)'s own max - min in this run plus
(polls of the streamed run) x (median flush_launch).  Writes one JSON line to profiles/stream_bench.json and prints it.  Needs a GPU.

    python tools/bench_stream.py [--images 64] [--slots 16] [--cap-lo 100] [--cap-hi 768] [--flush 16 25] [--repeats 5] [--flush-only]
"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stat(xs, unit="ms"):
    return {f"median_{unit}": statistics.median(xs), f"min_{unit}": min(xs), f"max_{unit}": max(xs), "n": len(xs)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def flush_windows(eng, S, F, calls, reps):
    """ops.slot_flush over the engine's slot state as the last run left it, back to back: microseconds per call, one value per window.
    Every window starts with the marks at 1, so its first calls move F entries per slot, as a poll does, and the later ones find nothing
    new (a poll moves at most slots x F x 8 bytes: the launch is what is measured either way)."""
    from acai_omr_amd import ops
    eng._flush_setup(S, F)
    eng._flush_ld = 0
    out = []
    for _ in range(reps + 1):
        eng.slot_mark.fill_(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            ops.slot_flush(eng.seqs, eng.logprobs, eng.slot_t, eng.finished, eng.slot_mark, S, F, eng._flush_dev)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / calls * 1e6)
    return out[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--cap-lo", type=int, default=100)
    ap.add_argument("--cap-hi", type=int, default=768)
    ap.add_argument("--flush", type=int, nargs="+", default=[16, 25])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--page-len", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--flush-only", action="store_true", help="one short streamed run, then the flush windows alone (the run to trace)")
    ap.add_argument("--no-page", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream: needs a GPU (a CPU run says nothing about these paths)")
    import bench
    from acai_omr_amd.config import InferenceEvent
    from acai_omr_amd.inference.vitomr_inference import (continuous_inference, page_inference, streamed_continuous_inference,
                                                         streamed_page_inference)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(a.seed)
    n_img = 4 if a.flush_only else a.images
    caps = torch.linspace(a.cap_lo, a.cap_hi, n_img).round().int()[torch.randperm(n_img, generator=g)].tolist()   # spread evenly, order shuffled
    imgs = [torch.rand(1, 512, 2048, generator=g) for _ in range(n_img)]
    vit = bench.build_model(dev, a.slots)
    bench._suppress_eos(vit)
    eng = vit.decoder.decoder_blocks.engine(dev)
    STEP = InferenceEvent.STEP.value

    def silent():
        return continuous_inference(vit, imgs, "cuda", max_inference_len=caps, slots=a.slots)

    def streamed(F):
        def run():
            first, n_steps, t0 = None, 0, time.perf_counter()
            for ev in streamed_continuous_inference(vit, imgs, "cuda", max_inference_len=caps, slots=a.slots, flush_interval=F):
                if ev["type"] == STEP:
                    n_steps += 1
                    if first is None:
                        first = (time.perf_counter() - t0) * 1e3
            return first, n_steps
        return run

    res = {"when": datetime.datetime.now().isoformat(timespec="seconds"), "device": torch.cuda.get_device_name(0),
           "weights": "random init, <eos> suppressed", "images": n_img, "image": [512, 2048], "slots": a.slots,
           "caps": {"lo": a.cap_lo, "hi": a.cap_hi, "tokens": sum(c - 1 for c in caps)}}
    if a.flush_only:
        streamed(a.flush[0])()
        res["flush_launch"] = {str(F): stat(flush_windows(eng, a.slots, F, a.calls, a.reps), "us") for F in a.flush}
        print(json.dumps(res))
        return
    want = silent()
    t_a, t_b, first, polls, events = [], {F: [] for F in a.flush}, {F: [] for F in a.flush}, {}, {}
    for F in a.flush:   # warm-up of every path, and the streamed rows against the silent ones
        rows = {}
        for ev in streamed_continuous_inference(vit, imgs, "cuda", max_inference_len=caps, slots=a.slots, flush_interval=F):
            if ev["type"] == InferenceEvent.INFERENCE_FINISH.value:
                rows[ev["payload"]["image"]] = ev["payload"]["sequence"]
        assert all(torch.equal(rows[i][0], want[0][i, :rows[i].shape[1]]) for i in range(n_img)), "streamed rows differ from continuous_inference's"
        polls[F] = eng.slot_polls
    for _ in range(a.repeats):   # alternated: one call of each path per round
        t_a.append(timed(silent)[0])
        polls["silent"] = eng.slot_polls
        for F in a.flush:
            ms, (f, n_steps) = timed(streamed(F))
            t_b[F].append(ms)
            first[F].append(f)
            events[F] = n_steps
    res["continuous_inference"] = {**stat(t_a), "polls": polls["silent"]}
    res["streamed_continuous_inference"] = {str(F): {**stat(t_b[F]), "polls": polls[F], "step_events": events[F],
                                                     "first_step": stat(first[F])} for F in a.flush}
    res["flush_launch"] = {str(F): stat(flush_windows(eng, a.slots, F, a.calls, a.reps), "us") for F in a.flush}
    F = 16 if 16 in a.flush else a.flush[0]
    excess = statistics.median(t_b[F]) - statistics.median(t_a)
    allowed = (max(t_a) - min(t_a)) + polls[F] * res["flush_launch"][str(F)]["median_us"] / 1e3
    res["bar"] = {"flush_interval": F, "streamed_minus_silent_ms": excess, "allowed_ms": allowed, "holds": bool(excess <= allowed),
                  "allowed_is": "max - min of continuous_inference in this run + polls x median flush launch alone"}
    if not a.no_page:
        import bench_page
        from acai_omr_amd.config import PE_MAX_HEIGHT, PE_MAX_WIDTH
        from acai_omr_amd.page import DetectConfig
        from acai_omr_amd.utils import DynamicResize
        resize = DynamicResize(16, bench_page.MAX_IMG_SEQ_LEN, PE_MAX_HEIGHT, PE_MAX_WIDTH, False)
        page = torch.from_numpy(bench_page.a4_page()[0]).to(dev)
        cfg = DetectConfig()
        kw = dict(boxes=None, max_inference_len=a.page_len, slots=a.slots, detect=cfg)

        def whole():
            return page_inference(vit, page, "cuda", resize, **kw)

        def whole_streamed():
            first, t0, last = None, time.perf_counter(), None
            for ev in streamed_page_inference(vit, page, "cuda", resize, flush_interval=F, **kw):
                if first is None and ev["type"] == STEP:
                    first = (time.perf_counter() - t0) * 1e3
                last = ev
            return first, last["payload"]["result"]

        r, (_, s) = whole(), whole_streamed()
        assert torch.equal(r.seqs, s.seqs) and torch.equal(r.log_probs, s.log_probs) and r.boxes == s.boxes
        t_p, t_s, f_s = [], [], []
        for _ in range(a.repeats):
            t_p.append(timed(whole)[0])
            ms, (f, _) = timed(whole_streamed)
            t_s.append(ms)
            f_s.append(f)
        res["page"] = {"page": [bench_page.H, bench_page.W], "systems": len(r), "max_len": a.page_len, "flush_interval": F,
                       "page_inference": stat(t_p), "streamed_page_inference": {**stat(t_s), "first_step": stat(f_s)}}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Microseconds per launch of decode_attn_kernel<bf16, 8, RAGGED> at the two ends of what a greedy step asks of decode attention:

  stream   the headline cross attention: 8 sequences x 16 heads x 4096 keys of d_h 64 (134 MB of K/V per launch), chunk 1024, the four
           splits merged inside the launch; 12 K/V sets are cycled so that every launch streams from HBM (12 x 134 MB >> Infinity Cache)
  chain    the same kernel with nothing to stream: 16 keys per (sequence, head), one split, the workgroup writes the output itself.  What
           is left is the launch's dependent chain - argument fetch, length, q, one key group, wave merge, LDS, store - which is all the
           self-attention launch of an early step consists of (that form has no entry of its own in the C ABI).

48 launches back to back, captured once into a graph and replayed (a Python loop cannot issue a 2 us kernel every 2 us), HIP events
around the replay, best and median of `--repeats` replays.  A/B: run it once per library (ACAI_OMR_LIB=path/to/other/libacai_omr_hip.so).

    python tools/bench_dattn_latency.py [--launches 48] [--repeats 20]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(B, H, dh, n_keys, sets, dev):
    g = torch.Generator(device="cpu").manual_seed(7)
    q = torch.randn(B, H * dh, generator=g).to(dev) * 2
    total = B * H * n_keys * dh
    kv = [(torch.randn(total, device=dev).to(torch.bfloat16), torch.randn(total, device=dev).to(torch.bfloat16)) for _ in range(sets)]
    off = torch.arange(B, dtype=torch.int64, device=dev) * (H * n_keys * dh)
    ln = torch.full((B,), n_keys, dtype=torch.int32, device=dev)
    return q, kv, off, ln


def time_form(name, n_keys, chunk, sets, launches, repeats, dev):
    from acai_omr_amd import _lib, ops
    L = _lib.lib()
    B, H, dh = 8, 16, 64
    q, kv, off, ln = build(B, H, dh, n_keys, sets, dev)
    nsplit = max(1, -(-n_keys // chunk))
    partial = torch.empty(B * H * nsplit * (dh + 2), dtype=torch.float32, device=dev)
    out = torch.empty(B, H * dh, dtype=torch.float32, device=dev)
    tickets = torch.zeros(B * H, dtype=torch.int32, device=dev)

    def launch(i):
        k, v = kv[i % sets]
        _lib.check(L.acai_decode_attn(q.data_ptr(), q.stride(0), k.data_ptr(), v.data_ptr(), off.data_ptr(), ln.data_ptr(), partial.data_ptr(),
                                      out.data_ptr(), out.stride(0), B, H, dh, dh, chunk, nsplit, _lib.ACAI_BF16, 1, tickets.data_ptr(), ops._st()),
                   "acai_decode_attn")

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for i in range(sets):
            launch(i)
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            for i in range(launches):
                launch(i)
        graph.replay()
        s.synchronize()
        times = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            graph.replay()
            e1.record(s)
            s.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / launches)
    assert bool(torch.isfinite(out).all()) and int(tickets.abs().sum()) == 0
    return dict(form=name, keys=n_keys, chunk=chunk, nsplit=nsplit, us_per_launch_best=min(times), us_per_launch_median=statistics.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dattn_latency: needs a GPU")
    dev = torch.device("cuda:0")
    from acai_omr_amd import _lib
    res = [time_form("stream", 4096, 1024, 12, a.launches, a.repeats, dev), time_form("chain", 16, 1024, 1, a.launches, a.repeats, dev)]
    print(json.dumps(dict(library=_lib.LIB_PATH, launches=a.launches, repeats=a.repeats, forms=res)))


if __name__ == "__main__":
    main()

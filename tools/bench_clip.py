"""Clipping by the global gradient norm inside the fused AdamW step, measured.

The full-size ViTOMR training model of bench.py's teacher-forced leg (random init, fp32 master weights), a random fp32 gradient on every
parameter, one FusedAdamW over all of them.  In ONE process, alternating, each call timed with device events on the launch stream:

  (a) the parent commit's path: torch.nn.utils.clip_grad_norm_(params, max_norm=1.0), then optimizer.step()
  (b) optimizer.step(max_grad_norm=1.0): sums, norm, clipped step
  (c) optimizer.step() alone

All three are warmed first.  A repeat is the mean of `--calls` consecutive calls between two events (host work of a call - the tables, the
ATen dispatch - is inside, as it is in a training step); reported are the median and the range over `--repeats` repeats.  The acceptance
condition is that (b)'s median is not above (a)'s by more than (a)'s own range in the same run.  The kernels alone (tables already on the
device, back-to-back launches between two events): acai_grad_norm (both launches), acai_adamw_step_clipped, acai_adamw_step.

One JSON line on stdout, the same written to --out.  `--write-readme FILE.json` (no GPU needed) puts the figures of such a file into
README.md and DESIGN.md section 6, between the bench_clip markers.

  python tools/bench_clip.py --out profiles/clip_bench.json
  python tools/bench_clip.py --write-readme profiles/clip_bench.json
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEGIN, END = "<!-- bench_clip:begin -->", "<!-- bench_clip:end -->"


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def stats(xs):
    return dict(us=xs, median=median(xs), min=min(xs), max=max(xs))


def measure(a):
    import torch
    sys.path.insert(0, ROOT)
    from acai_omr_amd import _lib, ops
    from acai_omr_amd.config import ENCODER_FINE_TUNE_DEPTH, MAX_LMX_SEQ_LEN, NUM_DECODER_LAYERS, PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH
    from acai_omr_amd.models.models import FineTuneOMREncoder, OMRDecoder, ScheduledSamplingViTOMR
    from acai_omr_amd.optim import CHUNK, FusedAdamW
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = FineTuneOMREncoder(PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH, ENCODER_FINE_TUNE_DEPTH, transformer_dropout=0.0)
    dec = OMRDecoder(MAX_LMX_SEQ_LEN, os.path.join(ROOT, "lmx_vocab.txt"), num_layers=NUM_DECODER_LAYERS, transformer_dropout=0.0)
    model = ScheduledSamplingViTOMR(enc, None, dec, transition_head_dropout=0.0).to(dev).train()
    params = [p for p in model.parameters() if p.dtype == torch.float32]
    g = torch.Generator(device=dev).manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, device=dev, dtype=torch.float32)
    n_elems = sum(p.numel() for p in params)
    opt = FusedAdamW(params, lr=1e-6, betas=(0.9, 0.95), weight_decay=0.05)

    def path_a():
        torch.nn.utils.clip_grad_norm_(params, max_norm=1.0)
        opt.step()

    variants = (("a_torch_clip_then_step", path_a), ("b_step_max_grad_norm", lambda: opt.step(max_grad_norm=1.0)), ("c_step_alone", lambda: opt.step()))
    for _ in range(a.warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(a.repeats):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.calls * 1e3)
    paths = {name: stats(v) for name, v in times.items()}
    pa, pb = paths["a_torch_clip_then_step"], paths["b_step_max_grad_norm"]
    spread = pa["max"] - pa["min"]

    # the kernels alone, on the tables of one step
    active = opt._active()
    tdev, ctd, cod, n_chunks = opt._build(active, dev, [float(st["step"]) for _, _, st in active])
    garr = (_lib.AcaiAdamWGroup * 1)()
    garr[0].lr, garr[0].beta1, garr[0].beta2, garr[0].eps, garr[0].weight_decay = 1e-6, 0.9, 0.95, 1e-8, 0.05
    gdev = ops.h2d(torch.frombuffer(bytearray(bytes(garr)), dtype=torch.uint8), dev)
    c0d, work = opt._layout[4], torch.empty(n_chunks, dtype=torch.float64, device=dev)
    result = torch.empty(_lib.GRAD_NORM_WORDS, dtype=torch.float32, device=dev)
    norms = torch.empty(len(active), dtype=torch.float32, device=dev)
    skipped = torch.zeros((), dtype=torch.int32, device=dev)
    L, st = _lib.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    launches = (
        ("acai_grad_norm", lambda: L.acai_grad_norm(tdev.data_ptr(), ctd.data_ptr(), cod.data_ptr(), c0d.data_ptr(), len(active), n_chunks, CHUNK, 1.0, 1.0,
                                                    work.data_ptr(), norms.data_ptr(), result.data_ptr(), st)),
        ("acai_adamw_step_clipped", lambda: L.acai_adamw_step_clipped(tdev.data_ptr(), gdev.data_ptr(), ctd.data_ptr(), cod.data_ptr(), n_chunks, CHUNK, 1.0,
                                                                      result.data_ptr(), 1, skipped.data_ptr(), st)),
        ("acai_adamw_step", lambda: L.acai_adamw_step(tdev.data_ptr(), gdev.data_ptr(), ctd.data_ptr(), cod.data_ptr(), n_chunks, CHUNK, 1.0, st)))
    kern = {name: [] for name, _ in launches}
    for _ in range(a.repeats):
        for name, fn in launches:
            assert fn() == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            kern[name].append(e0.elapsed_time(e1) / a.calls * 1e3)
    kernels = {name: stats(v) for name, v in kern.items()}
    gn = kernels["acai_grad_norm"]["median"]
    return dict(device=torch.cuda.get_device_name(0), tensors=len(params), parameters=n_elems, chunks=n_chunks, repeats=a.repeats, calls_per_repeat=a.calls,
                warmup=a.warmup, paths=paths, b_minus_a_us=pb["median"] - pa["median"], a_range_us=spread, b_within_a_range=pb["median"] - pa["median"] <= spread,
                b_minus_c_us=pb["median"] - paths["c_step_alone"]["median"], kernels=kernels, grad_norm_gb_per_s=4.0 * n_elems / (gn * 1e-6) / 1e9,
                skipped_steps=int(opt.skipped_steps), grad_norm=float(opt.grad_norm),
                note="device events around `calls_per_repeat` consecutive calls, microseconds per call; paths include their host work, kernels do not")


def render(res, indent=""):
    def f(v):
        return f"{v['median']:.0f} us ({v['min']:.0f} .. {v['max']:.0f})"
    P, K = res["paths"], res["kernels"]
    text = (f"Measured (`tools/bench_clip.py`, `profiles/clip_bench.json`; one MI355X, bench.py's full-size training model: {res['tensors']} tensors, "
            f"{res['parameters'] / 1e6:.1f} M parameters, {res['chunks']} chunks; one process, the three paths alternated, warmed, {res['repeats']} repeats of "
            f"{res['calls_per_repeat']} calls each between device events, median (min .. max) per call, host work included): "
            f"(a) `clip_grad_norm_` + `step()`, the parent's path, {f(P['a_torch_clip_then_step'])}; (b) `step(max_grad_norm=1.0)` {f(P['b_step_max_grad_norm'])}; "
            f"(c) `step()` alone {f(P['c_step_alone'])}.  (b) - (a) = {res['b_minus_a_us']:+.0f} us against (a)'s own range of {res['a_range_us']:.0f} us in "
            f"this run ({'inside' if res['b_within_a_range'] else 'OUTSIDE'} the bar); clipping costs (b) - (c) = {res['b_minus_c_us']:+.0f} us per step.  "
            f"Kernels alone, back to back: `acai_grad_norm` (both launches) {f(K['acai_grad_norm'])}, {res['grad_norm_gb_per_s'] / 1e3:.2f} TB/s over the "
            f"gradients; `acai_adamw_step_clipped` {f(K['acai_adamw_step_clipped'])}; `acai_adamw_step` {f(K['acai_adamw_step'])}.")
    words, lines, cur = text.split(" "), [], indent
    for w in words:     # wrapped at 140 columns, as the documents are
        if len(cur) + len(w) + 1 > 140 and cur.strip():
            lines.append(cur.rstrip())
            cur = indent
        cur += w + " "
    lines.append(cur.rstrip())
    return "\n".join([BEGIN] + lines + [indent + END])


def write_readme(path):
    res = json.loads(open(path).read().strip().splitlines()[-1])
    for name in ("README.md", "DESIGN.md"):     # the same block in both: README beside optim.py, DESIGN.md section 6
        doc = os.path.join(ROOT, name)
        text = open(doc).read()
        if BEGIN not in text or END not in text:
            raise SystemExit(f"{name} has no {BEGIN} ... {END} block")
        head, rest = text.split(BEGIN, 1)
        indent = head[head.rindex("\n") + 1:]      # the block keeps the indentation its begin marker has (README: inside a list item)
        open(doc, "w").write(head + render(res, indent) + rest.split(END, 1)[1])
        print(name, "updated from", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--write-readme", default=None, metavar="JSON")
    a = ap.parse_args()
    if a.write_readme:
        return write_readme(a.write_readme)
    line = json.dumps(measure(a))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

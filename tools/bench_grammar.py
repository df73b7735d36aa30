"""Grammar-constrained decoding and the grammar scan, measured.

1. The constrained greedy step against the greedy step of the PARENT COMMIT: bench.py's decode (8 images of 512x2048, bf16, random-init
   full-size model), 256 steps.  The parent's step can only be run from the parent's tree (its library lacks the new symbols), so every
   repeat is a child process of its own: --parent-tree names a checkout of the parent commit with its library built, and the children
   alternate parent, this tree, parent, ... (5 each).  A child builds the model, prefills, captures the graphs in an untimed cold run and
   reports the median of 3 timed runs of `steps` steps (host clock from the call to DecodeEngine.greedy to its return: arming, the replays,
   one poll at the end); this tree's child times plain greedy and greedy under a bigram automaton (S = 227, every token but <bos> / <pad>
   allowed everywhere) in turn.  Reported: every repeat, the medians, the parent's own repeat-to-repeat spread (max - min over its
   median), and the differences against that spread plus 1 %.
2. acai_grammar_scan on 128 rollouts of 768 tokens: a bigram automaton (103 KB: the LDS path) and one of 4096 states (1.9 MB: the global
   path); a hipGraph-free loop of launches timed with device events, median of 5 windows of 50 launches.

One JSON line on stdout, the same written to --out.  `--write-design FILE.json` (no GPU needed) puts the figures of such a file into
DESIGN.md section 6, between the bench_grammar markers.

  python tools/bench_grammar.py --parent-tree ../parent --out profiles/grammar_bench.json
  python tools/bench_grammar.py --write-design profiles/grammar_bench.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEGIN, END = "<!-- bench_grammar:begin -->", "<!-- bench_grammar:end -->"


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


# ---- a child: one repeat of the step timing, from the tree it is pointed at --------------------------------------------------------------
def worker(a):
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from torch.amp import autocast
    from acai_omr_amd.inference.vitomr_inference import set_up_omr_inference
    dev = torch.device("cuda:0")
    torch.manual_seed(0)   # bench.py's weights
    vitomr, _ = set_up_omr_inference(os.path.join(os.path.abspath(a.tree), "lmx_vocab.txt"), max_batch_size=a.batch, cache_dtype=torch.bfloat16,
                                     device="cuda")
    vitomr = vitomr.eval()
    g = torch.Generator().manual_seed(1000)   # bench.py's rank-0 images
    imgs = [torch.rand(1, a.height, a.width, generator=g).to(dev) for _ in range(a.batch)]
    blocks = vitomr.decoder.decoder_blocks
    with torch.no_grad():
        lat32, _, lens = vitomr.encoder.forward_packed(imgs)
        with autocast(device_type="cuda", dtype=torch.bfloat16):
            mem = vitomr.transition_head.forward_packed(lat32)
        blocks.prepare_caches_packed(None, mem, lens)
    eng = blocks.engine(dev)
    T = a.steps + 1
    variants = {"greedy": {}}
    if a.grammar:
        from acai_omr_amd.grammar import TokenAutomaton
        dec = vitomr.decoder
        V = dec.vocab_size
        nxt = torch.arange(V).repeat(V, 1)
        nxt[:, dec.bos_idx] = nxt[:, dec.pad_idx] = -1
        variants["grammar"] = {"grammar": TokenAutomaton.from_transitions(nxt, dec.bos_idx, pad_idx=dec.pad_idx, bos_idx=dec.bos_idx,
                                                                          eos_idx=dec.eos_idx).to(dev)}
    times = {k: [] for k in variants}
    with torch.no_grad():
        for name, kw in variants.items():       # cold: code objects, graph capture
            eng.greedy(T, poll=T, **kw)
        torch.cuda.synchronize()
        for _ in range(3):
            for name, kw in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, _, done = eng.greedy(T, poll=T, **kw)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
                assert done == a.steps
    print("RESULT " + json.dumps({k: median(v) / a.steps for k, v in times.items()}))


def run_child(tree, a, grammar):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--steps", str(a.steps), "--batch", str(a.batch),
           "--height", str(a.height), "--width", str(a.width)] + (["--grammar"] if grammar else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"child failed ({tree}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


# ---- the scan -----------------------------------------------------------------------------------------------------------------------------
def bench_scan(R=128, ld=768):
    import torch
    sys.path.insert(0, ROOT)
    from acai_omr_amd import ops
    from acai_omr_amd.grammar import TokenAutomaton
    dev = torch.device("cuda:0")
    toks = [ln.strip() for ln in open(os.path.join(ROOT, "lmx_vocab.txt")) if ln.strip()]
    V, ids = len(toks), dict(pad_idx=toks.index("<pad>"), bos_idx=toks.index("<bos>"), eos_idx=toks.index("<eos>"))
    g = torch.Generator().manual_seed(5)
    nxt = torch.arange(V).repeat(V, 1)
    nxt[torch.rand(V, V, generator=g) < 0.2] = -1
    nxt[:, 3] = 3
    nxt[:, ids["bos_idx"]] = nxt[:, ids["pad_idx"]] = -1
    S = 4096
    big = torch.randint(0, S, (S, V), generator=g)
    big[torch.rand(S, V, generator=g) < 0.2] = -1
    big[:, 3] = 7
    big[:, ids["bos_idx"]] = big[:, ids["pad_idx"]] = -1
    autos = {"bigram_lds": TokenAutomaton.from_transitions(nxt, ids["bos_idx"], **ids), "states4096_global": TokenAutomaton.from_transitions(big, 0, **ids)}
    rows = torch.randint(3, V, (R, ld), generator=g)
    rows[:, 0] = ids["bos_idx"]
    lens = torch.randint(ld // 2, ld + 1, (R,), generator=g, dtype=torch.int32)
    rows[torch.arange(R), lens.long() - 1] = ids["eos_idx"]
    out = {}
    for name, a in autos.items():
        want = a.violations(rows, lens)
        ad, rd, ln = a.to(dev), rows.to(dev), lens.to(dev)
        got = ops.grammar_scan(rd, ln, ad)
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), name
        win = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(50):
                ops.grammar_scan(rd, ln, ad)
            e1.record()
            torch.cuda.synchronize()
            win.append(e0.elapsed_time(e1) / 50 * 1e3)
        out[name] = dict(states=a.states, table_bytes=a.states * V * 2, us_per_launch=median(win), us_min=min(win), us_max=max(win),
                         tokens=int(lens.sum()), violations=int(want[0].sum()))
    return dict(rollouts=R, tokens_per_rollout=ld, note="device events around 50 launches (each with its two output allocations), median of 5 windows; "
                "results checked against TokenAutomaton.violations first", **out)


# ---- DESIGN.md ---------------------------------------------------------------------------------------------------------------------------
def render(res):
    st, sc = res["step"], res["scan"]
    lines = [BEGIN,
             f"`tools/bench_grammar.py`, {res['device']}: {st['workload']}; {st['repeats']} child processes per tree, alternated, each the median of 3 runs.",
             "",
             "| ms per step | repeats | median | min .. max |", "|---|---|---|---|"]
    for key, label in (("parent_greedy", "parent commit, greedy"), ("greedy", "this tree, greedy"), ("grammar", "this tree, greedy under the bigram automaton")):
        v = st[key]
        lines.append(f"| {label} | {', '.join(f'{x:.4f}' for x in v['ms_per_step'])} | {v['median']:.4f} | {v['min']:.4f} .. {v['max']:.4f} |")
    lines += ["",
              f"The parent's own repeat-to-repeat spread is {st['parent_spread_pct']:.2f} % of its median; the bar is that spread plus 1 % = "
              f"{st['bar_pct']:.2f} %.  Plain greedy on this tree: {st['greedy_vs_parent_pct']:+.2f} % against the parent's median; the constrained "
              f"step: {st['grammar_vs_parent_pct']:+.2f} % against the parent's greedy step, {st['grammar_vs_greedy_pct']:+.2f} % against this tree's.",
              "",
              f"`acai_grammar_scan`, {sc['rollouts']} rollouts of up to {sc['tokens_per_rollout']} tokens: "
              + "; ".join(f"{k} ({v['states']} states, {v['table_bytes'] / 1024:.0f} KB) {v['us_per_launch']:.1f} us per launch "
                          f"({v['us_min']:.1f} .. {v['us_max']:.1f})" for k, v in sc.items() if isinstance(v, dict)) + f".  {sc['note']}.",
              END]
    return "\n".join(lines)


def write_design(path):
    res = json.loads(open(path).read().strip().splitlines()[-1])
    design = os.path.join(ROOT, "DESIGN.md")
    text = open(design).read()
    if BEGIN not in text or END not in text:
        raise SystemExit(f"DESIGN.md has no {BEGIN} ... {END} block")
    head, rest = text.split(BEGIN, 1)
    open(design, "w").write(head + render(res) + rest.split(END, 1)[1])
    print("DESIGN.md section 6 updated from", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--out", default=None)
    ap.add_argument("--write-design", default=None, metavar="JSON")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--grammar", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.write_design:
        return write_design(a.write_design)
    if a.worker:
        return worker(a)
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    if not a.parent_tree or not os.path.isdir(os.path.join(a.parent_tree, "acai_omr_amd")):
        raise SystemExit("--parent-tree must name a checkout of the parent commit (with its library built)")
    reps = {"parent_greedy": [], "greedy": [], "grammar": []}
    for _ in range(a.repeats):
        reps["parent_greedy"].append(run_child(a.parent_tree, a, False)["greedy"])
        r = run_child(ROOT, a, True)
        reps["greedy"].append(r["greedy"])
        reps["grammar"].append(r["grammar"])
    step = {k: dict(ms_per_step=v, median=median(v), min=min(v), max=max(v)) for k, v in reps.items()}
    pm = step["parent_greedy"]["median"]
    spread = (step["parent_greedy"]["max"] - step["parent_greedy"]["min"]) / pm * 100
    step.update(workload=f"{a.batch} images of {a.height}x{a.width}, bf16, {a.steps} greedy steps from replayed graphs, bench.py's random-init weights",
                repeats=a.repeats, parent_spread_pct=spread, bar_pct=spread + 1.0,
                greedy_vs_parent_pct=(step["greedy"]["median"] / pm - 1) * 100, grammar_vs_parent_pct=(step["grammar"]["median"] / pm - 1) * 100,
                grammar_vs_greedy_pct=(step["grammar"]["median"] / step["greedy"]["median"] - 1) * 100)
    out = dict(device=torch.cuda.get_device_name(0), step=step, scan=bench_scan())
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

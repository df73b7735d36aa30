"""Prompt prefill: time from the call to the FIRST FREE TOKEN after a known prompt, bf16, bench.py's random-init weights (full-size decoder),
one process, the variants alternated round by round (tools/bench_prompt.py's set-up: the prompt is the model's own greedy output with
<eos> suppressed, --prompt tokens long).

Per workload (one 256x1024 image, and 8 images of 512x2048) the variants are:
  prompt   DecodeEngine.greedy(prompt=...): one acai_decode_prompt_step per prompt token, in replayed graphs;
  spec_D7  DecodeEngine.speculative(7, prompt=...): 8 prompt tokens per verify step;
  prefill  DecodeEngine.greedy(prompt=..., prefill=True): one teacher-forced pass over the prompt (eager launches), the self K/V scatter
           per layer, the arm kernel, then one prompt step for the free token.
and, for prompt and prefill alone, a sweep over short prompts (--sweep depths) that shows from which depth the pass pays.
Every variant is timed between two device events around the call (so the host's work inside the call counts), after an untimed cold run
that captures the graphs; the cross-K/V prefill of the memories is outside the window.  Before timing, prefill's forced tokens must equal
prompt mode's and its log-probs lie within the project's pass-versus-decode bar (0.07 in bf16); whether the free token is the same is
reported, not required (random-init weights decide it on near-ties).  Reported: median / min / max over --rounds in ms.
One JSON line on stdout, the same written to --out.

  python tools/bench_prefill.py --rounds 7 --prompt 512 --out profiles/prefill_bench.json
  (--variants prefill --sweep "" --rounds 1: the prefilled runs alone, for a kernel-trace run)
"""
import argparse
import json
import os
import sys

import torch
from torch.amp import autocast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def memory(vitomr, imgs):
    with torch.no_grad():
        lat32, _, lens = vitomr.encoder.forward_packed(imgs)
        with autocast(device_type="cuda", dtype=torch.bfloat16):
            return vitomr.transition_head.forward_packed(lat32), lens


def stats(xs):
    s = sorted(xs)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


def bench_workload(vitomr, dev, n_img, height, width, P, sweep, names, rounds):
    blocks = vitomr.decoder.decoder_blocks
    eng = blocks.engine(dev)
    g = torch.Generator().manual_seed(1000)
    imgs = [torch.rand(1, height, width, generator=g).to(dev) for _ in range(n_img)]
    mem, lens = memory(vitomr, imgs)

    def prepare(D):
        blocks.prepare_caches_packed(None, mem, lens, group_size=D + 1, per_row_cross=D > 0)
        torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        with torch.no_grad():
            out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def run(name, prompts, T):
        if name == "spec_D7":
            prepare(7)
            ms, (s, lp, _) = timed(lambda: eng.speculative(T, 7, prompt=prompts))
        else:
            prepare(0)
            ms, (s, lp, _) = timed(lambda: eng.greedy(T, prompt=prompts, prefill=name == "prefill"))
        return ms, (s[:, :T].clone(), lp[:, :T].clone())

    prepare(0)
    with torch.no_grad():
        s, _, _ = eng.greedy(P + 2)
    own = s.clone()

    def measure(depth, variants):
        T = depth + 2   # <bos>, the prompt, the first free token
        prompts = [own[i, 1:1 + depth].clone() for i in range(n_img)]
        ref, res = None, {}
        for name in variants:   # cold runs double as the check
            _, out = run(name, prompts, T)
            if name == "prompt":
                ref = out
            elif name == "prefill" and ref is not None:
                assert torch.equal(out[0][:, :depth + 1], ref[0][:, :depth + 1]), "prefill: forced tokens differ from prompt mode's"
                err = float((out[1][:, :depth + 1] - ref[1][:, :depth + 1]).abs().max())
                assert err <= 0.07, f"prefill: log-probs differ from prompt mode's by {err}"
                res["prefill_check"] = dict(max_abs_logprob_diff=err, free_token_equal=bool(torch.equal(out[0][:, -1], ref[0][:, -1])))
        times = {name: [] for name in variants}
        for _ in range(rounds):
            for name in variants:
                times[name].append(run(name, prompts, T)[0])
        for name in variants:
            res[name] = stats(times[name])
        return res

    out = dict(images=n_img, patches=lens, prompt_tokens=P, ms_to_first_free_token=measure(P, names))
    short = [n for n in names if n != "spec_D7"]
    if sweep and short:
        out["sweep_ms_to_first_free_token"] = {str(c): measure(c, short) for c in sweep}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=512, help="prompt tokens")
    ap.add_argument("--sweep", default="1,2,4,8,16,64", help="comma-separated short prompt depths, prompt mode against prefill")
    ap.add_argument("--variants", default="prompt,spec_D7,prefill")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    from acai_omr_amd.inference.vitomr_inference import set_up_omr_inference
    torch.manual_seed(0)   # bench.py's weights
    vitomr, _ = set_up_omr_inference(os.path.join(ROOT, "lmx_vocab.txt"), max_batch_size=64, cache_dtype=torch.bfloat16, device="cuda")
    vitomr = vitomr.eval()
    with torch.no_grad():
        vitomr.decoder.unembed.bias[vitomr.decoder.eos_idx] = -1e4   # <eos> suppressed: the greedy output fills the prompt
    sweep = [int(c) for c in a.sweep.split(",") if c]
    names = [n for n in a.variants.split(",") if n]
    res = {"1x256x1024": bench_workload(vitomr, dev, 1, 256, 1024, a.prompt, sweep, names, a.rounds),
           "8x512x2048": bench_workload(vitomr, dev, 8, 512, 2048, a.prompt, sweep, names, a.rounds)}
    out = dict(workload="ms from the call to the first free token after a prompt of the model's own greedy output (<eos> suppressed), bf16, "
                        "random-init full-size decoder, max batch size 64; prompt = DecodeEngine.greedy(prompt=), spec_D7 = "
                        "DecodeEngine.speculative(7, prompt=), prefill = DecodeEngine.greedy(prompt=, prefill=True); between device events "
                        "around the call, cross-K/V prefill of the memories outside the window, graphs captured in an untimed cold run, "
                        "variants alternated, median (min, max) of rounds",
               prompt_tokens=a.prompt, rounds=a.rounds, device=torch.cuda.get_device_name(dev), workloads=res)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

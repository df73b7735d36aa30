"""Prompted decoding: time from the call to the FIRST FREE TOKEN after a known prompt, bf16, bench.py's random-init weights (full-size
decoder), one process, the variants interleaved round by round.  The prompt is the model's own greedy output with <eos> suppressed (its
logit bias set to -1e4), --prompt tokens long, so every variant must reproduce the greedy tokens and log-probs - checked before timing.

Per workload (default one 256x1024 image, and 8 images of 512x2048) the variants are:
  host     the host-stepped route that needs no prompt mode: ViTOMR.cached_get_next_token once per token (acai_decode_logits: one launch
           sequence per token from the host, no hipGraph), the known tokens fed back, one device synchronise at the end;
  prompt   DecodeEngine.greedy(prompt=...): acai_decode_prompt_step in replayed graphs, the tables uploaded inside the window;
  spec_D   DecodeEngine.speculative(D, prompt=...): acai_decode_spec_prompt_step, D + 1 prompt tokens per verify step (D = 7; D = 3 as well
           for the batch of 8, where D = 7 makes 64 decode rows);
  greedy   DecodeEngine.greedy over the same number of steps, for the step time beside prompt mode's.
Every variant is timed with a host clock from the call to a device synchronise after it; the cross-K/V prefill is outside the window, the
graphs are captured in an untimed cold run.  Reported: median / min / max over --rounds, ms per step, and the step counts.
One JSON line on stdout, the same written to --out.

  python tools/bench_prompt.py --rounds 7 --prompt 512 --out profiles/prompt_bench.json
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


def memory(vitomr, imgs):
    with torch.no_grad():
        lat32, _, lens = vitomr.encoder.forward_packed(imgs)
        with autocast(device_type="cuda", dtype=torch.bfloat16):
            return vitomr.transition_head.forward_packed(lat32), lens


def stats(xs):
    s = sorted(xs)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


def bench_workload(vitomr, dev, n_img, height, width, P, Ds, rounds):
    blocks = vitomr.decoder.decoder_blocks
    eng = blocks.engine(dev)
    T = P + 2   # <bos>, P prompt tokens, the first free token
    g = torch.Generator().manual_seed(1000)
    imgs = [torch.rand(1, height, width, generator=g).to(dev) for _ in range(n_img)]
    mem, lens = memory(vitomr, imgs)

    def prepare(D):
        blocks.prepare_caches_packed(None, mem, lens, group_size=D + 1, per_row_cross=D > 0)
        torch.cuda.synchronize()

    def timed(fn):
        t0 = time.perf_counter()
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def run_greedy():
        prepare(0)
        dt, (s, lp, _) = timed(lambda: eng.greedy(T))
        return dt, T - 1, (s.clone(), lp.clone())

    def run_prompt(prompts):
        prepare(0)
        dt, (s, lp, _) = timed(lambda: eng.greedy(T, prompt=prompts))
        return dt, T - 1, (s.clone(), lp.clone())

    def run_spec(D, prompts):
        prepare(D)
        dt, (s, lp, st) = timed(lambda: eng.speculative(T, D, prompt=prompts))
        return dt, int(st.max()), (s.clone(), lp.clone())

    def run_host(prompts):
        prepare(0)
        seqs = torch.full((n_img, T), vitomr.decoder.pad_idx, dtype=torch.long, device=dev)
        seqs[:, 0] = vitomr.decoder.bos_idx
        lps = torch.zeros(n_img, T, device=dev)
        known = torch.stack(prompts).to(dev)

        def loop():
            for t in range(1, T):
                idx, lp = vitomr.cached_get_next_token(seqs, t, None)
                if t <= P:   # the known token and the model's log-prob of it: what a scoring caller reads from the step's logits
                    seqs[:, t] = known[:, t - 1]
                else:
                    seqs[:, t] = idx
                lps[:, t] = lp
            return seqs
        dt, s = timed(loop)
        return dt, T - 1, (s, lps)

    _, _, ref = run_greedy()   # cold: code objects, graph capture
    prompts = [ref[0][i, 1:1 + P].clone() for i in range(n_img)]
    variants = [("greedy", run_greedy), ("prompt", lambda: run_prompt(prompts)), ("host", lambda: run_host(prompts))]
    variants += [(f"spec_D{D}", lambda D=D: run_spec(D, prompts)) for D in Ds]
    steps_of = {}
    for name, fn in variants:   # cold runs double as the equality check
        _, steps_of[name], out = fn()
        if name == "host":   # (torch's arg-max and log_softmax: the free token may differ on a tie, the log-probs are not bitwise the kernels')
            assert torch.equal(out[0][:, :P + 1], ref[0][:, :P + 1]) and float((out[1][:, :T] - ref[1]).abs().max()) < 0.1, name
            continue
        assert torch.equal(out[0][:, :T], ref[0]), f"{name}: tokens differ from greedy"
        assert torch.equal(out[1][:, :T], ref[1]), f"{name}: log-probs differ from greedy"
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(fn()[0])
    res = dict(images=n_img, patches=lens, prompt_tokens=P, cross_chunk=eng.cross_chunk, equal_to_greedy=True)
    for name, _ in variants:
        ms = stats([t * 1e3 for t in times[name]])
        res[name] = dict(ms_to_first_free_token=ms, steps=steps_of[name], ms_per_step=ms["median"] / steps_of[name])
    res["prompt_over_greedy_step"] = res["prompt"]["ms_per_step"] / res["greedy"]["ms_per_step"]
    res["host_over_prompt"] = res["host"]["ms_to_first_free_token"]["median"] / res["prompt"]["ms_to_first_free_token"]["median"]
    for D in Ds:
        r = res[f"spec_D{D}"]
        r["expected_steps"] = -(-(P + 1) // (D + 1))
        r["prompt_over_spec"] = res["prompt"]["ms_to_first_free_token"]["median"] / r["ms_to_first_free_token"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=512, help="prompt tokens")
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
    res = {"1x256x1024": bench_workload(vitomr, dev, 1, 256, 1024, a.prompt, (7,), a.rounds),
           "8x512x2048": bench_workload(vitomr, dev, 8, 512, 2048, a.prompt, (7, 3), a.rounds)}
    out = dict(workload="time from the call to the first free token after a prompt of the model's own greedy output (<eos> suppressed), bf16, "
                        "random-init full-size decoder, max batch size 64; host = cached_get_next_token per token, prompt = "
                        "DecodeEngine.greedy(prompt=), spec_D = DecodeEngine.speculative(D, prompt=); prefill outside the window, graphs "
                        "captured in an untimed cold run, variants interleaved, median of rounds",
               prompt_tokens=a.prompt, rounds=a.rounds, device=torch.cuda.get_device_name(dev), workloads=res)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

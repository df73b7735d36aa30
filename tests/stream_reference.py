"""Reference statements for streamed continuous batching (DecodeEngine.continuous(flush=), acai_decode_slot_flush), in numpy and plain
Python: nothing here needs a device.

  flush_reference   the flush contract of include/acai_omr_hip.h, slot by slot;
  predict_events    the exact event skeleton of a streamed run, from each image's final length: the engine's loop driven through the real
                    acai_omr_amd.scheduler.SlotScheduler against a model device whose rows stop at the given lengths."""
import numpy as np


def flush_reference(seqs, logprobs, slot_t, finished, mark, B, ld, out_tok, out_lp, hdr):
    """The contract of acai_decode_slot_flush on numpy arrays: seqs int64 / logprobs fp32 (rows, pitch), slot_t / finished / mark int32
    (rows,), out_tok int32 / out_lp fp32 (B, ld) and hdr int32 (B, 4) as they were before the call.  Returns (out_tok, out_lp, hdr, mark)
    after it, as copies; entries past a slot's n keep what they held.  A refused call (ld < 1, ld above the pitch, fewer than B rows,
    B < 1) returns None: nothing is written."""
    pitch = seqs.shape[1]
    rows = min(a.shape[0] for a in (seqs, logprobs, slot_t, finished, mark))
    if B < 1 or rows < B or ld < 1 or ld > pitch:
        return None
    out_tok, out_lp, hdr, mark = out_tok.copy(), out_lp.copy(), hdr.copy(), mark.copy()
    for s in range(B):
        fin = int(finished[s] != 0)
        end = int(slot_t[s]) + 1 if fin else int(slot_t[s])
        m = int(mark[s])
        n = min(max(end - m, 0), ld)
        out_tok[s, :n] = seqs[s, m:m + n].astype(np.int32)
        out_lp[s, :n] = logprobs[s, m:m + n]
        hdr[s] = (n, m, fin, 0)
        mark[s] = m + n
    return out_tok, out_lp, hdr, mark


def predict_events(lengths, caps, slots, flush_interval):
    """lengths[i]: image i's tokens after <bos> in its final row (its <eos> included; 0 for a cap below 2); caps[i] its cap.  Returns the
    polls of a streamed run as a list of (steps, finishes): steps = [(image, start, n)] in slot order - the row's indices
    start .. start + n - 1 handed out at that poll - and finishes = [image] in slot order.  The images with a cap below 2 are the first
    entry, ([], skipped), when there are any: they finish before anything is decoded.

    The loop is DecodeEngine._continuous's: admit, run chunk(flush_interval) steps, poll - flush every slot (a slot holding image i at local
    progress d has written min(d + steps, lengths[i]) tokens and stops there), advance, refill - and again until the scheduler is done."""
    from acai_omr_amd.scheduler import SlotScheduler
    lengths, caps = [int(x) for x in lengths], [int(c) for c in caps]
    assert len(lengths) == len(caps)
    for L, c in zip(lengths, caps):
        assert (L == 0 if c < 2 else 1 <= L <= c - 1), (L, c)
    sc = SlotScheduler(caps, slots)
    polls = [([], list(sc.skipped))] if sc.skipped else []
    written = [0] * slots   # tokens the slot's image has written, and how many of them were handed out
    sent = [0] * slots
    for s, _ in sc.admit():
        written[s] = sent[s] = 0
    n = sc.chunk(flush_interval)
    while n > 0:
        steps, fin = [], [1] * slots   # (an idle slot is parked: finished, nothing to send)
        for s, i in enumerate(sc.image):
            if i is None:
                continue
            written[s] = min(written[s] + n, lengths[i])
            fin[s] = int(written[s] == lengths[i])
            if written[s] > sent[s]:
                steps.append((i, 1 + sent[s], written[s] - sent[s]))
                sent[s] = written[s]
        freed = sc.advance(n, fin)
        polls.append((steps, [i for _, i in freed]))
        for s, _ in sc.admit():
            written[s] = sent[s] = 0
        n = sc.chunk(flush_interval)
    assert sc.done
    return polls


def flatten_events(polls):
    """predict_events' polls as one list: ("step", image, start, n) and ("finish", image), in the order the generator yields them."""
    out = []
    for steps, finishes in polls:
        out += [("step",) + st for st in steps]
        out += [("finish", i) for i in finishes]
    return out

"""Case builders shared by tests/test_speculative_cpu.py and tests/test_gpu_spec_accept.py: states of ONE speculative accept-and-draft launch
(speculative_reference.SpecState), the logits planted on them, and the histories that take the prompt-lookup drafter past its first 64
candidate ends.  Every builder asserts on the CPU the property that names its case, so a case is known to discriminate without a GPU.

Logits: a row's planted arg-max is 3.0 over entries in [-1, 1), so it leads by at least 2.0 (bar of the tests: 1.0) and no tolerance is needed
for tokens; a named tie makes two entries bit-equal."""
from dataclasses import dataclass, field

import torch

import select_reference as SEL
import speculative_reference as SR

NONE = SR.NONE
BOS, PAD, EOS = 0, 1, 2
SENT_TOK = -4242                 # an impossible id: seqs past the history, tab, next
SENT_F32 = 0x7FC0DEAD            # a NaN bit pattern: logprobs and x on the device
HOT = 3.0


def gen(*key):
    s = 23
    for k in key:
        s = (s * 1000003 + int(k) + 54321) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def make_cfg(V, B, max_len, Tmax, E=8, seed=0, eos=EOS, pad=PAD, bos=BOS):
    g = gen(V, B, E, seed)
    return SEL.Cfg(V=V, B=B, max_len=max_len, Tmax=Tmax, eos=eos, bos=bos, pad=pad, emb=torch.randn(V, E, generator=g),
                   pos=torch.randn(Tmax, E, generator=g))


@dataclass
class Img:
    """One image before a verify step: the tokens of indices 0 .. t - 1, the D drafts under verification, the planted arg-max of rows 0 .. D
    (None: left random) and what the case expects the step to write (None: not asserted by the builder's user)."""
    prefix: list
    drafts: list
    greedy: list
    cap: int = None
    finished: int = 0
    t: int = None                # (default: len(prefix))
    steps: int = 0
    ties: dict = field(default_factory=dict)   # row -> index made bit-equal to the planted arg-max
    expect: int = None           # tokens the step writes
    name: str = ""


def build_state(cfg, D, pitch, imgs, rows=None, cache=0):
    """The state before the launch: sentinels wherever the images say nothing (finished[images .. B - 1] = 7: never to be touched)."""
    assert cfg.B == len(imgs) * (D + 1)
    st = SR.new_spec_state(cfg, D, pitch, rows, fill_tok=SENT_TOK, fill_tab=SENT_TOK, fill_next=SENT_TOK, cache=cache)
    st.seqs[:, 0] = SENT_TOK
    st.finished[len(imgs):cfg.B] = 7
    for i, im in enumerate(imgs):
        t = len(im.prefix) if im.t is None else im.t
        st.seqs[i, :len(im.prefix)] = torch.tensor(im.prefix, dtype=torch.int64)
        st.t[i], st.cap[i], st.finished[i], st.steps[i] = t, cfg.max_len if im.cap is None else im.cap, im.finished, im.steps
        if 1 <= t <= len(im.prefix):
            st.next[i, 0] = im.prefix[t - 1]
        assert len(im.drafts) == D
        st.next[i, 1:D + 1] = torch.tensor(im.drafts, dtype=torch.int64)
    return st


def plant_logits(cfg, D, imgs, *key):
    R = D + 1
    lg = torch.rand(cfg.B, cfg.V, generator=gen(cfg.B, cfg.V, *key)) * 2 - 1
    for i, im in enumerate(imgs):
        for j, tok in enumerate(im.greedy):
            if tok is not None:
                lg[i * R + j, tok] = HOT
                if j in im.ties:
                    lg[i * R + j, im.ties[j]] = HOT
    return lg


def check_margins(lg, imgs, D):
    """The planted arg-max leads by at least 1.0 (a tie: exactly 0 to its partner, at least 1.0 to the rest)."""
    R = D + 1
    for i, im in enumerate(imgs):
        for j, tok in enumerate(im.greedy):
            if tok is None:
                continue
            row = lg[i * R + j].clone()
            assert float(row[tok]) == float(row.max())
            row[tok] = -9.0
            if j in im.ties:
                assert float(row[im.ties[j]]) == HOT
                row[im.ties[j]] = -9.0
            assert float(row.max()) <= HOT - 1.0


# ---- a. the accept rule ------------------------------------------------------------------------------------------------------------------
def _toks(V):
    """Tokens a case may emit without ending the image: everything but <eos>."""
    return [v for v in range(V) if v != EOS]


def accept_images(D, V, max_len, seed=0):
    """The images of test a for one D and V (see the issue's list); each carries the number of tokens its step must write."""
    g = gen(D, V, seed, 7)
    ok = _toks(V)
    pick = lambda: ok[int(torch.randint(0, len(ok), (1,), generator=g))]
    other = lambda tok: next(v for v in ok if v != tok)
    imgs = []

    def add(name, greedy, drafts, expect, t0=None, cap=None, ties=None):
        t0 = t0 if t0 is not None else 2 + int(torch.randint(0, 6, (1,), generator=g))
        imgs.append(Img(prefix=[BOS] + [pick() for _ in range(t0 - 1)], drafts=list(drafts), greedy=list(greedy), cap=cap, ties=ties or {},
                        expect=expect, name=name))

    def run():
        gr = [pick() for _ in range(D + 1)]
        return gr, gr[:D]   # every draft right: draft j = g_{j-1}

    for n in range(D + 1):   # n drafts accepted, draft n + 1 wrong
        gr, dr = run()
        if n < D:
            dr[n] = other(gr[n])
        add(f"n{n}", gr, dr, n + 1)
    gr, dr = run()
    dr[0] = NONE
    add("none_first", gr, dr, 1)
    if D >= 3:
        gr, dr = run()
        dr[D // 2] = NONE
        add("none_middle", gr, dr, D // 2 + 1)
    if D >= 2:   # draft 1 wrong, draft 2 equal to g_1 by chance: the step stops at 1
        gr, dr = run()
        dr[0] = other(gr[0])
        assert dr[1] == gr[1]
        add("wrong_then_right", gr, dr, 1)
    gr, dr = run()
    gr[0] = EOS
    dr[0] = EOS
    add("eos_g0", gr, dr, 1)
    if D >= 2:
        gr, dr = run()
        gr[1] = EOS
        dr[1] = EOS   # (draft 2 = g_1 = <eos> is right as well: the cut, not a mismatch, ends the run)
        add("eos_accepted", gr, dr, 2)
    gr, dr = run()   # <eos> is the token after the last accepted draft
    n = max(D - 1, 1)
    gr[n] = EOS
    if n < D:
        dr[n] = other(EOS)
    add("eos_after_last", gr, dr, n + 1)
    gr, dr = run()
    if D >= 2:
        add("cap_inside", gr, dr, 2, t0=5, cap=7)
    add("cap_at_end", gr, dr, D + 1, t0=5, cap=5 + D + 1)
    add("t_is_cap_minus_1", gr, dr, 1, t0=6, cap=7)
    assert max_len >= 5 + D + 1 + 1, "cap_at_end must sit below max_len"
    if V >= 3:
        lo, hi = ok[0], ok[1]
        for name, draft, expect in (("tie_lower_is_draft", lo, 2), ("tie_higher_is_draft", hi, 1)):
            gr, dr = run()
            gr[0], dr[0] = lo, draft
            add(name, gr, dr + [], expect if D >= 1 else 1, ties={0: hi})
            if D >= 2:
                imgs[-1].drafts[1] = other(gr[1])   # (stop after g_1 at the latest)
    for p in sorted({0, 63, 64, V - 1}):
        if p < V and p != EOS:
            gr, dr = run()
            gr[0], dr[0] = p, p
            if D >= 2:
                dr[1] = other(gr[1])
            add(f"argmax_at_{p}", gr, dr, 2)
    return imgs


# ---- d. the drafter on long histories ----------------------------------------------------------------------------------------------------
def distinct_history(t, seed=0, V=512):
    """<bos> then t - 1 distinct tokens from [3, V)."""
    perm = (torch.randperm(V - 3, generator=gen(t, seed, 5)) + 3).tolist()
    assert t - 1 <= len(perm)
    return [BOS] + perm[:t - 1]


def plant_suffix(h, m, e):
    """Copies the last m tokens of h to h[e - m:e] (in place); e = m puts them on <bos> too."""
    t = len(h)
    assert m <= e <= t - 1
    if e > t - m:   # overlapping: the copy and the suffix share tokens - a constant run is the only solution
        for p in range(e - m, t):
            h[p] = h[t - 1]
    else:
        h[e - m:e] = h[t - m:t]
    return h


def windowed_proposals(seq, D, ngram, window=64):
    """A WRONG drafter: it looks only at the `window` most recent candidate ends.  The far cases must tell it from the reference."""
    L = len(seq)
    for m in range(min(ngram, L - 1), 0, -1):
        for e in range(L - 1, max(m, L - window) - 1, -1):
            if seq[e - m:e] == seq[L - m:]:
                prop = list(seq[e:min(e + D, L)])
                return prop + [NONE] * (D - len(prop))
    return [NONE] * D


def ballot_of(t, e):
    """Which run of 64 candidate ends (from the most recent, t - 1, down) holds e."""
    return (t - 1 - e) // 64


def single_occurrence_histories(ngram, D):
    """(name, history) for t in {66, 130, 150, 199} with the ONE earlier occurrence of the last m = ngram tokens ending at t - 1, t - 64,
    t - 65, t - 129 and m, wherever that end exists for the t."""
    out = []
    for t in (66, 130, 150, 199):
        for name, e in (("e_t-1", t - 1), ("e_t-64", t - 64), ("e_t-65", t - 65), ("e_t-129", t - 129), ("e_m", ngram)):
            m = ngram
            if not (m <= e <= t - 1) or (e != m and e - m < 1) or (t - m < e < t - 1):
                continue
            h = plant_suffix(distinct_history(t, seed=e), m, e)
            assert SR.ngram_match(h, ngram) == (m, e), (t, name, SR.ngram_match(h, ngram))
            far = ballot_of(t, e) >= 1
            assert far == (e <= t - 65)
            ref, bad = SR.ngram_proposals(h, D, ngram), windowed_proposals(h, D, ngram)
            assert ref[0] != NONE
            assert (ref != bad) == far, (t, name, "a drafter that searches 64 ends must differ exactly on the far cases")
            out.append((f"t{t}_{name}", h))
    return out


def special_histories(D):
    """(name, history, ngram, accepted, cap) of the further drafter cases; `accepted` drafts are written by the launch itself."""
    out = []
    t = 150
    h = distinct_history(t, seed=1)   # two occurrences, first and second ballot: the nearer wins
    h[t - 10 - 3:t - 10] = h[t - 3:]
    h[t - 100 - 3:t - 100] = h[t - 3:]
    assert SR.ngram_match(h, 3) == (3, t - 10) and ballot_of(t, t - 10) == 0 and ballot_of(t, t - 100) == 1
    out.append(("nearer_of_two", h, 3, 0, None))
    h = distinct_history(t, seed=2)   # a trigram far back against a 1-gram near: the longer wins
    h[t - 100 - 3:t - 100] = h[t - 3:]
    h[t - 6] = h[t - 1]
    assert SR.ngram_match(h, 3) == (3, t - 100) and SR.ngram_match(h, 1) == (1, t - 5) and ballot_of(t, t - 100) == 1
    out.append(("longer_far_beats_shorter_near", h, 3, 0, None))
    h = distinct_history(t, seed=3)   # no trigram anywhere, a bigram in the third ballot
    h[t - 140 - 2:t - 140] = h[t - 2:]
    assert SR.ngram_match(h, 3) == (2, t - 140) and ballot_of(t, t - 140) == 2
    assert SR.ngram_proposals(h, D, 3) != windowed_proposals(h, D, 3)
    out.append(("bigram_in_third_ballot", h, 3, 0, None))
    h = distinct_history(t, seed=4)
    assert SR.ngram_match(h, 8) is None
    out.append(("no_occurrence", h, 8, 0, None))
    h = [BOS, 7]
    assert SR.ngram_match(h, 3) is None
    out.append(("t2_shorter_than_ngram", h, 3, 0, None))
    h = [BOS, 7, 7]
    assert SR.ngram_match(h, 8) == (1, 2)
    out.append(("t3_shorter_than_ngram", h, 8, 0, None))
    if D >= 2:   # the suffix includes tokens this launch writes: two drafts are accepted and the new tail completes the repeat
        h = distinct_history(t, seed=5)
        h[t - 80 - 3:t - 80] = h[t - 3:]
        assert SR.ngram_match(h, 3) == (3, t - 80) and SR.ngram_match(h[:t - 3], 3) is None and ballot_of(t, t - 80) == 1
        out.append(("suffix_written_by_this_launch", h, 3, 2, None))
    h = distinct_history(t, seed=6)   # the cut t' + j < cap: only slot 1 survives
    h[t - 70 - 3:t - 70] = h[t - 3:]
    prop = SR.ngram_proposals(h, D, 3)
    assert all(v != NONE for v in prop)
    out.append(("cut_at_cap", h, 3, 0, t + 2))
    return out


def history_image(h, D, accepted=0, cap=None):
    """The image whose verify step leaves the history h: the launch writes its last 1 + accepted tokens (the drafts of the first `accepted`
    slots are right, the rest none)."""
    t0 = len(h) - 1 - accepted
    assert t0 >= 1
    return Img(prefix=h[:t0], drafts=[h[t0 + j] if j < accepted else NONE for j in range(D)], greedy=h[t0:] + [None] * (D - accepted), cap=cap,
               expect=1 + accepted)


# ---- toy streams: logits as a function of the prefix --------------------------------------------------------------------------------------
def prefix_logits(prefix, tok, V):
    """Deterministic logits of the row that has consumed `prefix` (none = <pad>): entries in [-1, 1), the arg-max `tok` at 3.0."""
    s = sum((p + 1) * (int(v) + 3) for p, v in enumerate(prefix)) % 8191
    lg = ((torch.arange(V) * 37 + s * 101) % 89).float() / 44.5 - 1.0
    lg[tok] = HOT
    return lg


def toy_logits(cfg, D, st, nxts):
    """The logits of a verify step on the state st: row j of image i has consumed seq[:t] + drafts[:j] and its arg-max is nxts[i] of that."""
    R = D + 1
    lg = torch.zeros(cfg.B, cfg.V)
    for i, nxt in enumerate(nxts):
        if int(st.finished[i]):
            continue
        t = int(st.t[i])
        seq = [int(v) for v in st.seqs[i, :t]]
        dr = [int(v) if int(v) >= 0 else cfg.pad for v in st.next[i, 1:D + 1]]
        for j in range(R):
            pre = seq + dr[:j]
            lg[i * R + j] = prefix_logits(pre, nxt(pre), cfg.V)
    return lg


def periodic_stream(period, offset, V, eos_at=None, lo=3):
    """next_token of a stream that repeats `period` distinct tokens; <eos> once the prefix has eos_at tokens."""
    assert lo + offset + period <= V

    def nxt(prefix):
        if eos_at is not None and len(prefix) == eos_at:
            return EOS
        return lo + offset + len(prefix) % period
    return nxt

"""spec_accept_kernel (decode_select.hip: the one launch that closes every step of acai_decode_spec_arm / _spec_step / _spec_prompt_arm /
_spec_prompt_step) launched ALONE through acai_debug_decode_spec_accept on a state and logits each case writes itself, against the float64
state transition speculative_reference.spec_step.  No model is built.

Every launch: seqs past the history, tab and next hold an impossible id and logprobs and x a NaN bit pattern before the first launch of a
case; after a launch everything the reference marks `touched` must hold the reference's value and everything else, bit for bit, what was
there before.  Device and reference start from the same state and evolve on their own; they are compared after every launch.

Bars: tokens, t, cap, steps, flags, counters, next and tab integer-equal; x bit-equal (one fp32 addition per element); log-probs (1) bit-equal
to what ops.debug_decode_select writes for the same logits - SELECT_ARGMAX, and SELECT_PROMPT at the row's prompt position for a forced row -
since the header promises the log-probs of acai_decode_step run token by token, and (2) against float64 by test_gpu_select_kernels._lp_check
(fp32 within 1e-5; ACAI_GEMM_ROUND_BF16: the rounded float64 value or its bf16 neighbour).  The planted arg-max of every row leads by at
least 1.0 (spec_accept_cases.check_margins) except in the named ties, where two entries are bit-equal: tokens need no tolerance.

Every row of a live image has finite logits and no NaN: a row without one is outside the selection launches' contract."""
import math
import time

import pytest
import torch

import spec_accept_cases as SC
import speculative_reference as SR
from acai_omr_amd import ops
from decode_support import dev  # noqa: F401
from test_gpu_select_kernels import SENT_LP, _lp_check

pytestmark = pytest.mark.gpu

NONE, BOS, PAD, EOS = SR.NONE, SC.BOS, SC.PAD, SC.EOS
STATS = dict(lp_max=0.0, lp_min=math.inf, launches=0, chain_steps=None)


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.perf_counter()
    yield
    print(f"\nspec accept kernel: {STATS['launches']} launches in {time.perf_counter() - t0:.1f} s of wall time; fp32 log-prob error against float64: "
          f"largest {STATS['lp_max']:.3g}, smallest {STATS['lp_min']:.3g} (bar 1e-5); verify steps of the chained run {STATS['chain_steps']}")


def _bits(t):
    return t.contiguous().view(torch.int32)


class Run:
    """The device buffers of one case beside the reference state; step() launches once and compares everything."""

    def __init__(self, dev, cfg, D, st, *, ngram=0, drafts=None, prompt=None, round_lp=False):
        self.dev, self.cfg, self.D, self.ref, self.ngram, self.drafts, self.prompt, self.bf = dev, cfg, D, st, ngram, drafts, prompt, round_lp
        self.i32 = i32 = lambda v: torch.as_tensor(v).to(torch.int32).to(dev).contiguous()
        nan = lambda *s: torch.full(s, SC.SENT_F32, dtype=torch.int32).view(torch.float32).to(dev)
        rows = st.tab.shape[0]
        self.d = dict(logits=torch.zeros(cfg.B, cfg.V, device=dev), seqs=st.seqs.to(dev), logprobs=nan(rows, cfg.max_len), step=i32(st.step),
                      finished=i32(st.finished), x=nan(cfg.B, cfg.emb.shape[1]), emb=cfg.emb.to(dev), pos=cfg.pos.to(dev))
        self.sp = dict(D=D, ngram=ngram, t=i32(st.t), cap=i32(st.cap), steps=i32(st.steps), tab=i32(st.tab), next=i32(st.next),
                       drafts=None if drafts is None else i32(drafts))
        self.pr = None if prompt is None else dict(tok=i32(prompt["tok"]), len=i32(prompt["len"]))

    def launch(self, logits, arm=False):
        d, c = self.d, self.cfg
        if logits is not None:
            d["logits"].copy_(logits)
        ops.debug_decode_spec_accept(None if arm else d["logits"], d["seqs"], d["logprobs"], d["step"], d["finished"], spec=self.sp,
                                     max_len=c.max_len, Tmax=c.Tmax, eos=c.eos, pad=c.pad, emb=d["emb"], pos=d["pos"], x=d["x"],
                                     round_lp=self.bf, arm=arm, prompt=self.pr, B=c.B, V=c.V)
        torch.cuda.synchronize()
        STATS["launches"] += 1

    def step(self, logits, arm=False):
        """logits: CPU fp32 [B, V] (None with arm).  -> the reference state after the launch (the device agreed with all of it)."""
        d, sp, before = self.d, self.sp, self.ref
        r = SR.spec_step(before, logits, self.cfg, self.D, arm=arm, ngram=self.ngram or None, drafts=self.drafts, prompt=self.prompt)
        lp0, x0 = d["logprobs"].cpu(), d["x"].cpu()
        self.launch(logits, arm)
        for name, got, want in (("seqs", d["seqs"], r.seqs), ("t", sp["t"], r.t), ("cap", sp["cap"], r.cap), ("steps", sp["steps"], r.steps),
                                ("tab", sp["tab"], r.tab), ("next", sp["next"], r.next), ("finished", d["finished"], r.finished)):
            g = got.cpu().long()
            bad = g != want
            assert not bool(bad.any()), (name, bad.nonzero().tolist()[:8], g[bad][:8].tolist(), want[bad][:8].tolist())
        assert d["step"].cpu().tolist() == r.step, ("step", d["step"].cpu().tolist(), r.step)
        live, got = r.touched["seqs"], d["logprobs"].cpu()
        assert torch.equal(_bits(got)[~live], _bits(lp0)[~live]), "a log-prob outside the launch's writes was touched"
        if bool(live.any()):
            _lp_check(torch.where(live, got, torch.full_like(got, SENT_LP)), r.logprobs, live, self.bf)
            if not self.bf:
                w = r.logprobs[live]
                err = (got[live].double() - w).abs() / w.abs().clamp(min=1.0)
                STATS["lp_max"], STATS["lp_min"] = max(STATS["lp_max"], float(err.max())), min(STATS["lp_min"], float(err.min()))
            self._against_select(before, r, got)
        wx = torch.where(r.touched["x"][:, None], r.x, x0)
        gx = d["x"].cpu()
        assert torch.equal(_bits(gx), _bits(wx)), ("x", (_bits(gx) != _bits(wx)).any(1).nonzero().flatten().tolist())
        self.ref = r
        return r

    def _select(self, form, t, max_len, Tmax, prompt=None):
        c, dev = self.cfg, self.dev
        seqs, lps = torch.zeros(c.B, max_len, dtype=torch.int64, device=dev), torch.zeros(c.B, max_len, device=dev)
        ops.debug_decode_select(form, self.d["logits"], seqs, lps, self.i32([t, 0]), torch.zeros(c.B + 1, dtype=torch.int32, device=dev),
                                max_len=max_len, Tmax=Tmax, eos=c.eos, bos=c.bos, pad=c.pad, round_lp=self.bf, chained=False, prompt=prompt)
        torch.cuda.synchronize()
        return seqs[:, t].cpu(), lps[:, t].cpu()

    def _against_select(self, before, r, got):
        """Every written log-prob is, bit for bit, the selection launch's of the greedy / prompted step for the same logits."""
        c, R = self.cfg, self.D + 1
        tok0, lp0 = self._select(ops.SELECT_ARGMAX, 1, 2, 2)
        forced_at = {}
        for i, n in enumerate(r.written):
            _, forced = SR.prompt_row(self.prompt, i, c)
            for j in range(n or 0):
                idx, b = int(before.t[i]) + j, i * R + j
                if forced(idx) != NONE:
                    forced_at.setdefault(idx, []).append((i, b))
                else:
                    assert int(r.seqs[i, idx]) == int(tok0[b]), ("token of the greedy selection", i, j)
                    assert int(_bits(got[i, idx:idx + 1])) == int(_bits(lp0[b:b + 1])), ("log-prob bits of the greedy selection", i, j, got[i, idx], lp0[b])
        if forced_at:
            images = c.B // R
            pr = dict(tok=self.i32(self.prompt["tok"][:images].repeat_interleave(R, 0)), len=self.i32(self.prompt["len"][:images].repeat_interleave(R, 0)))
        for idx, where in forced_at.items():
            tok1, lp1 = self._select(ops.SELECT_PROMPT, idx, c.max_len, c.Tmax, pr)
            for i, b in where:
                assert int(r.seqs[i, idx]) == int(tok1[b]), ("token of the prompted selection", i, idx)
                assert int(_bits(got[i, idx:idx + 1])) == int(_bits(lp1[b:b + 1])), ("log-prob bits of the prompted selection", i, idx, got[i, idx], lp1[b])


def _one(dev, cfg, D, imgs, pitch, key, **kw):
    """One verify launch on the images; -> (run, reference state after it)."""
    cache = kw.pop("cache", 3)
    lg = SC.plant_logits(cfg, D, imgs, *key)
    SC.check_margins(lg, imgs, D)
    run = Run(dev, cfg, D, SC.build_state(cfg, D, pitch, imgs, cache=cache), **kw)
    return run, run.step(lg)


# ---- a. the accept rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("round_lp", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [3, 65, 512])
@pytest.mark.parametrize("D", range(1, 8))
def test_a_accept_rule(dev, D, V, round_lp):
    imgs = SC.accept_images(D, V, 24)
    cfg = SC.make_cfg(V, len(imgs) * (D + 1), 24, 28, E=4)
    _, r = _one(dev, cfg, D, imgs, 26, (D, V), ngram=3, round_lp=round_lp)
    assert r.written == [im.expect for im in imgs], [(im.name, w, im.expect) for im, w in zip(imgs, r.written) if w != im.expect]


# ---- b. who is touched -------------------------------------------------------------------------------------------------------------------
def test_b_who_is_touched(dev):
    """pitch == max_len == cap == Tmax = 16.  Image 1 ends its step at t' = 15, so its table entries t' - 1 .. t' - 1 + D run to index 17: the
    two past the pitch would land in the row of image 2, which is finished and holds the sentinel."""
    D, V, T = 3, 65, 16
    g = SC.gen(31)
    toks = lambda n: [BOS] + torch.randint(3, V, (n - 1,), generator=g).tolist() if n else []
    right = [11, 12, 13, 14]
    imgs = [SC.Img(toks(5), right[:3], right, finished=1), SC.Img(toks(13), [11, 40, 13], right, expect=2), SC.Img(toks(9), right[:3], right, finished=1),
            SC.Img([], right[:3], right, t=0), SC.Img(toks(16), right[:3], right, t=16), SC.Img(toks(4), [NONE] * 3, right, expect=1),
            SC.Img(toks(7), right[:3], right, finished=2), SC.Img(toks(6), [11, EOS, 13], [11, EOS, 13, 14], expect=2)]
    cfg = SC.make_cfg(V, len(imgs) * (D + 1), T, T, E=8)
    run, r = _one(dev, cfg, D, imgs, T, (37,), ngram=2)
    assert r.written == [None, 2, None, None, None, 1, None, 2]
    assert r.finished.tolist() == [1, 0, 1, 1, 1, 0, 2, 1] + [7] * (cfg.B - 8) + [2]
    assert int(r.t[1]) == 15 and r.touched["tab"][1].nonzero().flatten().tolist() == [14, 15] and not bool(r.touched["tab"][2].any())
    for i in (0, 2, 3, 4, 6, 7):
        assert not bool(r.touched["next"][i].any()) and not bool(r.touched["tab"][i].any()) and not bool(r.touched["x"][i * 4:i * 4 + 4].any())
    for i in (0, 2, 3, 4, 6):
        assert not bool(r.touched["seqs"][i].any()) and int(r.steps[i]) == 0
    assert run.d["finished"][8:cfg.B].cpu().tolist() == [7] * (cfg.B - 8)


# ---- c. workgroup shapes -----------------------------------------------------------------------------------------------------------------
def _random_images(n, D, seed, T=24):
    """Each image its own t, cap and number of right drafts; tokens from six symbols, so that bigrams repeat and the drafter proposes."""
    g = SC.gen(n, D, seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    sym = lambda: 3 + ri(0, 5)
    imgs = []
    for _ in range(n):
        t0 = ri(1, T - 4)
        gr = [sym() if ri(0, 9) else EOS for _ in range(D + 1)]
        dr = gr[:D]
        k = ri(0, D)
        if k < D:
            dr[k] = NONE if ri(0, 1) else 9 + ri(0, 3)   # (outside the six symbols: wrong)
        imgs.append(SC.Img([BOS] + [sym() for _ in range(t0 - 1)], dr, gr, cap=ri(t0 + 1, T)))
    return imgs


@pytest.mark.parametrize("images,D", [(1, 1), (1, 7), (2, 3), (3, 2), (20, 1), (9, 7)])
def test_c_workgroup_shapes(dev, images, D):
    """B = 2, 8, 8, 9, 40, 72: the 256, 512 and 1024 thread launches, more rows than waves, more images than waves.  Three launches."""
    V, T = 65, 24
    cfg = SC.make_cfg(V, images * (D + 1), T, T + 2, E=8)
    wrote = 0
    for seed in (0, 1, 2):
        _, r = _one(dev, cfg, D, _random_images(images, D, seed), T, (images, D, seed), ngram=2, round_lp=seed == 2)
        wrote += sum(n or 0 for n in r.written)
    assert wrote >= 3 * images


# ---- d. the drafter on long histories ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 4, 7])
@pytest.mark.parametrize("ngram", [1, 3, 8])
def test_d_drafter_long_histories(dev, ngram, D):
    """max_len = pitch = 200, Tmax = 208, V = 512; one image per history (spec_accept_cases: each builder asserts what names it - the match's
    (m, e), its ballot, that a drafter which looks at 64 ends only would differ).  The launch writes the history's last token(s), so every
    suffix holds a token of this launch."""
    cases = [(name, h, 0, None) for name, h in SC.single_occurrence_histories(ngram, D)]
    cases += [(name, h, acc, cap) for name, h, ng, acc, cap in SC.special_histories(D) if ng == ngram]
    imgs = [SC.history_image(h, D, acc, cap) for _, h, acc, cap in cases]
    cfg = SC.make_cfg(512, len(imgs) * (D + 1), 200, 208, E=4)
    _, r = _one(dev, cfg, D, imgs, 200, (ngram, D), ngram=ngram)
    far = 0
    for i, (name, h, acc, cap) in enumerate(cases):
        t = len(h)
        want = [v if t + j < (cap or 200) else NONE for j, v in enumerate(SR.ngram_proposals(h, D, ngram), start=1)]
        assert int(r.t[i]) == t and [int(v) for v in r.next[i, 1:D + 1]] == want, name
        hit = SR.ngram_match(h, ngram)
        far += hit is not None and SC.ballot_of(t, hit[1]) >= 1 and want[0] != NONE
    assert far >= 5, "matches past the first 64 candidate ends that reach next[]"


# ---- e. the draft table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prompted", [False, True], ids=["plain", "prompted"])
def test_e_draft_table(dev, prompted):
    """Ids -1, V and V + 5 are none; a table is ignored while a prompted image is inside its prompt; the entry at pitch - 1 belongs to a slot
    whose prediction index reaches cap, so it is none although the table holds a token, and tab[pitch - 1] is written."""
    D, V, T = 3, 65, 16
    g = SC.gen(41)
    toks = lambda n: [BOS] + torch.randint(3, V, (n - 1,), generator=g).tolist()
    gr = [20, 21, 22, 23]
    imgs = [SC.Img(toks(4), [NONE] * 3, gr, expect=1), SC.Img(toks(4), [NONE] * 3, gr, expect=1), SC.Img(toks(4), [NONE] * 3, gr, expect=1),
            SC.Img(toks(12), [NONE] * 3, gr, expect=1)]
    table = torch.full((4, T), NONE, dtype=torch.int64)
    table[0, 5:8] = torch.tensor([-1, V, V + 5])
    table[1, 5:8], table[2, 5:8], table[3, 12:16] = torch.tensor([4, 5, 6]), torch.tensor([7, 8, 9]), torch.tensor([30, 31, 32, 33])
    ptok = torch.full((4, T), -3, dtype=torch.int64)
    ptok[2, 1:11] = torch.arange(40, 50)
    prompt = dict(tok=ptok, len=torch.tensor([0, 0, 10, 0])) if prompted else None
    cfg = SC.make_cfg(V, 16, T, T + 4, E=8)
    _, r = _one(dev, cfg, D, imgs, T, (43,), drafts=table, prompt=prompt)
    nx = r.next[:, :4].tolist()
    assert nx[0] == [20, NONE, NONE, NONE] and nx[1] == [20, 4, 5, 6] and nx[3] == [20, 31, 32, NONE]
    assert nx[2] == ([43, 44, 45, 46] if prompted else [20, 7, 8, 9])   # (inside the prompt, index 4 is forced to the prompt's 43)
    assert bool(r.touched["tab"][3, T - 1]) and int(r.tab[3, T - 1]) == 8 * 4 + 3


# ---- f. the prompted instantiation ---------------------------------------------------------------------------------------------------------
def _prompt_images(V):
    """Prompt tokens cycle through 10, 11, 12 (so that an n-gram source WOULD propose at every t'); the planted arg-max of a forced row is
    another token.  -> (images, prompt tok [n, 17], len)."""
    T, D = 16, 3
    cyc = lambda p: 10 + (p - 1) % 3
    tok = torch.tensor([[-5] + [cyc(p) for p in range(1, T + 1)]] * 7)
    pre = lambda t: [BOS] + [cyc(p) for p in range(1, t)]
    G = [20, 21, 22, 23]   # planted: never a prompt token
    imgs, lens = [], []
    # len inside the step: rows 0, 1 forced (indices 4, 5), row 2 greedy, draft 3 none
    imgs.append(SC.Img(pre(4), [cyc(4), cyc(5), NONE], G, expect=3, name="len_inside_step")), lens.append(5)
    # len >= cap is clamped to 15; cap 8 cuts the run at index 7
    imgs.append(SC.Img(pre(5), [cyc(5), cyc(6), NONE], G, cap=8, expect=3, name="len_above_cap")), lens.append(99)
    # a forced <eos> at len
    tok[2, 5] = EOS
    imgs.append(SC.Img(pre(4), [cyc(4), EOS, NONE], G, expect=2, name="forced_eos")), lens.append(5)
    # an id outside [0, V) at index 5: row 1 is greedy (21), row 2 forced again
    tok[3, 5] = V + 3
    imgs.append(SC.Img(pre(4), [cyc(4), 21, NONE], G, expect=3, name="id_outside")), lens.append(6)
    # t' == len: one prompt draft, none beyond, no fall-back
    imgs.append(SC.Img(pre(4), [cyc(4), cyc(5), cyc(6)], G, expect=4, name="t_new_is_len")), lens.append(8)
    # t' == len + 1: the usual source takes over
    imgs.append(SC.Img(pre(4), [cyc(4), cyc(5), cyc(6)], G, expect=4, name="t_new_is_len_plus_1")), lens.append(7)
    # len 0 among prompted images: plain greedy
    imgs.append(SC.Img(pre(4), [20, 21, 40], G, expect=3, name="len_zero")), lens.append(0)
    return imgs, tok, torch.tensor(lens)


@pytest.mark.parametrize("round_lp", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("source", ["ngram", "table"])
def test_f_prompted(dev, source, round_lp):
    D, V, T = 3, 65, 16
    imgs, tok, lens = _prompt_images(V)
    cfg = SC.make_cfg(V, len(imgs) * (D + 1), T, T + 4, E=8)
    table = torch.full((len(imgs), 18), NONE, dtype=torch.int64)
    table[:, 4:12] = torch.arange(50, 58)
    kw = dict(ngram=2) if source == "ngram" else dict(drafts=table)
    _, r = _one(dev, cfg, D, imgs, 18, (47,), prompt=dict(tok=tok, len=lens), round_lp=round_lp, **kw)
    assert r.written == [im.expect for im in imgs]
    by = {im.name: i for i, im in enumerate(imgs)}
    i = by["len_inside_step"]
    assert r.seqs[i, 4:7].tolist() == [10, 11, 22] and int(r.t[i]) == 7, "forced, forced (neither the arg-max), then greedy"
    assert r.seqs[by["len_above_cap"], 5:8].tolist() == [11, 12, 10] and int(r.finished[by["len_above_cap"]]) == 1
    assert r.seqs[by["forced_eos"], 4:6].tolist() == [10, EOS] and int(r.finished[by["forced_eos"]]) == 1
    assert r.seqs[by["id_outside"], 4:7].tolist() == [10, 21, 12]
    i = by["t_new_is_len"]
    assert int(r.t[i]) == 8 and r.next[i, :4].tolist() == [10, 11, NONE, NONE], "one prompt draft, none beyond, no fall-back"
    assert SR.ngram_proposals([int(v) for v in r.seqs[i, :8]], D, 2)[0] != NONE and int(table[i, 8]) >= 0, "the fall-back would have proposed"
    i = by["t_new_is_len_plus_1"]
    assert int(r.t[i]) == 8 and r.seqs[i, 4:8].tolist() == [10, 11, 12, 10]
    assert r.next[i, 1:4].tolist() == (SR.ngram_proposals([int(v) for v in r.seqs[i, :8]], D, 2) if source == "ngram" else [54, 55, 56])
    assert r.seqs[by["len_zero"], 4:7].tolist() == [20, 21, 22]


@pytest.mark.parametrize("arm", [False, True], ids=["verify", "arm"])
def test_f_prompt_of_length_zero_is_the_unprompted_launch(dev, arm):
    """Bit for bit on the same state, every buffer."""
    D, V, T, n = 3, 65, 24, 5
    cfg = SC.make_cfg(V, n * (D + 1), T, T + 2, E=8)
    imgs = _random_images(n, D, 5)
    lg = SC.plant_logits(cfg, D, imgs, 53)
    prompt = dict(tok=torch.randint(3, V, (n, T), generator=SC.gen(59)), len=torch.zeros(n, dtype=torch.int64))
    a = Run(dev, cfg, D, SC.build_state(cfg, D, T, imgs), ngram=2)
    b = Run(dev, cfg, D, SC.build_state(cfg, D, T, imgs), ngram=2, prompt=prompt)
    a.step(None if arm else lg, arm=arm), b.step(None if arm else lg, arm=arm)
    for name in ("seqs", "step", "finished"):
        assert torch.equal(a.d[name], b.d[name]), name
    for name in ("t", "cap", "steps", "tab", "next"):
        assert torch.equal(a.sp[name], b.sp[name]), name
    assert torch.equal(_bits(a.d["logprobs"]), _bits(b.d["logprobs"])) and torch.equal(_bits(a.d["x"]), _bits(b.d["x"]))


# ---- g. arm ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["ngram", "table", "prompt"])
@pytest.mark.parametrize("D", [1, 3, 7])
def test_g_arm(dev, D, source):
    """arm = 1 on the armed state (t = 1, <bos>), logits = None: no token, steps and step[1] stay; tab[i][0 .. D], next and x are written."""
    V, T, n = 65, 12, 4
    cfg = SC.make_cfg(V, n * (D + 1), T, T + 2, E=8)
    st = SR.new_spec_state(cfg, D, T, fill_tok=SC.SENT_TOK, fill_tab=SC.SENT_TOK, fill_next=SC.SENT_TOK, cache=0)
    st.cap[:] = torch.tensor([T, 2, 3, T])
    table = torch.randint(3, V, (n, T), generator=SC.gen(61))
    table[1, 1] = V + 1
    ptok = torch.randint(3, V, (n, T + 1), generator=SC.gen(67))
    kw = dict(ngram=3) if source == "ngram" else dict(drafts=table) if source == "table" else dict(ngram=3, prompt=dict(tok=ptok, len=torch.tensor([0, 1, 5, 99])))
    run = Run(dev, cfg, D, st, **kw)
    r = run.step(None, arm=True)
    assert not bool(r.touched["seqs"].any()) and r.steps.tolist() == [0] * n and r.step == [1, 0] and int(r.finished[cfg.B]) == n
    assert bool(r.touched["x"].all()) and bool(r.touched["tab"][:, :min(D + 1, T)].all()) and r.tab[0, :D + 1].tolist() == list(range(D + 1))
    assert r.next[:, 0].tolist() == [BOS] * n and r.next[1, 1:D + 1].tolist() == [NONE] * D, "cap = 2: every slot would predict index >= cap"
    if source == "ngram":
        assert r.next[0, 1:D + 1].tolist() == [NONE] * D
    if source == "table":
        assert r.next[0, 1:D + 1].tolist() == table[0, 1:D + 1].tolist() and r.next[2, 1:D + 1].tolist() == [int(table[2, 1])] + [NONE] * (D - 1)
    if source == "prompt":
        assert r.next[3, 1:D + 1].tolist() == ptok[3, 1:D + 1].tolist() and r.next[0, 1:D + 1].tolist() == [NONE] * D


def test_g_write_index_clamp(dev):
    """A verify step with step[1] = Tmax - 1: the table entries name cache position Tmax - 1 and step[1] stays."""
    D, V, T = 2, 65, 12
    imgs = _random_images(3, D, 7, T)
    for im in imgs:
        im.cap, im.greedy = T, [5, 6, 7]
    cfg = SC.make_cfg(V, 9, T, T, E=4)
    _, r = _one(dev, cfg, D, imgs, T, (71,), ngram=2, cache=T - 1)
    vals = r.tab[r.touched["tab"]]
    assert r.step == [1, T - 1] and vals.numel() >= 3 and bool((vals // 8 == T - 1).all())


# ---- h. a chained run --------------------------------------------------------------------------------------------------------------------
def test_h_chained_run(dev):
    """3 images, D = 4, ngram = 3, max_len = 200: periodic streams of periods 5, 9 and 70 (the third finds its match only in the second run of
    64 candidate ends), the first ends by <eos> at index 140.  Every step's logits are planted on the host from the reference state, which
    has just been held equal to the device's."""
    D, V, T, ngram = 4, 512, 200, 3
    nxts = [SC.periodic_stream(5, 0, V, eos_at=140), SC.periodic_stream(9, 10, V), SC.periodic_stream(70, 30, V)]
    cfg = SC.make_cfg(V, 3 * (D + 1), T, T + 8, E=4)
    run = Run(dev, cfg, D, SR.new_spec_state(cfg, D, T, fill_tok=SC.SENT_TOK, fill_tab=SC.SENT_TOK, fill_next=SC.SENT_TOK), ngram=ngram)
    r = run.step(None, arm=True)
    second_ballot = 0
    for _ in range(T - 1):
        if int(r.finished[cfg.B]) == 0:
            break
        r = run.step(SC.toy_logits(cfg, D, r, nxts))
        if not int(r.finished[2]):
            hit = SR.ngram_match([int(v) for v in r.seqs[2, :int(r.t[2])]], ngram)
            second_ballot += hit is not None and SC.ballot_of(int(r.t[2]), hit[1]) == 1
    assert int(r.finished[cfg.B]) == 0 and second_ballot > 10
    steps = []
    for i, nxt in enumerate(nxts):
        greedy = SR.greedy_decode(nxt, BOS, EOS, T)
        _, n, _ = SR.speculative_decode(nxt, BOS, EOS, T, D, SR.ngram_source(ngram))
        assert run.d["seqs"][i, :len(greedy)].cpu().tolist() == greedy and int(run.sp["t"][i]) == len(greedy)
        assert int(run.sp["steps"][i]) == n
        steps.append(n)
    assert len(SR.greedy_decode(nxts[0], BOS, EOS, T)) == 141 and steps[2] < 120
    STATS["chain_steps"] = steps


# ---- i. next-input widths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [4, 252, 256, 260, 1024])
def test_i_next_input_widths(dev, E):
    D, V, T = 2, 65, 12
    imgs = _random_images(3, D, 11, T)
    for im in imgs:
        im.cap, im.greedy, im.drafts = T, [5, 6, 7], [5, NONE]
    cfg = SC.make_cfg(V, 9, T, T + 2, E=E)
    _, r = _one(dev, cfg, D, imgs, T, (E,), ngram=2)
    assert bool(r.touched["x"].all())


# ---- j. refusals -------------------------------------------------------------------------------------------------------------------------
_REFUSALS = [
    ("null_seqs", dict(seqs=None)), ("null_logprobs", dict(logprobs=None)), ("null_step", dict(step=None)), ("null_finished", dict(finished=None)),
    ("null_emb", dict(emb=None)), ("null_pos", dict(pos=None)), ("null_x", dict(x=None)), ("null_logits_verify", dict(logits=None)),
    ("B_zero", dict(B=0)), ("V_zero", dict(V=0)), ("E_zero", dict(E=0)), ("max_len_one", dict(max_len=1)), ("max_len_above_Tmax", dict(Tmax=11)),
    ("null_spec", dict(spec=None)), ("null_t", dict(spec=("t", None))), ("null_cap", dict(spec=("cap", None))), ("null_steps", dict(spec=("steps", None))),
    ("null_tab", dict(spec=("tab", None))), ("null_next", dict(spec=("next", None))), ("D_zero", dict(spec=("D", 0))), ("D_eight", dict(spec=("D", 8))),
    ("B_not_multiple", dict(spec=("D", 2))), ("spec_rows", dict(spec=("rows", 1))), ("pitch_below_max_len", dict(spec=("pitch", 11))),
    ("pitch_above_Tmax", dict(spec=("pitch", 15))), ("ngram_zero", dict(spec=("ngram", 0))), ("ngram_nine", dict(spec=("ngram", 9))),
    ("null_prompt_tok", dict(prompt=("tok", None))), ("null_prompt_len", dict(prompt=("len", None))), ("prompt_pitch", dict(prompt=("pitch", 11))),
    ("prompt_rows", dict(prompt=("rows", 1))),
]


@pytest.mark.parametrize("name,change", _REFUSALS, ids=[c[0] for c in _REFUSALS])
def test_j_refusals(dev, name, change):
    """Every condition the entry validates raises with the entry's name in acai_last_error, and nothing is launched: every buffer keeps its
    sentinel.  (The unchanged call is a valid verify step of two images: test_j_the_unchanged_call_is_accepted.)"""
    args, kw, state = _refusal_call(dev)
    for k, v in change.items():
        if k in args:
            args[k] = v
        elif isinstance(v, tuple):
            kw[k] = dict(kw[k] or _refusal_prompt(dev), **{v[0]: v[1]})
        else:
            kw[k] = v
    if args["logits"] is None:
        kw.update(B=8, V=16)
    before = {k: v.clone() for k, v in state.items()}
    with pytest.raises(RuntimeError, match=r"\): acai_debug_decode_spec_accept: "):
        ops.debug_decode_spec_accept(args["logits"], args["seqs"], args["logprobs"], args["step"], args["finished"], **kw)
    torch.cuda.synchronize()
    for k, v in state.items():
        same = torch.equal(_bits(v), _bits(before[k])) if v.dtype == torch.float32 else torch.equal(v, before[k])
        assert same, (k, "a refused call wrote")


def _refusal_prompt(dev):
    return dict(tok=torch.full((2, 12), 5, dtype=torch.int32, device=dev), len=torch.zeros(2, dtype=torch.int32, device=dev))


def _refusal_call(dev):
    B, V, T, E, D = 8, 16, 12, 8, 3
    i32 = lambda *s, v=SC.SENT_TOK: torch.full(s, v, dtype=torch.int32, device=dev)
    nan = lambda *s: torch.full(s, SC.SENT_F32, dtype=torch.int32).view(torch.float32).to(dev)
    seqs = torch.full((2, T), SC.SENT_TOK, dtype=torch.int64, device=dev)
    seqs[:, :2] = torch.tensor([BOS, 5], device=dev)
    nxt = i32(2, 8)
    nxt[:, :4] = torch.tensor([5, NONE, NONE, NONE], dtype=torch.int32, device=dev)
    spec = dict(D=D, ngram=3, t=i32(2, v=2), cap=i32(2, v=T), steps=i32(2, v=0), tab=i32(2, 14), next=nxt)
    args = dict(logits=torch.zeros(B, V, device=dev), seqs=seqs, logprobs=nan(2, T), step=torch.tensor([1, 0], dtype=torch.int32, device=dev),
                finished=torch.zeros(B + 1, dtype=torch.int32, device=dev))
    args["logits"][:, 7] = 2.0
    kw = dict(spec=spec, max_len=T, Tmax=14, eos=EOS, pad=PAD, emb=torch.zeros(V, E, device=dev), pos=torch.zeros(14, E, device=dev), x=nan(B, E),
              prompt=None)
    state = dict(seqs=seqs, logprobs=args["logprobs"], step=args["step"], finished=args["finished"], x=kw["x"], t=spec["t"], steps=spec["steps"],
                 tab=spec["tab"], next=nxt)
    return args, kw, state


@pytest.mark.parametrize("prompted", [False, True], ids=["plain", "prompted"])
def test_j_the_unchanged_call_is_accepted(dev, prompted):
    args, kw, state = _refusal_call(dev)
    if prompted:
        kw["prompt"] = _refusal_prompt(dev)
    ops.debug_decode_spec_accept(args["logits"], args["seqs"], args["logprobs"], args["step"], args["finished"], **kw)
    torch.cuda.synchronize()
    assert state["seqs"][:, 2].tolist() == [7, 7] and state["t"].tolist() == [3, 3] and state["step"].tolist() == [1, 1]
    assert state["finished"].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 2]

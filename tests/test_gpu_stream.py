"""Streamed continuous batching on the GPU: acai_decode_slot_flush through ops.slot_flush, DecodeEngine.continuous(flush=) through
ViTOMR.streamed_continuous_generate, streamed_continuous_inference and streamed_page_inference.

Bars (every one an equality: streaming moves tokens, it computes nothing):
  * the kernel on synthetic slot state: outputs, headers and marks torch.equal to the numpy statement (tests/stream_reference.py), entries
    past a slot's n and the slot state itself untouched, a second call delivers what the first clamped off; refused calls write nothing;
  * end to end: INFERENCE_FINISH payloads equal iter_continuous_inference's tuples, the concatenated STEP tokens / log-probs equal those
    rows' spans bitwise, and the event skeleton equals stream_reference.predict_events fed with the lengths continuous_inference
    returned - with a grammar and with an FP8 memory cache too;
  * a streamed run leaves continuous_inference, inference and a sampled continuous run bitwise as before and adds no graph key;
  * pages: ALL_INFERENCE_FINISH's result equals page_inference's, SYSTEMS_FOUND carries the boxes, STEP names the row's page and system,
    a page set without systems yields three events and encodes nothing."""
import numpy as np
import pytest
import torch

import page_reference as R
from conftest import load_golden
from decode_support import build_vitomr, dev, _memory, _same
from stream_reference import flatten_events, flush_reference, predict_events

pytestmark = pytest.mark.gpu

SENTINEL = -7


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------------------
def _slot_state(B, pitch, ld, rot, finpat, seed):
    """Synthetic slot state of B slots (2 spare rows behind them): per slot end - mark from {0, 1, 63, 64, 65, ld, ld + 3} (rotated by
    `rot`, cut to what the row holds), finished and running rows alternating, marks 1 .. 3."""
    g = np.random.default_rng(seed)
    rows = B + 2
    seqs = g.integers(0, 227, size=(rows, pitch), dtype=np.int64)
    lps = -g.random((rows, pitch), dtype=np.float32) * 9
    diffs = [0, 1, 63, 64, 65, ld, ld + 3]
    t, fin, mark = np.ones(rows, np.int32), np.ones(rows, np.int32), np.full(rows, 2, np.int32)
    for s in range(B):
        f = (s + finpat) % 2
        m = 1 + s % 3
        last = pitch if f else pitch - 1          # a finished row's t is its last index, a running row's the next one to write
        end = min(m + diffs[(s + rot) % 7], last)
        t[s], fin[s], mark[s] = end - f, f, m
    return seqs, lps, t, fin, mark


def _run_flush(dev, state, B, ld):
    """ops.slot_flush on the state with a sentinel-filled buffer -> (its three views and the buffer, the device copies of the state)."""
    from acai_omr_amd import ops
    seqs, lps, t, fin, mark = (torch.from_numpy(a.copy()).to(dev) for a in state)
    buf = torch.full((B * (4 + 2 * ld),), SENTINEL, dtype=torch.int32, device=dev)
    hdr, tok, lp = ops.slot_flush(seqs, lps, t, fin, mark, B, ld, buf)
    return (hdr, tok, lp, buf), (seqs, lps, t, fin, mark)


@pytest.mark.parametrize("ld", [1, 16, 64, 100])
@pytest.mark.parametrize("pitch", [48, 1536])
@pytest.mark.parametrize("B", [1, 5, 17])
def test_flush_kernel_equals_the_numpy_statement(dev, B, pitch, ld):
    from acai_omr_amd import ops
    if ld > pitch:   # ld above the row pitch: a refused call
        state = _slot_state(B, pitch, 16, 0, 0, 1)
        dv = [torch.from_numpy(a.copy()).to(dev) for a in state]
        buf = torch.full((B * (4 + 2 * ld),), SENTINEL, dtype=torch.int32, device=dev)
        with pytest.raises(RuntimeError, match="acai_decode_slot_flush"):
            ops.slot_flush(*dv, B, ld, buf)
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all()) and torch.equal(dv[4].cpu(), torch.from_numpy(state[4]))
        return
    for rot in range(7):          # every slot index meets every end - mark, finished and running
        for finpat in (0, 1):
            state = _slot_state(B, pitch, ld, rot, finpat, 100 * rot + finpat)
            (hdr, tok, lp, buf), dv = _run_flush(dev, state, B, ld)
            sent_i = np.full((B, ld), SENTINEL, np.int32)
            want = flush_reference(*state, B, ld, sent_i, sent_i.copy().view(np.float32), np.full((B, 4), SENTINEL, np.int32))
            assert want is not None
            what = (B, pitch, ld, rot, finpat)
            assert torch.equal(hdr.cpu(), torch.from_numpy(want[2])), what
            assert torch.equal(tok.cpu(), torch.from_numpy(want[0])), what
            assert torch.equal(lp.cpu().view(torch.int32), torch.from_numpy(want[1].view(np.int32))), what   # bitwise, sentinels included
            assert torch.equal(dv[4].cpu(), torch.from_numpy(want[3])), what
            for got, was in zip(dv[:4], state[:4]):   # seqs, logprobs, slot_t, finished: read only
                assert torch.equal(got.cpu(), torch.from_numpy(was)), what
            if rot in (5, 6):   # ld and ld + 3 are among the slots: the second call delivers the remainder on top of the first's buffer
                first = [x.cpu().clone() for x in (tok, lp.view(torch.int32), hdr)]
                ops.slot_flush(*dv, B, ld, buf)
                want2 = flush_reference(*state[:4], want[3], B, ld, first[0].numpy(), first[1].numpy().view(np.float32), first[2].numpy())
                assert torch.equal(hdr.cpu(), torch.from_numpy(want2[2])) and torch.equal(tok.cpu(), torch.from_numpy(want2[0])), what
                assert torch.equal(lp.cpu().view(torch.int32), torch.from_numpy(want2[1].view(np.int32))), what
                assert torch.equal(dv[4].cpu(), torch.from_numpy(want2[3])), what
                s = (6 - rot) % 7
                if s < B and ld + 7 <= pitch:   # the slot with end - mark = ld + 3 is there and uncut: 3 entries were left over
                    assert want[2][s, 0] == ld and want2[2][s].tolist()[:2] == [min(3, ld), want[2][s, 1] + ld], what


def test_flush_parked_slots_emit_nothing(dev):
    """mark equal to end: the parked slot of the engine (finished, t = 1, mark 2) and a running slot whose news was all sent."""
    from acai_omr_amd import ops
    B, pitch, ld = 6, 48, 16
    seqs, lps, t, fin, mark = _slot_state(B, pitch, ld, 0, 0, 3)
    t[:], fin[:], mark[:] = 1, 1, 2
    t[3], fin[3], mark[3] = 9, 0, 9
    (hdr, tok, lp, buf), dv = _run_flush(dev, (seqs, lps, t, fin, mark), B, ld)
    assert hdr.cpu().tolist() == [[0, 2, 1, 0]] * 3 + [[0, 9, 0, 0]] + [[0, 2, 1, 0]] * 2
    assert bool((buf[4 * B:] == SENTINEL).all()) and torch.equal(dv[4].cpu(), torch.from_numpy(mark))


def test_flush_refused_calls_write_nothing(dev):
    from acai_omr_amd import _lib, ops
    B, pitch, ld = 5, 48, 16
    state = _slot_state(B, pitch, ld, 2, 1, 9)

    def fresh():
        return ([torch.from_numpy(a.copy()).to(dev) for a in state],
                torch.full((B * (4 + 2 * ld),), SENTINEL, dtype=torch.int32, device=dev))

    def untouched(dv, buf):
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())
        for got, was in zip(dv, state):
            assert got is None or torch.equal(got.cpu(), torch.from_numpy(was))

    for k in range(5):   # a null operand
        dv, buf = fresh()
        dv[k] = None
        with pytest.raises(RuntimeError, match="null"):
            ops.slot_flush(*dv, B, ld, buf)
        untouched(dv, buf)
    for bad_ld in (0, -3, pitch + 1):
        dv, buf = fresh()
        big = torch.full((B * (4 + 2 * (pitch + 1)),), SENTINEL, dtype=torch.int32, device=dev)
        with pytest.raises(RuntimeError, match="ld"):
            ops.slot_flush(*dv, B, bad_ld, big)
        untouched(dv, big)
    dv, buf = fresh()
    dv[4] = dv[4][:B - 1].contiguous()   # rows < B
    with pytest.raises(RuntimeError, match="rows"):
        ops.slot_flush(*dv, B, ld, buf)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    # the output pointers, through the C ABI itself
    dv, buf = fresh()
    hdr, tok, lp = ops.slot_flush_views(buf, B, ld)
    L, st = _lib.lib(), ops._st()
    ptr = [x.data_ptr() for x in dv]
    for outs in ((None, lp.data_ptr(), hdr.data_ptr()), (tok.data_ptr(), None, hdr.data_ptr()), (tok.data_ptr(), lp.data_ptr(), None)):
        assert L.acai_decode_slot_flush(ptr[0], ptr[1], pitch, ptr[2], ptr[3], ptr[4], B + 2, B, ld, *outs, st) != 0
        assert b"null" in L.acai_last_error()
    untouched(dv, buf)
    assert L.acai_decode_slot_flush(ptr[0], ptr[1], pitch, ptr[2], ptr[3], ptr[4], B + 2, 0, ld, tok.data_ptr(), lp.data_ptr(), hdr.data_ptr(), st) != 0
    untouched(dv, buf)


# ---- 2. end to end -------------------------------------------------------------------------------------------------------------------------
_MODELS = {}
CACHE_LEN = 32   # the fixtures' positional tables have 24 rows and flush_interval 25 is one of the cases: the caches are built 32 long


def _model(name, cdt, dev, fp8=False):
    """(model, the fixture's images three times over, per-image caps mixing 0, 1, 2, 5 and the fixture's max_len), built once.  The
    decoder's cache is CACHE_LEN long - the positional table padded with zero rows that no cap reaches - so that a flush interval above
    every cap is still one the cache admits; every row decodes as in the fixture's own model."""
    key = (name, cdt, fp8)
    if key not in _MODELS:
        fx = load_golden(name)
        imgs = list(fx["imgs"]) * 3
        T = fx["cfg"]["max_len"]
        caps = [[T, 0, 5, 1, T, 2, 5, T, 2][k % 9] for k in range(len(imgs))]
        sd, pe = dict(fx["state_dict"]), fx["state_dict"]["decoder.pos_embedding"]
        sd["decoder.pos_embedding"] = torch.cat([pe, pe.new_zeros(CACHE_LEN - T, pe.shape[1])])
        m = build_vitomr(dict(fx["cfg"], max_len=CACHE_LEN), sd, dev, cdt, max_batch=len(imgs) + 1,
                         memory_cache_dtype=torch.float8_e4m3fn if fp8 else None)
        _MODELS[key] = (m, imgs, caps)
    return _MODELS[key]


def _types():
    from acai_omr_amd.config import InferenceEvent
    return InferenceEvent


def _check_stream(events, ref, caps, slots, F, tagged=None):
    """events: the STEP / INFERENCE_FINISH part of a streamed run; ref: {image: (seqs, log_probs, mask)} as iter_continuous_inference
    yields them.  The three end-to-end bars of the module docstring; tagged: per image the (page, system) its payloads must carry."""
    E = _types()
    lengths = [max(int(ref[i][2].sum()) - 1, 0) for i in range(len(caps))]
    skeleton, chunks, finished = [], {i: [] for i in range(len(caps))}, []
    for ev in events:
        p = ev["payload"]
        i = p["image"]
        if tagged is not None:
            assert (p["page"], p["system"]) == tagged[i]
        if ev["type"] == E.STEP.value:
            tok, lp = p["tokens"], p["log_probs"]
            assert tok.dtype == torch.int32 and lp.dtype == torch.float32 and not tok.is_cuda and not lp.is_cuda
            assert tok.dim() == 2 and tok.shape[0] == 1 and tok.shape == lp.shape and i not in finished
            skeleton.append(("step", i, p["start"], tok.shape[1]))
            chunks[i].append((tok, lp))
        else:
            assert ev["type"] == E.INFERENCE_FINISH.value
            skeleton.append(("finish", i))
            finished.append(i)
            _same((p["sequence"], p["log_probs"], p["mask"]), ref[i])
    assert skeleton == flatten_events(predict_events(lengths, caps, slots, F)), (slots, F)
    for i, L in enumerate(lengths):
        seq, lps, _ = ref[i]
        if L == 0:
            assert not chunks[i]
            continue
        tok, lp = torch.cat([c[0] for c in chunks[i]], dim=1), torch.cat([c[1] for c in chunks[i]], dim=1)
        assert torch.equal(tok, seq[:, 1:1 + L].cpu().to(torch.int32)) and torch.equal(lp, lps[:, 1:1 + L].cpu()), (i, slots, F)


def _streamed(m, imgs, caps, slots, F, **kw):
    """The whole event list of streamed_continuous_inference, its frame checked -> the STEP / INFERENCE_FINISH part."""
    from acai_omr_amd.inference.vitomr_inference import streamed_continuous_inference
    E = _types()
    ev = list(streamed_continuous_inference(m, imgs, "cuda", max_inference_len=caps, slots=slots, flush_interval=F, **kw))
    assert ev[0] == {"type": E.ENCODING_START.value, "payload": None} and ev[-1] == {"type": E.ALL_INFERENCE_FINISH.value, "payload": None}
    assert ev[1] == {"type": E.ENCODING_FINISH.value, "payload": {"images": len(imgs)}}
    return ev[2:-1]


def _reference(m, imgs, caps, slots, **kw):
    from acai_omr_amd.inference.vitomr_inference import iter_continuous_inference
    return {i: (s, l, k) for i, s, l, k in iter_continuous_inference(m, imgs, "cuda", max_inference_len=caps, slots=slots, **kw)}


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["vitomr_dh64b", "vitomr_small"])
def test_streamed_continuous_inference(dev, name, cdt):
    """bf16: the inference entry points (they decode a bf16 memory).  fp32: ViTOMR.streamed_continuous_generate on the fp32 memories
    against _continuous_packed_iter, the generator iter_continuous_inference wraps."""
    from acai_omr_amd import engine as EG
    m, imgs, caps = _model(name, cdt, dev)
    N, bf = len(imgs), cdt == torch.bfloat16
    lat, mask = _memory(m, imgs, bf)
    mem32, lens = EG.unpad_rows(lat, mask)
    for slots in (1, 2, N + 1):
        if bf:
            ref = _reference(m, imgs, caps, slots)
        else:
            with torch.no_grad():
                ref = {i: (s, l, k) for i, s, l, k in m._continuous_packed_iter(mem32, None, lens, caps, slots)}
        assert sorted(ref) == list(range(N))
        for F in (1, 5, 25):
            if bf:
                ev = _streamed(m, imgs, caps, slots, F)
            else:
                with torch.no_grad():
                    ev = list(m.streamed_continuous_generate(lat, mask, max_len=caps, slots=slots, flush_interval=F))
            _check_stream(ev, ref, caps, slots, F)
    # the model-level generator with one cap for all, against cached_continuous_generate's batch
    T = max(caps)
    with torch.no_grad():
        ev = list(m.streamed_continuous_generate(lat, mask, max_len=T, slots=2, flush_interval=5))
        seqs, lps, _ = m.cached_continuous_generate(lat, mask, max_len=T, slots=2)
    ref = {i: m._mask_and_clip_capped(seqs[i:i + 1], lps[i:i + 1], [T]) for i in range(N)}   # each row clipped to its own length
    _check_stream(ev, ref, [T] * N, 2, 5)


def test_streamed_with_a_grammar(dev):
    """The restrictive automaton of tests/test_gpu_grammar.py's pattern, cut from this model's own plain greedy rows."""
    import test_gpu_grammar as TG
    m, imgs, caps = _model("vitomr_dh64b", torch.bfloat16, dev)
    T = load_golden("vitomr_dh64b")["cfg"]["gen_len"]
    lat, mask = _memory(m, imgs[:len(imgs) // 3], True)
    a, _ = TG._restrictive(m, TG._greedy(m, lat, mask, T, True))
    plain = _reference(m, imgs, caps, 2)
    ref = _reference(m, imgs, caps, 2, grammar=a)
    assert any(int(ref[i][0][0, 1]) != int(plain[i][0][0, 1]) for i in ref if caps[i] >= 2)   # the constraint binds
    for F in (1, 5):
        _check_stream(_streamed(m, imgs, caps, 2, F, grammar=a), ref, caps, 2, F)


def test_streamed_with_an_fp8_memory_cache(dev):
    m, imgs, caps = _model("vitomr_small", torch.bfloat16, dev, fp8=True)
    assert m.decoder.decoder_blocks.engine(dev).cross_fp8
    ref = _reference(m, imgs, caps, 2)
    for F in (1, 5):
        _check_stream(_streamed(m, imgs, caps, 2, F), ref, caps, 2, F)


def test_a_streamed_run_leaves_the_other_modes_alone(dev):
    from acai_omr_amd import engine as EG
    from acai_omr_amd.inference.vitomr_inference import continuous_inference, inference
    m, imgs, caps = _model("vitomr_dh64b", torch.bfloat16, dev)
    n = len(imgs) // 3
    T = max(caps)
    lat, mask = _memory(m, imgs, True)
    mem32, lens = EG.unpad_rows(lat.float(), mask)
    U = torch.rand(len(imgs), T, generator=torch.Generator().manual_seed(4)).to(dev)

    def others():
        with torch.no_grad():
            sampled = m._continuous_packed(mem32, None, lens, T, 2, sample=(5, 1.3), uniforms=U)
        return continuous_inference(m, imgs, "cuda", max_inference_len=caps, slots=2) + inference(m, imgs[:n], "cuda", max_inference_len=T) + sampled

    before = others()
    eng = m.decoder.decoder_blocks.engine(dev)
    keys = set(eng.graphs)
    assert any(k[4] == ("slot",) for k in keys)
    for F in (1, 5, 25):
        _streamed(m, imgs, caps, 2, F)
    assert set(eng.graphs) == keys          # streaming replays the slot graphs that were there
    assert eng._mode == ("greedy",) and eng._flush_ld == 0
    _same(others(), before)
    assert set(eng.graphs) == keys


def test_streamed_value_errors(dev):
    from acai_omr_amd.inference.vitomr_inference import streamed_continuous_inference, streamed_page_inference
    from acai_omr_amd.utils import DynamicResize
    m, imgs, caps = _model("vitomr_dh64b", torch.bfloat16, dev)
    Tmax = CACHE_LEN
    lat, mask = _memory(m, imgs, True)
    tr = DynamicResize(16, 32, 4, 8, True)
    page = torch.from_numpy(R.synthetic_page()[0])
    for bad in (0, -1, 2.5, "5", None, True, Tmax + 1):   # at the call: no event has been asked for
        with pytest.raises(ValueError, match="flush_interval"):
            streamed_continuous_inference(m, imgs, "cuda", max_inference_len=caps, slots=2, flush_interval=bad)
        with pytest.raises(ValueError, match="flush_interval"):
            m.streamed_continuous_generate(lat, mask, max_len=max(caps), slots=2, flush_interval=bad)
        with pytest.raises(ValueError, match="flush_interval"):
            streamed_page_inference(m, page, "cuda", tr, boxes=[(14, 37, 191, 74)], max_inference_len=12, flush_interval=bad)
    assert next(streamed_continuous_inference(m, imgs, "cuda", max_inference_len=caps, slots=2, flush_interval=Tmax))["payload"] is None
    eng = m.decoder.decoder_blocks.engine(dev)
    with pytest.raises(ValueError, match="sample"):   # rollouts have no consumer for a stream
        eng.continuous(lat.float()[0], None, [lat.shape[1]], [5], 1, sample=(5, 1.0), flush=4)
    with pytest.raises(ValueError, match="flush"):
        eng.continuous(lat.float()[0], None, [lat.shape[1]], [5], 1, flush=0)
    with pytest.raises(TypeError, match="TokenAutomaton"):
        streamed_continuous_inference(m, imgs, "cuda", max_inference_len=caps, flush_interval=5, grammar="lmx")


# ---- 3. pages ------------------------------------------------------------------------------------------------------------------------------
TRUTH = [(14, 37, 191, 74), (14, 107, 191, 123), (14, 167, 191, 204)]
DETECT = dict(min_ink=1, merge_gap=4, min_height=8, line_len=100, min_line_rows=5, margin=0)


@pytest.fixture(scope="module")
def pages(dev):
    from acai_omr_amd.utils import DynamicResize
    fx = load_golden("vitomr_dh64b")
    cfg = fx["cfg"]
    assert (cfg["P"], cfg["pe_h"], cfg["pe_w"]) == (16, 4, 8)
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.bfloat16, max_batch=2)   # 2 slots: the third system is a refill
    return m, DynamicResize(16, 32, 4, 8, True), torch.from_numpy(R.synthetic_page()[0]).float() / 255.0


def _page_events(m, pages_in, tr, F=5, **kw):
    """streamed_page_inference against page_inference on the same arguments: the frame, the layout, the rows and the stream."""
    from acai_omr_amd.inference.vitomr_inference import page_inference, streamed_page_inference
    E = _types()
    want = page_inference(m, pages_in, "cuda", tr, max_inference_len=12, **kw)
    ev = list(streamed_page_inference(m, pages_in, "cuda", tr, max_inference_len=12, flush_interval=F, **kw))
    assert [e["type"] for e in ev[:3]] == [E.ENCODING_START.value, E.SYSTEMS_FOUND.value, E.ENCODING_FINISH.value]
    assert ev[0]["payload"] is None and ev[2]["payload"] == {"images": len(want)} and ev[-1]["type"] == E.ALL_INFERENCE_FINISH.value
    layout, res = ev[1]["payload"]["layout"], ev[-1]["payload"]["result"]
    assert layout.seqs is None and layout.log_probs is None and layout.seq_mask is None
    for r in (layout, res):   # the geometry and the stage reports: the layout has them before anything is encoded
        assert r.boxes == want.boxes and r.angles == want.angles and r.quads == want.quads and r.orientations == want.orientations
        assert r.system_page == want.system_page and r.sizes == want.sizes and r.windows == want.windows and len(r) == len(want)
        assert r.page_sizes == want.page_sizes and r.source_sizes == want.source_sizes and r.flattened == want.flattened
        assert r.quality == want.quality and r.system_staff_space == want.system_staff_space
        for s in range(len(want)):
            assert r.box_corners(s) == want.box_corners(s) and r.to_page_xy(s, 3.0, 2.0) == want.to_page_xy(s, 3.0, 2.0)
    assert torch.equal(res.seqs, want.seqs) and torch.equal(res.log_probs, want.log_probs) and torch.equal(res.seq_mask, want.seq_mask)
    assert res.patches_kept == want.patches_kept and res.patches_total == want.patches_total
    ref = {i: m._mask_and_clip_capped(want.seqs[i:i + 1, :12], want.log_probs[i:i + 1, :12], [12]) for i in range(len(want))}
    tagged = [(p, want.system_page[:i].count(p)) for i, p in enumerate(want.system_page)]
    _check_stream(ev[3:-1], ref, [12] * len(want), 2, F, tagged)
    return want, ev


def test_streamed_page_inference_with_boxes(dev, pages):
    m, tr, page = pages
    want, _ = _page_events(m, page, tr, boxes=TRUTH)
    assert want.boxes == [TRUTH] and len(want) == 3
    _page_events(m, page, tr, F=1, boxes=TRUTH)


def test_streamed_page_inference_detects(dev, pages):
    from acai_omr_amd.page import DetectConfig
    m, tr, page = pages
    cfg = DetectConfig(0.5, DETECT["min_ink"], DETECT["merge_gap"], DETECT["min_height"], 0.5, DETECT["min_line_rows"], DETECT["margin"], 64)
    want, ev = _page_events(m, [page, torch.ones(100, 120), page], tr, detect=cfg)
    assert want.boxes == [TRUTH, [], TRUTH] and want.system_page == [0, 0, 0, 2, 2, 2]
    steps = [e["payload"] for e in ev if e["type"] == _types().STEP.value]
    assert {(p["image"], p["page"], p["system"]) for p in steps} == {(0, 0, 0), (1, 0, 1), (2, 0, 2), (3, 2, 0), (4, 2, 1), (5, 2, 2)}


def test_streamed_page_inference_with_deskew_and_assess(dev, pages):
    m, tr, page = pages
    want, _ = _page_events(m, page, tr, boxes=TRUTH, deskew=True, assess=True)
    assert len(want) == 3 and want.quality[0] is not None


def test_streamed_page_inference_without_systems(dev, pages, monkeypatch):
    from acai_omr_amd.inference import vitomr_inference as VI
    from acai_omr_amd.page import DetectConfig
    m, tr, _ = pages
    E = _types()
    cfg = DetectConfig(0.5, DETECT["min_ink"], DETECT["merge_gap"], DETECT["min_height"], 0.5, DETECT["min_line_rows"], DETECT["margin"], 64)
    blank = torch.ones(100, 120)

    def never(*a, **k):
        raise AssertionError("a page set without systems must not be split or encoded")
    monkeypatch.setattr(VI, "_encode_chunks", never)
    monkeypatch.setattr(VI, "_page_encode", never)
    for kw in (dict(detect=cfg), dict(boxes=[[], []])):
        ev = list(VI.streamed_page_inference(m, [blank, blank], "cuda", tr, max_inference_len=12, flush_interval=5, **kw))
        assert [e["type"] for e in ev] == [E.ENCODING_START.value, E.SYSTEMS_FOUND.value, E.ALL_INFERENCE_FINISH.value]
        res = ev[-1]["payload"]["result"]
        assert len(res) == 0 and res.boxes == [[], []] and res.seqs is None and len(ev[1]["payload"]["layout"]) == 0

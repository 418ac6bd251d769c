"""Pipelined decode stepping (LLMEngine.step_pipelined / drain) must hand
every stream exactly the tokens and the finish reason of the synchronous
step() loop.  CPU: torch_ref twin of decode_advance + eager forward, the
same bookkeeping as on the GPU."""

import numpy as np
import pytest
import torch

from hyperspot import ops
from hyperspot.engine import EngineConfig, LLMEngine, SamplingParams

PROMPTS = [[(7 * i + 3 * j + 1) % 500 + 4 for j in range(12 + i)]
           for i in range(6)]          # 12..17 tokens: pages are crossed early


def _engine(pipeline=True, **kw):
    kw.setdefault("num_gpu_blocks", 128)
    cfg = EngineConfig(model="tiny-llama", max_num_seqs=8,
                       max_num_batched_tokens=512, max_model_len=256,
                       pipeline_decode=pipeline, **kw)
    return LLMEngine(cfg)


def _run(eng, pipelined, reqs, late=None, abort=None, expect_inflight=None):
    """reqs: [(rid, prompt, sampling)].  late: (call_no, [(rid, prompt,
    sampling)]) added before that call.  abort: (rid, n_tokens): abort rid
    once it has n_tokens.  Returns {rid: (tokens, finish_reason)}."""
    if expect_inflight is None:
        expect_inflight = pipelined and eng.config.pipeline_decode
    streams = {}
    for rid, p, sp in reqs:
        eng.add_request(p, sp, request_id=rid)
        streams[rid] = [[], None]
    step = eng.step_pipelined if pipelined else eng.step
    calls = 0
    aborted = False
    saw_inflight = False
    while eng.has_work():
        if late is not None and calls == late[0]:
            for rid, p, sp in late[1]:
                eng.add_request(p, sp, request_id=rid)
                streams[rid] = [[], None]
        for o in step():
            s = streams[o.request_id]
            assert s[1] is None, "output after finish"
            s[0].append(o.token_id)
            if o.finished:
                s[1] = o.finish_reason
        saw_inflight |= eng._inflight is not None
        if abort is not None and not aborted \
                and len(streams[abort[0]][0]) >= abort[1]:
            if pipelined:
                assert eng._inflight is not None   # a step IS in flight
            eng.abort_request(abort[0])
            aborted = True
        calls += 1
        assert calls < 2000
    if expect_inflight:
        assert saw_inflight, "the pipelined path never engaged"
    assert eng.drain() == []
    return {k: (v[0], v[1]) for k, v in streams.items()}


def _both(reqs, **kw):
    eng_kw = kw.pop("eng_kw", {})
    sync_eng = _engine(**eng_kw)
    free0 = sync_eng.runner.block_manager.num_free
    ref = _run(sync_eng, False, reqs, **kw)
    assert sync_eng.runner.block_manager.num_free == free0
    pipe_eng = _engine(**eng_kw)
    got = _run(pipe_eng, True, reqs, **kw)
    # (g) no page leaked, none left behind a deferred free
    assert pipe_eng.runner.block_manager.num_free == free0
    assert not pipe_eng.runner.block_manager.row_of
    return ref, got


def _greedy(n, **kw):
    return SamplingParams(temperature=0.0, max_tokens=n, **kw)


def test_staggered_max_tokens():
    reqs = [(f"r{i}", p, _greedy(3 + 7 * i)) for i, p in enumerate(PROMPTS)]
    ref, got = _both(reqs)
    assert got == ref
    assert [len(ref[f"r{i}"][0]) for i in range(6)] == \
        [3 + 7 * i for i in range(6)]


def test_stop_tokens_mid_run():
    sp = _greedy(40, ignore_eos=True)
    base = _run(_engine(), False,
                [(f"r{i}", p, sp) for i, p in enumerate(PROMPTS)])
    # stop ids taken from what rows 0..2 are seen to emit mid-run
    reqs = []
    for i, p in enumerate(PROMPTS):
        stops = (base[f"r{i}"][0][5 + 4 * i],) if i < 3 else ()
        reqs.append((f"r{i}", p, _greedy(40, stop_token_ids=stops)))
    ref, got = _both(reqs)
    assert got == ref
    reasons = [ref[f"r{i}"][1].value for i in range(6)]
    assert "stop" in reasons and "length" in reasons
    assert any(len(ref[f"r{i}"][0]) < 40 for i in range(3))


def test_requests_arriving_mid_decode():
    reqs = [(f"r{i}", p, _greedy(20)) for i, p in enumerate(PROMPTS[:3])]
    late = (6, [(f"l{i}", p, _greedy(15))
                for i, p in enumerate(PROMPTS[3:])])
    ref, got = _both(reqs, late=late)
    assert got == ref
    assert all(len(got[f"l{i}"][0]) == 15 for i in range(3))


def test_abort_while_step_in_flight():
    reqs = [(f"r{i}", p, _greedy(30)) for i, p in enumerate(PROMPTS[:4])]
    full = _run(_engine(), False, reqs)
    pipe_eng = _engine()
    free0 = pipe_eng.runner.block_manager.num_free
    got = _run(pipe_eng, True, reqs, abort=("r1", 9))
    assert pipe_eng.runner.block_manager.num_free == free0
    for rid in ("r0", "r2", "r3"):
        assert got[rid] == full[rid]
    toks, reason = got["r1"]
    assert reason is None and 9 <= len(toks) < 30
    assert toks == full["r1"][0][:len(toks)]


def test_small_pool_forces_preemption():
    reqs = [("a", list(range(1, 31)), _greedy(40)),
            ("b", list(range(40, 70)), _greedy(40))]
    ref, got = _both(reqs, eng_kw={"num_gpu_blocks": 9})
    assert got == ref
    big = _run(_engine(), True, reqs)
    assert big["a"][0][-10:] == got["a"][0][-10:]


def test_guided_and_stochastic_rows_fall_back():
    reqs = [("g", PROMPTS[0], _greedy(12, response_format="json")),
            ("t", PROMPTS[1], SamplingParams(temperature=0.8, max_tokens=12,
                                             seed=5)),
            ("p", PROMPTS[2], _greedy(12))]
    sync_eng = _engine()
    ref = _run(sync_eng, False, reqs)
    got = _run(_engine(), True, reqs, expect_inflight=False)
    assert got == ref
    # once only greedy, unguided rows are left the fast path takes over
    reqs2 = [("g", PROMPTS[0], _greedy(4, response_format="json")),
             ("p", PROMPTS[2], _greedy(30))]
    ref2, got2 = _both(reqs2)
    assert got2 == ref2


def test_switch_off_is_the_synchronous_loop():
    reqs = [(f"r{i}", p, _greedy(9)) for i, p in enumerate(PROMPTS[:3])]
    eng = _engine(pipeline=False)
    got = _run(eng, True, reqs)
    assert got == _run(_engine(), False, reqs)


def test_step_after_pipelined_step_drains_first():
    eng = _engine()
    eng.add_request(PROMPTS[0], _greedy(8), request_id="x")
    toks = []
    toks += [o.token_id for o in eng.step_pipelined()]     # prefill
    toks += [o.token_id for o in eng.step_pipelined()]     # fills the pipe
    assert eng._inflight is not None and eng.has_work()
    while eng.has_work():
        toks += [o.token_id for o in eng.step()]
    ref = _engine().generate([PROMPTS[0]], _greedy(8))[0]
    assert toks == ref


# ---- decode_advance reference semantics vs a plain numpy recomputation ----

def _np_advance(ids, pos, lens, slots, bt, sampled, ctl, page):
    rows = len(ids)
    n_live = ctl[4 * rows]
    if n_live < 0:
        return
    src, nb, hid, hpos = (ctl[k * rows:(k + 1) * rows] for k in range(4))
    for r in range(rows):
        if r >= n_live or src[r] < -1 or src[r] >= rows:
            ids[r], pos[r], lens[r], slots[r] = 0, 0, 1, -1
            continue
        if src[r] >= 0:
            ids[r], p = sampled[src[r]], pos[r] + 1
        else:
            ids[r], p = hid[r], hpos[r]
        pos[r], lens[r] = p, p + 1
        if p // page >= bt.shape[1]:
            slots[r] = -1
            continue
        if nb[r] >= 0:
            bt[r, p // page] = nb[r]
        slots[r] = bt[r, p // page] * page + p % page


def test_decode_advance_ref_matches_numpy():
    rng = np.random.default_rng(0)
    rows, max_blocks, page = 8, 4, 16
    ids = rng.integers(0, 500, rows)
    pos = np.array([13, 14, 15, 30, 7, 62, 0, 0])
    lens = (pos + 1).astype(np.int32)
    slots = rng.integers(0, 99, rows)
    bt = rng.integers(0, 64, (rows, max_blocks)).astype(np.int32)
    sampled = rng.integers(0, 500, rows)
    ctl = np.full(4 * rows + 4, -1, dtype=np.int32)
    ctl[:rows] = [3, 0, 1, 2, -1, 4, -2, -2]            # permuted gather
    ctl[rows:2 * rows] = [-1, -1, 41, -1, -1, -1, -1, -1]   # pos 16: install
    ctl[2 * rows + 4] = 77
    ctl[3 * rows + 4] = 0                                # host row at pos 0
    ctl[4 * rows] = 6
    t = [torch.from_numpy(a.copy()) for a in
         (ids, pos, lens, slots, bt, sampled, ctl)]
    ops.decode_advance(*t, page)
    _np_advance(ids, pos, lens, slots, bt, sampled, ctl, page)
    for a, b in zip(t[:5], (ids, pos, lens, slots, bt)):
        assert np.array_equal(a.numpy(), b)
    assert slots[2] == 41 * 16 and bt[2, 1] == 41      # page start, installed
    assert slots[5] == bt[5, 3] * 16 + 15              # last table column
    assert list(slots[6:]) == [-1, -1] and list(lens[6:]) == [1, 1]
    # pass-through leaves everything alone
    before = [a.clone() for a in t[:5]]
    t[6][4 * rows] = -1
    ops.decode_advance(*t, page)
    for a, b in zip(t[:5], before):
        assert torch.equal(a, b)

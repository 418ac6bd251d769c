"""JSON-mode rows in the pipelined decode (EngineConfig.device_guided): with
the flag on, step_pipelined() keeps a batch with JSON rows on the fast path
and hands every stream the tokens, finish reason and logprob records of the
synchronous step() loop; with the flag off, and for schema and tool-call
rows either way, it falls back.  CPU: torch twins of the two guided kernels
and the eager forward, the same bookkeeping as on the GPU."""

import json

import pytest

from hyperspot.engine import EngineConfig, LLMEngine, SamplingParams
from hyperspot.engine.guided import JsonByteMachine

PROMPTS = [[(7 * i + 3 * j + 1) % 500 + 4 for j in range(12 + i)]
           for i in range(8)]          # 12..19 tokens: pages are crossed early
EOS = 2


def _engine(**kw):
    kw.setdefault("num_gpu_blocks", 128)
    cfg = EngineConfig(model="tiny-llama", max_num_seqs=8,
                       max_num_batched_tokens=512, max_model_len=256, **kw)
    return LLMEngine(cfg, eos_token_id=EOS)


def _run(eng, pipelined, reqs, late=None, abort=None, expect_inflight=None):
    """reqs: [(rid, prompt, sampling)].  late: (call_no, more reqs) added
    before that call.  abort: (rid, n_tokens).  Returns ({rid: (tokens,
    finish_reason, records)}, {rid: Request})."""
    if expect_inflight is None:
        expect_inflight = pipelined
    streams, handles = {}, {}

    def add(rid, p, sp):
        eng.add_request(p, sp, request_id=rid)
        handles[rid] = eng.scheduler.waiting[-1]
        assert handles[rid].request_id == rid
        streams[rid] = [[], None, []]

    for r in reqs:
        add(*r)
    step = eng.step_pipelined if pipelined else eng.step
    calls = 0
    aborted = False
    saw_inflight = False
    while eng.has_work():
        if late is not None and calls == late[0]:
            for r in late[1]:
                add(*r)
        for o in step():
            s = streams[o.request_id]
            assert s[1] is None, "output after finish"
            s[0].append(o.token_id)
            s[2].append(None if o.logprobs is None else
                        (o.logprobs.token_id, o.logprobs.logprob,
                         o.logprobs.top))
            if o.finished:
                s[1] = o.finish_reason.value
        saw_inflight |= eng._inflight is not None
        if abort is not None and not aborted \
                and len(streams[abort[0]][0]) >= abort[1]:
            if pipelined:
                assert eng._inflight is not None   # a step IS in flight
            eng.abort_request(abort[0])
            aborted = True
        calls += 1
        assert calls < 2000
    assert saw_inflight == expect_inflight, \
        "the pipelined path " + ("never engaged" if expect_inflight
                                 else "engaged")
    assert eng.drain() == []
    return {k: tuple(v) for k, v in streams.items()}, handles


def _both(reqs, eng_kw=None, **kw):
    eng_kw = dict(eng_kw or {})
    sync_eng = _engine(**eng_kw)
    free0 = sync_eng.runner.block_manager.num_free
    ref, _ = _run(sync_eng, False, reqs, **kw)
    assert sync_eng.runner.block_manager.num_free == free0
    pipe_eng = _engine(**eng_kw)
    got, handles = _run(pipe_eng, True, reqs, **kw)
    assert pipe_eng.runner.block_manager.num_free == free0    # no page leaked
    assert not pipe_eng.runner.block_manager.row_of
    return ref, got, handles


def _check_json(stream, whole=True):
    """The stream is a prefix of valid JSON (it feeds a fresh machine), and
    one that stopped by itself is a whole document."""
    toks, reason, _ = stream
    m = JsonByteMachine()
    for t in toks:
        assert t == EOS or 4 <= t < 260, t
        m.feed_token(t)                    # ValueError = a masked byte
    if reason == "stop" and whole:
        assert toks[-1] == EOS and m.done
        json.loads(bytes(t - 4 for t in toks[:-1]).decode("utf-8", "replace"))
    return m


def _mixed(n_json=4, n_plain=3, max_tokens=40, **kw):
    """JSON rows and plain rows interleaved; every other JSON row may not
    stop at EOS, so it runs to max_tokens behind the closed document."""
    reqs = []
    kinds = []
    for k in range(max(n_json, n_plain)):
        kinds += [True] * (k < n_json) + [False] * (k < n_plain)
    for i, is_json in enumerate(kinds):
        extra = dict(kw)
        if is_json:
            extra.update(response_format="json", ignore_eos=i % 4 == 2)
        extra.setdefault("temperature", 0.0)
        reqs.append((("j" if is_json else "p") + str(i), PROMPTS[i % 8],
                     SamplingParams(max_tokens=max_tokens - 3 * i, **extra)))
    return reqs


def _json_ids(reqs):
    return [rid for rid, _, sp in reqs if sp.response_format == "json"]


def test_mixed_batch_stays_pipelined_and_equals_step():
    reqs = _mixed()
    assert len(_json_ids(reqs)) == 4
    ref, got, _ = _both(reqs, eng_kw={"device_guided": True})
    assert got == ref
    reasons = set()
    for rid in _json_ids(reqs):
        _check_json(got[rid])
        reasons.add(got[rid][1])
    # some document closed and stopped by itself, some row ran out of tokens
    assert reasons == {"stop", "length"}
    # the plain rows are what they are without any JSON row in the batch
    alone, _ = _run(_engine(), True,
                    [r for r in reqs if r[0] not in _json_ids(reqs)])
    for rid, s in alone.items():
        assert got[rid] == s


def test_flag_off_never_engages_while_a_json_row_runs():
    """The parent's behaviour, and the test that fails without the feature:
    the same batch, equal lengths so that a JSON row runs to the last step."""
    reqs = [(rid, p, SamplingParams(
        temperature=0.0, max_tokens=24, response_format=sp.response_format,
        ignore_eos=True)) for rid, p, sp in _mixed()]
    off, _ = _run(_engine(), True, reqs, expect_inflight=False)
    on, _ = _run(_engine(device_guided=True), True, reqs, expect_inflight=True)
    ref, _ = _run(_engine(), False, reqs)
    assert off == ref and on == ref
    for rid in _json_ids(reqs):
        _check_json(on[rid])


@pytest.mark.parametrize("flags,extra", [
    (dict(device_penalties=True, max_penalty_seqs=8),
     dict(frequency_penalty=1.2, repetition_penalty=1.3)),
    (dict(device_sampling=True), dict(temperature=0.9, top_k=30, seed=11)),
    (dict(device_logprobs=True), dict(logprobs=5)),
    (dict(device_penalties=True, max_penalty_seqs=8, device_sampling=True,
          device_logprobs=True),
     dict(presence_penalty=0.8, temperature=0.7, top_p=0.9, seed=3,
          logprobs=2)),
])
def test_with_the_other_device_flags(flags, extra):
    # equal max_tokens and no stops: both loops run the same batch shapes at
    # every step, so the records' floats agree exactly (a row that stops is
    # seen one step late by the pipelined loop, whose last batches are then
    # one row larger, and the CPU GEMM rounds by shape)
    reqs = [(rid, p, SamplingParams(**dict(
        extra, max_tokens=24, ignore_eos=True,
        temperature=sp.temperature, response_format=sp.response_format)))
        for rid, p, sp in _mixed(**extra)]
    ref, got, _ = _both(reqs, eng_kw=dict(device_guided=True, **flags))
    assert got == ref                       # tokens, reasons and records
    for rid in _json_ids(reqs):
        _check_json(got[rid])
        if "logprobs" in extra:
            # a record describes the masked logits: the chosen token has a
            # finite logprob and no alternative lies outside the grammar
            m = JsonByteMachine()
            for (tid, lp, top), t in zip(got[rid][2], got[rid][0]):
                ok, eos = m.allowed()
                legal = {b + 4 for b in ok} | ({EOS} if eos else set())
                assert tid == t and lp > float("-inf")
                assert {i for i, _ in top} <= legal
                m.feed_token(t)


def test_late_arrival():
    reqs = _mixed(n_json=2, n_plain=2, max_tokens=30)
    late = (6, [("jl", PROMPTS[5], SamplingParams(
                    temperature=0.0, max_tokens=18, response_format="json")),
                ("pl", PROMPTS[6], SamplingParams(temperature=0.0,
                                                  max_tokens=15))])
    ref, got, _ = _both(reqs, eng_kw={"device_guided": True}, late=late)
    assert got == ref
    for rid in _json_ids(reqs) + ["jl"]:
        _check_json(got[rid])


def test_abort_while_a_step_is_in_flight():
    reqs = [(rid, p, SamplingParams(
        temperature=0.0, max_tokens=30, ignore_eos=True,
        response_format=sp.response_format))
        for rid, p, sp in _mixed(n_json=2, n_plain=2)]
    victim = _json_ids(reqs)[0]
    full, _ = _run(_engine(device_guided=True), False, reqs)
    eng = _engine(device_guided=True)
    free0 = eng.runner.block_manager.num_free
    got, _ = _run(eng, True, reqs, abort=(victim, 9))
    assert eng.runner.block_manager.num_free == free0
    for rid in got:
        if rid != victim:
            assert got[rid] == full[rid]
    toks, reason, _ = got[victim]
    assert reason is None and 9 <= len(toks) < 30
    assert toks == full[victim][0][:len(toks)]
    for rid in _json_ids(reqs):
        _check_json(got[rid])


def test_small_pool_preempts_a_json_row():
    # the youngest row is the victim: the JSON row
    reqs = [("a", list(range(5, 35)), SamplingParams(temperature=0.0,
                                                     max_tokens=40)),
            ("j", list(range(40, 70)), SamplingParams(
                temperature=0.0, max_tokens=40, response_format="json",
                ignore_eos=True))]
    ref, got, handles = _both(reqs, eng_kw={"device_guided": True,
                                            "num_gpu_blocks": 9})
    assert got == ref
    assert len(handles["j"].prompt_token_ids) > 30        # it was preempted
    # Known quirk, shared by both paths: the outputs folded into the prompt
    # are lost to the grammar, which starts over behind them.  Each part is
    # a prefix of valid JSON; the whole stream need not be.
    cut = len(handles["j"].prompt_token_ids) - 30
    _check_json((got["j"][0][:cut], None, None))
    _check_json((got["j"][0][cut:], None, None))


@pytest.mark.parametrize("kw", [
    dict(response_format="tool_call", tool_names=("f", "g")),
    dict(response_format="json",
         response_schema={"type": "object",
                          "properties": {"a": {"type": "integer"}}}),
    dict(response_schema={"type": "array"}),
])
def test_schema_and_tool_call_rows_still_fall_back(kw):
    reqs = [("g", PROMPTS[0], SamplingParams(temperature=0.0, max_tokens=14,
                                             ignore_eos=True, **kw)),
            ("j", PROMPTS[1], SamplingParams(temperature=0.0, max_tokens=14,
                                             ignore_eos=True,
                                             response_format="json")),
            ("p", PROMPTS[2], SamplingParams(temperature=0.0, max_tokens=14))]
    ref, _ = _run(_engine(device_guided=True), False, reqs)
    got, _ = _run(_engine(device_guided=True), True, reqs,
                  expect_inflight=False)
    assert got == ref


def test_too_deep_for_the_device_falls_back():
    """A machine nested deeper than the device state holds keeps the batch
    on the synchronous step; pack() is never asked to truncate."""
    eng = _engine(device_guided=True)
    eng.add_request(PROMPTS[0], SamplingParams(
        temperature=0.0, max_tokens=8, response_format="json"),
        request_id="deep")
    req = eng.scheduler.waiting[-1]
    outs = eng.step_pipelined()                           # the prefill
    assert len(outs) == 1 and eng.scheduler.running == [req]
    assert eng._pipe_eligible()
    deep = JsonByteMachine()
    for _ in range(257):
        deep.feed(ord("["))
    deep.consumed = len(req.output_token_ids)
    req._guided = deep
    assert not eng._pipe_eligible()
    eng.abort_request("deep")


def test_default_config_has_no_guided_state():
    eng = _engine()
    assert eng.config.device_guided is False
    assert "gd_state" not in eng.runner._pipe_ctl_io(4, "cpu")
    on = _engine(device_guided=True).runner._pipe_ctl_io(4, "cpu")
    assert on["gd_state"].shape == (4, 11) and bool((on["gd_state"] == -1).all())

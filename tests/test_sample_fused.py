"""Tie-exact top-k/top-p sampling (ops.sample_fused): the torch twin against
a float64 reference, and the engine with EngineConfig.device_sampling on the
CPU: seeded stochastic rows get from step_pipelined() exactly the tokens
and finish reasons of step()."""

import importlib.util
import pathlib

import pytest
import torch

from hyperspot import ops
from hyperspot.engine import EngineConfig, LLMEngine, SamplingParams
from hyperspot.ops import torch_ref

_spec = importlib.util.spec_from_file_location(
    "sample_fused_ref",
    pathlib.Path(__file__).with_name("sample_fused_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


# ---- torch_ref.sample_fused against the float64 reference ----

@pytest.mark.parametrize("vocab", [512, 1003])
def test_ref_matches_fp64_reference(vocab):
    rows = 16
    logits, u = R.make_logits(rows, vocab, seed=vocab)
    t, p, k = R.row_params(rows)
    out = torch_ref.sample_fused(logits, t, p, k, u)
    assert out.dtype == torch.long and out.shape == (rows,)
    R.check_rows(logits, t, p, k, u, out)
    # fp32 logits (the CPU engine's) go the same way, through the op
    out32 = ops.sample_fused(logits.float(), t, p, k, u)
    assert torch.equal(out32, out)
    buf = torch.empty(rows, dtype=torch.long)
    assert ops.sample_fused(logits, t, p, k, u, out=buf) is buf
    assert torch.equal(buf, out)


def _one(x, t, k, p, u):
    x = torch.tensor([x], dtype=torch.float32).to(torch.bfloat16)
    out = torch_ref.sample_fused(
        x, torch.tensor([t], dtype=torch.float32),
        torch.tensor([p], dtype=torch.float32),
        torch.tensor([k], dtype=torch.int32),
        torch.tensor([u], dtype=torch.float32))
    ref = R.Ref(x[0], t, k, p)
    R.check_token(ref, out[0], u)
    return int(out[0]), ref


def test_tie_straddling_top_k_keeps_all_tied():
    #      0    1    2    3    4    5
    x = [1.0, 3.0, 2.0, 2.0, 0.5, 2.0]
    seen = set()
    for i in range(40):
        tok, ref = _one(x, 1.0, 2, 1.0, (i + 0.5) / 40)
        assert ref.kept.tolist() == [False, True, True, True, False, True]
        seen.add(tok)
    assert seen == {1, 2, 3, 5}        # k = 2, yet all three ties can come


def test_tie_group_straddling_top_p_is_kept_whole():
    # weights 4 : 1 : 1 : 1 (+ a far tail): the mass above the tie group is
    # 4/7.0001 < p = 0.7, and 5/7 of the way through it p is passed
    x = [0.0, 2.0, 0.0, 0.0, -9.0]
    t = 2.0 / 1.3862943611198906       # exp(2/t) = 4
    seen = set()
    for i in range(64):
        tok, ref = _one(x, t, 0, 0.7, (i + 0.5) / 64)
        assert ref.kept.tolist() == [True, True, True, True, False]
        seen.add(tok)
    assert seen == {0, 1, 2, 3}


def test_p_not_positive_keeps_the_maximum_group():
    x = [1.0, 4.0, 0.0, 4.0, 3.0]
    for p in (0.0, -1.0):
        seen = set()
        for u in (0.0, 0.3, 0.6, 0.99):
            tok, ref = _one(x, 1.0, 0, p, u)
            assert ref.kept.tolist() == [False, True, False, True, False]
            seen.add(tok)
        assert seen == {1, 3}


def test_minus_inf_is_never_returned():
    ninf = float("-inf")
    x = [ninf, 1.0, ninf, 0.0, ninf]
    for u in (0.0, 0.5, 0.9999999):
        tok, _ = _one(x, 1.0, 0, 1.0, u)
        assert tok in (1, 3)
    assert _one(x, 1.0, 0, 1.0, 0.0)[0] == 1
    assert _one(x, 1.0, 3, 0.99, 0.9999999)[0] == 3


def test_fallback_is_a_kept_token():
    # u at the largest float below 1: whether or not the running sum gets
    # past u * Z', the answer is the last KEPT token, never vocab - 1
    x = [0.0, 5.0, 4.0, 5.0, -3.0, -4.0]
    u = 1.0 - 2.0 ** -24
    tok, ref = _one(x, 1.0, 3, 1.0, u)
    assert tok == 3 and not bool(ref.kept[5])
    tok, ref = _one(x, 1.0, 0, 0.9, u)
    assert tok == 3
    # u == 1 cannot be crossed at all: the fallback proper
    out = torch_ref.sample_fused(
        torch.tensor([x]), torch.tensor([1.0]), torch.tensor([1.0]),
        torch.tensor([3], dtype=torch.int32), torch.tensor([1.0]))
    assert int(out[0]) == 3


def test_greedy_rows_and_k_at_least_vocab():
    logits, u = R.make_logits(4, 300, seed=1)
    t = torch.tensor([0.0, 1.0, 0.0, 1.0])
    p = torch.ones(4)
    out_off = torch_ref.sample_fused(logits, t, p, torch.zeros(
        4, dtype=torch.int32), u)
    out_big = torch_ref.sample_fused(logits, t, p, torch.tensor(
        [300, 300, 10 ** 8, 10 ** 8], dtype=torch.int32), u)
    assert torch.equal(out_off, out_big)
    assert torch.equal(out_off[::2], logits[::2].float().argmax(-1))


# ---- the engine with device_sampling, CPU ----

def test_device_sampling_is_off_by_default():
    assert EngineConfig().device_sampling is False


PROMPTS = [[(7 * i + 3 * j + 1) % 500 + 4 for j in range(12 + i)]
           for i in range(7)]


def _engine(**kw):
    cfg = EngineConfig(model="tiny-llama", max_num_seqs=8,
                       max_num_batched_tokens=512, max_model_len=256,
                       num_gpu_blocks=128, device_sampling=True, **kw)
    return LLMEngine(cfg)


def _mix(n, stops=None):
    """Greedy rows among seeded stochastic ones, staggered max_tokens."""
    stops = stops or {}
    kinds = [dict(temperature=0.0),
             dict(temperature=0.8, seed=5),
             dict(temperature=1.2, top_k=20, seed=7),
             dict(top_p=0.9, seed=9)]          # temperature 1.0
    return [(f"r{i}", PROMPTS[i],
             SamplingParams(max_tokens=n + 5 * i,
                            stop_token_ids=stops.get(i, ()),
                            **kinds[i % 4]))
            for i in range(5)]


def _run(eng, pipelined, reqs, late=None):
    streams = {}
    for rid, p, sp in reqs:
        eng.add_request(p, sp, request_id=rid)
        streams[rid] = [[], None]
    step = eng.step_pipelined if pipelined else eng.step
    calls, engaged = 0, False
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
        engaged |= eng._inflight is not None
        calls += 1
        assert calls < 2000
    assert eng.drain() == []
    return {k: (v[0], v[1]) for k, v in streams.items()}, engaged


def _both(reqs, late=None):
    sync = _engine()
    free0 = sync.runner.block_manager.num_free
    ref, engaged = _run(sync, False, reqs, late)
    assert not engaged
    pipe = _engine()
    got, engaged = _run(pipe, True, reqs, late)
    bm = pipe.runner.block_manager
    assert bm.num_free == free0 and not bm.row_of       # no page leaked
    return ref, got, engaged


def test_pipelined_stochastic_rows_equal_synchronous():
    base, _ = _run(_engine(), False, _mix(18))
    # rows 1 and 2 (stochastic) stop on a token they emit mid-run
    stops = {1: (base["r1"][0][6],), 2: (base["r2"][0][11],)}
    reqs = _mix(18, stops)
    late = (7, [("l0", PROMPTS[5], SamplingParams(
                    temperature=0.8, seed=5, max_tokens=9)),
                ("l1", PROMPTS[6], SamplingParams(
                    temperature=0.0, max_tokens=13))])
    ref, got, engaged = _both(reqs, late)
    assert engaged, "the pipelined path never engaged"
    assert got == ref
    assert ref["r1"][1].value == "stop" and len(ref["r1"][0]) <= 7
    assert ref["r3"][1].value == "length" and len(ref["r3"][0]) == 33
    assert len(ref["l0"][0]) == 9
    # the stochastic rows did sample: not the greedy continuation
    greedy, _ = _run(_engine(), False, [
        (rid, p, SamplingParams(temperature=0.0, max_tokens=sp.max_tokens))
        for rid, p, sp in _mix(18)])
    assert any(greedy[f"r{i}"][0] != base[f"r{i}"][0] for i in (1, 2, 3))


def test_flag_off_stochastic_rows_still_drain():
    cfg = EngineConfig(model="tiny-llama", max_num_seqs=8,
                       max_num_batched_tokens=512, max_model_len=256,
                       num_gpu_blocks=128)
    _, engaged = _run(LLMEngine(cfg), True, _mix(6)[:3])
    assert not engaged


def test_guided_row_still_falls_back():
    reqs = [("g", PROMPTS[0], SamplingParams(
                temperature=0.0, max_tokens=12, response_format="json")),
            ("t", PROMPTS[1], SamplingParams(
                temperature=0.8, max_tokens=12, seed=5)),
            ("p", PROMPTS[2], SamplingParams(
                temperature=0.0, max_tokens=12))]
    ref, _ = _run(_engine(), False, reqs)
    got, engaged = _run(_engine(), True, reqs)
    assert not engaged               # never while the guided row runs
    assert got == ref
    # once the guided row is gone, the stochastic one pipelines
    reqs[0] = ("g", PROMPTS[0], SamplingParams(
        temperature=0.0, max_tokens=4, response_format="json"))
    reqs[1] = ("t", PROMPTS[1], SamplingParams(
        temperature=0.8, max_tokens=30, seed=5))
    ref, got, engaged = _both(reqs)
    assert engaged and got == ref

"""Per-token logprobs on the CPU: the torch twin of the token_logprobs
kernel against the float64 reference, and the engine's records on both
stepping paths (the eager twin stands in for the kernel)."""

import importlib.util
import pathlib

import pytest
import torch

import hyperspot.ops
from hyperspot.engine import EngineConfig, LLMEngine, SamplingParams
from hyperspot.ops import torch_ref

_spec = importlib.util.spec_from_file_location(
    "logprobs_ref", pathlib.Path(__file__).with_name("logprobs_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

NINF = float("-inf")


# ---- the torch twin ----

@pytest.mark.parametrize("rows,vocab", [(16, 512), (16, 1003), (16, 4099),
                                        (4, 128256)])
def test_twin_matches_reference(rows, vocab):
    logits, chosen, n_top = R.make_rows(rows, vocab, seed=vocab)
    val, idx = torch_ref.token_logprobs(logits, chosen, n_top)
    rval, ridx = R.reference(logits, chosen, n_top)
    assert val.dtype == torch.float32 and idx.dtype == torch.int32
    assert torch.equal(idx.long(), ridx)
    assert R.max_abs_err(val, rval) < 1e-5      # float64 sums, one f32 cast


def test_twin_leaves_rows_that_did_not_ask():
    logits, chosen, n_top = R.make_rows(10, 512, seed=1)
    val = torch.full((10, 21), 7.0)
    idx = torch.full((10, 21), 7, dtype=torch.int32)
    v2, i2 = torch_ref.token_logprobs(logits, chosen, n_top, val, idx)
    assert v2 is val and i2 is idx
    skip = n_top < 0
    assert bool((val[skip] == 7.0).all()) and bool((idx[skip] == 7).all())
    rval, ridx = R.reference(logits, chosen, n_top)
    assert torch.equal(idx[~skip].long(), ridx[~skip])


def test_twin_ties_and_non_finite():
    vocab = 1003
    logits = torch.full((4, vocab), NINF, dtype=torch.bfloat16)
    logits[0, [7, 500, 1002]] = torch.tensor([1.0, 2.0, 0.5],
                                             dtype=torch.bfloat16)
    logits[1] = R.make_rows(1, vocab, seed=3)[0][0]
    logits[1, 100:200] = 30.0                   # a tied maximum
    logits[2] = logits[1]
    logits[2, 5] = float("nan")
    logits[2, 6] = float("inf")
    chosen = torch.tensor([3, 150, 6, vocab])   # -inf, tie, +inf, outside
    n_top = torch.tensor([5, 5, 5, 5], dtype=torch.int32)
    val, idx = torch_ref.token_logprobs(logits, chosen, n_top)
    rval, ridx = R.reference(logits, chosen, n_top)
    assert torch.equal(idx.long(), ridx)
    R.max_abs_err(val, rval)
    assert idx[0, 1:6].tolist() == [500, 7, 1002, 0, 1]
    assert val[0, 4:6].tolist() == [NINF, NINF] and val[0, 0] == NINF
    assert idx[1, 1:6].tolist() == [100, 101, 102, 103, 104]
    assert val[2, 0] == NINF
    assert val[3].tolist() == [NINF] * 21       # nothing finite in the row
    assert idx[3, 0] == vocab


# ---- the engine ----

PROMPTS = [[(7 * i + 3 * j + 1) % 500 + 4 for j in range(12 + i)]
           for i in range(6)]


def _engine(**kw):
    cfg = EngineConfig(model="tiny-llama", max_num_seqs=8,
                       max_num_batched_tokens=512, max_model_len=256,
                       num_gpu_blocks=128, **kw)
    return LLMEngine(cfg)


def _requests(max_tokens=9):
    """Rows cycle: greedy logprobs=0, greedy logprobs=5, no logprobs."""
    kinds = [dict(logprobs=0), dict(logprobs=5), dict()]
    return [(f"r{i}", p, SamplingParams(temperature=0.0, ignore_eos=True,
                                        max_tokens=max_tokens,
                                        **kinds[i % 3]))
            for i, p in enumerate(PROMPTS)]


def _run(eng, pipelined, reqs):
    """{rid: ([token], finish_reason, [record])}, and whether a pipelined
    step was ever in flight."""
    out = {}
    for rid, p, sp in reqs:
        eng.add_request(p, sp, request_id=rid)
        out[rid] = ([], [], [])
    step = eng.step_pipelined if pipelined else eng.step
    engaged = False
    calls = 0
    while eng.has_work():
        for o in step():
            toks, fin, recs = out[o.request_id]
            toks.append(o.token_id)
            recs.append(o.logprobs)
            if o.finished:
                fin.append(o.finish_reason)
        engaged |= eng._inflight is not None
        calls += 1
        assert calls < 2000
    assert eng.drain() == []
    assert not eng.runner.block_manager.row_of
    return out, engaged


def _plain(rec):
    return None if rec is None else (rec.token_id, rec.logprob, rec.top)


def test_records_match_log_softmax(monkeypatch):
    seen = []       # (logits, chosen, n_top) of every call
    real = hyperspot.ops.token_logprobs

    def spy(logits, chosen, n_top, *a, **kw):
        seen.append((logits.clone(), chosen.clone(), n_top.clone()))
        return real(logits, chosen, n_top, *a, **kw)

    monkeypatch.setattr(hyperspot.ops, "token_logprobs", spy)
    eng = _engine()
    reqs = _requests()
    out, _ = _run(eng, False, reqs)
    assert seen, "the op was never called"
    # every call, row by row, against log_softmax and the reference order
    want = {}       # (token, rounded logprob) -> reference top list
    n_records = 0
    for logits, chosen, n_top in seen:
        lsm = torch.log_softmax(logits.double(), -1)
        rval, ridx = R.reference(logits, chosen.cpu(), n_top.cpu())
        for r in range(logits.shape[0]):
            n = int(n_top[r])
            if n < 0:
                continue
            n_records += 1
            c = int(chosen[r])
            assert abs(float(rval[r, 0]) - float(lsm[r, c])) < 1e-9
            want.setdefault(c, []).append(
                (float(rval[r, 0]),
                 [(int(t), float(v)) for t, v in
                  zip(ridx[r, 1:1 + n], rval[r, 1:1 + n])]))
    got = 0
    for i, (rid, _, sp) in enumerate(reqs):
        toks, fin, recs = out[rid]
        assert len(toks) == 9 and len(recs) == 9
        if sp.logprobs is None:
            assert recs == [None] * 9
            continue
        for tok, rec in zip(toks, recs):
            got += 1
            assert rec.token_id == tok
            assert len(rec.top) == sp.logprobs
            cands = [w for w in want[tok]
                     if abs(w[0] - rec.logprob) < 1e-5]
            assert cands, "no call produced this record"
            assert any(
                [t for t, _ in w[1]] == [t for t, _ in rec.top]
                and all(abs(a[1] - b[1]) < 1e-5
                        for a, b in zip(w[1], rec.top))
                for w in cands)
            if sp.logprobs:
                assert rec.top[0][0] == tok      # greedy: the argmax
                assert rec.top[0][1] == rec.logprob
                lps = [v for _, v in rec.top]
                assert lps == sorted(lps, reverse=True)
    assert got == n_records == 4 * 9


def test_device_logprobs_pipeline_equals_step():
    reqs = _requests()
    ref, engaged = _run(_engine(device_logprobs=True), False, reqs)
    assert not engaged
    got, engaged = _run(_engine(device_logprobs=True), True, reqs)
    assert engaged, "step_pipelined never engaged with device_logprobs"
    for rid in ref:
        assert got[rid][0] == ref[rid][0]
        assert got[rid][1] == ref[rid][1]
        assert [_plain(r) for r in got[rid][2]] == \
            [_plain(r) for r in ref[rid][2]]
    assert any(r is not None for r in got["r1"][2])


def test_flag_off_stays_synchronous_with_same_records():
    reqs = _requests()
    ref, _ = _run(_engine(device_logprobs=True), False, reqs)
    got, engaged = _run(_engine(), True, reqs)
    assert not engaged, "a logprob row entered the pipeline without the flag"
    for rid in ref:
        assert got[rid][0] == ref[rid][0]
        assert [_plain(r) for r in got[rid][2]] == \
            [_plain(r) for r in ref[rid][2]]
    # without logprob rows the same engine does pipeline
    plain = [(rid, p, SamplingParams(temperature=0.0, ignore_eos=True,
                                     max_tokens=9))
             for rid, p, _ in reqs]
    out, engaged = _run(_engine(), True, plain)
    assert engaged
    assert all(r is None for v in out.values() for r in v[2])


@pytest.mark.parametrize("bad", [21, -1])
def test_out_of_range_logprobs_is_refused(bad):
    eng = _engine()
    with pytest.raises(ValueError):
        eng.add_request(PROMPTS[0], SamplingParams(logprobs=bad))
    assert not eng.has_work()


def test_guided_row_reports_only_legal_tokens():
    from hyperspot.engine.guided import SchemaMachine
    # a schema-shaped JSON row: the skeleton leaves one legal byte at most
    # steps, a boolean value two
    schema = {"type": "object", "required": ["ok"],
              "properties": {"ok": {"type": "boolean"}}}
    eng = _engine()
    eng.add_request(PROMPTS[0], SamplingParams(
        temperature=1.0, seed=7, max_tokens=40, response_format="json",
        response_schema=schema, logprobs=5), request_id="g")
    m = SchemaMachine(schema)
    short = 0
    n = 0
    while eng.has_work():
        for o in eng.step():
            rec = o.logprobs
            allow, eos_ok = m.allowed()
            legal = {b + 4 for b in allow} | ({2} if eos_ok else set())
            assert rec.token_id == o.token_id and rec.token_id in legal
            assert rec.logprob > NINF
            assert 1 <= len(rec.top) <= 5
            assert all(v > NINF and t in legal for t, v in rec.top)
            assert len(rec.top) == min(5, len(legal))
            short += len(rec.top) < 5
            n += 1
            if not o.finished or o.token_id != 2:
                m.feed_token(o.token_id)
    assert n > 0 and short > 0, "no step had fewer than five legal tokens"

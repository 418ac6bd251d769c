"""Presence / frequency / repetition penalties on the CPU: the torch twins
of the penalty kernels against the numpy reference, bit for bit, and the
engine on both stepping paths (the eager twin stands in for the kernels)."""

import importlib.util
import pathlib

import numpy as np
import pytest
import torch

import hyperspot.ops as ops
from hyperspot.engine import EngineConfig, LLMEngine, SamplingParams
from hyperspot.ops import torch_ref

_spec = importlib.util.spec_from_file_location(
    "penalties_ref", pathlib.Path(__file__).with_name("penalties_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _build(table, histories, order):
    sl, toks, off, plen = R.flat_histories(histories, order)
    torch_ref.penalty_build(table, _t(sl), _t(toks), _t(off), _t(plen))


# ---- the reference's own hand cases ----

def test_reference_hand_cases():
    for l, r, f, c, p, prompt_only, want in R.HAND_CASES:
        bits = R.bf16_bits(torch.tensor([l, 9.0], dtype=torch.bfloat16))
        hist = [0] if prompt_only else [0] * c
        out = R.penalise_row(bits, hist, 1 if prompt_only else 0, r, p, f)
        got = R.from_bits(out).float().tolist()
        assert got == [want, 9.0], (l, r, f, c, p, got)


def test_reference_rounding_and_table():
    q = np.array([1.0, 1.00390625, 1.01171875, -np.inf, np.nan],
                 dtype=np.float32)             # 1 + 2^-8 ties to even
    b = R.f32_to_bf16_bits(q)
    assert b[:4].tolist() == [0x3f80, 0x3f80, 0x3f82, 0xff80]
    assert (b[4] & 0x7fff) > 0x7f80
    row = R.table_row([5, 5, 7, 5, 9, 600, -1], 2, 16)
    assert row[5] == 2 * 1 + 1 and row[7] == 2 and row[9] == 2
    assert int(row.sum()) == 7


# ---- the torch twins ----

@pytest.mark.parametrize("vocab", [512, 1003])
def test_twin_matches_reference(vocab):
    rows = 16
    logits, slot, rep, pres, freq, hist = R.make_case(rows, vocab, seed=vocab)
    table = torch.full((rows, vocab), 0x5a5a5a5, dtype=torch.int32)  # garbage
    order = sorted(hist, key=lambda s: (s * 7) % 16)
    _build(table, hist, order)
    for sl, (h, n) in hist.items():
        assert np.array_equal(table[sl].numpy(), R.table_row(h, n, vocab))
    want = R.reference(logits, slot, rep, pres, freq, hist)
    before = R.bf16_bits(logits)
    torch_ref.penalty_apply(logits, _t(slot), _t(rep), _t(pres), _t(freq),
                            table)
    got = R.bf16_bits(logits)
    assert np.array_equal(got, want)
    # rows without a slot and logits of unseen tokens keep their bits
    assert np.array_equal(got[slot < 0], before[slot < 0])
    for i in np.nonzero(slot >= 0)[0]:
        unseen = table[int(slot[i])].numpy() == 0
        assert np.array_equal(got[i][unseen], before[i][unseen])
    assert (got != before).any()


def test_twin_hand_cases():
    for l, r, f, c, p, prompt_only, want in R.HAND_CASES:
        logits = torch.tensor([[l, 9.0]], dtype=torch.bfloat16)
        table = torch.tensor([[1 if prompt_only else 2 * c, 0]],
                             dtype=torch.int32)
        torch_ref.penalty_apply(
            logits, torch.zeros(1, dtype=torch.int32), torch.tensor([r]),
            torch.tensor([p]), torch.tensor([f]), table)
        assert logits.float().tolist() == [[want, 9.0]]


def test_twin_special_values():
    vals = [float("inf"), float("-inf"), float("nan"), 0.0, -0.0, 3.0]
    logits = torch.tensor([vals, vals], dtype=torch.bfloat16)
    before = R.bf16_bits(logits)
    table = torch.tensor([[4] * 6, [0] * 6], dtype=torch.int32)
    torch_ref.penalty_apply(
        logits, torch.tensor([0, 1], dtype=torch.int32),
        torch.tensor([2.0, 2.0]), torch.tensor([0.5, 0.5]),
        torch.tensor([0.25, 0.25]), table)
    got = R.bf16_bits(logits)
    want = R.reference(R.from_bits(before), [0, 1], [2.0] * 2, [0.5] * 2,
                       [0.25] * 2, {0: ([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5],
                                        0), 1: ([], 0)})
    assert np.array_equal(got, want)
    assert got[0, 0] == 0x7f80 and got[0, 1] == 0xff80       # inf stays
    assert got[0, 2] == before[0, 2]                         # NaN as it was
    assert np.array_equal(got[1], before[1])                 # -0 kept, too
    assert before[1, 4] == 0x8000


def test_note_accumulates_to_the_rebuilt_table():
    vocab = 1003
    g = np.random.default_rng(5)
    hist = {0: (g.integers(0, vocab, 50), 20), 2: (g.integers(0, 9, 30), 30),
            1: (np.zeros(0, dtype=np.int64), 0)}
    table = torch.full((3, vocab), -7, dtype=torch.int32)
    _build(table, hist, [2, 0, 1])
    slot = torch.tensor([1, -1, 0, 2], dtype=torch.int32)    # row 1: no slot
    new = {0: [], 1: [], 2: []}
    for k in range(6):
        sampled = torch.from_numpy(g.integers(0, 9, 4))
        if k == 2:
            sampled[0] = -1                                  # outside: skipped
            sampled[2] = vocab
        torch_ref.penalty_note(table, slot, sampled)
        for row, sl in enumerate(slot.tolist()):
            if sl >= 0:
                new[sl].append(int(sampled[row]))
    again = torch.full((3, vocab), 99, dtype=torch.int32)
    grown = {sl: (np.concatenate([h, np.asarray(new[sl], dtype=np.int64)]),
                  n) for sl, (h, n) in hist.items()}
    _build(again, grown, [0, 1, 2])
    assert torch.equal(table, again)


# ---- the engine ----

PROMPTS = [[(7 * i + 3 * j + 1) % 500 + 4 for j in range(12 + i)]
           for i in range(6)]
PEN = [dict(frequency_penalty=1.5), dict(presence_penalty=-1.0,
                                         repetition_penalty=1.3),
       dict(), dict(repetition_penalty=0.8, frequency_penalty=0.4,
                    presence_penalty=0.7)]


def _engine(**kw):
    kw.setdefault("num_gpu_blocks", 128)
    cfg = EngineConfig(model="tiny-llama", max_num_seqs=8,
                       max_num_batched_tokens=512, max_model_len=256, **kw)
    return LLMEngine(cfg)


def _requests(max_tokens=14, stochastic=False, prompts=PROMPTS):
    """Rows cycle through PEN (every third one carries no penalty)."""
    out = []
    for i, p in enumerate(prompts):
        kw = dict(PEN[i % len(PEN)])
        if stochastic and i % 2:
            kw.update(temperature=0.9, top_p=0.9, seed=100 + i)
        else:
            kw.update(temperature=0.0)
        out.append((f"r{i}", p, SamplingParams(
            ignore_eos=True, max_tokens=max_tokens + i, **kw)))
    return out


def _run(eng, pipelined, reqs):
    out = {}
    for rid, p, sp in reqs:
        eng.add_request(p, sp, request_id=rid)
        out[rid] = ([], [])
    step = eng.step_pipelined if pipelined else eng.step
    engaged = False
    calls = 0
    while eng.has_work():
        for o in step():
            toks, fin = out[o.request_id]
            assert not fin, "output after finish"
            toks.append(o.token_id)
            if o.finished:
                fin.append(o.finish_reason)
        engaged |= eng._inflight is not None
        calls += 1
        assert calls < 2000
    assert eng.drain() == []
    assert not eng.runner.block_manager.row_of
    return out, engaged


def test_slots_encode_the_history_at_every_step(monkeypatch):
    """Wrap ops.penalty_apply on the synchronous path: each penalty row's
    slot holds exactly that request's prompt and generated tokens."""
    eng = _engine(num_gpu_blocks=9)          # small pool: folds a prompt
    reqs = [("a", list(range(1, 31)), SamplingParams(
                temperature=0.0, max_tokens=40, frequency_penalty=0.5)),
            ("b", list(range(40, 70)), SamplingParams(
                temperature=0.0, max_tokens=40, repetition_penalty=1.2))]
    first = {rid: list(p) for rid, p, _ in reqs}
    real = ops.penalty_apply
    seen = {"calls": 0, "folded": False, "batch": None}
    real_sample = eng.runner._sample

    def sample(logits, requests):
        seen["batch"] = requests
        return real_sample(logits, requests)

    def spy(logits, slot, rep, pres, freq, table):
        seen["calls"] += 1
        rows = [(i, s) for i, s in enumerate(slot.tolist()) if s >= 0]
        assert rows
        for i, s in rows:
            r = seen["batch"][i]
            assert r.sampling.penalized
            full = r.prompt_token_ids + r.output_token_ids
            n0 = len(first[r.request_id])
            assert full[:n0] == first[r.request_id]
            assert len(full) - r.num_generated == n0
            seen["folded"] |= len(r.prompt_token_ids) > n0
            want = R.table_row(full, n0, table.shape[1])
            assert np.array_equal(table[s].numpy(), want), r.request_id
            assert float(rep[i]) == np.float32(r.sampling.repetition_penalty)
            assert float(freq[i]) == np.float32(r.sampling.frequency_penalty)
        return real(logits, slot, rep, pres, freq, table)

    monkeypatch.setattr(eng.runner, "_sample", sample)
    monkeypatch.setattr(ops, "penalty_apply", spy)
    out, _ = _run(eng, False, reqs)
    assert seen["calls"] >= 40 and seen["folded"]
    assert all(len(out[rid][0]) == 40 for rid in ("a", "b"))


def test_frequency_penalty_changes_the_greedy_stream():
    p = PROMPTS[0]
    base, _ = _run(_engine(), False, [("x", p, SamplingParams(
        temperature=0.0, max_tokens=24, ignore_eos=True))])
    pen, _ = _run(_engine(), False, [("x", p, SamplingParams(
        temperature=0.0, max_tokens=24, ignore_eos=True,
        frequency_penalty=1.5))])
    assert len(pen["x"][0]) == 24 and pen["x"][0] != base["x"][0]
    # explicit neutral values are no penalties at all
    neutral, _ = _run(_engine(), False, [("x", p, SamplingParams(
        temperature=0.0, max_tokens=24, ignore_eos=True,
        presence_penalty=0.0, frequency_penalty=0.0,
        repetition_penalty=1.0))])
    assert neutral == base


def test_rows_without_penalties_are_not_disturbed():
    mixed = _requests()
    plain = [(rid, p, sp) for rid, p, sp in mixed if not sp.penalized]
    assert plain and len(plain) < len(mixed)
    got, _ = _run(_engine(), False, mixed)
    alone = [(rid, p, SamplingParams(temperature=0.0, ignore_eos=True,
                                     max_tokens=sp.max_tokens))
             for rid, p, sp in mixed]
    base, _ = _run(_engine(), False, alone)
    for rid, _, sp in mixed:
        if sp.penalized:
            assert got[rid] != base[rid]
        else:
            assert got[rid] == base[rid]


@pytest.mark.parametrize("stochastic", [False, True])
def test_pipelined_equals_synchronous(stochastic):
    kw = dict(device_penalties=True, device_sampling=stochastic)
    reqs = _requests(stochastic=stochastic)
    ref, _ = _run(_engine(**kw), False, reqs)
    got, engaged = _run(_engine(**kw), True, reqs)
    assert engaged, "the pipelined path never engaged"
    assert got == ref
    off, engaged = _run(_engine(device_sampling=stochastic), True, reqs)
    assert off == ref                    # flag off: the rows take step()


def test_pipelined_equals_synchronous_through_preemption():
    reqs = [("a", list(range(1, 31)), SamplingParams(
                temperature=0.0, max_tokens=40, frequency_penalty=0.6,
                presence_penalty=0.3)),
            ("b", list(range(40, 70)), SamplingParams(
                temperature=0.0, max_tokens=40, repetition_penalty=1.25))]
    kw = dict(device_penalties=True, num_gpu_blocks=9)
    ref, _ = _run(_engine(**kw), False, reqs)
    got, engaged = _run(_engine(**kw), True, reqs)
    assert engaged and got == ref
    big, _ = _run(_engine(device_penalties=True), True, reqs)
    assert big == ref                    # the folded prompt changed nothing


def test_more_penalty_rows_than_slots_take_the_synchronous_step():
    reqs = _requests(max_tokens=8)
    assert sum(sp.penalized for _, _, sp in reqs) > 2
    ref, _ = _run(_engine(), False, reqs)
    eng = _engine(device_penalties=True, max_penalty_seqs=2)
    launched = []
    real = eng.runner.pipe_launch
    eng.runner.pipe_launch = lambda seed=None: launched.append(
        sum(r.sampling.penalized for r in eng.scheduler.running)) \
        or real(seed)
    got, _ = _run(eng, True, reqs)
    assert got == ref
    assert all(n <= 2 for n in launched)
    assert eng.runner._pen_table.shape[0] == 2


def test_no_penalty_row_no_penalty_op(monkeypatch):
    called = []
    for name in ("penalty_build", "penalty_apply", "penalty_note"):
        monkeypatch.setattr(ops, name,
                            lambda *a, _n=name, **k: called.append(_n))
    eng = _engine()
    reqs = [(f"r{i}", p, SamplingParams(temperature=0.0, max_tokens=9))
            for i, p in enumerate(PROMPTS[:3])]
    _run(eng, True, reqs)
    _run(eng, False, reqs)
    assert called == [] and eng.runner._pen_table is None


@pytest.mark.parametrize("kw", [
    dict(presence_penalty=2.5), dict(presence_penalty=-2.01),
    dict(frequency_penalty=float("nan")), dict(frequency_penalty=3),
    dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0),
    dict(repetition_penalty=float("inf")), dict(presence_penalty="1"),
])
def test_add_request_refuses(kw):
    eng = _engine()
    with pytest.raises(ValueError):
        eng.add_request(PROMPTS[0], SamplingParams(max_tokens=2, **kw))
    assert not eng.has_work()
    eng.add_request(PROMPTS[0], SamplingParams(
        max_tokens=2, presence_penalty=2, frequency_penalty=-2.0,
        repetition_penalty=1e-3))

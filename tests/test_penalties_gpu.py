"""The penalty kernels on the GPU (csrc/penalties.hip) against the numpy
reference, bit for bit: build + apply over poisoned tables, shuffled slots,
rows off the 16-byte grid, batch independence, penalty_note, the binding's
refusals, capture into a graph, and the pipelined engine with
device_penalties against the synchronous step() loop.

There is no tolerance anywhere: every operation of the contract is a single
correctly rounded fp32 operation on both sides, and the table holds
integers."""

import importlib.util
import pathlib

import numpy as np
import pytest
import torch

from hyperspot import ops

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "penalties_ref", pathlib.Path(__file__).with_name("penalties_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

POISON = 0x5a5a5a5


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _build(table, histories, order):
    sl, toks, off, plen = R.flat_histories(histories, order)
    ops.penalty_build(table, _d(sl), _d(toks), _d(off), _d(plen))


def _on_device(logits, vocab):
    """The rows as a contiguous [rows, vocab] view that starts 3 elements
    into its buffer: off the 16-byte grid at any vocabulary."""
    rows = logits.shape[0]
    buf = torch.zeros(rows * vocab + 16, dtype=torch.bfloat16, device="cuda")
    view = buf[3:3 + rows * vocab].view(rows, vocab)
    view.copy_(logits)
    assert view.data_ptr() % 16 == 6 and view.is_contiguous()
    return buf, view


@pytest.mark.parametrize("rows,vocab", [(16, 512), (16, 1003), (16, 4099),
                                        (4, 128256)])
def test_build_and_apply_match_reference(rows, vocab):
    nslots = rows + 3
    logits, slot, rep, pres, freq, hist = R.make_case(
        rows, vocab, seed=vocab, max_slots=nslots)
    table = torch.full((nslots, vocab), POISON, dtype=torch.int32,
                       device="cuda")
    order = sorted(hist, key=lambda s: (s * 7) % nslots)      # shuffled
    _build(table, hist, order)
    tab = table.cpu().numpy()
    for sl in range(nslots):
        if sl in hist:
            h, n = hist[sl]
            assert np.array_equal(tab[sl], R.table_row(h, n, vocab)), sl
        else:
            assert (tab[sl] == POISON).all()                  # not its row
    want = R.reference(logits, slot, rep, pres, freq, hist)
    before = R.bf16_bits(logits)
    if vocab == 1003:
        buf, lg = _on_device(logits, vocab)
    else:
        buf = lg = logits.cuda()
    ops.penalty_apply(lg, _d(slot), _d(rep), _d(pres), _d(freq), table)
    torch.cuda.synchronize()
    got = R.bf16_bits(lg)
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(int(i), int(j), hex(before[i, j]), hex(got[i, j]),
                            hex(want[i, j])) for i, j in bad[:8]]
    assert np.array_equal(got[slot < 0], before[slot < 0])
    assert (got != before).any()
    if vocab == 1003:                     # nothing outside the view written
        flat = R.bf16_bits(buf)
        assert not flat[:3].any() and not flat[3 + rows * vocab:].any()
    assert np.array_equal(table.cpu().numpy(), tab)           # read only


@pytest.mark.parametrize("vocab", [1003, 4099])
def test_row_alone_equals_row_in_batch(vocab):
    rows = 10
    logits, slot, rep, pres, freq, hist = R.make_case(rows, vocab, seed=4)
    table = torch.zeros(rows, vocab, dtype=torch.int32, device="cuda")
    _build(table, hist, sorted(hist))
    lg = logits.cuda()
    ops.penalty_apply(lg, _d(slot), _d(rep), _d(pres), _d(freq), table)
    batch = R.bf16_bits(lg)
    for r in (1, 2, 4, 9):                # odd rows start off the 16-byte grid
        assert slot[r] >= 0
        one = logits[r:r + 1].clone().cuda()
        ops.penalty_apply(one, _d(slot[r:r + 1]), _d(rep[r:r + 1]),
                          _d(pres[r:r + 1]), _d(freq[r:r + 1]), table)
        assert np.array_equal(R.bf16_bits(one)[0], batch[r])


def test_hand_cases():
    for l, r, f, c, p, prompt_only, want in R.HAND_CASES:
        lg = torch.tensor([[l, 9.0]], dtype=torch.bfloat16, device="cuda")
        table = torch.tensor([[1 if prompt_only else 2 * c, 0]],
                             dtype=torch.int32, device="cuda")
        ops.penalty_apply(lg, torch.zeros(1, dtype=torch.int32, device="cuda"),
                          torch.tensor([r], device="cuda"),
                          torch.tensor([p], device="cuda"),
                          torch.tensor([f], device="cuda"), table)
        assert lg.float().cpu().tolist() == [[want, 9.0]]


def test_note_accumulates_to_the_rebuilt_table():
    vocab = 4099
    g = np.random.default_rng(5)
    hist = {0: (g.integers(0, vocab, 50), 20), 2: (g.integers(0, 9, 30), 30),
            1: (np.zeros(0, dtype=np.int64), 0)}
    table = torch.full((3, vocab), POISON, dtype=torch.int32, device="cuda")
    _build(table, hist, [2, 0, 1])
    slot = torch.tensor([1, -1, 0, 2], dtype=torch.int32, device="cuda")
    new = {0: [], 1: [], 2: []}
    for k in range(6):
        sampled = torch.from_numpy(g.integers(0, 9, 4))
        if k == 2:
            before = table.clone()
            bad = torch.tensor([-1, 3, vocab, 1 << 40])      # row 1: no slot
            ops.penalty_note(table, slot, bad.cuda())
            assert torch.equal(table, before)
        ops.penalty_note(table, slot, sampled.cuda())
        for row, sl in enumerate(slot.tolist()):
            if sl >= 0:
                new[sl].append(int(sampled[row]))
    again = torch.full((3, vocab), 99, dtype=torch.int32, device="cuda")
    grown = {sl: (np.concatenate([h, np.asarray(new[sl], dtype=np.int64)]),
                  n) for sl, (h, n) in hist.items()}
    _build(again, grown, [0, 1, 2])
    assert torch.equal(table, again)


def test_binding_checks_its_arguments():
    C = ops._native()
    vocab = 64
    table = torch.zeros(4, vocab, dtype=torch.int32, device="cuda")
    slot = torch.tensor([0, 1, -1, 2], dtype=torch.int32, device="cuda")
    sampled = torch.tensor([1, 2, 3, 4], device="cuda")
    lg = torch.zeros(4, vocab, dtype=torch.bfloat16, device="cuda")
    one = torch.ones(4, device="cuda")
    C.penalty_note(table, slot, sampled)
    C.penalty_apply(lg, slot, one, one, one, table)
    with pytest.raises(RuntimeError):
        C.penalty_note(table.long(), slot, sampled)              # dtype
    with pytest.raises(RuntimeError):
        C.penalty_note(table.t().contiguous().t(), slot, sampled)
    with pytest.raises(RuntimeError):
        C.penalty_note(table[:, :32], slot, sampled)             # strided
    with pytest.raises(RuntimeError):
        C.penalty_note(table, slot[:3], sampled)                 # a row short
    with pytest.raises(RuntimeError):
        C.penalty_note(table, slot, sampled.int())
    with pytest.raises(RuntimeError):
        C.penalty_note(table, slot.cpu(), sampled)
    with pytest.raises(RuntimeError):
        C.penalty_apply(lg, slot, one[:3], one, one, table)
    with pytest.raises(RuntimeError):
        C.penalty_apply(lg, slot[:3], one, one, one, table)
    with pytest.raises(RuntimeError):
        C.penalty_apply(lg[:, :32].contiguous(), slot, one, one, one, table)
    with pytest.raises(RuntimeError):
        C.penalty_apply(lg.float(), slot, one, one, one, table)
    with pytest.raises(RuntimeError):
        C.penalty_build(table, slot, sampled.int(), slot, slot)  # offsets n+1
    torch.cuda.synchronize()


def test_capturable_apply_sample_note():
    rows, vocab, nslots = 10, 4099, 12
    logits, slot, rep, pres, freq, hist = R.make_case(
        rows, vocab, seed=9, max_slots=nslots)
    table = torch.full((nslots, vocab), POISON, dtype=torch.int32,
                       device="cuda")
    _build(table, hist, sorted(hist))
    lg = torch.empty(rows, vocab, dtype=torch.bfloat16, device="cuda")
    sampled = torch.zeros(rows, dtype=torch.long, device="cuda")
    par = [_d(slot), _d(rep), _d(pres), _d(freq)]

    def tail():
        ops.penalty_apply(lg, *par, table)
        ops.greedy_sample(lg, out=sampled)
        ops.penalty_note(table, par[0], sampled)

    keep = table.clone()
    lg.copy_(logits)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tail()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tail()
    table.copy_(keep)
    # the reference loop: penalise, argmax, append to the history
    hist = {sl: (np.asarray(h, dtype=np.int64), n)
            for sl, (h, n) in hist.items()}
    for it in range(3):
        fresh = R.make_case(rows, vocab, seed=20 + it)[0]
        for i in range(rows):
            fresh[i, (7 * i + 13 * 2) % vocab] = -1.0      # no NaN: argmax
            fresh[i, (7 * i) % vocab] = 2.0                # no +inf either
        lg.copy_(fresh)
        g.replay()
        torch.cuda.synchronize()
        want = R.reference(fresh, slot, rep, pres, freq, hist)
        assert np.array_equal(R.bf16_bits(lg), want)
        toks = R.from_bits(want).float().argmax(-1)
        assert torch.equal(sampled.cpu(), toks)
        for i, sl in enumerate(slot.tolist()):
            if sl >= 0:
                h, n = hist[sl]
                hist[sl] = (np.append(h, int(toks[i])), n)
        tab = table.cpu().numpy()
        for sl, (h, n) in hist.items():
            assert np.array_equal(tab[sl], R.table_row(h, n, vocab))


# ---- engine ----

def _run(batch, pipelined, stochastic):
    from hyperspot.engine import EngineConfig, LLMEngine, SamplingParams
    cfg = EngineConfig(model="tiny-llama-d128", max_num_seqs=64,
                       max_num_batched_tokens=2048, max_model_len=128,
                       num_gpu_blocks=512, graph_batch_sizes=(4, 8),
                       prefill_graph_sizes=(), device_penalties=True,
                       max_penalty_seqs=8, device_sampling=stochastic,
                       device_logprobs=stochastic)
    eng = LLMEngine(cfg, device="cuda:0")
    free0 = eng.runner.block_manager.num_free
    pens = [dict(frequency_penalty=1.5),
            dict(presence_penalty=-1.0, repetition_penalty=1.3),
            dict(),
            dict(repetition_penalty=0.8, frequency_penalty=0.4,
                 presence_penalty=0.7)]
    for i in range(batch):
        prompt = [(5 * i + 3 * j + 1) % 500 + 4 for j in range(14 + i % 5)]
        kw = dict(pens[i % 4])
        if stochastic:
            kw.update(logprobs=[0, 5, None][i % 3])
            if i % 2:
                kw.update(temperature=0.9, top_k=40, seed=7 + i)
        kw.setdefault("temperature", 0.0)
        eng.add_request(prompt, SamplingParams(max_tokens=16, ignore_eos=True,
                                               **kw), request_id=f"r{i}")
    out = {f"r{i}": [[], None, []] for i in range(batch)}
    step = eng.step_pipelined if pipelined else eng.step
    engaged = False
    while eng.has_work():
        for o in step():
            s = out[o.request_id]
            s[0].append(o.token_id)
            s[2].append(None if o.logprobs is None else
                        (o.logprobs.token_id, o.logprobs.logprob,
                         o.logprobs.top))
            if o.finished:
                s[1] = o.finish_reason.value
        engaged |= eng._inflight is not None
    assert engaged == pipelined
    assert eng.runner.block_manager.num_free == free0
    return out


@pytest.mark.parametrize("stochastic", [False, True])
def test_pipelined_engine_equals_synchronous(stochastic):
    # equal max_tokens, no stops: the same graph and shapes run every step,
    # so tokens, finish reasons and the records' floats agree exactly
    ref = _run(7, False, stochastic)
    got = _run(7, True, stochastic)
    assert got == ref
    plain = _run_plain(7) if not stochastic else None
    for i in range(7):
        toks, fin, recs = ref[f"r{i}"]
        assert len(toks) == 16 and fin == "length"
        if plain is not None and i % 4 == 2:
            assert toks == plain[f"r{i}"]        # no penalty: undisturbed
    if plain is not None:
        assert any(ref[f"r{i}"][0] != plain[f"r{i}"] for i in (0, 1, 3))


def _run_plain(batch):
    """The same prompts, greedy and without any penalty, flags off."""
    from hyperspot.engine import EngineConfig, LLMEngine, SamplingParams
    cfg = EngineConfig(model="tiny-llama-d128", max_num_seqs=64,
                       max_num_batched_tokens=2048, max_model_len=128,
                       num_gpu_blocks=512, graph_batch_sizes=(4, 8),
                       prefill_graph_sizes=())
    eng = LLMEngine(cfg, device="cuda:0")
    prompts = [[(5 * i + 3 * j + 1) % 500 + 4 for j in range(14 + i % 5)]
               for i in range(batch)]
    outs = eng.generate(prompts, SamplingParams(temperature=0.0,
                                                max_tokens=16,
                                                ignore_eos=True))
    assert eng.runner._pen_table is None
    return {f"r{i}": o for i, o in enumerate(outs)}

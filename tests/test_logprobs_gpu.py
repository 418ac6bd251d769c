"""token_logprobs on the GPU: the kernel against the float64 reference (ids
exact, values within a derived bound), untouched rows and padding columns,
batch independence, ties, non-finite logits, the binding's refusals,
capture into a graph, and the pipelined engine with device_logprobs against
the synchronous step() loop.

Value bound: a thread of the 256-wide workgroup adds at most 504 positive
fp32 terms at vocab 128256 (63 vectors of 8; 501 on average), and the block
tree adds 8 more levels, so the normaliser carries at most 512 * 2^-24 ~
3.1e-5 relative error; exp, log and the two subtractions at |lp| < 32 add
under 1e-5.  1e-4 absolute covers both; ids admit no tolerance, bf16 logits
order exactly."""

import importlib.util
import pathlib

import pytest
import torch

from hyperspot import ops

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "logprobs_ref", pathlib.Path(__file__).with_name("logprobs_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

NINF = float("-inf")
TOL = 1e-4
SENT_V, SENT_I = 123.5, -77


def _call(logits, chosen, n_top):
    """Kernel on sentinel-filled outputs -> (val, id) on the CPU."""
    rows = logits.shape[0]
    val = torch.full((rows, 21), SENT_V, dtype=torch.float32, device="cuda")
    idx = torch.full((rows, 21), SENT_I, dtype=torch.int32, device="cuda")
    v, i = ops.token_logprobs(logits.cuda(), chosen.cuda(), n_top.cuda(),
                              val, idx)
    torch.cuda.synchronize()
    assert v is val and i is idx
    return val.cpu(), idx.cpu()


def _check(logits, chosen, n_top, val, idx):
    """ids exact, values within TOL; rows with n_top < 0 hold the
    sentinels.  Returns the largest value error."""
    rval, ridx = R.reference(
        logits, chosen, n_top,
        torch.full((logits.shape[0], 21), SENT_V, dtype=torch.float64),
        torch.full((logits.shape[0], 21), SENT_I, dtype=torch.long))
    assert torch.equal(idx.long(), ridx)
    err = R.max_abs_err(val, rval)
    assert err < TOL, err
    return err


@pytest.mark.parametrize("rows,vocab", [(16, 512), (16, 1003), (16, 4099),
                                        (4, 128256)])
def test_kernel_matches_fp64_reference(rows, vocab):
    logits, chosen, n_top = R.make_rows(rows, vocab, seed=vocab)
    val, idx = _call(logits, chosen, n_top)
    err = _check(logits, chosen, n_top, val, idx)
    print(f"V={vocab}: largest logprob error {err:.3g}")
    # rows that did not ask keep the sentinels; columns past n are padding
    for r in range(rows):
        n = int(n_top[r])
        if n < 0:
            assert bool((val[r] == SENT_V).all())
            assert bool((idx[r] == SENT_I).all())
        else:
            assert bool((idx[r, 1 + n:] == -1).all())
            assert bool((val[r, 1 + n:] == NINF).all())
            assert bool((idx[r, 1:1 + n] >= 0).all())
    # the same launch again: bit-identical
    val2, idx2 = _call(logits, chosen, n_top)
    assert torch.equal(val2, val) and torch.equal(idx2, idx)


@pytest.mark.parametrize("vocab", [1003, 4099])
def test_row_alone_equals_row_in_batch(vocab):
    logits, chosen, n_top = R.make_rows(10, vocab, seed=4)
    val, idx = _call(logits, chosen, n_top)
    for r in (1, 3, 4, 8):            # odd rows start off the 16-byte grid
        v1, i1 = _call(logits[r:r + 1].clone(), chosen[r:r + 1],
                       n_top[r:r + 1])
        assert torch.equal(v1[0], val[r]) and torch.equal(i1[0], idx[r])


def test_ties_resolve_by_ascending_id():
    vocab = 128256
    logits = R.make_rows(3, vocab, seed=8)[0]
    # a maximum tied over ids 100..199
    logits[0, 100:200] = 30.0
    # three distinct top values above a 50-token tie group
    logits[1, [70000, 9, 128255]] = torch.tensor([33.0, 32.0, 31.0],
                                                 dtype=torch.bfloat16)
    group = torch.arange(50) * 2001 + 17
    logits[1, group] = 30.0
    # a tie group on every 997th id: it crosses every chunk of the walk
    # and straddles the cut (one value above it, n = 20)
    logits[2, 5] = 31.0
    every = torch.arange(0, vocab, 997)
    logits[2, every] = 30.0
    chosen = torch.tensor([150, 9, 997 * 100])
    n_top = torch.tensor([5, 20, 20], dtype=torch.int32)
    val, idx = _call(logits, chosen, n_top)
    _check(logits, chosen, n_top, val, idx)
    assert idx[0, 1:6].tolist() == [100, 101, 102, 103, 104]
    assert idx[1, 1:21].tolist() == [70000, 9, 128255] + group[:17].tolist()
    assert idx[2, 1:21].tolist() == [5] + every[:19].tolist()
    assert val[0, 0] == val[0, 1] and val[2, 0] == val[2, 2]
    # -0 and +0 are one tie group
    z = torch.full((1, 1003), -4.0, dtype=torch.bfloat16)
    z[0, [900, 10, 400]] = torch.tensor([-0.0, 0.0, -0.0],
                                        dtype=torch.bfloat16)
    val, idx = _call(z, torch.tensor([400]), torch.tensor([3],
                                                          dtype=torch.int32))
    assert idx[0, :4].tolist() == [400, 10, 400, 900]
    assert val[0, 0] == val[0, 1] == val[0, 3]


def test_robustness_rows():
    vocab = 1003
    base = R.make_rows(1, vocab, seed=5)[0][0]
    logits = base.repeat(8, 1)
    logits[0] = NINF
    logits[0, [7, 500, 1002]] = torch.tensor([1.0, 2.0, 0.5],
                                             dtype=torch.bfloat16)
    logits[1, 5] = float("nan")
    logits[1, 6] = float("inf")
    logits[1, 1002] = -float("nan")
    logits[2] = NINF                            # nothing finite
    logits[3, 44] = NINF
    chosen = torch.tensor([500, 6, 3, 44, vocab, -1, 5, 0])
    n_top = torch.tensor([5, 20, 5, 1, 5, 5, -1, 0], dtype=torch.int32)
    val, idx = _call(logits, chosen, n_top)
    _check(logits, chosen, n_top, val, idx)
    assert idx[0, 1:6].tolist() == [500, 7, 1002, 0, 1]
    assert bool(torch.isfinite(val[0, 1:4]).all())
    assert val[0, 4:6].tolist() == [NINF, NINF]
    assert val[1, 0] == NINF                    # chosen on +inf
    assert not set(idx[1, 1:].tolist()) & {5, 6, 1002}
    assert val[2].tolist() == [NINF] * 21
    assert idx[2, :6].tolist() == [3, 0, 1, 2, 3, 4]
    assert val[3, 0] == NINF and val[3, 1] > NINF
    # chosen outside the vocabulary: -inf, the alternatives undisturbed
    for r in (4, 5):
        assert val[r, 0] == NINF and int(idx[r, 0]) == int(chosen[r])
        assert torch.equal(idx[r, 1:], idx[4, 1:])
        assert torch.equal(val[r, 1:], val[4, 1:])
    assert bool((val[6] == SENT_V).all())
    assert idx[7].tolist() == [0] + [-1] * 20


def test_binding_checks_its_arguments():
    logits, chosen, n_top = R.make_rows(4, 64, seed=0)
    lg, ch, nt = logits.cuda(), chosen.cuda(), n_top.cuda()
    val = torch.empty(4, 21, dtype=torch.float32, device="cuda")
    idx = torch.empty(4, 21, dtype=torch.int32, device="cuda")
    C = ops._native()
    C.token_logprobs(val, idx, lg, ch, nt)
    with pytest.raises(RuntimeError):
        C.token_logprobs(val, idx, lg, ch, nt.long())          # dtype
    with pytest.raises(RuntimeError):
        C.token_logprobs(val, idx, lg, ch, nt[:3])             # a row short
    with pytest.raises(RuntimeError):
        C.token_logprobs(val, idx, lg.t().contiguous().t(), ch, nt)
    with pytest.raises(RuntimeError):
        C.token_logprobs(val, idx, lg, ch.cpu(), nt)
    with pytest.raises(RuntimeError):
        C.token_logprobs(val[:, :20].contiguous(), idx, lg, ch, nt)
    with pytest.raises(RuntimeError):
        C.token_logprobs(val, torch.empty(4, 22, dtype=torch.int32,
                                          device="cuda"), lg, ch, nt)
    torch.cuda.synchronize()


def test_capturable():
    rows, vocab = 10, 4099
    logits, chosen, n_top = R.make_rows(rows, vocab, seed=9)
    lg, ch, nt = logits.cuda(), chosen.cuda(), n_top.cuda()
    val = torch.full((rows, 21), SENT_V, dtype=torch.float32, device="cuda")
    idx = torch.full((rows, 21), SENT_I, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.token_logprobs(lg, ch, nt, val, idx)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.token_logprobs(lg, ch, nt, val, idx)
    val.fill_(SENT_V)
    idx.fill_(SENT_I)
    g.replay()
    torch.cuda.synchronize()
    _check(logits, chosen, n_top, val.cpu(), idx.cpu())
    # new per-row parameters, in place: the same graph follows them
    chosen2 = (chosen + 17) % vocab
    n_top2 = n_top.roll(2)
    ch.copy_(chosen2)
    nt.copy_(n_top2)
    val.fill_(SENT_V)
    idx.fill_(SENT_I)
    g.replay()
    torch.cuda.synchronize()
    _check(logits, chosen2, n_top2, val.cpu(), idx.cpu())
    ev, ei = _call(logits, chosen2, n_top2)
    assert torch.equal(val.cpu(), ev) and torch.equal(idx.cpu(), ei)


# ---- engine ----

def _run(batch, pipelined, eager, staggered):
    from hyperspot.engine import EngineConfig, LLMEngine, SamplingParams
    cfg = EngineConfig(model="tiny-llama-d128", max_num_seqs=64,
                       max_num_batched_tokens=2048, max_model_len=128,
                       num_gpu_blocks=512, graph_batch_sizes=(4, 8),
                       prefill_graph_sizes=(), device_sampling=True,
                       device_logprobs=True, enforce_eager=eager)
    eng = LLMEngine(cfg, device="cuda:0")
    free0 = eng.runner.block_manager.num_free
    kinds = [dict(temperature=0.0, logprobs=0),
             dict(temperature=0.0, logprobs=5),
             dict(temperature=0.0),
             dict(temperature=0.9, top_k=40, seed=7, logprobs=20)]
    for i in range(batch):
        prompt = [(5 * i + 3 * j + 1) % 500 + 4 for j in range(14 + i % 5)]
        sp = SamplingParams(max_tokens=12 + 5 * (i % 3) if staggered else 16,
                            ignore_eos=True, **kinds[i % 4])
        eng.add_request(prompt, sp, request_id=f"r{i}")
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


@pytest.mark.parametrize("batch,eager", [(3, False), (7, False), (3, True)])
def test_pipelined_engine_equals_synchronous(batch, eager):
    # equal max_tokens, no stops: the same graph and shapes run every
    # step, so the records agree exactly, floats included
    ref = _run(batch, False, eager, staggered=False)
    got = _run(batch, True, eager, staggered=False)
    assert got == ref
    for i in range(batch):
        toks, fin, recs = ref[f"r{i}"]
        assert len(toks) == 16 and fin == "length"
        want = [0, 5, None, 20][i % 4]
        if want is None:
            assert recs == [None] * 16
            continue
        for tok, (cid, lp, top) in zip(toks, recs):
            assert cid == tok and lp <= 0.0 and len(top) == want
            if want and i % 4 != 3:
                assert top[0] == (tok, lp)       # greedy: the argmax
    # rows leave at different times: buckets and re-seeds differ between
    # the two loops, so only what does not depend on them is compared
    ref = _run(batch, False, eager, staggered=True)
    got = _run(batch, True, eager, staggered=True)
    for rid in ref:
        assert got[rid][0] == ref[rid][0] and got[rid][1] == ref[rid][1]
        assert len(got[rid][2]) == len(ref[rid][2])
        assert [r and (r[0], len(r[2])) for r in got[rid][2]] == \
            [r and (r[0], len(r[2])) for r in ref[rid][2]]

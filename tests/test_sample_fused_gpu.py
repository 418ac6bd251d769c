"""sample_fused on the GPU: the kernel against the float64 reference (kept
set and CDF interval of every returned token), its distribution, greedy
rows, capture into a graph, and the pipelined engine with device_sampling
against the synchronous step() loop, token for token."""

import importlib.util
import pathlib

import pytest
import torch

from hyperspot import ops

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "sample_fused_ref",
    pathlib.Path(__file__).with_name("sample_fused_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


def _gpu(*ts):
    return [t.cuda() for t in ts]


def _call(logits, t, p, k, u):
    out = ops.sample_fused(*_gpu(logits, t, p, k, u))
    torch.cuda.synchronize()
    return out.cpu()


# 1003 and 4099 are no multiples of 8: rows start off the 16-byte grid and
# end inside a vector.  Row 7 of each cycle has k = 10^8 >= V: off.
@pytest.mark.parametrize("rows,vocab", [(16, 512), (16, 1003), (16, 4099),
                                        (8, 128256)])
def test_kernel_matches_fp64_reference(rows, vocab):
    logits, u = R.make_logits(rows, vocab, seed=vocab)
    t, p, k = R.row_params(rows)
    out = _call(logits, t, p, k, u)
    margin = R.check_rows(logits, t, p, k, u, out)
    print(f"V={vocab}: smallest top-p margin {margin:.3g}")
    # k >= V is k off
    k_off = torch.where(k >= vocab, torch.zeros_like(k), k)
    assert torch.equal(_call(logits, t, p, k_off, u), out)


@pytest.mark.parametrize("tkp", [(0.8, 0, 1.0), (0.8, 40, 0.95)])
def test_distribution_on_stratified_uniforms(tkp):
    n, vocab = 4096, 512
    row, _ = R.make_logits(1, vocab, seed=11)
    ref = R.Ref(row[0], *tkp)
    assert ref.margin > R.TOL
    u = (torch.arange(n, dtype=torch.float64) + 0.5) / n
    t = torch.full((n,), tkp[0], dtype=torch.float32)
    k = torch.full((n,), tkp[1], dtype=torch.int32)
    p = torch.full((n,), tkp[2], dtype=torch.float32)
    u32 = u.to(torch.float32)
    out = _call(row.expand(n, vocab).contiguous(), t, p, k, u32)
    got = torch.bincount(out, minlength=vocab)
    want = torch.bincount(
        torch.searchsorted(ref.cdf, u32.double(), right=True).clamp(
            max=vocab - 1), minlength=vocab)
    assert int(got[~ref.kept].sum()) == 0, "a dropped token was returned"
    assert int((got - want).abs().max()) <= 1


def test_greedy_rows():
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(64, 128256, generator=g) * 3).to(
        torch.bfloat16).cuda()
    logits[5, 100:200] = logits[5].max()            # a tied maximum
    zeros = torch.zeros(64, device="cuda")
    ones = torch.ones(64, device="cuda")
    k = torch.full((64,), 40, dtype=torch.int32, device="cuda")
    u = torch.rand(64, generator=g).cuda()
    want = ops.greedy_sample(logits)
    assert torch.equal(ops.sample_fused(logits, zeros, ones * 0.9, k, u),
                       want)
    # every other row stochastic: the greedy rows are unchanged
    t = zeros.clone()
    t[1::2] = 0.8
    out = ops.sample_fused(logits, t, ones * 0.9, k, u)
    assert torch.equal(out[0::2], want[0::2])
    assert not torch.equal(out[1::2], want[1::2])


def test_robustness_rows():
    vocab = 1003
    ninf = float("-inf")
    logits = torch.full((6, vocab), ninf, dtype=torch.bfloat16)
    logits[:, [7, 500, 1002]] = torch.tensor(
        [1.0, 2.0, 0.5], dtype=torch.bfloat16)
    logits[3] = R.make_logits(1, vocab, seed=5)[0][0]
    logits[4] = logits[3]
    logits[5] = logits[3]
    t = torch.tensor([1.0, 0.7, 1.0, 1.0, 1.0, 1.0])
    p = torch.tensor([1.0, 0.9, 1.0, 1.0, 1.0, 0.5])
    k = torch.tensor([0, 2, 1, 1, 0, 0], dtype=torch.int32)
    u = torch.tensor([0.999, 0.0, 0.5, 0.7, 0.0, 0.0])
    out = _call(logits, t, p, k, u)
    R.check_rows(logits, t, p, k, u, out, need_margin=False)
    assert out[:3].tolist() == [1002, 7, 500]
    assert int(out[3]) == int(logits[3].float().argmax())     # k = 1
    assert int(out[4]) == 0 and int(out[5]) >= 0              # u = 0
    # nothing finite at all: the argmax convention, no fault
    dead = torch.full((2, vocab), ninf, dtype=torch.bfloat16)
    assert _call(dead, t[:2], p[:2], k[:2], u[:2]).tolist() == [0, 0]


def test_deterministic():
    logits, u = R.make_logits(32, 4099, seed=2)
    t, p, k = R.row_params(32)
    a = _call(logits, t, p, k, u)
    b = _call(logits, t, p, k, u)
    assert torch.equal(a, b)


def test_binding_checks_its_arguments():
    logits, u = R.make_logits(4, 64, seed=0)
    t, p, k = R.row_params(4)
    lg, t, p, k, u = _gpu(logits, t, p, k, u)
    out = torch.empty(4, dtype=torch.long, device="cuda")
    C = ops._native()
    with pytest.raises(RuntimeError):
        C.sample_fused(out, lg, t, p, k[:3], u)
    with pytest.raises(RuntimeError):
        C.sample_fused(out, lg, t, p, k.long(), u)
    with pytest.raises(RuntimeError):
        C.sample_fused(out, lg.t().contiguous().t(), t, p, k, u)
    with pytest.raises(RuntimeError):
        C.sample_fused(out, lg, t.cpu(), p, k, u)


def test_capturable():
    rows, vocab = 16, 4099
    logits, u = R.make_logits(rows, vocab, seed=9)
    t, p, k = R.row_params(rows)
    lg, t, p, k, u = _gpu(logits, t, p, k, u)
    out = torch.zeros(rows, dtype=torch.long, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.sample_fused(lg, t, p, k, u, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.sample_fused(lg, t, p, k, u, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.sample_fused(lg, t, p, k, u))
    # new per-row parameters, in place: the same graph follows them
    u.copy_(torch.rand(rows, generator=torch.Generator().manual_seed(1)))
    k.fill_(3)
    g.replay()
    torch.cuda.synchronize()
    eager = ops.sample_fused(lg, t, p, k, u)
    assert torch.equal(out, eager)
    R.check_rows(logits, t.cpu(), p.cpu(), k.cpu(), u.cpu(), out.cpu(),
                 need_margin=False)


# ---- engine ----

def _run(batch, pipelined, eager, stops=None):
    from hyperspot.engine import EngineConfig, LLMEngine, SamplingParams
    cfg = EngineConfig(model="tiny-llama-d128", max_num_seqs=64,
                       max_num_batched_tokens=2048, max_model_len=128,
                       num_gpu_blocks=512, graph_batch_sizes=(4, 8),
                       prefill_graph_sizes=(), device_sampling=True,
                       enforce_eager=eager)
    eng = LLMEngine(cfg, device="cuda:0")
    free0 = eng.runner.block_manager.num_free
    kinds = [dict(temperature=0.0),
             dict(temperature=0.8, seed=5),
             dict(temperature=1.2, top_k=20, seed=7),
             dict(top_p=0.9, seed=9)]
    for i in range(batch):
        prompt = [(5 * i + 3 * j + 1) % 500 + 4 for j in range(14 + i % 5)]
        sp = SamplingParams(max_tokens=11 if i == 1 else 24 + 3 * (i % 4),
                            stop_token_ids=(stops or {}).get(i, ()),
                            **kinds[i % 4])
        eng.add_request(prompt, sp, request_id=f"r{i}")
    out = {f"r{i}": [[], None] for i in range(batch)}
    step = eng.step_pipelined if pipelined else eng.step
    engaged = False
    while eng.has_work():
        for o in step():
            out[o.request_id][0].append(o.token_id)
            if o.finished:
                out[o.request_id][1] = o.finish_reason.value
        engaged |= eng._inflight is not None
    assert engaged == pipelined
    assert eng.runner.block_manager.num_free == free0
    return out


@pytest.mark.parametrize("batch,eager", [(3, False), (7, False), (3, True)])
def test_pipelined_engine_equals_synchronous(batch, eager):
    base = _run(batch, False, eager)
    # a stochastic row stops on a token it is seen to emit mid-run
    stops = {2: (base["r2"][0][9],)}
    ref = _run(batch, False, eager, stops)
    got = _run(batch, True, eager, stops)
    assert got == ref
    assert ref["r2"][1] == "stop" and len(ref["r2"][0]) <= 10
    assert len(ref["r1"][0]) == 11 and ref["r1"][1] == "length"

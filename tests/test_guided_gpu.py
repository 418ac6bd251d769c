"""The guided-decoding kernels on the GPU (csrc/guided.hip) against their
torch twins, exact by value: the mask over vocabularies on and off the
16-byte grid, guided and unguided rows interleaved, states from the corpus
walk plus DEAD and the depth cap; the advance over every (state, token) pair
of the walk in one launch; the binding's refusals, capture into a graph, and
the pipelined engine with device_guided against the synchronous step() loop.

There is no tolerance anywhere: the state is integers, and the mask either
leaves a logit alone or makes it -inf."""

import importlib.util
import pathlib

import pytest
import torch

from hyperspot import ops
from hyperspot.engine.guided import JsonByteMachine
from hyperspot.ops import torch_ref as TR

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "guided_ref", pathlib.Path(__file__).with_name("guided_ref.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

W = TR.GUIDED_WORDS
POISON = [-1, 0x5a5a5a5, -7, 0x7fffffff, 12345, -1, -1, 3, 3, 3, 3]


def _pool():
    """States to draw from: the walk's distinct ones, DEAD, the cap."""
    pool = [w for w, _ in G.distinct_states()]
    deep = G.nested(TR.GUIDED_MAX_DEPTH, "mixed")
    deep_arr = G.nested(TR.GUIDED_MAX_DEPTH)
    almost = G.nested(TR.GUIDED_MAX_DEPTH - 1)
    return pool, [G.dead_state(), deep.pack(), deep_arr.pack(),
                  almost.pack()]


def _states(rows, seed):
    """Guided and -1 rows interleaved (odd rows unguided, with poison in
    the words behind the -1)."""
    pool, special = _pool()
    g = torch.Generator().manual_seed(seed)
    out = []
    for r in range(rows):
        if r % 2:
            out.append(POISON)
        elif (r // 2) < len(special) and seed % 2:
            out.append(special[(r // 2 + seed) % len(special)])
        else:
            out.append(pool[int(torch.randint(len(pool), (1,),
                                              generator=g))])
    return torch.tensor(out, dtype=torch.int32)


def _bits(x):
    return x.view(torch.int16)


@pytest.mark.parametrize("vocab", [264, 261, 512])
@pytest.mark.parametrize("rows", [1, 2, 3, 4, 5])
def test_mask_matches_twin(rows, vocab):
    for seed in (2 * rows, 2 * rows + 1):
        st = _states(rows, seed)
        lg = G.finite_logits(rows, vocab, seed=seed, dtype=torch.bfloat16)
        want = lg.clone()
        TR.guided_json_mask(want, st)
        got = lg.cuda()
        if vocab == 261 and rows >= 3:
            assert got[1].data_ptr() % 16 and got[2].data_ptr() % 16
        ops.guided_json_mask(got, st.cuda())
        torch.cuda.synchronize()
        got = got.cpu()
        assert torch.equal(got, want)
        un = st[:, 0] < 0
        assert torch.equal(_bits(got[un]), _bits(lg[un]))     # bit-identical
        keep = want > float("-inf")
        assert torch.equal(_bits(got)[keep], _bits(lg)[keep])  # kept bits
        assert bool((~keep[~un]).any())


def test_mask_off_the_grid_writes_nothing_outside():
    """The rows as a view that starts 3 elements into its buffer."""
    rows, vocab = 5, 261
    st = _states(rows, 7)
    st[3] = torch.tensor(G.dead_state(), dtype=torch.int32)   # guided odd row
    lg = G.finite_logits(rows, vocab, seed=7, dtype=torch.bfloat16)
    want = lg.clone()
    TR.guided_json_mask(want, st)
    buf = torch.full((rows * vocab + 16,), 1.5, dtype=torch.bfloat16,
                     device="cuda")
    view = buf[3:3 + rows * vocab].view(rows, vocab)
    view.copy_(lg)
    assert view.data_ptr() % 16 == 6 and view.is_contiguous()
    ops.guided_json_mask(view, st.cuda())
    torch.cuda.synchronize()
    assert torch.equal(view.cpu(), want)
    flat = buf.cpu()
    assert bool((flat[:3] == 1.5).all())
    assert bool((flat[3 + rows * vocab:] == 1.5).all())


def test_mask_large_vocabulary():
    rows, vocab = 3, 128256
    st = _states(rows, 11)
    st[1] = torch.tensor(G.nested(3, "mixed").pack(), dtype=torch.int32)
    st[2, 0] = -1
    lg = G.finite_logits(rows, vocab, seed=5, dtype=torch.bfloat16)
    want = lg.clone()
    TR.guided_json_mask(want, st)
    got = lg.cuda()
    ops.guided_json_mask(got, st.cuda())
    torch.cuda.synchronize()
    got = got.cpu()
    assert torch.equal(got, want)
    assert torch.equal(_bits(got[2]), _bits(lg[2]))
    assert bool((got[:2, 260:] == float("-inf")).all())


def test_advance_matches_twin_in_one_launch():
    steps = G.distinct_steps()
    pool, special = _pool()
    states = [s for s, _, _ in steps]
    toks = [t for _, t, _ in steps]
    # every state of the walk against bytes it mostly refuses, the special
    # states against everything, tokens outside the bytes, unguided rows
    for k, w in enumerate(pool):
        for b in (k % 256, (37 * k + 11) % 256, ord('"'), ord("}")):
            states.append(w)
            toks.append(b + 4)
    for w in special:
        for b in range(256):
            states.append(w)
            toks.append(b + 4)
    for k, t in enumerate((0, 1, 2, 3, 260, 511, 128255, 1 << 40, -1)):
        states.append(pool[(7 * k) % len(pool)])
        toks.append(t)
    for t in (5, ord("[") + 4):
        states.append(POISON)
        toks.append(t)
    assert len(states) > 500
    st = torch.tensor(states, dtype=torch.int32)
    tok = torch.tensor(toks, dtype=torch.long)
    want = st.clone()
    TR.guided_json_advance(want, tok)
    n = len(steps)
    assert torch.equal(want[:n], torch.tensor([a for _, _, a in steps],
                                              dtype=torch.int32))
    assert int((want[:, 0] == TR.GUIDED_DEAD).sum()) > 100
    got = st.cuda()
    ops.guided_json_advance(got, tok.cuda())
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want)


def test_words_no_machine_packs_read_as_dead():
    """Any word values: both kernels stay inside the row and the logits."""
    bad = [[99] + [0] * 10, [0, 0, 257] + [0] * 8, [0, 0, -5] + [0] * 8,
           [17, 0, 2 ** 31 - 1] + [-1] * 8, [8, 0, 0] + [0] * 8,
           [8, (3 << 4) | (7 << 6), 0] + [0] * 8,
           [2 ** 31 - 1] * 11, [1, -1, 0] + [-1] * 8, [3, -1, 0] + [0] * 8]
    st = torch.tensor(bad, dtype=torch.int32)
    lg = G.finite_logits(len(bad), 264, seed=9, dtype=torch.bfloat16)
    want = lg.clone()
    TR.guided_json_mask(want, st)
    got = lg.cuda()
    ops.guided_json_mask(got, st.cuda())
    assert torch.equal(got.cpu(), want)
    for tok in (ord("]") + 4, ord("}") + 4, ord("1") + 4):
        t = torch.full((len(bad),), tok, dtype=torch.long)
        w = st.clone()
        TR.guided_json_advance(w, t)
        g = st.cuda()
        ops.guided_json_advance(g, t.cuda())
        torch.cuda.synchronize()
        assert torch.equal(g.cpu(), w)


def test_binding_checks_its_arguments():
    C = ops._native()
    st = torch.tensor([JsonByteMachine().pack()] * 4, dtype=torch.int32,
                      device="cuda")
    lg = torch.zeros(4, 264, dtype=torch.bfloat16, device="cuda")
    tok = torch.tensor([5, 6, 7, 8], device="cuda")
    C.guided_json_mask(lg, st)
    C.guided_json_advance(st, tok)
    with pytest.raises(RuntimeError, match="260"):
        C.guided_json_mask(lg[:, :256].contiguous(), st)     # V < 260
    with pytest.raises(ValueError, match="260"):
        ops.guided_json_mask(lg[:, :259].contiguous(), st)
    with pytest.raises(RuntimeError):
        C.guided_json_mask(lg.float(), st)                   # dtype
    with pytest.raises(RuntimeError):
        C.guided_json_mask(lg, st.long())
    with pytest.raises(RuntimeError):
        C.guided_json_mask(lg, st[:3])                       # a row short
    with pytest.raises(RuntimeError):
        C.guided_json_mask(lg, st[:, :10].contiguous())      # words
    with pytest.raises(RuntimeError):
        C.guided_json_mask(lg[:, :262], st)                  # strided
    with pytest.raises(RuntimeError):
        C.guided_json_mask(lg, st.cpu())
    with pytest.raises(RuntimeError):
        C.guided_json_advance(st, tok.int())
    with pytest.raises(RuntimeError):
        C.guided_json_advance(st[:3], tok)
    with pytest.raises(RuntimeError):
        C.guided_json_advance(st, tok.cpu())
    torch.cuda.synchronize()


def test_capturable_mask_sample_advance():
    """The graph's tail on its own: documents come out of a replayed graph
    whose logits favour the document's next byte."""
    docs = [d for d in G.corpus() if 8 <= len(d) <= 40][:5]
    rows, vocab = 2 * len(docs), 512
    st = torch.full((rows, W), -1, dtype=torch.int32)
    st[::2] = torch.tensor(JsonByteMachine().pack(), dtype=torch.int32)
    st = st.cuda()
    lg = torch.empty(rows, vocab, dtype=torch.bfloat16, device="cuda")
    sampled = torch.zeros(rows, dtype=torch.long, device="cuda")

    def tail():
        ops.guided_json_mask(lg, st)
        ops.greedy_sample(lg, out=sampled)
        ops.guided_json_advance(st, sampled)

    keep = st.clone()
    lg.zero_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tail()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tail()
    st.copy_(keep)
    out = [[] for _ in docs]
    for pos in range(max(len(d) for d in docs) + 1):
        fresh = G.finite_logits(rows, vocab, seed=pos, dtype=torch.bfloat16)
        fresh[:, 300] = 50.0                    # outside the grammar: masked
        for i, d in enumerate(docs):
            fresh[2 * i, d[pos] + 4 if pos < len(d) else 2] = 40.0
        lg.copy_(fresh)
        g.replay()
        torch.cuda.synchronize()
        toks = sampled.cpu().tolist()
        for i in range(len(docs)):
            out[i].append(toks[2 * i])
            assert toks[2 * i + 1] == 300       # unguided rows: undisturbed
    for d, o in zip(docs, out):
        assert bytes(t - 4 for t in o[:len(d)]) == d
        assert o[len(d):] == [2] * (len(o) - len(d))
    assert bool((st[1::2] == -1).all())


# ---- engine ----

def _run(pipelined, others):
    from hyperspot.engine import EngineConfig, LLMEngine, SamplingParams
    flags = dict(device_penalties=True, max_penalty_seqs=8,
                 device_sampling=True, device_logprobs=True) if others else {}
    cfg = EngineConfig(model="tiny-llama-d128", max_num_seqs=64,
                       max_num_batched_tokens=2048, max_model_len=128,
                       num_gpu_blocks=512, graph_batch_sizes=(4, 8),
                       prefill_graph_sizes=(), device_guided=True, **flags)
    eng = LLMEngine(cfg, device="cuda:0", eos_token_id=2)
    free0 = eng.runner.block_manager.num_free
    batch = 7
    for i in range(batch):
        prompt = [(5 * i + 3 * j + 1) % 500 + 4 for j in range(14 + i % 5)]
        kw = {}
        if i % 2 == 0:
            kw.update(response_format="json")                # 4 of the 7
        if others:
            kw.update(logprobs=[0, 5, None][i % 3])
            if i % 4 != 1:
                kw.update(frequency_penalty=0.7, repetition_penalty=1.2)
            if i % 3:
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


@pytest.mark.parametrize("others", [False, True])
def test_pipelined_engine_equals_synchronous(others):
    # equal max_tokens, no stops: the same graph and shapes run every step,
    # so tokens, finish reasons and the records' floats agree exactly
    ref = _run(False, others)
    got = _run(True, others)
    assert got == ref
    for i in range(7):
        toks, fin, _ = got[f"r{i}"]
        assert len(toks) == 16 and fin == "length"
        if i % 2 == 0:
            m = JsonByteMachine()
            for t in toks:
                m.feed_token(t)                # ValueError = a masked byte
            assert all(t == 2 or 4 <= t < 260 for t in toks)

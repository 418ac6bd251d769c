"""GPU side of the decode pipeline: the decode_advance kernel against its
torch_ref twin, and the pipelined engine (captured graphs with the
device-side head and the argmax tail) against the synchronous step() loop,
token for token."""

import pytest
import torch

from hyperspot import ops
from hyperspot.ops import torch_ref

pytestmark = pytest.mark.gpu


def _advance_case():
    rows, max_blocks, page = 8, 2, 16
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 500, (rows,), generator=g)
    # rows 0..3 step to positions 14, 15 (page end), 16 (page start: new_blk
    # installs) and 31 (last slot of the last table column); row 4 is a
    # host-id row at position 0; rows 5..7 are padding
    pos = torch.tensor([13, 14, 15, 30, 99, 7, 7, 7])
    lens = (pos + 1).to(torch.int32)
    slots = torch.randint(0, 99, (rows,), generator=g)
    bt = torch.randint(0, 64, (rows, max_blocks), generator=g).to(torch.int32)
    sampled = torch.randint(0, 500, (rows,), generator=g)
    ctl = torch.full((4 * rows + 4,), -1, dtype=torch.int32)
    ctl[:rows] = torch.tensor([2, 3, 0, 1, -1, -2, -2, -2])   # permuted
    ctl[rows + 2] = 57
    ctl[2 * rows + 4] = 321
    ctl[3 * rows + 4] = 0
    ctl[4 * rows] = 5
    return [ids, pos, lens, slots, bt, sampled, ctl], page


def test_decode_advance_matches_ref():
    t, page = _advance_case()
    ref = [x.clone() for x in t]
    torch_ref.decode_advance(*ref, page)
    dev = [x.cuda() for x in t]
    ops.decode_advance(*dev, page)
    torch.cuda.synchronize()
    for name, a, b in zip(("ids", "pos", "lens", "slots", "tables"),
                          dev[:5], ref[:5]):
        assert torch.equal(a.cpu(), b), name
    ids, pos, lens, slots, bt = ref[:5]
    assert pos.tolist() == [14, 15, 16, 31, 0, 0, 0, 0]
    assert ids[:5].tolist() == [int(t[5][2]), int(t[5][3]), int(t[5][0]),
                                int(t[5][1]), 321]
    assert int(bt[2, 1]) == 57 and int(slots[2]) == 57 * 16
    assert int(slots[3]) == int(t[4][3, 1]) * 16 + 15     # last column
    assert slots[5:].tolist() == [-1, -1, -1]
    assert lens[5:].tolist() == [1, 1, 1] and ids[5:].tolist() == [0, 0, 0]
    # pass-through: the host filled the inputs, the kernel leaves them
    dev[6][4 * 8] = -1
    before = [x.clone() for x in dev[:5]]
    ops.decode_advance(*dev, page)
    torch.cuda.synchronize()
    for a, b in zip(dev[:5], before):
        assert torch.equal(a, b)


def _run(batch, sizes, pipelined, stops=None):
    from hyperspot.engine import EngineConfig, LLMEngine, SamplingParams
    cfg = EngineConfig(model="tiny-llama-d128", max_num_seqs=64,
                       max_num_batched_tokens=2048, max_model_len=128,
                       num_gpu_blocks=512, graph_batch_sizes=sizes,
                       prefill_graph_sizes=())
    eng = LLMEngine(cfg, device="cuda:0")
    free0 = eng.runner.block_manager.num_free
    for i in range(batch):
        p = [(5 * i + 3 * j + 1) % 500 + 4 for j in range(14 + i % 5)]
        sp = SamplingParams(
            temperature=0.0,
            max_tokens=11 if i == 1 else 40,          # a max_tokens row
            stop_token_ids=(stops or {}).get(i, ()))
        eng.add_request(p, sp, request_id=f"r{i}")
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


@pytest.mark.parametrize("batch,sizes", [(5, (4, 8)), (33, (32, 48))])
def test_pipelined_engine_equals_synchronous(batch, sizes):
    base = _run(batch, sizes, False)
    # rows 0 and 3 stop on a token they are seen to emit mid-run
    stops = {0: (base["r0"][0][20],), 3: (base["r3"][0][27],)}
    ref = _run(batch, sizes, False, stops)
    got = _run(batch, sizes, True, stops)
    assert got == ref
    assert ref["r0"][1] == "stop" and len(ref["r0"][0]) <= 21
    assert len(ref["r1"][0]) == 11 and ref["r1"][1] == "length"
    assert len(ref["r2"][0]) == 40 and ref["r2"][1] == "length"

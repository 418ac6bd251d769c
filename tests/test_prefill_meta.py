"""Prefill step metadata (CPU): a step that packs a chunked-prefill
continuation beside a fresh request carries each request's chunk_start as
``meta.ctx_start`` — what the flash prefill over the paged cache consumes —
and attention over that metadata still equals the per-row reference."""

import torch

import hyperspot.ops as ops
from hyperspot.engine import EngineConfig, SamplingParams
from hyperspot.engine.model_runner import ModelRunner
from hyperspot.engine.request import Request
from hyperspot.engine.scheduler import Scheduler
from hyperspot.ops import torch_ref as R


def _mixed_step(**kw):
    """Step 2 of: A (100 tokens, budget 64) + B (20 tokens) -> A's
    continuation chunk (64, 36) packed with the fresh B (0, 20)."""
    cfg = EngineConfig(model="tiny-llama", max_num_seqs=4,
                       max_num_batched_tokens=64, max_model_len=256,
                       num_gpu_blocks=64, enforce_eager=True, seed=5, **kw)
    runner = ModelRunner(cfg, device="cpu")
    sched = Scheduler(cfg, runner.block_manager)
    sp = SamplingParams(temperature=0.0, max_tokens=2)
    a = Request(request_id="a", sampling=sp,
                prompt_token_ids=[(i * 7) % 500 + 3 for i in range(100)])
    b = Request(request_id="b", sampling=sp,
                prompt_token_ids=[(i * 11) % 500 + 3 for i in range(20)])
    sched.add(a)
    sched.add(b)
    first = sched.schedule()
    assert [(r.chunk_start, r.chunk_len) for r in first.requests] == [(0, 64)]
    _, meta1 = runner._prefill_inputs(first)
    second = sched.schedule()
    assert [r.request_id for r in second.requests] == ["a", "b"]
    _, meta2 = runner._prefill_inputs(second)
    return runner, first, meta1, second, meta2


def test_ctx_start_is_chunk_start_for_mixed_step():
    _, first, meta1, second, meta = _mixed_step()
    # a fresh-only step: ctx_start is all zero and the fresh kernel applies
    assert meta1.fresh_prefill is True
    assert meta1.ctx_start.dtype == torch.int32
    assert meta1.ctx_start.tolist() == [0]
    # continuation + fresh request in one step
    want = [r.chunk_start for r in second.requests]
    assert want == [64, 0]
    assert meta.ctx_start.dtype == torch.int32
    assert meta.ctx_start.tolist() == want
    assert meta.fresh_prefill is False
    assert meta.seq_start.tolist() == [0, 36, 56]
    assert meta.max_seqlen == 36
    assert torch.equal(meta.ctx_lens,
                       (meta.positions + 1).to(torch.int32))
    # positions restart from each request's ctx_start
    ss = meta.seq_start.tolist()
    for z, cs in enumerate(want):
        n = ss[z + 1] - ss[z]
        assert meta.positions[ss[z]:ss[z + 1]].tolist() == \
            list(range(cs, cs + n))
        # the block table covers every page the step's rows attend
        assert meta.block_tables.shape[1] >= (cs + n + 15) // 16


def test_paged_mfma_follows_engine_config():
    """The MFMA kernel over the paged cache is opt-in: off by default, so a
    default engine computes what it always did."""
    assert EngineConfig().prefill_paged_mfma is False
    assert _mixed_step()[4].paged_mfma is False
    assert _mixed_step(prefill_paged_mfma=True)[4].paged_mfma is True


def test_cpu_attention_matches_paged_ref_for_mixed_step():
    runner, _, _, second, meta = _mixed_step()
    spec = runner.spec
    H, KV, D = spec.num_heads, spec.num_kv_heads, spec.head_dim
    g = torch.Generator().manual_seed(3)
    k_cache = torch.randn(runner.kv_caches[0][0].shape, generator=g)
    v_cache = torch.randn(k_cache.shape, generator=g)
    T = int(meta.seq_start[-1])
    q = torch.randn(T, H, D, generator=g)
    k = torch.randn(T, KV, D, generator=g)   # unused off the fresh path
    v = torch.randn(T, KV, D, generator=g)
    scale = D ** -0.5
    out = ops.attention(q, k, v, k_cache, v_cache, meta, scale)
    ref = R.prefill_attn_paged(q, k_cache, v_cache, meta.block_tables,
                               meta.ctx_lens, meta.row_seq, scale)
    assert torch.equal(out, ref)
    # the same thing stated per sequence from (seq_start, ctx_start): row i
    # of sequence z attends cache positions 0 .. ctx_start[z] + i
    ss = meta.seq_start.tolist()
    BS = k_cache.shape[2]
    for z, cs in enumerate(meta.ctx_start.tolist()):
        n = ss[z + 1] - ss[z]
        pos = torch.arange(cs + n)
        blk = meta.block_tables[z, pos // BS].long()
        ks = k_cache[blk, :, pos % BS]          # [cs+n, KV, D]
        vs = v_cache[blk, :, pos % BS]
        qs = q[ss[z]:ss[z + 1]].view(n, KV, H // KV, D)
        att = torch.einsum("mkgd,nkd->kgmn", qs, ks) * scale
        masked = pos[None, :] > (cs + torch.arange(n))[:, None]
        att = att.masked_fill(masked, float("-inf"))
        o = torch.einsum("kgmn,nkd->mkgd", att.softmax(-1), vs)
        assert torch.allclose(out[ss[z]:ss[z + 1]], o.reshape(n, H, D),
                              atol=1e-5, rtol=1e-5)

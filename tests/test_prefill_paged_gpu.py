"""GPU tests for the MFMA flash prefill over the paged KV cache
(csrc/attn_prefill_paged_mfma.hip): continuation chunks, prefix hits, fp8
caches, strided q, row-invariance against the fresh-prefill kernel, and the
engine paths that dispatch to it.

Every cache is poisoned: each slot no valid position uses, every unused
page and the page that block-table padding points at hold NaN (byte 0x7f
for e4m3fn).  An over-read shows up as a NaN in ``out``, never as a fault.
"""

import functools

import pytest
import torch

import hyperspot.ops as ops
from hyperspot.ops import torch_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
D, BS, NB = 128, 16, 64
SCALE = D ** -0.5
# fp32-reference tolerance of test_attn_prefill_mfma_vs_ref: same math
TOL = 2.5e-2


def setup_module():
    assert ops.have_native(), \
        "hyperspot._C must be built on GPU boxes (python csrc/build.py)"


def _poisoned_cache(KV, fp8):
    if fp8:
        return torch.full((NB, KV, BS, D), 0x7f, dtype=torch.uint8)
    return torch.full((NB, KV, BS, D), float("nan"), dtype=torch.bfloat16)


def _as_cache(t, fp8):
    return t.view(torch.float8_e4m3fn) if fp8 else t


def _write(cache, fp8, pages, pos, vals):
    """vals [len(pos), KV, D] (fp32) -> cache slots of positions `pos`."""
    blk = pages[pos // BS]
    if fp8:
        cache[blk, :, pos % BS] = vals.to(torch.float8_e4m3fn) \
            .view(torch.uint8)
    else:
        cache[blk, :, pos % BS] = vals.bfloat16()


@functools.lru_cache(maxsize=None)
def _case(cases, H, KV, fp8, seed=0):
    """cases: tuple of (ctx_start, n).  Returns CPU tensors + the fp32
    reference, built once per distinct case and shared between tests."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(NB, generator=g)
    nan_page, free = int(perm[-1]), perm[:-1]
    need = [(cs + n + BS - 1) // BS for cs, n in cases]
    assert sum(need) <= NB - 1
    max_blocks = max(need) + 2
    bt = torch.full((len(cases), max_blocks), nan_page, dtype=torch.int32)
    kc, vc = _poisoned_cache(KV, fp8), _poisoned_cache(KV, fp8)
    used = 0
    for z, (cs, n) in enumerate(cases):
        pages = free[used:used + need[z]]
        used += need[z]
        bt[z, :need[z]] = pages.to(torch.int32)
        if n == 0:
            continue          # nothing of this sequence may be touched
        pos = torch.arange(cs + n)
        _write(kc, fp8, pages, pos,
               torch.randn(cs + n, KV, D, generator=g))
        _write(vc, fp8, pages, pos,
               torch.randn(cs + n, KV, D, generator=g) * (0.5 if fp8 else 1))
    T = sum(n for _, n in cases)
    q = (torch.randn(T, H, D, generator=g) * (0.5 if fp8 else 1)).bfloat16()
    starts = [0]
    for _, n in cases:
        starts.append(starts[-1] + n)
    positions = torch.cat([torch.arange(cs, cs + n) for cs, n in cases])
    row_seq = torch.cat([torch.full((n,), z, dtype=torch.int32)
                         for z, (_, n) in enumerate(cases)])
    kc, vc = _as_cache(kc, fp8), _as_cache(vc, fp8)
    ref = R.prefill_attn_paged(q.float(), kc.float(), vc.float(), bt,
                               (positions + 1).to(torch.int32), row_seq,
                               SCALE)
    assert torch.isfinite(ref).all()
    return dict(q=q, kc=kc, vc=vc, bt=bt, ref=ref,
                seq_start=torch.tensor(starts, dtype=torch.int32),
                ctx_start=torch.tensor([cs for cs, _ in cases],
                                       dtype=torch.int32),
                max_n=max(n for _, n in cases))


def _run(c, max_seqlen=None, q=None):
    from hyperspot import _C
    q = c["q"].to(DEV) if q is None else q
    out = torch.full(q.shape, float("nan"), dtype=torch.bfloat16, device=DEV)
    _C.attn_prefill_paged_mfma(
        out, q, c["kc"].to(DEV), c["vc"].to(DEV), c["bt"].to(DEV),
        c["seq_start"].to(DEV), c["ctx_start"].to(DEV),
        c["max_n"] if max_seqlen is None else max_seqlen, SCALE)
    return out.float().cpu()


def _check(out, ref):
    assert torch.isfinite(out).all(), \
        f"{(~torch.isfinite(out)).sum().item()} non-finite outputs"
    err = (out - ref).abs().max().item()
    print(f"max_abs_err={err:.5f}")
    assert torch.allclose(out, ref, atol=TOL, rtol=TOL), err


# (a) continuation shapes: 48 page- but not tile-aligned, 100 not
# page-aligned, 300 rows cross the 256-row q tile, (0, 64) mixes a fresh
# request in; group 8; MHA
SHAPES = [
    (((48, 33), (100, 7), (0, 64), (256, 300)), 8, 2),
    (((17, 16), (63, 1)), 8, 1),
    (((130, 260),), 4, 4),
]


@pytest.mark.parametrize("cases,H,KV", SHAPES)
def test_continuation_vs_ref(cases, H, KV):
    c = _case(cases, H, KV, False)
    _check(_run(c), c["ref"])


def test_empty_workgroups_when_max_seqlen_exceeds_every_seq():
    """max_seqlen 600 -> three q tiles per (seq, head); tiles 2 and 3 own no
    row of any sequence and must return before touching anything."""
    c = _case(((48, 33), (100, 7)), 8, 2, False)
    _check(_run(c, max_seqlen=600), c["ref"])


def test_empty_sequence_between_real_ones():
    """n_z == 0 is legal: its (all-poison) block-table row is never read."""
    c = _case(((48, 33), (20, 0), (0, 64)), 8, 2, False)
    assert c["seq_start"].tolist() == [0, 33, 33, 97]
    _check(_run(c), c["ref"])


# (c) e4m3fn caches; reference over cache.float(): kernel math only
@pytest.mark.parametrize("cases,H,KV", SHAPES[:2])
def test_fp8_cache_vs_dequant_ref(cases, H, KV):
    c = _case(cases, H, KV, True)
    assert c["kc"].dtype == torch.float8_e4m3fn
    _check(_run(c), c["ref"])


# (d) q as a view into the fused qkv projection buffer
def test_strided_q_view():
    cases, H, KV = SHAPES[0]
    c = _case(cases, H, KV, False)
    T = c["q"].shape[0]
    qkv = torch.full((T, (H + 2 * KV) * D), float("nan"),
                     dtype=torch.bfloat16, device=DEV)
    qkv[:, :H * D] = c["q"].to(DEV).view(T, H * D)
    q = qkv[:, :H * D].view(T, H, D)
    assert not q.is_contiguous() and q.stride(0) == (H + 2 * KV) * D
    _check(_run(c, q=q), c["ref"])


# (b) row-invariance: the chunk-invariance guarantee
def test_rows_match_fresh_kernel_whole_and_chunked():
    """With ctx_start = 0 every row equals the fresh-prefill kernel's, and
    so do the rows of the 300-token sequence computed as chunks (0, 192)
    and (192, 108).  Bit for bit: both kernels instantiate one body
    (csrc/attn_prefill_core.h), so no difference is licensed."""
    from hyperspot import _C
    lens, H, KV = [5, 300, 64], 8, 2
    T = sum(lens)
    g = torch.Generator().manual_seed(11)
    q = torch.randn(T, H, D, generator=g).bfloat16().to(DEV)
    k = torch.randn(T, KV, D, generator=g).bfloat16().to(DEV)
    v = torch.randn(T, KV, D, generator=g).bfloat16().to(DEV)
    starts = [0, 5, 305, 369]
    ss = torch.tensor(starts, dtype=torch.int32, device=DEV)
    fresh = torch.empty_like(q)
    _C.attn_prefill_mfma(fresh, q, k, v, ss, max(lens), SCALE)

    perm = torch.randperm(NB, generator=g)
    nan_page, free = int(perm[-1]), perm[:-1]
    need = [(n + BS - 1) // BS for n in lens]
    bt = torch.full((3, max(need) + 2), nan_page, dtype=torch.int32)
    kc = _poisoned_cache(KV, False).to(DEV)
    vc = _poisoned_cache(KV, False).to(DEV)
    pages, used = [], 0
    for z, n in enumerate(lens):
        pages.append(free[used:used + need[z]])
        bt[z, :need[z]] = pages[z].to(torch.int32)
        used += need[z]

    def write(z, lo, hi):
        pos = torch.arange(lo, hi)
        blk = pages[z][pos // BS].to(DEV)
        rows = slice(starts[z] + lo, starts[z] + hi)
        kc[blk, :, (pos % BS).to(DEV)] = k[rows]
        vc[blk, :, (pos % BS).to(DEV)] = v[rows]

    # the 300-token sequence first, as two chunks against a cache that
    # holds only what the engine would have written by then
    bt1 = bt[1:2].to(DEV)
    chunked = torch.full((300, H, D), float("nan"), dtype=torch.bfloat16,
                         device=DEV)
    for lo, hi in ((0, 192), (192, 300)):
        write(1, lo, hi)
        _C.attn_prefill_paged_mfma(
            chunked[lo:hi], q[5 + lo:5 + hi], kc, vc, bt1,
            torch.tensor([0, hi - lo], dtype=torch.int32, device=DEV),
            torch.tensor([lo], dtype=torch.int32, device=DEV), hi - lo,
            SCALE)
    write(0, 0, 5)
    write(2, 0, 64)
    whole = torch.full_like(q, float("nan"))
    _C.attn_prefill_paged_mfma(
        whole, q, kc, vc, bt.to(DEV), ss,
        torch.zeros(3, dtype=torch.int32, device=DEV), max(lens), SCALE)

    fresh = fresh.float().cpu()
    for name, got, want in (("whole", whole.float().cpu(), fresh),
                            ("chunked", chunked.float().cpu(),
                             fresh[5:305])):
        assert torch.isfinite(got).all(), name
        diff = (got != want).sum().item()
        print(f"{name}: {diff} of {got.numel()} elements differ, "
              f"max_abs_diff={(got - want).abs().max().item():.3e}")
        assert torch.equal(got, want), name


def test_binding_rejects_bad_arguments():
    from hyperspot import _C
    c = _case(((17, 16), (63, 1)), 8, 1, False)
    args = dict(q=c["q"].to(DEV), kc=c["kc"].to(DEV), vc=c["vc"].to(DEV),
                bt=c["bt"].to(DEV), ss=c["seq_start"].to(DEV),
                cs=c["ctx_start"].to(DEV))

    def call(**kw):
        a = dict(args, **kw)
        out = torch.empty(a["q"].shape, dtype=torch.bfloat16, device=DEV)
        _C.attn_prefill_paged_mfma(out, a["q"], a["kc"], a["vc"], a["bt"],
                                   a["ss"], a["cs"], 16, SCALE)

    with pytest.raises(RuntimeError, match="head_dim must be 128"):
        call(q=torch.zeros(17, 8, 64, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        call(vc=torch.zeros(NB, 1, BS, D, dtype=torch.float8_e4m3fn,
                            device=DEV))
    with pytest.raises(RuntimeError, match="bfloat16 or float8_e4m3fn"):
        call(kc=args["kc"].half(), vc=args["vc"].half())
    with pytest.raises(RuntimeError, match="page size must be 16"):
        call(kc=torch.zeros(NB, 1, 32, D, dtype=torch.bfloat16, device=DEV),
             vc=torch.zeros(NB, 1, 32, D, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(RuntimeError, match="ctx_start must be"):
        call(cs=args["cs"][:1].contiguous())
    with pytest.raises(RuntimeError, match="block_tables"):
        call(bt=args["bt"].long())


@pytest.mark.parametrize("rows,enabled,mfma", [
    (16, True, False), (17, True, True), (17, False, False)])
def test_op_layer_dispatch(monkeypatch, rows, enabled, mfma):
    """ops.attention on a continuation step: the new kernel runs only when
    the step asks for it (meta.paged_mfma, off by default) and its longest
    chunk is above the short-chunk rule (decode-shaped steps stay on the
    per-row kernel); either way the result is the reference's."""
    from hyperspot.models.llama import ForwardMeta
    assert ops._PAGED_MFMA_MAX_PER_ROW == 16
    ran = []
    for name in ("attn_prefill_paged_mfma", "paged_attn"):
        real = getattr(ops._C, name)
        monkeypatch.setattr(
            ops._C, name,
            lambda *a, _r=real, _n=name: (ran.append(_n), _r(*a))[1])
    cases = ((40, rows), (100, 7))
    c = _case(cases, 8, 2, False)
    positions = torch.cat([torch.arange(cs, cs + n) for cs, n in cases])
    meta = ForwardMeta(
        mode="prefill", positions=positions.to(DEV), slot_mapping=None,
        seq_start=c["seq_start"].to(DEV), max_seqlen=rows,
        fresh_prefill=False, ctx_start=c["ctx_start"].to(DEV),
        paged_mfma=enabled,
        ctx_lens=(positions + 1).to(torch.int32).to(DEV),
        row_seq=torch.cat([torch.full((n,), z, dtype=torch.int32)
                           for z, (_, n) in enumerate(cases)]).to(DEV),
        block_tables=c["bt"].to(DEV))
    q = c["q"].to(DEV)
    # the poison stays in: the per-row kernel, too, must not let the unused
    # slots of a partly filled page reach its result
    kc, vc = c["kc"].to(DEV), c["vc"].to(DEV)
    out = ops.attention(q, None, None, kc, vc, meta, SCALE)
    assert ran == ["attn_prefill_paged_mfma" if mfma else "paged_attn"]
    _check(out.float().cpu(), c["ref"])


# (e) engine level, on the head-dim-128 tiny preset.  220 tokens: with a
# 64-token budget the chunks are (0,64) (64,64) (128,64) (192,28), and a
# prefix hit leaves 28 rows — every continuation step is above the
# short-chunk rule, so with prefill_paged_mfma on all of them run the new
# kernel
PROMPT = [(i * 37) % 500 + 3 for i in range(220)]


def _engine(**kw):
    from hyperspot.engine import EngineConfig, LLMEngine
    base = dict(model="tiny-llama-d128", max_num_seqs=4,
                max_num_batched_tokens=8192, max_model_len=512,
                num_gpu_blocks=128, enforce_eager=True, seed=4,
                prefill_paged_mfma=True)
    base.update(kw)
    return LLMEngine(EngineConfig(**base), device="cuda:0")


@pytest.fixture
def paged_calls(monkeypatch):
    """Counts launches of the new kernel made through the op layer."""
    real = ops._C.attn_prefill_paged_mfma
    calls = []

    def counting(*a):
        calls.append(1)
        return real(*a)

    monkeypatch.setattr(ops._C, "attn_prefill_paged_mfma", counting)
    return calls


def test_engine_chunked_prefill_matches_unchunked(paged_calls):
    from hyperspot.engine import SamplingParams
    sp = SamplingParams(temperature=0.0, max_tokens=6)
    whole = _engine().generate([PROMPT], sp)[0]
    assert len(paged_calls) == 0          # fresh prefill: the other kernel
    chunked = _engine(max_num_batched_tokens=64).generate([PROMPT], sp)[0]
    # continuation chunks (64,64) (128,64) (192,28) x 2 layers
    assert len(paged_calls) == 6, len(paged_calls)
    assert len(whole) == 6
    assert chunked == whole
    # off (the default): the same steps stay on the per-row kernel
    from hyperspot.engine import EngineConfig
    assert EngineConfig().prefill_paged_mfma is False
    off = _engine(max_num_batched_tokens=64, prefill_paged_mfma=False)
    assert len(off.generate([PROMPT], sp)[0]) == 6
    assert len(paged_calls) == 6, len(paged_calls)


def test_engine_prefix_caching_matches_uncached(paged_calls):
    from hyperspot.engine import SamplingParams
    sp = SamplingParams(temperature=0.0, max_tokens=4)
    plain = _engine().generate([PROMPT], sp)[0]
    assert len(paged_calls) == 0
    eng = _engine(enable_prefix_caching=True)
    a = eng.generate([PROMPT], sp)[0]
    assert len(paged_calls) == 0          # first run: nothing cached yet
    b = eng.generate([PROMPT], sp)[0]     # prefix hit: starts mid-prompt
    assert eng.runner.block_manager.cache_hits == 1
    assert len(paged_calls) == 2, len(paged_calls)
    assert a == plain and b == plain


def test_engine_fp8_kv_chunked_prefill(paged_calls):
    """fp8 KV + chunked prefill runs the new kernel on an e4m3fn cache.
    Tokens are not compared with an unchunked fp8 run: the fresh path reads
    the chunk's own K/V unquantized, so it may legitimately differ."""
    from hyperspot.engine import SamplingParams
    eng = _engine(max_num_batched_tokens=64, kv_dtype="fp8")
    assert eng.runner.kv_caches[0].dtype == torch.float8_e4m3fn
    out = eng.generate([PROMPT],
                       SamplingParams(temperature=0.0, max_tokens=6))[0]
    assert len(out) == 6
    assert len(paged_calls) == 6, len(paged_calls)

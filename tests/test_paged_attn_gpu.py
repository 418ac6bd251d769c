"""paged_attn (csrc/attn_paged.hip) over poisoned caches: the D=128 v3
kernel (bf16 and e4m3fn caches, every GQA group, page split with its merge
kernel), the D=64 generic kernel, per-row (row_seq) mode with a strided q,
bit-exactness at one token of context, and the combinations the launcher
must refuse.

Caches come from paged_cache_ref.py: random page permutations, NaN in every
slot no valid position uses.  `out` and the split workspace start as NaN
too, so a row, a head or a z-block that is skipped shows as well.  The
reference (torch_ref, over cache.float()) slices to the valid length, so
poison never enters it.

Precondition kept, not tested: ctx_lens >= 1.  Padding rows of the runner
carry 1, and a row of length 0 has no defined result.
"""

import functools
import importlib.util
import pathlib

import pytest
import torch

import hyperspot.ops as ops
from hyperspot.ops import torch_ref as R

pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, pathlib.Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


P = _load("paged_cache_ref")

DEV = "cuda"
TOL = 2e-2          # the project's tolerance for this kernel, atol and rtol
# one token; both sides of a page edge; fewer pages than the four waves;
# more pages than one round of 4 * split
LENS = (1, 15, 16, 17, 48, 63, 64, 65, 100, 257)
GROUPS_128 = [(1, 2), (2, 2), (4, 2), (8, 1), (8, 2)]     # (group, KV)


def setup_module():
    assert ops.have_native(), \
        "hyperspot._C must be built on GPU boxes (python csrc/build.py)"


@functools.lru_cache(maxsize=None)
def _decode_case(group, KV, D, fp8):
    """CPU tensors + fp32 reference, built once and shared between tests."""
    g = torch.Generator().manual_seed(1000 * D + 10 * group + KV)
    kc, vc, bt, _ = P.build(LENS, KV, D, fp8, g)
    q = (torch.randn(len(LENS), group * KV, D, generator=g)
         * (0.5 if fp8 else 1)).bfloat16()
    lens = torch.tensor(LENS, dtype=torch.int32)
    ref = R.paged_attn_decode(q.float(), kc.float(), vc.float(), bt, lens,
                              D ** -0.5)
    assert torch.isfinite(ref).all()
    return dict(q=q, kc=kc, vc=vc, bt=bt, lens=lens, ref=ref)


def _workspace(rows, H, D, split):
    if split == 1:
        return None
    return torch.full((rows * H * split * (D + 2),), float("nan"),
                      dtype=torch.float32, device=DEV)


def _run(q, kc, vc, bt, lens, row_seq=None, split=1):
    from hyperspot import _C
    rows, H, D = q.shape
    out = torch.full((rows, H, D), float("nan"), dtype=torch.bfloat16,
                     device=DEV)
    _C.paged_attn(out, q, kc.to(DEV), vc.to(DEV), bt.to(DEV), lens.to(DEV),
                  None if row_seq is None else row_seq.to(DEV), D ** -0.5,
                  _workspace(rows, H, D, split), split)
    return out.float().cpu()


def _check(out, ref):
    bad = ~torch.isfinite(out)
    assert not bad.any(), \
        f"{int(bad.sum())} non-finite outputs, rows " \
        f"{bad.flatten(1).any(1).nonzero().flatten().tolist()}"
    err = (out - ref).abs().max().item()
    print(f"max_abs_err={err:.5f}")
    assert torch.allclose(out, ref, atol=TOL, rtol=TOL), err


@pytest.mark.parametrize("split", [1, 2, 16])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("group,KV", GROUPS_128)
def test_v3_decode_over_poisoned_cache(group, KV, fp8, split):
    """With split 16 a z-block owns pages 4z..4z+3 of every 64: for all
    but the longest row most z-blocks own nothing and must merge as
    empty."""
    c = _decode_case(group, KV, 128, fp8)
    out = _run(c["q"].to(DEV), c["kc"], c["vc"], c["bt"], c["lens"],
               split=split)
    _check(out, c["ref"])


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("group,KV", GROUPS_128)
def test_v3_decode_through_op_layer(group, KV, fp8):
    """ops.paged_attn_decode picks the split and sizes the workspace."""
    c = _decode_case(group, KV, 128, fp8)
    assert ops._attn_split(len(LENS), KV) > 1
    out = ops.paged_attn_decode(c["q"].to(DEV), c["kc"].to(DEV),
                                c["vc"].to(DEV), c["bt"].to(DEV),
                                c["lens"].to(DEV), 128 ** -0.5)
    _check(out.float().cpu(), c["ref"])


@pytest.mark.parametrize("group", [1, 2, 4, 8])
def test_generic_d64_decode_over_poisoned_cache(group):
    c = _decode_case(group, 2, 64, False)
    out = _run(c["q"].to(DEV), c["kc"], c["vc"], c["bt"], c["lens"])
    _check(out, c["ref"])


# ---- row_seq mode: several rows per sequence, each with its own depth ----

ROW_SEQ = [0] * 5 + [1] * 20
ROW_CTX = list(range(31, 36)) + list(range(1, 21))


@functools.lru_cache(maxsize=None)
def _row_case(group, KV, D, fp8):
    g = torch.Generator().manual_seed(77 + 1000 * D + 10 * group + KV)
    kc, vc, bt, _ = P.build((35, 20), KV, D, fp8, g)
    T, H = len(ROW_SEQ), group * KV
    q = (torch.randn(T, H, D, generator=g) * (0.5 if fp8 else 1)).bfloat16()
    ctx = torch.tensor(ROW_CTX, dtype=torch.int32)
    row_seq = torch.tensor(ROW_SEQ, dtype=torch.int32)
    ref = R.prefill_attn_paged(q.float(), kc.float(), vc.float(), bt, ctx,
                               row_seq, D ** -0.5)
    assert torch.isfinite(ref).all()
    return dict(q=q, kc=kc, vc=vc, bt=bt, ctx=ctx, row_seq=row_seq, ref=ref)


@pytest.mark.parametrize("group,KV,D,fp8", [
    (4, 2, 128, False), (4, 2, 128, True),
    (8, 2, 128, False), (8, 2, 128, True),
    (4, 2, 64, False), (8, 2, 64, False)])
def test_row_seq_mode_with_strided_q(group, KV, D, fp8):
    """Rows 31..35 tokens deep on one sequence and 1..20 deep on the
    other; q is a view into the fused qkv buffer, whose K and V parts hold
    NaN.  Every row but those at depth 16 and 32 ends in a partial page,
    and what lies beyond its depth there is poison or real tokens of later
    positions; neither may be seen."""
    c = _row_case(group, KV, D, fp8)
    T, H = c["q"].shape[:2]
    qkv = torch.full((T, (H + 2 * KV) * D), float("nan"),
                     dtype=torch.bfloat16, device=DEV)
    qkv[:, :H * D] = c["q"].to(DEV).view(T, H * D)
    q = qkv[:, :H * D].view(T, H, D)
    assert not q.is_contiguous() and q.stride(0) == (H + 2 * KV) * D
    out = _run(q, c["kc"], c["vc"], c["bt"], c["ctx"], row_seq=c["row_seq"])
    _check(out, c["ref"])


# ---- one token of context: softmax weight exactly 1 ----------------------

@pytest.mark.parametrize("group,KV,D,split", [
    (1, 2, 128, 1), (4, 2, 128, 1), (8, 2, 128, 1),
    (1, 2, 128, 2), (4, 2, 128, 2), (8, 2, 128, 2),
    (4, 2, 64, 1), (8, 2, 64, 1)])
def test_ctx1_output_is_v_bit_for_bit(group, KV, D, split):
    g = torch.Generator().manual_seed(5)
    B, H = 3, group * KV
    kc, vc, bt, pages = P.build((1,) * B, KV, D, False, g)
    q = torch.randn(B, H, D, generator=g).bfloat16()
    out = _run(q.to(DEV), kc, vc, bt, torch.ones(B, dtype=torch.int32),
               split=split)
    v = torch.stack([vc[int(pages[z][0]), :, 0] for z in range(B)])
    want = v[:, :, None, :].expand(B, KV, group, D).reshape(B, H, D)
    assert torch.equal(out.bfloat16().view(torch.int16),
                       want.contiguous().view(torch.int16))


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("group,KV", [(2, 2), (4, 2), (8, 1)])
def test_ctx1_fp8_decodes_every_code_exactly(group, KV, split):
    """The V rows of two sequences hold all 254 finite e4m3fn codes in
    code order (0 in place of the two NaN codes).  Every code is exact in
    bf16, so the output must be code.float(): an exhaustive check of the
    in-kernel fp8 -> f32 decode and of its byte order."""
    D, B, H = 128, 2, group * KV
    g = torch.Generator().manual_seed(6)
    bt, pages, nb = P.layout((1,) * B, 3, g)
    kc, vc = P.poisoned(nb, KV, D, True), P.poisoned(nb, KV, D, True)
    code = torch.arange(256, dtype=torch.uint8).view(B, 1, D)
    code[(code & 0x7f) == 0x7f] = 0
    for z in range(B):
        P.write(kc, True, pages[z], torch.arange(1),
                torch.randn(1, KV, D, generator=g))
        P.write(vc, True, pages[z], torch.arange(1),
                code[z:z + 1].expand(1, KV, D))
    q = (torch.randn(B, H, D, generator=g) * 0.5).bfloat16()
    out = _run(q.to(DEV), P.as_cache(kc, True), P.as_cache(vc, True), bt,
               torch.ones(B, dtype=torch.int32), split=split)
    want = code.view(P.FP8).float().expand(B, H, D)
    assert torch.isfinite(want).all()
    assert torch.equal(out, want), \
        f"{int((out != want).sum())} of {want.numel()} decoded values differ"


# ---- refused combinations -------------------------------------------------

@pytest.mark.parametrize("H,KV,D,fp8,split", [
    (6, 2, 128, False, 1),      # group 3 at D=128
    (8, 2, 96, False, 1),       # head dim 96
    (8, 2, 64, True, 1),        # fp8 cache at D=64
    (8, 2, 64, False, 2),       # page split at D=64
], ids=["group3_d128", "d96", "fp8_d64", "split2_d64"])
def test_unsupported_combinations_raise(H, KV, D, fp8, split):
    """An unsupported shape is an error, never a launch that leaves `out`
    unwritten or runs another kernel."""
    g = torch.Generator().manual_seed(7)
    kc, vc, bt, _ = P.build((5, 20), KV, D, fp8, g)
    q = torch.randn(2, H, D, generator=g).bfloat16().to(DEV)
    with pytest.raises(RuntimeError):
        _run(q, kc, vc, bt, torch.tensor([5, 20], dtype=torch.int32),
             split=split)
    torch.cuda.synchronize()

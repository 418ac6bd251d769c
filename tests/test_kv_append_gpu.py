"""rope_kv_append (csrc/rope_kv.hip): all three instantiations (D=128 bf16
and e4m3fn caches, D=64 bf16) on views into one fused qkv buffer, against
the float64 rotation in fp8_ref.py.

What is pinned: which bytes of the caches are written and that nothing else
is; that the bf16 cache holds the rotated k and the input v bit-for-bit;
the fp8 codes (V: one rounding of a bf16 value, exact; K: within one
ordinal of the float64 rotation rounded once, at most 1e-3 of them not
identical); that the fp8 cache saturates to +-448 and never stores a NaN
byte for finite or infinite input (NaN input is unspecified); and that the
cache the kernel writes is one paged_attn can read.

The CPU test holds the float64 rotation and its fp32 twin together on the
same inputs, so the 1e-3 cap can only be reached by the kernel.
"""

import functools
import importlib.util
import pathlib

import pytest
import torch

import hyperspot.ops as ops
from hyperspot.ops import torch_ref as R


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, pathlib.Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


F = _load("fp8_ref")
P = _load("paged_cache_ref")

gpu = pytest.mark.gpu
DEV = "cuda"
BS = P.BS
# H * D/4 = 384 (q) work items at D=128: 1.5 passes of the 256 threads
T, H, KV, NB, MAX_POS = 9, 12, 3, 8, 256
POS = [0, MAX_POS - 1, 2, 5, 9, 100, 101, 4, 7]
# page 1 gets two tokens; token 7 is not appended
SLOTS = [0, 17, 2, 18, 127, 33, 40, -1, 55]
SENTINEL = 0xa5
ROPE_TOL = 3e-2     # the project's tolerance for the rotated bf16 q/k
CODE_CAP = 1e-3
TWIN_CAP = 1e-4


@functools.lru_cache(maxsize=None)
def _inputs(D):
    g = torch.Generator().manual_seed(D)
    qkv = torch.randn(T, (H + 2 * KV) * D, generator=g).bfloat16()
    cos_sin = R.rope_cos_sin(torch.arange(MAX_POS), D, 500000.0)
    return qkv, cos_sin, torch.tensor(POS), torch.tensor(SLOTS)


def _split(qkv, D):
    t = qkv.shape[0]
    return (qkv[:, :H * D].view(t, H, D),
            qkv[:, H * D:(H + KV) * D].view(t, KV, D),
            qkv[:, (H + KV) * D:].view(t, KV, D))


def test_cpu_rope_twin_matches_fp64_on_fp8_codes():
    qkv, cos_sin, pos, _ = _inputs(128)
    k = _split(qkv, 128)[1]
    F.compare_codes(F.to_codes(F.rope32(k, cos_sin, pos)),
                    F.to_codes(F.rope64(k, cos_sin, pos)),
                    "rope fp32 twin", TWIN_CAP)


# ---- GPU -------------------------------------------------------------------

def _native():
    assert ops.have_native(), \
        "hyperspot._C must be built on GPU boxes (python csrc/build.py)"
    from hyperspot import _C
    return _C


def _sentinel_cache(nb, D, fp8, byte=SENTINEL):
    width = 1 if fp8 else 2
    raw = torch.full((nb, KV, BS, D * width), byte, dtype=torch.uint8,
                     device=DEV)
    return raw, raw.view(P.FP8 if fp8 else torch.bfloat16)


def _append(D, fp8):
    """Runs the kernel on the shared inputs.  Returns the qkv buffer after
    the call (CPU), and the raw bytes of both caches [NB, KV, BS, bytes]."""
    _C = _native()
    qkv0, cos_sin, pos, slots = _inputs(D)
    qkv = qkv0.to(DEV)
    q, k, v = _split(qkv, D)
    assert not k.is_contiguous() and k.stride(0) == (H + 2 * KV) * D
    kraw, kc = _sentinel_cache(NB, D, fp8)
    vraw, vc = _sentinel_cache(NB, D, fp8)
    _C.rope_kv_append(q, k, v, pos.to(DEV), cos_sin.to(DEV), slots.to(DEV),
                      kc, vc)
    return qkv.cpu(), kraw.cpu(), vraw.cpu()


def _written_rows(raw, slots):
    """[n, KV, bytes] cache rows of the appended tokens, after checking
    that every other byte still holds the sentinel."""
    live = slots[slots >= 0]
    assert live.unique().numel() == live.numel()
    rest = raw.clone()
    rest[live // BS, :, live % BS] = SENTINEL
    assert (rest == SENTINEL).all(), \
        f"{int((rest != SENTINEL).sum())} bytes written outside the slots"
    return raw[live // BS, :, live % BS]


def _check_rotation_and_v(qkv, D):
    qkv0, cos_sin, pos, _ = _inputs(D)
    q, k, v = _split(qkv, D)
    q0, k0, v0 = _split(qkv0, D)
    assert torch.equal(v.contiguous().view(torch.int16),
                       v0.contiguous().view(torch.int16)), "v was modified"
    for got, src in ((q, q0), (k, k0)):
        want = F.rope64(src, cos_sin, pos)
        assert torch.allclose(got.double(), want, atol=ROPE_TOL,
                              rtol=ROPE_TOL)


@gpu
@pytest.mark.parametrize("D", [128, 64])
def test_bf16_cache_holds_rotated_k_and_v_bit_for_bit(D):
    qkv, kraw, vraw = _append(D, False)
    _check_rotation_and_v(qkv, D)
    slots = _inputs(D)[3]
    live = slots >= 0
    _, k, v = _split(qkv, D)
    got_k = _written_rows(kraw, slots).view(torch.int16)
    got_v = _written_rows(vraw, slots).view(torch.int16)
    assert torch.equal(got_k, k[live].contiguous().view(torch.int16))
    assert torch.equal(got_v, v[live].contiguous().view(torch.int16))


@gpu
def test_fp8_cache_codes():
    D = 128
    qkv, kraw, vraw = _append(D, True)
    _check_rotation_and_v(qkv, D)
    qkv0, cos_sin, pos, slots = _inputs(D)
    live = slots >= 0
    _, k0, v0 = _split(qkv0, D)
    got_v = _written_rows(vraw, slots)
    assert torch.equal(got_v, F.to_codes(v0[live])), \
        f"{int((got_v != F.to_codes(v0[live])).sum())} V codes differ"
    got_k = _written_rows(kraw, slots)
    F.compare_codes(got_k, F.to_codes(F.rope64(k0, cos_sin, pos)[live]),
                    "fp8 K cache", CODE_CAP)


BIG = [448.0, 464.0, 480.0, 1000.0, torch.finfo(torch.bfloat16).max,
       float("inf")]


@gpu
def test_fp8_cache_saturates_and_never_stores_nan():
    """Position 0 rotates by the identity, so k reaches the convert as
    planted.  Inf * sin(0) makes the planted element's rotation partner
    NaN, so the infinities sit in a token of their own and only the
    planted elements of that token are looked at."""
    _C = _native()
    D, n = 128, len(BIG)
    qkv = torch.zeros(2, (H + 2 * KV) * D, dtype=torch.bfloat16)
    q, k, v = _split(qkv, D)
    vals = torch.tensor(BIG + [-x for x in BIG])
    fin = torch.isfinite(vals)
    # token 0: the finite values, in both halves of the head dim of k
    k[0, 0, :2 * n][fin] = vals[fin].bfloat16()
    k[0, 1, 64:64 + 2 * n][fin] = vals[fin].bfloat16()
    v[0, 2, 5:5 + 2 * n][fin] = vals[fin].bfloat16()
    # token 1: +-Inf
    k[1, 0, :2 * n][~fin] = vals[~fin].bfloat16()
    k[1, 1, 64:64 + 2 * n][~fin] = vals[~fin].bfloat16()
    v[1, 2, 5:5 + 2 * n][~fin] = vals[~fin].bfloat16()
    qkv = qkv.to(DEV)
    q, k, v = _split(qkv, D)
    cos_sin = R.rope_cos_sin(torch.arange(4), D, 500000.0)
    kraw, kc = _sentinel_cache(2, D, True)
    vraw, vc = _sentinel_cache(2, D, True)
    slots = torch.tensor([3, 20])
    _C.rope_kv_append(q, k, v, torch.zeros(2, dtype=torch.long, device=DEV),
                      cos_sin.to(DEV), slots.to(DEV), kc, vc)
    got_k = _written_rows(kraw.cpu(), slots)
    got_v = _written_rows(vraw.cpu(), slots)
    want = torch.tensor([F.CODE_MAX_POS] * n + [F.CODE_MAX_NEG] * n,
                        dtype=torch.uint8)
    for tok, m in ((0, fin), (1, ~fin)):
        for name, got in (("k lo", got_k[tok, 0, :2 * n]),
                          ("k hi", got_k[tok, 1, 64:64 + 2 * n]),
                          ("v", got_v[tok, 2, 5:5 + 2 * n])):
            assert torch.equal(got[m], want[m]), \
                (name, tok, [hex(int(c)) for c in got[m]])
    # nothing NaN anywhere in the finite token or in V; all else is zero
    assert not F.is_nan_code(got_k[0]).any()
    assert not F.is_nan_code(got_v).any()
    got_k[0, 0, :2 * n] = 0
    got_k[0, 1, 64:64 + 2 * n] = 0
    got_v[:, 2, 5:5 + 2 * n] = 0
    assert not (got_k[0] & 0x7f).any() and not (got_v & 0x7f).any()


@gpu
def test_d64_with_fp8_cache_raises():
    _C = _native()
    D = 64
    qkv0, cos_sin, pos, slots = _inputs(D)
    q, k, v = _split(qkv0.to(DEV), D)
    _, kc = _sentinel_cache(NB, D, True)
    _, vc = _sentinel_cache(NB, D, True)
    with pytest.raises(RuntimeError):
        _C.rope_kv_append(q, k, v, pos.to(DEV), cos_sin.to(DEV),
                          slots.to(DEV), kc, vc)
    torch.cuda.synchronize()


@gpu
def test_append_then_attend_fp8():
    """Three ragged sequences appended by the kernel into a NaN-poisoned
    e4m3fn pool, then read by paged_attn; the reference attends over the
    reference-quantised cache (float64 rotation, one rounding)."""
    _C = _native()
    D, Hq, lens = 128, 12, (5, 16, 37)
    g = torch.Generator().manual_seed(9)
    bt, pages, nb = P.layout(lens, 2, g)
    n = sum(lens)
    pos = torch.cat([torch.arange(m) for m in lens])
    slots = torch.cat([pages[z][torch.arange(m) // BS] * BS
                       + torch.arange(m) % BS for z, m in enumerate(lens)])
    qkv0 = torch.randn(n, (Hq + 2 * KV) * D, generator=g).bfloat16()
    cos_sin = R.rope_cos_sin(torch.arange(64), D, 500000.0)
    qkv = qkv0.to(DEV)
    q, k, v = _split(qkv, D)
    kraw, kc = _sentinel_cache(nb, D, True, byte=F.CODE_NAN)
    vraw, vc = _sentinel_cache(nb, D, True, byte=F.CODE_NAN)
    _C.rope_kv_append(q, k, v, pos.to(DEV), cos_sin.to(DEV), slots.to(DEV),
                      kc, vc)
    # decode: one fresh query per sequence over its whole length
    qd = (torch.randn(len(lens), Hq, D, generator=g) * 0.5).bfloat16()
    ctx = torch.tensor(lens, dtype=torch.int32)
    out = torch.full(qd.shape, float("nan"), dtype=torch.bfloat16,
                     device=DEV)
    _C.paged_attn(out, qd.to(DEV), kc, vc, bt.to(DEV), ctx.to(DEV), None,
                  D ** -0.5, None, 1)
    _, k0, v0 = _split(qkv0, D)
    kref, vref = P.poisoned(nb, KV, D, True), P.poisoned(nb, KV, D, True)
    kref[slots // BS, :, slots % BS] = F.to_codes(F.rope64(k0, cos_sin, pos))
    vref[slots // BS, :, slots % BS] = F.to_codes(v0)
    ref = R.paged_attn_decode(qd.float(), kref.view(P.FP8).float(),
                              vref.view(P.FP8).float(), bt, ctx, D ** -0.5)
    assert torch.isfinite(ref).all()
    out = out.float().cpu()
    assert torch.isfinite(out).all()
    err = (out - ref).abs().max().item()
    print(f"max_abs_err={err:.5f}")
    assert torch.allclose(out, ref, atol=2e-2, rtol=2e-2), err

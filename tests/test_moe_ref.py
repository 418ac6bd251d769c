"""Keeps tests/moe_ref.py honest, on the CPU: align_check accepts a plain
sort and rejects planted faults, every lattice input the GPU tests use is
exact in bf16, and the staged float64 chain equals the per-expert loop.
"""

import importlib.util
import pathlib

import numpy as np
import pytest
import torch

_spec = importlib.util.spec_from_file_location(
    "moe_ref", pathlib.Path(__file__).with_name("moe_ref.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

BM = M.MOE_BM


def _layout(name):
    T, K, E, ids = M.ROUTING[name]
    flat = ids.reshape(-1)
    nt = M.ntiles_for(flat.size, E)
    return flat, E, nt, M.python_align(flat, E, nt)


def test_routing_cases_are_what_they_claim():
    want = {
        "decode1": [0, 0, 0, 1, 0, 1, 0, 0], "full": [0, 0, 256, 0],
        "over": [257, 0, 0, 0], "tight": [257, 257, 1, 1],
        "ragged": [0, 300, 5, 0, 64, 231, 0, 0], "single": [40],
        "empty": [0, 0, 0, 0]}
    for name, counts in want.items():
        T, K, E, ids = M.ROUTING[name]
        assert ids.shape == (T, K)
        assert np.bincount(ids.reshape(-1), minlength=E).tolist() == counts
    T, K, E, ids = M.ROUTING["wide"]
    assert (ids[:, 0] != ids[:, 1]).all() and ids.max() < 64
    assert M.ntiles_for(T * K, E) == 65
    # tight: the padded length is exactly what the op allocates
    assert M.ntiles_for(516, 4) * BM == 2 * 512 + 2 * 256
    T, K, E, ids = M.XCD9
    assert M.ntiles_for(T * K, E) == 9 == -(-1025 // BM) + -(-769 // BM)


@pytest.mark.parametrize("name", list(M.ROUTING))
def test_align_check_accepts_plain_sort(name):
    flat, E, nt, (sid, te, inv) = _layout(name)
    M.align_check(flat, E, sid, te, inv)


def _planted(fault):
    """One fault at a time in the ragged layout (experts 1, 2, 4, 5 at
    sorted rows 0, 512, 768, 1024; 5 tiles used of 11)."""
    flat, E, nt, (sid, te, inv) = _layout("ragged")
    sid, te, inv = sid.copy(), te.copy(), inv.copy()
    if fault == "off_grid":          # expert 2's segment one row late
        sid[513:518] = sid[512:517].copy()
        sid[512] = -1
        inv[sid[513:518]] = np.arange(513, 518)
    elif fault == "duplicate":       # a pair twice in expert 2's segment
        sid[513] = sid[512]
    elif fault == "wrong_expert":    # swap a pair of expert 2 and expert 4
        a, b = sid[512], sid[768]
        sid[512], sid[768] = b, a
        inv[a], inv[b] = 768, 512
    elif fault == "tile_expert":     # shifted by one tile
        te[1:] = te[:-1].copy()
    elif fault == "inv_pad":         # inv_pos pointing at a pad row
        inv[sid[512]] = 600
    elif fault == "past_end":        # live entry past the last segment
        sid[5 * BM + 3] = 0
    return flat, E, sid, te, inv


@pytest.mark.parametrize("fault", ["off_grid", "duplicate", "wrong_expert",
                                   "tile_expert", "inv_pad", "past_end"])
def test_align_check_rejects_planted_fault(fault):
    with pytest.raises(AssertionError):
        M.align_check(*_planted(fault))


@pytest.mark.parametrize("plain", [False, True])
@pytest.mark.parametrize("name,fp8,N,K", sorted(set(M.GEMM_SHAPES)))
def test_lattice_gemm_is_exact_in_bf16(name, fp8, N, K, plain):
    # the generator asserts |sum| <= 256 for every (row, expert) pairing
    x, w, xs, ws = M.gemm_lattice(name, N, K, fp8, plain)
    assert x.abs().max() <= 2 and w.abs().max() <= 1
    flat, E, nt, (sid, te, inv) = _layout(name)
    Ktop = M.ROUTING[name][1]
    valid, ref, S = M.gemm_ref64(x, w, sid, te, 0 if plain else Ktop, xs, ws)
    assert valid.sum() == flat.size
    assert M.bf16_exact(ref[valid])
    assert torch.equal(M.round_bf16(ref[valid]).double(), ref[valid])
    if fp8:
        assert M.bf16_exact(xs) and len(ws.unique()) == 7
        assert len(xs) < 8 or len(xs.unique()) > 1
        assert x.to(torch.float8_e4m3fn).float().equal(x)


@pytest.mark.parametrize("name", ["ragged", "tight"])
def test_lattice_scales_tell_sorted_row_from_token(name):
    """An fp8 epilogue reading xs[p] (sorted row) for xs[pair / gather_div]
    (token) must change valid outputs without leaving the xs buffer: many
    rows p < T carry a different scale than their token."""
    T, K, E, ids = M.ROUTING[name]
    flat, E, nt, (sid, te, inv) = _layout(name)
    _, _, xs, _ = M.gemm_lattice(name, 256, 256, True, False)
    p = np.nonzero(sid[:T] >= 0)[0]
    differ = (xs[p] != xs[sid[p] // K]).sum().item()
    assert differ >= (100 if name == "ragged" else 4), differ


def test_lattice_xcd9_is_exact_in_bf16():
    x, w, _, _ = M.gemm_lattice("xcd9", 4352, 128, False, False,
                                routing=M.XCD9)
    assert x.shape == (1794, 128) and w.shape == (2, 4352, 128)


@pytest.mark.parametrize("name,H,I", M.OP_SHAPES)
@pytest.mark.parametrize("fp8", [False, True])
def test_lattice_op_first_gemm_is_exact(name, H, I, fp8):
    x, w13, w2, xs, w13s, w2s, wts = M.op_lattice(name, H, I, fp8)
    flat, E, nt, (sid, te, inv) = _layout(name)
    valid, ref, _ = M.gemm_ref64(x, w13, sid, te, M.ROUTING[name][1],
                                 xs, w13s)
    assert M.bf16_exact(ref[valid]) and M.bf16_exact(wts)


@pytest.mark.parametrize("T,K,hidden", [(1, 1, 8), (300, 2, 2056)])
def test_lattice_combine_is_exact_in_bf16(T, K, hidden):
    y, wts = M.lattice_combine_inputs(T, K, 2 * T * K, hidden, 5)
    inv = torch.randperm(2 * T * K)[:T * K]
    ref, _ = M.combine_ref64(y, wts, inv, K)
    assert M.bf16_exact(ref)


def test_round_bf16_rounds_once():
    # 1 + 2^-8 + 2^-30 is above the bf16 tie; through fp32 it lands ON the
    # tie and rounds to even (down)
    v = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -30, 3.0, -0.0, 2.0 ** -130],
                     dtype=torch.float64)
    got = M.round_bf16(v).double()
    assert got[0] == 1 + 2.0 ** -7 and got[1] == 3.0
    assert got[3] == 2.0 ** -130
    assert M.bf16_ulp(torch.tensor([1.0, 1.99, 2.0]).double()).tolist() == \
        [2.0 ** -7, 2.0 ** -7, 2.0 ** -6]


@pytest.mark.parametrize("name", ["ragged", "tight", "decode1"])
def test_staged_chain_matches_per_expert_loop(name):
    """gemm_ref64 -> silu_mul_ref64 -> gemm_ref64 -> combine_ref64 on randn
    inputs against the per-expert loop of test_moe_grouped_ffn_matches_ref
    in float64."""
    T, K, E, ids = M.routing_case(name)
    H, I = 64, 32
    g = torch.Generator().manual_seed(3)
    x = (0.3 * torch.randn(T, H, generator=g)).double()
    w13 = (0.05 * torch.randn(E, 2 * I, H, generator=g)).double()
    w2 = (0.05 * torch.randn(E, H, I, generator=g)).double()
    wts = torch.rand(T, K, generator=g).double()
    flat, E, nt, (sid, te, inv) = _layout(name)

    valid, h1, _ = M.gemm_ref64(x, w13, sid, te, K)
    a = M.silu_mul_ref64(h1)
    valid2, y, _ = M.gemm_ref64(a, w2, sid, te, 0)
    assert torch.equal(valid, valid2)
    out, _ = M.combine_ref64(y, wts, inv, K)

    ref = torch.zeros(T, H, dtype=torch.float64)
    for t in range(T):
        for k in range(K):
            e = int(ids[t, k])
            gu = x[t] @ w13[e].t()
            gg, uu = gu[:I], gu[I:]
            ref[t] += wts[t, k] * ((gg * torch.sigmoid(gg) * uu) @ w2[e].t())
    assert torch.isfinite(out).all()
    rel = ((out - ref).abs().max() / ref.abs().max()).item()
    assert rel <= 1e-12, rel


def test_silu_ref_edges():
    g = torch.tensor([0.0, -0.0, 88.0, -88.0, 1e4, -1e4])
    u = torch.full((6,), 3.0)
    r = M.silu_mul_ref64(torch.cat([g, u])[None])[0]
    assert r[0] == 0 and r[1] == 0 and r[4] == 3e4
    assert r[5] == 0 and torch.signbit(r[5])
    assert abs(r[2] / (88.0 * 3) - 1) < 1e-30 or r[2] == 264.0
    assert -1e-33 < r[3] < 0

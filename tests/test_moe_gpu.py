"""The MoE kernels of csrc/moe.hip, stage by stage through hyperspot._C
with buffers the test owns, against the references in moe_ref.py: align
exactly, the grouped GEMMs (bf16 and e4m3fn) exactly on lattice inputs and
within a rounding bound on randn inputs, silu_mul and combine against
float64, and the whole op against the staged chain.

No GEMM or combine is launched on an align result that has not passed
the host-side align_check.  Expert ids outside [0, E) are outside the
kernels' contract and are never fed.
"""

import functools
import importlib.util
import os
import pathlib
import subprocess
import sys

import pytest
import torch

import hyperspot.ops as ops

_spec = importlib.util.spec_from_file_location(
    "moe_ref", pathlib.Path(__file__).with_name("moe_ref.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

gpu = pytest.mark.gpu
DEV = "cuda"
BM = M.MOE_BM
NAN = float("nan")
BF, F8 = torch.bfloat16, torch.float8_e4m3fn


def _C():
    return ops._native()


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------ align
class Aligned:
    def __init__(self, T, K, E, ids):
        self.T, self.K, self.E = T, K, E
        self.ids = ids.to(DEV)
        self.flat = self.ids.reshape(-1).to(torch.int32)
        self.ntiles = M.ntiles_for(T * K, E)
        self.P = self.ntiles * BM
        self.sid = torch.full((self.P,), -7, dtype=torch.int32, device=DEV)
        self.te = torch.full((self.ntiles,), -7, dtype=torch.int32,
                             device=DEV)
        self.inv = torch.full((T * K,), -7, dtype=torch.int32, device=DEV)
        _C().moe_align(self.sid, self.te, self.inv, self.flat, E)
        self.sid_h, self.te_h = self.sid.cpu(), self.te.cpu()
        self.inv_h = self.inv.cpu()
        # the host check comes before anything is launched on the result
        M.align_check(self.flat.cpu().numpy(), E, self.sid_h.numpy(),
                      self.te_h.numpy(), self.inv_h.numpy())
        self.valid = self.sid_h >= 0
        self.used = (self.te_h >= 0).repeat_interleave(BM)


@functools.lru_cache(maxsize=None)
def aligned(name):
    if name == "xcd9":
        return Aligned(M.XCD9[0], M.XCD9[1], M.XCD9[2],
                       torch.from_numpy(M.XCD9[3].copy()))
    return Aligned(*M.routing_case(name))


@gpu
@pytest.mark.parametrize("name", M.GPU_CASES)
def test_align(name):
    al = aligned(name)       # prefilled with -7, checked on the host
    assert al.valid.sum().item() == al.T * al.K
    assert not (al.sid_h == -7).any() and not (al.te_h == -7).any()


# ----------------------------------------------------------- lattice GEMM
def _to_fp8_with_nan_rows(x, dead):
    q = x.to(F8)
    q.view(torch.uint8)[dead] = 0x7f          # e4m3fn NaN
    return q


def run_gemm(al, x, w, xs, ws, gather_div, splitk=1, wsp=None, out=None):
    """Launch one grouped GEMM into a NaN-prefilled out.  x/w are float32
    on the CPU holding bf16- (or, with scales, e4m3fn-) exact values, or
    already-quantised device tensors."""
    fp8 = xs is not None
    N = w.shape[1]
    if out is None:
        out = torch.full((al.P, N), NAN, dtype=BF, device=DEV)
    if fp8:
        _C().moe_gemm_fp8(out, x, xs, w, ws, al.sid, al.te, gather_div,
                          splitk, wsp)
    else:
        _C().moe_gemm(out, x, w, al.sid, al.te, gather_div, splitk, wsp)
    return out


def lattice_device_inputs(al, name, N, K, fp8, plain, routing=None):
    x, w, xs, ws = M.gemm_lattice(name, N, K, fp8, plain, routing)
    ref_in = (x, w, xs, ws)
    dead = ~al.valid
    if fp8:
        xd = x.to(F8)
        xsd = xs.clone()
        if plain:       # what GEMM 2 sees from an uninitialised h1
            xd = _to_fp8_with_nan_rows(x, dead)
            xsd[dead] = NAN
        dev_in = (xd.to(DEV), w.to(F8).to(DEV), xsd.to(DEV),
                  ws.reshape(-1).contiguous().to(DEV))
    else:
        xd = x.to(BF)
        if plain:
            xd[dead] = NAN
        dev_in = (xd.to(DEV), w.to(BF).to(DEV), None, None)
    return ref_in, dev_in


def check_lattice(al, out, ref_in, gather_div, what, unused_nan=True):
    """valid rows exact; pad rows of used tiles finite (gather mode);
    rows of unused tiles untouched.  Returns the count of differing
    elements (asserted 0)."""
    x, w, xs, ws = ref_in
    valid, ref, _ = M.gemm_ref64(x, w, al.sid_h, al.te_h, gather_div,
                                 xs, ws)
    assert torch.equal(valid, al.valid)
    o = out.cpu()
    want = M.round_bf16(ref[valid])
    assert torch.equal(want.double(), ref[valid]), "reference not exact"
    ndiff = (o[valid] != want).sum().item()
    print(f"{what}: {ndiff} of {want.numel()} elements differ")
    assert torch.equal(o[valid], want), (what, ndiff)
    if gather_div > 0:
        assert torch.isfinite(o[al.used & ~valid].float()).all(), \
            f"{what}: non-finite pad row in a used tile"
    if unused_nan:      # those blocks return before storing
        assert torch.isnan(o[~al.used].float()).all(), \
            f"{what}: a block of an unused tile stored"
    return ndiff


def lattice_gemm(name, fp8, N, K, plain, splitk=1, routing=None):
    al = aligned(name)
    gd = 0 if plain else al.K
    ref_in, (x, w, xs, ws) = lattice_device_inputs(al, name, N, K, fp8,
                                                   plain, routing)
    wsp = None
    if splitk > 1:
        wsp = torch.full((splitk * al.P * N,), NAN, dtype=torch.float32,
                         device=DEV)
    out = run_gemm(al, x, w, xs, ws, gd, splitk, wsp)
    what = f"{name} {'fp8' if fp8 else 'bf16'} N={N} K={K} " \
           f"{'plain' if plain else 'gather'} splitk={splitk}"
    check_lattice(al, out, ref_in, gd, what)
    return out.cpu()[al.valid]


# the two 6-chunk shapes run in the split-K test below, at splitk = 1 too
_GEMM_PARAMS = sorted(set(M.GEMM_SHAPES) - {("ragged", False, 256, 384),
                                            ("ragged", True, 256, 768)})


@gpu
@pytest.mark.parametrize("plain", [False, True], ids=["gather", "plain"])
@pytest.mark.parametrize("name,fp8,N,K", _GEMM_PARAMS)
def test_gemm_lattice_exact(name, fp8, N, K, plain):
    lattice_gemm(name, fp8, N, K, plain)


# ---------------------------------------------------------------- split-K
@gpu
@pytest.mark.parametrize("plain", [False, True], ids=["gather", "plain"])
@pytest.mark.parametrize("fp8,K", [(False, 384), (True, 768)],
                         ids=["bf16", "fp8"])
def test_gemm_splitk_exact(fp8, K, plain):
    """6 k-chunks; split 1, 2, 3 ways, each into a NaN-prefilled
    workspace, each exact and so equal to each other."""
    outs = [lattice_gemm("ragged", fp8, 256, K, plain, splitk=s)
            for s in (1, 2, 3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def _gemm_args(al, N, K, fp8, rows=None):
    rows = al.T if rows is None else rows
    out = torch.zeros(al.P, N, dtype=BF, device=DEV)
    if fp8:
        return [out, torch.zeros(rows, K, device=DEV).to(F8),
                torch.ones(rows, device=DEV),
                torch.zeros(al.E, N, K, device=DEV).to(F8),
                torch.ones(al.E * N, device=DEV), al.sid, al.te]
    return [out, torch.zeros(rows, K, dtype=BF, device=DEV),
            torch.zeros(al.E, N, K, dtype=BF, device=DEV), al.sid, al.te]


@gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_gemm_refuses_bad_splitk_and_alignment(fp8):
    al = aligned("ragged")
    fn = _C().moe_gemm_fp8 if fp8 else _C().moe_gemm
    K = 768 if fp8 else 384                     # 6 chunks
    base = _gemm_args(al, 256, K, fp8)

    def ws(n):
        return torch.zeros(n, dtype=torch.float32, device=DEV)
    full = al.P * 256
    with pytest.raises(RuntimeError):           # 4 does not divide 6
        fn(*base, al.K, 4, ws(4 * full))
    with pytest.raises(RuntimeError):           # one chunk per segment
        fn(*base, al.K, 6, ws(6 * full))
    with pytest.raises(RuntimeError):           # no workspace
        fn(*base, al.K, 2, None)
    with pytest.raises(RuntimeError):           # one element short
        fn(*base, al.K, 2, ws(2 * full - 1))
    with pytest.raises(RuntimeError):           # K = 192
        fn(*_gemm_args(al, 256, 192, fp8), al.K, 1, None)
    with pytest.raises(RuntimeError):           # N = 192
        fn(*_gemm_args(al, 192, K, fp8), al.K, 1, None)
    if fp8:
        with pytest.raises(RuntimeError):       # a single fp8 chunk
            fn(*_gemm_args(al, 256, 128, True), al.K, 1, None)
    _sync()


# ------------------------------------------------------- binding refusals
@gpu
def test_align_refuses_bad_shapes():
    T, K, E, ids = M.routing_case("ragged")
    flat = ids.reshape(-1).to(torch.int32).to(DEV)
    nt = M.ntiles_for(T * K, E)

    def i32(n):
        return torch.zeros(n, dtype=torch.int32, device=DEV)
    fn = _C().moe_align
    with pytest.raises(RuntimeError):           # sorted_ids != ntiles*256
        fn(i32(nt * BM - 1), i32(nt), i32(T * K), flat, E)
    with pytest.raises(RuntimeError):           # one tile short of worst
        fn(i32((nt - 1) * BM), i32(nt - 1), i32(T * K), flat, E)
    with pytest.raises(RuntimeError):           # inv_pos too short
        fn(i32(nt * BM), i32(nt), i32(T * K - 1), flat, E)
    with pytest.raises(RuntimeError):
        fn(i32(nt * BM), i32(nt), i32(T * K), flat, 0)
    big = M.ntiles_for(T * K, 65)
    with pytest.raises(RuntimeError):           # E > 64
        fn(i32(big * BM), i32(big), i32(T * K), flat, 65)
    _sync()


@gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_gemm_refuses_bad_shapes(fp8):
    al = aligned("ragged")
    fn = _C().moe_gemm_fp8 if fp8 else _C().moe_gemm
    N, K = 256, 256
    iw = 3 if fp8 else 2                         # index of w in the args
    isid = iw + (2 if fp8 else 1)

    def bad(mutate, gd=al.K, rows=None):
        a = _gemm_args(al, N, K, fp8, rows)
        mutate(a)
        with pytest.raises(RuntimeError):
            fn(*a, gd, 1, None)

    def set_(i, t):
        return lambda a: a.__setitem__(i, t(a[i]))
    bad(set_(0, lambda o: o[:-1].contiguous()))          # out rows
    bad(set_(0, lambda o: o[:, :128].contiguous()))      # out columns
    bad(set_(0, lambda o: o.reshape(-1)))                # out not 2-D
    bad(set_(isid, lambda s: s[:-1].contiguous()))       # sorted_ids short
    bad(set_(1, lambda x: x[:, :128].contiguous()))      # x.size(1) != K
    bad(lambda a: None, gd=0)                            # plain, T rows
    bad(lambda a: None, gd=0, rows=al.P - 1)
    bad(lambda a: None, gd=-1)
    bad(lambda a: None, rows=0)                          # pads read row 0
    if fp8:
        bad(set_(2, lambda s: s[:-1].contiguous()))      # xs short
        bad(set_(4, lambda s: s[:-1].contiguous()))      # ws short
    _sync()


@gpu
def test_combine_refuses_bad_shapes_and_skips_empty():
    T, K, H, P = 5, 2, 264, 32
    out = torch.zeros(T, H, dtype=BF, device=DEV)
    y = torch.zeros(P, H, dtype=BF, device=DEV)
    wts = torch.ones(T * K, device=DEV)
    inv = torch.zeros(T * K, dtype=torch.int32, device=DEV)
    fn = _C().moe_combine
    with pytest.raises(RuntimeError):
        fn(out, y[:, :256].contiguous(), wts, inv, K)
    with pytest.raises(RuntimeError):
        fn(out, y, wts[:-1].contiguous(), inv, K)
    with pytest.raises(RuntimeError):
        fn(out, y, wts, inv[:-1].contiguous(), K)
    with pytest.raises(RuntimeError):
        fn(out, y, wts, inv, 0)
    with pytest.raises(RuntimeError):           # T*topk mismatch
        fn(out, y, wts, inv, 1)
    # T == 0: nothing to launch
    fn(out[:0], y, wts[:0], inv[:0], K)
    _sync()


# ------------------------------------------------------------- randn GEMM
def _rounding_ratio(out, ref, S, K, c=1.0):
    """max |out - ref| / (2^-8 |ref| + c K 2^-23 S): one bf16 ulp for the
    final store plus twice the unit roundoff per accumulated term."""
    bound = 2.0 ** -8 * ref.abs() + c * K * 2.0 ** -23 * S
    return ((out.double() - ref).abs() / bound).max().item()


def _randn_inputs(al, N, K, fp8):
    from hyperspot.parallel.layers import quantize_weight_fp8
    g = torch.Generator().manual_seed(7)
    x = (0.3 * torch.randn(al.T, K, generator=g)).to(BF).to(DEV)
    w = (0.05 * torch.randn(al.E, N, K, generator=g)).to(BF).to(DEV)
    if not fp8:
        return x, w, None, None
    xq = ops.quant_fp8(x)
    qs = [quantize_weight_fp8(w[e]) for e in range(al.E)]
    wq = torch.stack([q.view(torch.uint8) for q, _ in qs]).view(F8)
    ws = torch.stack([s for _, s in qs]).reshape(-1).contiguous()
    return xq.data, wq, xq.scale, ws


@gpu
@pytest.mark.parametrize("fp8,K", [(False, 384), (True, 768)],
                         ids=["bf16", "fp8"])
def test_gemm_randn_within_rounding_bound(fp8, K):
    al = aligned("ragged")
    N = 256
    x, w, xs, ws = _randn_inputs(al, N, K, fp8)
    out = run_gemm(al, x, w, xs, ws, al.K)
    valid, ref, S = M.gemm_ref64(x, w, al.sid_h, al.te_h, al.K, xs, ws)
    o = out.cpu()[valid]
    assert torch.isfinite(o.float()).all()
    ratio = _rounding_ratio(o, ref[valid], S[valid], K)
    print(f"randn GEMM {'fp8' if fp8 else 'bf16'} K={K}: "
          f"max err/bound = {ratio:.4f}")
    assert ratio <= 1.0, ratio


# --------------------------------------------------------------- silu_mul
def _silu_within(out, ref):
    bound = M.bf16_ulp(ref) + 2.0 ** -20 * ref.abs()
    return ((out.double() - ref).abs() / bound).max().item()


@gpu
@pytest.mark.parametrize("rows,inter", [(3, 8), (5, 264), (2, 2056),
                                        (512, 256), (65536, 8)])
def test_silu_mul_vs_float64(rows, inter):
    g = torch.Generator().manual_seed(rows + inter)
    gu = (3.0 * torch.randn(rows, 2 * inter, generator=g)).to(BF)
    # __expf overflows to inf at -1e4 (silu must be -0) and underflows to
    # 0 at +1e4 (silu must be g); +-88 sits at the edge of fp32 range
    special = torch.tensor([0.0, -0.0, 88.0, -88.0, 1e4, -1e4, 1.0, -1.0])
    gu[0, :8] = special.to(BF)
    gu[rows - 1, inter - 8:inter] = special.to(BF)
    live = rows
    if (rows, inter) == (512, 256):      # an h1 with unused tiles behind
        gu[256:] = NAN
        gu[255, inter - 8:inter] = special.to(BF)
        live = 256
    out = torch.full((rows, inter), NAN, dtype=BF, device=DEV)
    _C().silu_mul(out, gu.to(DEV))
    o = out.cpu()
    ref = M.silu_mul_ref64(gu)
    assert torch.isfinite(o[:live].float()).all()
    ratio = _silu_within(o[:live], ref[:live])
    print(f"silu_mul {rows}x{inter}: max err/bound = {ratio:.4f}")
    assert ratio <= 1.0, ratio
    u = gu[0, inter:inter + 8].double()
    got = o[0, :8].double()
    assert got[4] == M.round_bf16(gu[0, 4].double() * u[4]).double()
    assert got[5] == 0 and got[0] == 0 and got[1] == 0
    assert torch.signbit(got[5]) == torch.signbit(-u[5])


# ---------------------------------------------------------------- combine
def _combine_setup(T, K, hidden, lattice):
    P = 2 * T * K + 3
    g = torch.Generator().manual_seed(T * 31 + K * 7 + hidden)
    inv = torch.randperm(P, generator=g)[:T * K].to(torch.int32)
    if lattice:
        y, wts = M.lattice_combine_inputs(T, K, P, hidden, 5)
    else:
        y = torch.randn(P, hidden, generator=g)
        p = torch.randn(T, 8, generator=g).softmax(-1)
        wts = p.topk(K, dim=-1).values
        if K > 1:
            wts = wts / wts.sum(-1, keepdim=True)
    y = y.to(BF)
    dead = torch.ones(P, dtype=torch.bool)
    dead[inv.long()] = False
    y[dead] = NAN                # rows no inv_pos points at
    out = torch.full((T, hidden), NAN, dtype=BF, device=DEV)
    _C().moe_combine(out, y.to(DEV), wts.float().reshape(-1).to(DEV),
                     inv.to(DEV), K)
    o = out.cpu()
    assert torch.isfinite(o.float()).all()
    ref, S = M.combine_ref64(y, wts.float(), inv, K)
    return o, ref, S


_COMBINE = [(T, K, h) for T in (1, 300) for K in (1, 2)
            for h in (8, 264, 2056)]


@gpu
@pytest.mark.parametrize("T,K,hidden", _COMBINE)
def test_combine_lattice_exact(T, K, hidden):
    o, ref, _ = _combine_setup(T, K, hidden, True)
    assert torch.equal(o, M.round_bf16(ref))
    assert torch.equal(o.double(), ref)


@gpu
@pytest.mark.parametrize("T,K,hidden", _COMBINE)
def test_combine_randn_vs_float64(T, K, hidden):
    o, ref, S = _combine_setup(T, K, hidden, False)
    bound = M.bf16_ulp(ref) + K * 2.0 ** -23 * S
    ratio = ((o.double() - ref).abs() / bound).max().item()
    print(f"combine T={T} K={K} hidden={hidden}: err/bound = {ratio:.4f}")
    assert ratio <= 1.0, ratio


# ----------------------------------------------------------------- the op
def _staged(al, fp8, x, w13, w2, xs, w13s, w2s, wts):
    """The op's own sequence through _C with buffers owned here, and every
    stage held to its reference on the kernel's previous output."""
    n = _C()
    H, I2, I = x.shape[1], w13.shape[1], w2.shape[2]
    per = 128 if fp8 else 64
    P, nt = al.P, al.ntiles
    h1 = torch.full((P, I2), NAN, dtype=BF, device=DEV)
    s1, ws1 = ops._moe_splitk(nt * (I2 // 128), H // per, P * I2, DEV)
    run_gemm(al, x, w13, xs, w13s, al.K, s1, ws1, out=h1)
    if fp8:
        a = ops.silu_mul_q(h1)
        a_x, a_s = a.data, a.scale
    else:
        a_x, a_s = ops.silu_mul(h1), None
    y = torch.full((P, H), NAN, dtype=BF, device=DEV)
    s2, ws2 = ops._moe_splitk(nt * (H // 128), I // per, P * H, DEV)
    run_gemm(al, a_x, w2, a_s, w2s, 0, s2, ws2, out=y)
    out = torch.full((al.T, H), NAN, dtype=BF, device=DEV)
    n.moe_combine(out, y, wts, al.inv, al.K)
    return h1, a_x, a_s, y, out, (s1, s2)


@gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("name,H,I", M.OP_SHAPES)
def test_op_matches_staged_chain(name, H, I, fp8):
    al = aligned(name)
    x, w13, w2, xs, w13s, w2s, wts = M.op_lattice(name, H, I, fp8)
    dt = F8 if fp8 else BF
    xd, w13d, w2d = (t.to(dt).to(DEV) for t in (x, w13, w2))
    wtsd = wts.to(DEV)
    if fp8:
        xsd = xs.to(DEV)
        w13sd = w13s.reshape(-1).contiguous().to(DEV)
        w2sd = w2s.reshape(-1).contiguous().to(DEV)
        got = ops.moe_ffn_fp8(ops.QTensor(xd, xsd), w13d, w13sd, w2d, w2sd,
                              wtsd, al.ids)
    else:
        xsd = w13sd = w2sd = None
        got = ops.moe_ffn(xd, w13d, w2d, wtsd, al.ids)
    h1, a_x, a_s, y, out, sk = _staged(al, fp8, xd, w13d, w2d, xsd, w13sd,
                                       w2sd, wtsd.reshape(-1).contiguous())
    print(f"op {name} H={H} fp8={fp8}: splitk = {sk}")
    assert torch.equal(got, out)

    # the reference chain: each stage from the kernel's previous output
    v = al.valid
    # (the op's split-K workspace is uninitialised, so with s1 > 1 the
    # reduce leaves garbage, not NaN, in the rows of unused tiles)
    check_lattice(al, h1, (x, w13, xs, w13s), al.K, f"op {name} h1",
                  unused_nan=sk[0] == 1)
    if not fp8:
        # h1 holds integers down to -256: below g = -88.7 the fp32
        # exp(-g) is inf and the kernel returns -0 for a silu(g) whose
        # magnitude is under 88.7 e^-88.7 < 2.7e-37, so that much per
        # unit of |u| is allowed on top of the silu_mul bound
        hv = h1.cpu()[v]
        a_ref = M.silu_mul_ref64(hv)
        bound = M.bf16_ulp(a_ref) + 2.0 ** -20 * a_ref.abs() + \
            2.7e-37 * hv[:, I:].double().abs()
        ra = ((a_x.cpu()[v].double() - a_ref).abs() / bound).max().item()
        print(f"op {name} H={H}: silu_mul err/bound = {ra:.4f}")
        assert ra <= 1.0, ra
    _, y_ref, y_S = M.gemm_ref64(a_x, w2d, al.sid_h, al.te_h, 0, a_s, w2sd)
    yk = y.cpu()
    # GEMM 2 here sees e4m3fn rows that span the format's whole range
    # against {-1, 0, 1}: cancellation that randn inputs never reach.  The
    # fp8 MFMA does not round once per product-add: torch._scaled_mm on
    # these inputs measured err/bound = 1.656 against gemm_ref64, and
    # moe_gemm_fp8 the same figure (profiles/r10_moe_f64.md), so the
    # accumulation term is twice the vendor GEMM's ratio.  bf16 holds c = 1.
    c = 2 * 1.656 if fp8 else 1.0
    ry = _rounding_ratio(yk[v], y_ref[v], y_S[v], I, c)
    print(f"op {name} H={H} fp8={fp8}: GEMM-2 err/bound = {ry:.4f}")
    assert ry <= 1.0, ry
    out_ref, _ = M.combine_ref64(yk, wts, al.inv_h, al.K)
    assert torch.equal(got.cpu(), M.round_bf16(out_ref))


@gpu
def test_op_empty_rank_launches_nothing():
    T, K, E, ids = M.routing_case("empty")
    H, I = 256, 256
    x = torch.zeros(0, H, dtype=BF, device=DEV)
    w13 = torch.zeros(E, 2 * I, H, dtype=BF, device=DEV)
    w2 = torch.zeros(E, H, I, dtype=BF, device=DEV)
    wts = torch.zeros(0, K, device=DEV)
    idd = ids.to(DEV)
    out = ops.moe_ffn(x, w13, w2, wts, idd)
    assert out.shape == (0, H) and out.dtype == BF
    q = ops.QTensor(x.to(F8), torch.zeros(0, device=DEV))
    out8 = ops.moe_ffn_fp8(q, w13.to(F8), torch.ones(E * 2 * I, device=DEV),
                           w2.to(F8), torch.ones(E * H, device=DEV), wts,
                           idd)
    assert out8.shape == (0, H) and out8.dtype == BF
    _sync()


# ---------------------------------------------------------------- XCD map
def xcd_child_main():
    """Runs in the child process, with HS_MOE_XCD=1 read at first launch:
    the bf16 lattice GEMM under the XCD-grouped block-to-tile map."""
    assert os.environ.get("HS_MOE_XCD") == "1"
    # 5 used tiles of 11 (not a multiple of 8), nx = 2
    lattice_gemm("ragged", False, 256, 128, False)
    # 9 used tiles, nx = 34: a second n-group
    lattice_gemm("xcd9", False, 4352, 128, False, routing=M.XCD9)
    _sync()


@gpu
def test_gemm_lattice_exact_under_xcd_map():
    """HS_MOE_XCD is read once per process, so a fresh child runs it (this
    process has the GPU open and must not replace its own program).  Kept
    last in the file: nothing is started after it."""
    child = pathlib.Path(__file__).with_name("moe_xcd_child.py")
    r = subprocess.run([sys.executable, str(child)],
                       env={**os.environ, "HS_MOE_XCD": "1"}, timeout=120,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]

"""CPU references for the MoE kernels of csrc/moe.hip (and silu_mul of
csrc/act.hip): an exact check of the align contract, lattice inputs on
which a correct grouped GEMM is exact, and float64 references for the
GEMM, SwiGLU and combine stages.  numpy/torch on the CPU only; the GPU
tests feed these with the kernels' own outputs, stage by stage.
"""

import numpy as np
import torch

MOE_BM = 256


def ntiles_for(num_pairs, E):
    """The tile count ops.moe_ffn allocates: worst-case padded length."""
    return (num_pairs + E * (MOE_BM - 1) + MOE_BM - 1) // MOE_BM


# ---------------------------------------------------------------- routing
def _counts_to_ids(counts, T, K):
    flat = np.concatenate([np.full(c, e, np.int32)
                           for e, c in enumerate(counts)])
    assert flat.size == T * K
    return flat.reshape(T, K)


def _ragged():
    # 300 tokens x top-2 over 8 experts: 0, 300, 5, 0, 64, 231, 0, 0 pairs,
    # all 600 slots shuffled.  (One slot of every token on expert 1 would
    # make that expert's sorted row p hold token p, and a kernel that
    # looked up its row's scale or data by sorted position would pass.)
    rng = np.random.default_rng(11)
    flat = _counts_to_ids([0, 300, 5, 0, 64, 231, 0, 0], 600, 1).reshape(-1)
    return rng.permutation(flat).reshape(300, 2)


def _wide():
    rng = np.random.default_rng(12)
    return np.stack([rng.choice(64, 2, replace=False)
                     for _ in range(64)]).astype(np.int32)


# name -> (T, K, E, ids [T, K] int32).  The smallest routings that reach
# each branch of align and of the GEMM's tile/wave bookkeeping.
ROUTING = {
    "decode1": (1, 2, 8, np.array([[3, 5]], np.int32)),
    "full": (256, 1, 4, _counts_to_ids([0, 0, 256, 0], 256, 1)),
    "over": (257, 1, 4, _counts_to_ids([257, 0, 0, 0], 257, 1)),
    "tight": (516, 1, 4, _counts_to_ids([257, 257, 1, 1], 516, 1)),
    "ragged": (300, 2, 8, _ragged()),
    "wide": (64, 2, 64, _wide()),
    "single": (40, 1, 1, np.zeros((40, 1), np.int32)),
    "empty": (0, 1, 4, np.zeros((0, 1), np.int32)),
}
GPU_CASES = [n for n in ROUTING if n != "empty"]
# the XCD-map case: 9 tiles, all used (5 + 4), at E = 2
XCD9 = (1794, 1, 2, _counts_to_ids([1025, 769], 1794, 1))


def routing_case(name):
    T, K, E, ids = ROUTING[name]
    return T, K, E, torch.from_numpy(ids.copy())


def python_align(flat_ids, E, ntiles):
    """The align contract by a plain stable sort."""
    flat = np.asarray(flat_ids, np.int64).reshape(-1)
    sorted_ids = np.full(ntiles * MOE_BM, -1, np.int32)
    tile_expert = np.full(ntiles, -1, np.int32)
    inv_pos = np.full(flat.size, -1, np.int32)
    pos = 0
    for e in range(E):
        pairs = np.nonzero(flat == e)[0]
        if pairs.size == 0:
            continue
        sorted_ids[pos:pos + pairs.size] = pairs
        inv_pos[pairs] = pos + np.arange(pairs.size)
        nt = -(-pairs.size // MOE_BM)
        tile_expert[pos // MOE_BM:pos // MOE_BM + nt] = e
        pos += nt * MOE_BM
    return sorted_ids, tile_expert, inv_pos


def align_check(flat_ids, E, sorted_ids, tile_expert, inv_pos):
    """Assert the integer contract of moe_align, exactly.  Order inside a
    segment is free (it comes from an LDS atomic): compared as sets."""
    flat = np.asarray(flat_ids, np.int64).reshape(-1)
    sid = np.asarray(sorted_ids, np.int64).reshape(-1)
    te = np.asarray(tile_expert, np.int64).reshape(-1)
    inv = np.asarray(inv_pos, np.int64).reshape(-1)
    assert sid.size == te.size * MOE_BM, (sid.size, te.size)
    assert inv.size == flat.size, (inv.size, flat.size)
    assert flat.size == 0 or (flat.min() >= 0 and flat.max() < E), \
        "expert id outside [0, E): outside the kernels' contract"
    pos = 0
    for e in range(E):
        want = np.nonzero(flat == e)[0]
        if want.size == 0:
            continue                      # nothing for an empty expert
        assert pos % MOE_BM == 0
        padded = -(-want.size // MOE_BM) * MOE_BM
        assert pos + padded <= sid.size, \
            f"expert {e}: segment [{pos}, {pos + padded}) past the buffer"
        seg = sid[pos:pos + padded]
        live = seg[seg >= 0]
        assert live.size == want.size, \
            f"expert {e}: {live.size} live entries in its segment at " \
            f"{pos}, wanted {want.size}"
        assert np.unique(live).size == live.size, \
            f"expert {e}: a pair appears twice in its segment"
        assert np.array_equal(np.sort(live), want), \
            f"expert {e}: segment at {pos} holds the wrong pairs"
        assert (seg[:want.size] >= 0).all() and (seg[want.size:] < 0).all(), \
            f"expert {e}: padding is not at the tail of the segment"
        t0, t1 = pos // MOE_BM, (pos + padded) // MOE_BM
        assert (te[t0:t1] == e).all(), \
            f"expert {e}: tile_expert[{t0}:{t1}] = {te[t0:t1]}"
        pos += padded
    assert (sid[pos:] < 0).all(), "live entry past the last segment"
    assert (te[pos // MOE_BM:] < 0).all(), \
        "tile_expert is not negative after the last segment"
    if flat.size:
        assert (inv >= 0).all() and (inv < sid.size).all(), \
            "inv_pos outside the sorted space"
        assert np.array_equal(sid[inv], np.arange(flat.size)), \
            "sorted_ids[inv_pos[p]] != p"


# ---------------------------------------------------------------- lattice
def bf16_exact(t):
    return torch.equal(t.double().to(torch.bfloat16).double(), t.double())


def lattice_inputs(rows, N, K, E, seed, fp8=False):
    """x [rows, K] in {-2..2} and w [E, N, K] in {-1, 0, 1} (float32,
    seeded, different for every row and every expert); for fp8 also
    per-row and per-(expert, column) power-of-two scales in [2^-3, 2^3].
    Every product and partial sum of x @ w[e]^T is a small integer, exact
    in fp32, and asserted here to satisfy |sum| <= 256 for EVERY (row,
    expert) pairing, so the result is exact in bf16 whatever the routing.
    """
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (rows, K), generator=g).float()
    w = torch.randint(-1, 2, (E, N, K), generator=g).float()
    worst = 0.0
    for e in range(E):
        # integers far below 2^24: the fp32 matmul is exact
        worst = max(worst, (x @ w[e].t()).abs().max().item())
    assert worst <= 256, f"lattice seed {seed}: |sum| reaches {worst}"
    if not fp8:
        return x, w, None, None
    xs = torch.exp2(torch.randint(-3, 4, (rows,), generator=g).float())
    ws = torch.exp2(torch.randint(-3, 4, (E, N), generator=g).float())
    return x, w, xs, ws


# (routing case, fp8, N, K) of every lattice GEMM the GPU tests run, each
# in gather and in plain mode: every case at 256x256, then the k-pipeline
# at 2, 3/4 and 6 chunks (64 bf16 or 128 fp8 elements per chunk) on ragged.
GEMM_SHAPES = (
    [(c, f, 256, 256) for c in GPU_CASES for f in (False, True)]
    + [("ragged", False, n, k) for k in (128, 384) for n in (128, 384)]
    + [("ragged", False, n, 256) for n in (128, 384)]
    + [("ragged", True, n, k) for k in (256, 384, 768) for n in (128, 384)]
    + [("ragged", False, 256, 384), ("ragged", True, 256, 768)]  # split-K
    + [("ragged", False, 256, 128)])                             # XCD map
OP_SHAPES = [(c, 256, 256) for c in GPU_CASES] + [("ragged", 768, 768)]


def gemm_lattice(name, N, K, fp8, plain, routing=None):
    """Lattice inputs for one GEMM test: x has T rows in gather mode and
    ntiles*256 (the whole sorted space) in plain mode."""
    import zlib
    T, Ktop, E, _ = routing or ROUTING[name]
    rows = ntiles_for(T * Ktop, E) * MOE_BM if plain else T
    seed = zlib.crc32(f"{name}/{N}/{K}/{fp8}/{plain}".encode()) & 0xffff
    return lattice_inputs(rows, N, K, E, seed, fp8)


def op_lattice(name, H, I, fp8):
    """Lattice inputs for the whole op: GEMM 1 is exact; w2 and the
    routing weights stay on the lattice ({-1,0,1}, powers of two) so that
    the combine of K <= 2 terms rounds once."""
    import zlib
    T, Ktop, E, _ = ROUTING[name]
    seed = zlib.crc32(f"op/{name}/{H}/{I}/{fp8}".encode()) & 0xffff
    x, w13, xs, w13s = lattice_inputs(T, 2 * I, H, E, seed, fp8)
    g = torch.Generator().manual_seed(seed + 1)
    w2 = torch.randint(-1, 2, (E, H, I), generator=g).float()
    w2s = torch.exp2(torch.randint(-3, 4, (E, H), generator=g).float())
    wts = torch.exp2(torch.randint(-1, 1, (T, Ktop), generator=g).float())
    return x, w13, w2, xs, w13s, (w2s if fp8 else None), wts


def lattice_combine_inputs(T, K, P, hidden, seed):
    """y [P, hidden] integers in [-8, 8] and weights [T, K] in {1/2, 1, 2}:
    every sum of K <= 2 terms is a multiple of 1/2 below 32, exact in
    bf16."""
    assert K <= 2
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(-8, 9, (P, hidden), generator=g).float()
    wts = torch.exp2(torch.randint(-1, 2, (T, K), generator=g).float())
    return y, wts


# ------------------------------------------------------------- references
def _f64(t):
    t = t.detach().cpu()
    # fp8 has no direct cast to float64; fp32 holds bf16 and fp8 exactly
    return t if t.dtype == torch.float64 else t.float().double()


def gemm_ref64(x, w, sorted_ids, tile_expert, gather_div, xs=None, ws=None):
    """float64 grouped GEMM over the kernel's own align output.

    Returns (valid [P] bool, ref [P, N], S [P, N]): for every valid sorted
    row the result and the magnitude sum S = sum_k |a_k b_k| (times the
    scales for fp8); rows that are padding or in unused tiles are NaN.
    """
    sid = torch.as_tensor(sorted_ids).cpu().long().reshape(-1)
    te = torch.as_tensor(tile_expert).cpu().long().reshape(-1)
    x64, w64 = _f64(x), _f64(w)
    P, N = sid.numel(), w64.shape[1]
    valid = sid >= 0
    ref = torch.full((P, N), float("nan"), dtype=torch.float64)
    S = torch.full((P, N), float("nan"), dtype=torch.float64)
    row_e = te.repeat_interleave(MOE_BM)
    assert (row_e[valid] >= 0).all(), "valid row in an unused tile"
    for e in row_e[valid].unique().tolist():
        p = torch.nonzero(valid & (row_e == e)).reshape(-1)
        src = sid[p] // gather_div if gather_div > 0 else p
        a = x64[src]
        r = a @ w64[e].t()
        s = a.abs() @ w64[e].abs().t()
        if xs is not None:
            sc = _f64(xs).reshape(-1)[src][:, None] * \
                _f64(ws).reshape(-1, N)[e][None, :]
            r, s = r * sc, s * sc
        ref[p], S[p] = r, s
    return valid, ref, S


def silu_mul_ref64(gate_up):
    """float64 silu(g) * u for gate_up [..., 2I] = (g | u)."""
    x = _f64(gate_up)
    i = x.shape[-1] // 2
    g, u = x[..., :i], x[..., i:]
    return g / (1.0 + torch.exp(-g)) * u


def combine_ref64(y, wts, inv_pos, K):
    """float64 out[t] = sum_k w[t, k] * y[inv_pos[t*K + k]] and the
    magnitude sum of the same terms."""
    inv = torch.as_tensor(inv_pos).cpu().long().reshape(-1, K)
    terms = _f64(wts).reshape(-1, K)[:, :, None] * _f64(y)[inv]
    return terms.sum(1), terms.abs().sum(1)


def bf16_ulp(ref):
    """Spacing of bf16 at |ref| (float64 tensor)."""
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** -126))
    return torch.exp2((e - 8).double())


def round_bf16(ref):
    """float64 -> bf16 in ONE round-to-nearest-even (a plain .to() goes
    through fp32 and rounds twice)."""
    u = bf16_ulp(ref)
    return (torch.round(ref / u) * u).to(torch.bfloat16)

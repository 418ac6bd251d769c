"""Shared by the sample_fused tests: the float64 reference of the sampling
semantics (one row at a time, by unique values, no sort of tokens) and the
validity check of a returned token against it."""

import numpy as np
import torch

TOL = 1e-5

# (temperature, top_k, top_p), taken in turn by the rows of a case
PARAMS = [(1.0, 0, 1.0), (0.7, 5, 1.0), (1.3, 0, 0.9), (0.8, 40, 0.95),
          (1.0, 1, 1.0), (1.0, 0, 1e-3), (0.5, 0, 0.5), (2.0, 10 ** 8, 0.99)]


def row_params(rows):
    """float32 temperature, float32 top_p, int32 top_k (k >= 2^31 clamps:
    any k >= V means off)."""
    tp = [PARAMS[r % len(PARAMS)] for r in range(rows)]
    return (torch.tensor([a[0] for a in tp], dtype=torch.float32),
            torch.tensor([a[2] for a in tp], dtype=torch.float32),
            torch.tensor([min(a[1], 2 ** 31 - 1) for a in tp],
                         dtype=torch.int32))


def make_logits(rows, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(rows, vocab, generator=g) * 3).to(torch.bfloat16)
    uniform = torch.rand(rows, generator=g)
    return logits, uniform


class Ref:
    """kept: bool[V]; w: float64[V] weights of the kept tokens (0 for the
    dropped and for -inf); cdf: inclusive running sum of w in vocabulary
    order over the kept mass; margin: min |G(v) - p| over the row's values
    (inf when top-p is off)."""

    def __init__(self, x, t, k, p):
        x = x.detach().cpu().double()
        V = x.numel()
        t = max(float(np.float32(t)), 1e-6)
        p = float(np.float32(p))
        k = int(k)
        kept = torch.ones(V, dtype=torch.bool)
        if 0 < k < V:
            kept = x >= torch.topk(x, k).values[-1]
        m = x[kept].max()
        w = torch.where(kept & torch.isfinite(x), torch.exp((x - m) / t),
                        torch.zeros_like(x))
        self.margin = float("inf")
        if p < 1:
            vals, inv = torch.unique(x, return_inverse=True)   # ascending
            mass = torch.zeros_like(vals).index_add_(0, inv, w)
            # mass strictly above each value
            above = mass.flip(0).cumsum(0).flip(0) - mass
            G = above / w.sum()
            live = mass > 0
            self.margin = float((G[live] - p).abs().min())
            keep_val = G < p
            keep_val[vals == m] = True
            kept = kept & keep_val[inv]
            w = torch.where(kept, w, torch.zeros_like(w))
        self.kept = kept
        self.w = w
        self.cdf = w.cumsum(0) / w.sum()
        self.argmax = int(x.float().argmax())


def check_token(ref, tok, u, tol=TOL):
    """tok is kept, carries weight, and u falls into its CDF interval."""
    tok = int(tok)
    u = float(np.float32(u))
    assert bool(ref.kept[tok]), f"token {tok} was dropped by top-k/top-p"
    assert float(ref.w[tok]) > 0, f"token {tok} has no weight"
    lo = float(ref.cdf[tok - 1]) if tok > 0 else 0.0
    hi = float(ref.cdf[tok])
    assert lo - tol <= u <= hi + tol, (tok, lo, u, hi)


def check_rows(logits, temperature, top_p, top_k, uniform, out,
               need_margin=True):
    """Every row of `out` against the reference; returns the smallest
    top-p margin met.  need_margin asserts the precondition under which
    the kept set is unambiguous: no G(v) within TOL of p."""
    margin = float("inf")
    for r in range(logits.shape[0]):
        t, k, p = float(temperature[r]), int(top_k[r]), float(top_p[r])
        ref = Ref(logits[r], t, k, p)
        if t == 0:
            assert int(out[r]) == ref.argmax
            continue
        margin = min(margin, ref.margin)
        if need_margin:
            assert ref.margin > TOL, (r, ref.margin)
        check_token(ref, out[r], uniform[r])
    return margin

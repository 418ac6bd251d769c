"""float64 reference of the token_logprobs contract, one row at a time.

A row's logprob is x - logsumexp over its finite logits; the alternatives
are the first n entries of a stable sort by (-x, id), with every non-finite
logit ranked below the finite ones (by id) and reported as -inf.  Nothing
here shares code with hyperspot.ops."""

import math

import torch

COLS = 21
N_CYCLE = [-1, 0, 1, 5, 20]
NINF = float("-inf")


def make_rows(rows, vocab, seed):
    """bf16 logits (randn * 3), a chosen token per row, n_top cycling
    N_CYCLE."""
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(rows, vocab, generator=g) * 3).to(torch.bfloat16)
    chosen = torch.randint(0, vocab, (rows,), generator=g)
    n_top = torch.tensor([N_CYCLE[i % len(N_CYCLE)] for i in range(rows)],
                         dtype=torch.int32)
    return logits, chosen, n_top


def row_logprobs(row):
    """float64 logprob of every token of one row (non-finite: -inf)."""
    x = row.double()
    fin = torch.isfinite(x)
    if not bool(fin.any()):
        return torch.full_like(x, NINF)
    xf = x[fin]
    m = xf.max()
    lse = m + torch.log(torch.exp(xf - m).sum())
    return torch.where(fin, x - lse, torch.full_like(x, NINF))


def row_order(row):
    """Token ids by (-x, id); non-finite logits last, by id."""
    x = row.double()
    key = torch.where(torch.isfinite(x), -x, torch.full_like(x, math.inf))
    return torch.sort(key, stable=True).indices


def reference(logits, chosen, n_top, val=None, idx=None):
    """(val float64 [rows, 21], id int64 [rows, 21]).  Rows with n_top < 0
    keep what `val` / `idx` hold (default: -inf / -1)."""
    rows, vocab = logits.shape
    val = torch.full((rows, COLS), NINF, dtype=torch.float64) \
        if val is None else val.double().clone()
    idx = torch.full((rows, COLS), -1, dtype=torch.long) \
        if idx is None else idx.long().clone()
    for r in range(rows):
        n = int(n_top[r])
        if n < 0:
            continue
        n = min(n, COLS - 1, vocab)
        lp = row_logprobs(logits[r])
        c = int(chosen[r])
        idx[r, 0] = c
        val[r, 0] = lp[c] if 0 <= c < vocab else NINF
        order = row_order(logits[r])[:n]
        idx[r, 1:1 + n] = order
        val[r, 1:1 + n] = lp[order]
        idx[r, 1 + n:] = -1
        val[r, 1 + n:] = NINF
    return val, idx


def max_abs_err(got_val, ref_val):
    """Largest |got - ref| over the finite reference entries; the -inf
    entries must match exactly."""
    fin = torch.isfinite(ref_val)
    assert torch.equal(torch.isfinite(got_val.double()), fin)
    assert bool((got_val.double()[~fin] == NINF).all())
    if not bool(fin.any()):
        return 0.0
    return float((got_val.double()[fin] - ref_val[fin]).abs().max())

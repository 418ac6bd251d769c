"""Shared by test_paged_attn_gpu.py and test_kv_append_gpu.py: poisoned
paged KV caches.

A cache built here looks like a pool whose pages were used before: pages
are handed out in a random permutation, and every slot at or beyond a
sequence's length in its last page, every unused page, and the page that
block-table padding points at hold NaN (byte 0x7f for e4m3fn).  A kernel
that lets such a slot reach its result shows a NaN in the output; it never
faults, because every page index is valid.
"""

import torch

BS = 16                      # tokens per page
FP8 = torch.float8_e4m3fn


def poisoned(nb, KV, D, fp8):
    """[nb, KV, BS, D] of NaN: bf16, or uint8 codes 0x7f for an fp8 cache
    (view it with as_cache once filled)."""
    if fp8:
        return torch.full((nb, KV, BS, D), 0x7f, dtype=torch.uint8)
    return torch.full((nb, KV, BS, D), float("nan"), dtype=torch.bfloat16)


def as_cache(t, fp8):
    return t.view(FP8) if fp8 else t


def write(cache, fp8, pages, pos, vals):
    """vals [len(pos), KV, D] -> the cache slots of positions `pos` of the
    sequence that owns `pages`.  Float values are rounded to the cache
    dtype; uint8 values are taken as e4m3fn codes."""
    blk = pages[pos // BS]
    if fp8:
        if vals.dtype != torch.uint8:
            vals = vals.float().to(FP8).view(torch.uint8)
        cache[blk, :, pos % BS] = vals
    else:
        cache[blk, :, pos % BS] = vals.bfloat16()


def layout(lens, spare, g):
    """Random page assignment for sequences of `lens` tokens: returns
    (block table [S, max_blocks] int32 padded with the NaN page, list of
    per-sequence page index tensors, number of pages in the pool)."""
    need = [(n + BS - 1) // BS for n in lens]
    nb = sum(need) + spare + 1
    perm = torch.randperm(nb, generator=g)
    nan_page, free = int(perm[-1]), perm[:-1]
    bt = torch.full((len(lens), max(need) + 2), nan_page, dtype=torch.int32)
    pages, used = [], 0
    for z, n in enumerate(need):
        pages.append(free[used:used + n])
        bt[z, :n] = pages[z].to(torch.int32)
        used += n
    return bt, pages, nb


def build(lens, KV, D, fp8, g, spare=3, v_scale=None):
    """Caches holding `lens[z]` random tokens for sequence z, poison
    everywhere else.  Returns (k_cache, v_cache, block_table, pages)."""
    bt, pages, nb = layout(lens, spare, g)
    kc, vc = poisoned(nb, KV, D, fp8), poisoned(nb, KV, D, fp8)
    if v_scale is None:
        v_scale = 0.5 if fp8 else 1.0
    for z, n in enumerate(lens):
        pos = torch.arange(n)
        write(kc, fp8, pages[z], pos, torch.randn(n, KV, D, generator=g))
        write(vc, fp8, pages[z], pos,
              torch.randn(n, KV, D, generator=g) * v_scale)
    return as_cache(kc, fp8), as_cache(vc, fp8), bt, pages

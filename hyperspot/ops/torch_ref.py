"""Pure-PyTorch reference implementations of every engine op.

These are the numerics ground truth for the CDNA4 HIP kernels (tests compare
the gfx950 kernels against these in fp32) and the CPU execution path for
CI — this container has no GPU.  They are written for clarity, not speed.

Conventions shared with the HIP kernels (csrc/):
  - token-major activations: x is [T, hidden] (T = flattened tokens of the
    whole batch, prefill + decode mixed)
  - q/k/v are [T, n_heads, head_dim] after the qkv projection split
  - paged KV cache: k_cache/v_cache are [num_blocks, kv_heads, block, head_dim]
  - slot_mapping[t] = block_id * block_size + offset for token t
  - RoPE is GPT-NeoX style (rotate halves, not interleaved pairs)
"""

from __future__ import annotations

import torch


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    dt = x.dtype
    xf = x.float()
    out = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (out * weight.float()).to(dt)


def fused_add_rmsnorm(x: torch.Tensor, residual: torch.Tensor,
                      weight: torch.Tensor, eps: float):
    """residual += x; return (rmsnorm(residual), residual)."""
    res = (residual.float() + x.float())
    out = res * torch.rsqrt(res.pow(2).mean(-1, keepdim=True) + eps)
    out = (out * weight.float()).to(x.dtype)
    return out, res.to(x.dtype)


def rope_cos_sin(positions: torch.Tensor, head_dim: int, theta: float,
                 dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Return [T, head_dim] table: first half cos, second half sin."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float32,
                                        device=positions.device) / head_dim))
    freqs = positions.float()[:, None] * inv[None, :]          # [T, D/2]
    return torch.cat([freqs.cos(), freqs.sin()], dim=-1).to(dtype)


def _rotate_neox(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor):
    # x: [T, H, D]; cos/sin: [T, D/2]
    d2 = x.shape[-1] // 2
    x1, x2 = x[..., :d2].float(), x[..., d2:].float()
    c, s = cos[:, None, :], sin[:, None, :]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(x.dtype)


def apply_rope(q: torch.Tensor, k: torch.Tensor, positions: torch.Tensor,
               theta: float):
    """In-place-semantics RoPE on q [T,H,D] and k [T,KV,D]."""
    d = q.shape[-1]
    table = rope_cos_sin(positions, d, theta)
    cos, sin = table[:, : d // 2], table[:, d // 2:]
    return _rotate_neox(q, cos, sin), _rotate_neox(k, cos, sin)


def kv_cache_append(k: torch.Tensor, v: torch.Tensor,
                    k_cache: torch.Tensor, v_cache: torch.Tensor,
                    slot_mapping: torch.Tensor) -> None:
    """Scatter k/v [T, KV, D] into paged caches [NB, KV, BS, D].

    An e4m3fn cache saturates like csrc/rope_kv.hip: finite |x| > 448 and
    +-Inf are stored as +-448, never as the NaN byte the plain torch
    convert writes from 465 up.
    """
    nb, kvh, bs, d = k_cache.shape
    blk = slot_mapping // bs
    off = slot_mapping % bs
    if k_cache.dtype == torch.float8_e4m3fn:
        k = k.float().clamp(-448.0, 448.0)
    if v_cache.dtype == torch.float8_e4m3fn:
        v = v.float().clamp(-448.0, 448.0)
    k_cache[blk, :, off] = k.to(k_cache.dtype)
    v_cache[blk, :, off] = v.to(v_cache.dtype)


def paged_attn_decode(q: torch.Tensor, k_cache: torch.Tensor,
                      v_cache: torch.Tensor, block_tables: torch.Tensor,
                      seq_lens: torch.Tensor, scale: float) -> torch.Tensor:
    """One-token-per-sequence attention over the paged cache.

    q: [B, H, D]; block_tables: [B, max_blocks] int32; seq_lens: [B] int32
    (length INCLUDING the current token, whose k/v are already in the cache).
    """
    B, H, D = q.shape
    nb, KV, BS, _ = k_cache.shape
    group = H // KV
    out = torch.empty_like(q)
    for b in range(B):
        n = int(seq_lens[b])
        nblk = (n + BS - 1) // BS
        blocks = block_tables[b, :nblk].long()
        k = k_cache[blocks].permute(1, 0, 2, 3).reshape(KV, nblk * BS, D)[:, :n]
        v = v_cache[blocks].permute(1, 0, 2, 3).reshape(KV, nblk * BS, D)[:, :n]
        qb = q[b].float().view(KV, group, D)                   # [KV, G, D]
        att = torch.einsum("kgd,knd->kgn", qb, k.float()) * scale
        p = att.softmax(-1)
        o = torch.einsum("kgn,knd->kgd", p, v.float())
        out[b] = o.reshape(H, D).to(q.dtype)
    return out


def prefill_attn_paged(q: torch.Tensor, k_cache: torch.Tensor,
                       v_cache: torch.Tensor, block_tables: torch.Tensor,
                       ctx_lens: torch.Tensor, row_seq: torch.Tensor,
                       scale: float) -> torch.Tensor:
    """Per-row causal attention over the paged cache (chunked-prefill
    continuation reference: row t attends slots 0..ctx_lens[t])."""
    T, H, D = q.shape
    nb, KV, BS, _ = k_cache.shape
    group = H // KV
    out = torch.empty_like(q)
    for t in range(T):
        si = int(row_seq[t])
        c = int(ctx_lens[t])
        nblk = (c + BS - 1) // BS
        blocks = block_tables[si, :nblk].long()
        k = k_cache[blocks].permute(1, 0, 2, 3).reshape(KV, nblk * BS,
                                                        D)[:, :c].float()
        v = v_cache[blocks].permute(1, 0, 2, 3).reshape(KV, nblk * BS,
                                                        D)[:, :c].float()
        qt = q[t].float().view(KV, group, D)
        att = torch.einsum("kgd,knd->kgn", qt, k) * scale
        p = att.softmax(-1)
        o = torch.einsum("kgn,knd->kgd", p, v)
        out[t] = o.reshape(H, D).to(q.dtype)
    return out


def prefill_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                 seq_start: torch.Tensor, scale: float) -> torch.Tensor:
    """Varlen causal self-attention for prefill.

    q [T,H,D], k/v [T,KV,D]; seq_start: [num_seqs+1] int32 cumulative offsets.
    """
    T, H, D = q.shape
    KV = k.shape[1]
    group = H // KV
    out = torch.empty_like(q)
    for i in range(seq_start.numel() - 1):
        s, e = int(seq_start[i]), int(seq_start[i + 1])
        n = e - s
        qs = q[s:e].float().view(n, KV, group, D)
        ks = k[s:e].float()
        vs = v[s:e].float()
        att = torch.einsum("mkgd,nkd->kgmn", qs, ks) * scale
        mask = torch.full((n, n), float("-inf"), device=q.device).triu(1)
        att = att + mask
        p = att.softmax(-1)
        o = torch.einsum("kgmn,nkd->mkgd", p, vs)
        out[s:e] = o.reshape(n, H, D).to(q.dtype)
    return out


def silu_mul(gate_up: torch.Tensor) -> torch.Tensor:
    """SwiGLU activation: input [T, 2*I] (gate | up) -> [T, I]."""
    i = gate_up.shape[-1] // 2
    g, u = gate_up[..., :i].float(), gate_up[..., i:].float()
    return (torch.nn.functional.silu(g) * u).to(gate_up.dtype)


def decode_advance(input_ids: torch.Tensor, positions: torch.Tensor,
                   seq_lens: torch.Tensor, slot_mapping: torch.Tensor,
                   block_tables: torch.Tensor, sampled_prev: torch.Tensor,
                   ctl: torch.Tensor, page: int) -> None:
    """Twin of csrc/decode_state.hip (in place, same row semantics)."""
    rows = input_ids.numel()
    max_blocks = block_tables.shape[1]
    n_live = int(ctl[4 * rows])
    if n_live < 0:
        return
    c = ctl[:4 * rows].view(4, rows).long()
    src, new_blk, host_ids, host_pos = c[0], c[1], c[2], c[3]
    r = torch.arange(rows, device=input_ids.device)
    live = (r < n_live) & (src >= -1) & (src < rows)
    dev = live & (src >= 0)
    ids = torch.where(dev, sampled_prev[src.clamp(0, rows - 1)], host_ids)
    pos = torch.where(dev, positions + 1, host_pos)
    input_ids.copy_(torch.where(live, ids, torch.zeros_like(ids)))
    positions.copy_(torch.where(live, pos, torch.zeros_like(pos)))
    seq_lens.copy_(torch.where(live, pos + 1,
                               torch.ones_like(pos)).to(seq_lens.dtype))
    bi = torch.div(pos, page, rounding_mode="floor")
    ok = live & (pos >= 0) & (bi < max_blocks)
    inst = ok & (new_blk >= 0)
    block_tables[r[inst], bi[inst]] = new_blk[inst].to(block_tables.dtype)
    blk = block_tables[r, bi.clamp(0, max_blocks - 1)].long()
    slot_mapping.copy_(torch.where(ok, blk * page + pos % page,
                                   torch.full_like(pos, -1)))


def sample(logits: torch.Tensor, temperature: torch.Tensor,
           top_p: torch.Tensor, top_k: torch.Tensor,
           uniform: torch.Tensor) -> torch.Tensor:
    """Per-row temperature / top-k / top-p sampling.

    logits [B, V] float; temperature/top_p [B] float; top_k [B] int
    (0 = off); uniform [B] in [0,1) drives the categorical draw so the HIP
    kernel and the reference are comparable given the same randoms.
    temperature == 0 selects greedy argmax for that row.
    """
    B, V = logits.shape
    out = torch.empty(B, dtype=torch.long, device=logits.device)
    lf = logits.float()
    for b in range(B):
        t = float(temperature[b])
        if t == 0.0:
            out[b] = int(lf[b].argmax())
            continue
        row = lf[b] / t
        k = int(top_k[b])
        if 0 < k < V:
            kth = row.topk(k).values[-1]
            row = row.masked_fill(row < kth, float("-inf"))
        probs = row.softmax(-1)
        p = float(top_p[b])
        if p < 1.0:
            sp, idx = probs.sort(descending=True)
            cum = sp.cumsum(-1)
            keep = cum - sp < p          # keep tokens until cumulative >= p
            sp = sp * keep
            sp = sp / sp.sum()
            # inverse-CDF draw on the sorted distribution
            c = sp.cumsum(-1)
            j = int(torch.searchsorted(c, uniform[b].to(c.dtype), right=False).clamp(max=V - 1))
            out[b] = int(idx[j])
        else:
            c = probs.cumsum(-1)
            j = int(torch.searchsorted(c, uniform[b].to(c.dtype), right=False).clamp(max=V - 1))
            out[b] = j
    return out


def sample_fused(logits: torch.Tensor, temperature: torch.Tensor,
                 top_p: torch.Tensor, top_k: torch.Tensor,
                 uniform: torch.Tensor) -> torch.Tensor:
    """Twin of csrc/sampling_fused.hip: tie-exact top-k / top-p sampling,
    vectorised over rows, on whatever device the inputs are on.

    x = logits, t = temperature, k = top_k, p = top_p, u = uniform:
      t == 0          argmax.
      0 < k < V       keep x >= the k-th largest x (ties at the cut stay).
      weights         w = exp((x - max) / max(t, 1e-6)) over what is kept.
      p < 1           keep a value's tokens while the mass strictly above
                      that value is < p * sum(w); the maximum always stays.
      draw            first kept token in vocabulary order whose inclusive
                      running sum exceeds u * (kept mass); the last kept
                      token with weight if rounding leaves none.
    Tokens of equal value are kept or dropped together, so no sort order
    enters the result.  Sums run in float64.
    """
    B, V = logits.shape
    dev = logits.device
    x = logits.double()
    t = temperature.to(dev).double()
    k = top_k.to(dev).long()
    p = top_p.to(dev).double()
    u = uniform.to(dev).double()
    greedy = logits.float().argmax(-1)
    xs, order = x.sort(-1, descending=True)
    k_on = (k > 0) & (k < V)
    kth = xs.gather(1, (torch.where(k_on, k, torch.ones_like(k)) - 1)[:, None])
    keep = (x >= kth) | ~k_on[:, None]
    m = xs[:, :1]
    w = torch.exp((x - m) / t.clamp_min(1e-6)[:, None])
    w = torch.where(keep & torch.isfinite(x), w, torch.zeros_like(w))
    w = torch.nan_to_num(w, nan=0.0, posinf=0.0)
    # mass strictly above each value: the exclusive running sum at the
    # first sorted position of the value's tie group
    ws = w.gather(1, order)
    excl = ws.cumsum(-1) - ws
    ar = torch.arange(V, device=dev).expand(B, V)
    first = torch.ones(B, V, dtype=torch.bool, device=dev)
    first[:, 1:] = xs[:, 1:] != xs[:, :-1]
    start = torch.where(first, ar, torch.zeros_like(ar)).cummax(-1).values
    above = excl.gather(1, start)
    z = ws.sum(-1, keepdim=True)
    keep_s = (above < p[:, None] * z) | (start == 0) | (p >= 1)[:, None]
    keep_p = torch.zeros_like(keep_s).scatter(1, order, keep_s)
    w = torch.where(keep_p, w, torch.zeros_like(w))
    c = w.cumsum(-1)
    hit = c > (u * c[:, -1])[:, None]
    tok = hit.int().argmax(-1)
    last = (V - 1) - (w > 0).flip(-1).int().argmax(-1)
    tok = torch.where(hit.any(-1), tok, last)
    dead = ~(w > 0).any(-1)
    return torch.where((temperature.to(dev) == 0) | dead, greedy, tok)


LOGPROB_COLS = 21       # the chosen token + up to 20 alternatives


def token_logprobs(logits: torch.Tensor, chosen: torch.Tensor,
                   n_top: torch.Tensor, out_val: torch.Tensor = None,
                   out_id: torch.Tensor = None):
    """Twin of csrc/logprobs.hip, vectorised over rows.

    logits [B, V]; chosen int64 [B]; n_top int32 [B].  Returns (val float32
    [B, 21], id int32 [B, 21]).  Per row, with n = min(n_top, 20):
      n_top < 0    the row did not ask: its outputs are left as they are
                   (fresh outputs hold id -1, value -inf).
      column 0     (chosen, logprob of chosen); -inf when chosen lies
                   outside [0, V) or on a non-finite logit.
      columns 1..n the first n tokens of a stable sort by (-logit, id).
      the rest     id -1, value -inf.
    logprob = x - logsumexp over the finite logits of the row as handed in
    (temperature 1, before top-k / top-p); non-finite logits weigh nothing,
    rank below every finite one and report -inf.  Sums run in float64.
    """
    B, V = logits.shape
    dev = logits.device
    ninf = float("-inf")
    if out_val is None:
        out_val = torch.full((B, LOGPROB_COLS), ninf, dtype=torch.float32,
                             device=dev)
    if out_id is None:
        out_id = torch.full((B, LOGPROB_COLS), -1, dtype=torch.int32,
                            device=dev)
    n = n_top.to(dev).long()
    ask = n >= 0
    if not bool(ask.any()):
        return out_val, out_id
    x = logits.double()
    fin = torch.isfinite(x)
    xf = torch.where(fin, x, torch.full_like(x, ninf))
    m = xf.max(-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    lse = m + torch.log(torch.exp(xf - m).sum(-1, keepdim=True))
    lp = torch.where(fin, x - lse, torch.full_like(x, ninf))
    K = min(LOGPROB_COLS - 1, V)
    order = torch.sort(-xf, dim=-1, stable=True).indices[:, :K]
    valid = torch.arange(K, device=dev)[None, :] < n.clamp(max=K)[:, None]
    val = torch.full((B, LOGPROB_COLS), ninf, dtype=torch.float64,
                     device=dev)
    idx = torch.full((B, LOGPROB_COLS), -1, dtype=torch.long, device=dev)
    val[:, 1:1 + K] = torch.where(valid, lp.gather(1, order),
                                  val[:, 1:1 + K])
    idx[:, 1:1 + K] = torch.where(valid, order, idx[:, 1:1 + K])
    c = chosen.to(dev).long()
    ok = (c >= 0) & (c < V)
    lpc = lp.gather(1, c.clamp(0, V - 1)[:, None]).squeeze(1)
    val[:, 0] = torch.where(ok, lpc, torch.full_like(lpc, ninf))
    idx[:, 0] = c
    out_val.copy_(torch.where(ask[:, None], val.to(out_val.dtype), out_val))
    out_id.copy_(torch.where(ask[:, None], idx.to(out_id.dtype), out_id))
    return out_val, out_id


def penalty_build(table: torch.Tensor, slots: torch.Tensor,
                  tokens: torch.Tensor, offsets: torch.Tensor,
                  prompt_len: torch.Tensor) -> None:
    """Twin of csrc/penalties.hip penalty_build.  table int32 [slots, V];
    row slots[i] := history tokens[offsets[i]:offsets[i+1]], the first
    prompt_len[i] of them prompt: word = 2 * count among the generated
    tokens + (token occurs in the prompt).  Ids outside [0, V) are skipped;
    whatever the row held before is gone."""
    S, V = table.shape
    off = offsets.tolist()
    for i, slot in enumerate(slots.tolist()):
        if slot < 0 or slot >= S:
            continue
        h = tokens[max(off[i], 0):off[i + 1]].long()
        n = int(prompt_len[i])
        ok = (h >= 0) & (h < V)
        pos = torch.arange(h.numel(), device=h.device)
        gen = torch.bincount(h[ok & (pos >= n)], minlength=V)
        pro = torch.bincount(h[ok & (pos < n)], minlength=V) > 0
        table[slot] = (2 * gen + pro.long()).to(torch.int32)


def penalty_apply(logits: torch.Tensor, slot: torch.Tensor,
                  rep: torch.Tensor, pres: torch.Tensor, freq: torch.Tensor,
                  table: torch.Tensor) -> None:
    """Twin of penalty_apply, in place on logits [R, V].  For rows with
    slot >= 0 and tokens whose table word is non-zero, in float32 and one
    rounded operation at a time (the kernel is held to the same bits):
        q = l / r if l > 0 else l * r
        q = q - f * c            c = word >> 1
        q = q - (p if c > 0 else 0)
    rounded to the logits' dtype.  Other logits, and NaN, keep their bits."""
    R = logits.shape[0]
    S = table.shape[0]
    sl = slot[:R].long()
    rows = torch.nonzero((sl >= 0) & (sl < S)).flatten()
    if rows.numel() == 0:
        return
    w = table[sl[rows]]
    c = w >> 1
    old = logits[rows]
    l = old.to(torch.float32)
    r = rep[:R][rows].to(torch.float32)[:, None]
    p = pres[:R][rows].to(torch.float32)[:, None]
    f = freq[:R][rows].to(torch.float32)[:, None]
    q = torch.where(l > 0, l / r, l * r)
    fc = f * c.to(torch.float32)
    q = q - fc
    q = q - torch.where(c > 0, p, torch.zeros_like(p))
    new = q.to(logits.dtype)
    logits[rows] = torch.where((w != 0) & ~torch.isnan(l), new, old)


def penalty_note(table: torch.Tensor, slot: torch.Tensor,
                 sampled: torch.Tensor) -> None:
    """Twin of penalty_note: table[slot[r], sampled[r]] += 2 for the rows
    r < len(sampled) with a slot and a token inside the vocabulary."""
    S, V = table.shape
    R = sampled.numel()
    sl = slot[:R].long()
    t = sampled.long()
    ok = (sl >= 0) & (sl < S) & (t >= 0) & (t < V)
    table.index_put_((sl[ok], t[ok]),
                     torch.full((int(ok.sum()),), 2, dtype=table.dtype,
                                device=table.device), accumulate=True)


# JSON-mode guided decoding on the device (csrc/guided.hip spells the state
# layout out).  A state row is GUIDED_WORDS int32 words: mode | flags | depth
# | 8 words of stack bits; the mode numbers index GUIDED_MODES, the modes of
# engine.guided.JsonByteMachine in the order of its allowed(), and GUIDED_DEAD
# follows them.
GUIDED_WORDS = 11
GUIDED_MODES = ("value", "value_first", "key", "key_first", "colon", "string",
                "escape", "hex", "lit", "num_minus", "num_zero", "num_int",
                "num_dot", "num_frac", "num_esign", "num_e", "num_exp", "end")
GUIDED_DEAD = len(GUIDED_MODES)         # 18: allows EOS only, sticky
GUIDED_MAX_DEPTH = 256                  # no '{' or '[' at this depth
GUIDED_BYTE_IDS = 4 + 256               # byte b is id b + 4, EOS is id 2
# the literals' bytes after the first, by literal number 1..3; a remaining
# b"e" is stored as number 1 whichever literal it ends
GUIDED_LITS = (b"", b"rue", b"alse", b"ull")

_G = {m: i for i, m in enumerate(GUIDED_MODES)}
_G_DIGITS = frozenset(b"0123456789")
_G_HEX = frozenset(b"0123456789abcdefABCDEF")
_G_ESC = frozenset(b'"\\/bfnrtu')
_G_EXP = frozenset(b"eE")
_G_TERMINABLE = (_G["num_zero"], _G["num_int"], _G["num_frac"], _G["num_exp"],
                 _G["end"])


def _guided_load(w):
    """(mode, in_key, hex_left, lit, lit_n, depth, top) of one state row
    (a list of ints, w[0] >= 0); top -1 = stack empty, 0 arr, 1 obj.  Words
    out of range read as GUIDED_DEAD, as in the kernels."""
    mode, f, depth = w[0], w[1], w[2]
    in_key, hex_left = f & 1, (f >> 1) & 7
    lit, lit_n = (f >> 4) & 3, (f >> 6) & 7
    if mode > GUIDED_DEAD or depth < 0 or depth > GUIDED_MAX_DEPTH:
        mode, depth = GUIDED_DEAD, 0
    if mode == _G["lit"] and (lit == 0 or lit_n < 1
                              or lit_n > len(GUIDED_LITS[lit])):
        mode = GUIDED_DEAD
    top = -1
    if depth > 0:
        d = depth - 1
        top = (w[3 + (d >> 5)] >> (d & 31)) & 1
    return mode, in_key, hex_left, lit, lit_n, depth, top


def _guided_allowed(mode: int, lit: int, lit_n: int, depth: int, top: int):
    """(frozenset of allowed bytes, eos_ok) of a loaded state."""
    end = frozenset() if top < 0 else frozenset(b",}" if top else b",]")
    start = set(b'"-tfn') | _G_DIGITS
    if depth < GUIDED_MAX_DEPTH:
        start |= set(b"{[")
    eos = top < 0 and mode in _G_TERMINABLE
    m = GUIDED_MODES[mode] if mode < GUIDED_DEAD else "DEAD"
    if m == "value":
        ok = start
    elif m == "value_first":
        ok = start | (set(b"]") if top >= 0 else set())
    elif m == "key":
        ok = set(b'"')
    elif m == "key_first":
        ok = set(b'"') | (set(b"}") if top >= 0 else set())
    elif m == "colon":
        ok = set(b":")
    elif m == "string":
        ok = set(range(0x20, 0x100))
    elif m == "escape":
        ok = _G_ESC
    elif m == "hex":
        ok = _G_HEX
    elif m == "lit":
        tail = GUIDED_LITS[lit]
        ok = {tail[len(tail) - lit_n]}
    elif m in ("num_minus", "num_dot", "num_esign"):
        ok = _G_DIGITS
    elif m == "num_zero":
        ok = set(b".") | _G_EXP | end
    elif m == "num_int":
        ok = _G_DIGITS | set(b".") | _G_EXP | end
    elif m == "num_frac":
        ok = _G_DIGITS | _G_EXP | end
    elif m == "num_e":
        ok = _G_DIGITS | set(b"+-")
    elif m == "num_exp":
        ok = _G_DIGITS | end
    elif m == "end":
        ok = end
    else:                               # DEAD: may only stop
        ok, eos = set(), True
    return frozenset(ok), eos


def guided_json_mask(logits: torch.Tensor, state: torch.Tensor) -> None:
    """Twin of csrc/guided.hip guided_json_mask, in place on logits [R, V]
    (V >= 260).  For the rows r < R with state[r, 0] >= 0 every token id the
    row's state does not allow becomes -inf: ids >= 260, ids 0, 1 and 3,
    id 2 (EOS) unless the top-level value is closed, id 4 + b unless byte b
    may come next.  Allowed logits, and the other rows, keep their bits."""
    R, V = logits.shape
    if V < GUIDED_BYTE_IDS:
        raise ValueError(
            f"guided_json_mask: the vocabulary must hold the "
            f"{GUIDED_BYTE_IDS} ids of the byte tokenizer, got {V}")
    st = state[:R].cpu()
    rows = torch.nonzero(st[:, 0] >= 0).flatten().tolist()
    if not rows:
        return
    keep = torch.zeros(len(rows), V, dtype=torch.bool)
    for k, r in enumerate(rows):
        mode, _, _, lit, lit_n, depth, top = _guided_load(st[r].tolist())
        ok, eos = _guided_allowed(mode, lit, lit_n, depth, top)
        if ok:
            keep[k, torch.tensor(sorted(ok)) + 4] = True
        keep[k, 2] = eos
    idx = torch.tensor(rows, device=logits.device)
    old = logits[idx]
    logits[idx] = torch.where(keep.to(logits.device), old,
                              torch.full_like(old, float("-inf")))


def _guided_feed(w, b: int) -> None:
    """One state row (a list of ints, w[0] >= 0) fed byte b, in place: the
    port of JsonByteMachine.feed that the advance kernel runs."""
    mode, in_key, hex_left, lit, lit_n, depth, top = _guided_load(w)
    ok, _ = _guided_allowed(mode, lit, lit_n, depth, top)
    if b not in ok:
        w[0] = GUIDED_DEAD
        return

    def push(obj):
        nonlocal depth
        if obj:
            w[3 + (depth >> 5)] |= 1 << (depth & 31)
        depth += 1

    def pop():
        nonlocal depth
        depth -= 1
        w[3 + (depth >> 5)] &= ~(1 << (depth & 31))

    def feed_end():
        if b == ord(","):
            return _G["key"] if top else _G["value"]
        pop()
        return _G["end"]

    m = GUIDED_MODES[mode]
    digit = b in _G_DIGITS
    if m in ("value", "value_first"):
        if m == "value_first" and b == ord("]"):
            pop()
            m = "end"
        elif b == ord('"'):
            in_key, m = 0, "string"
        elif b == ord("{"):
            push(1)
            m = "key_first"
        elif b == ord("["):
            push(0)
            m = "value_first"
        elif b == ord("-"):
            m = "num_minus"
        elif b == ord("0"):
            m = "num_zero"
        elif digit:
            m = "num_int"
        else:
            lit = 1 if b == ord("t") else 2 if b == ord("f") else 3
            lit_n = len(GUIDED_LITS[lit])
            m = "lit"
    elif m in ("key", "key_first"):
        if b == ord("}"):
            pop()
            m = "end"
        else:
            in_key, m = 1, "string"
    elif m == "colon":
        m = "value"
    elif m == "string":
        if b == 0x22:
            m = "colon" if in_key else "end"
        elif b == 0x5C:
            m = "escape"
    elif m == "escape":
        if b == ord("u"):
            hex_left, m = 4, "hex"
        else:
            m = "string"
    elif m == "hex":
        hex_left -= 1
        if hex_left <= 0:
            hex_left, m = 0, "string"
    elif m == "lit":
        lit_n -= 1
        if lit_n == 0:
            lit, m = 0, "end"
        elif lit_n == 1 and lit == 2:
            lit = 1
    elif m == "num_minus":
        m = "num_zero" if b == ord("0") else "num_int"
    elif m in ("num_zero", "num_int", "num_frac", "num_exp"):
        if b == ord("."):
            m = "num_dot"
        elif b in _G_EXP and m != "num_exp":
            m = "num_e"
        elif digit and m != "num_zero":
            pass
        else:
            m = GUIDED_MODES[feed_end()]
    elif m == "num_dot":
        m = "num_frac"
    elif m == "num_e":
        m = "num_exp" if digit else "num_esign"
    elif m == "num_esign":
        m = "num_exp"
    else:                               # end
        m = GUIDED_MODES[feed_end()]
    w[0] = _G[m]
    w[1] = in_key | (hex_left << 1) | (lit << 4) | (lit_n << 6)
    w[2] = depth


def _guided_i32(x: int) -> int:
    """Python int -> the int32 with the same low 32 bits."""
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def guided_json_advance(state: torch.Tensor, sampled: torch.Tensor) -> None:
    """Twin of guided_json_advance: state[r] := state[r] fed sampled[r] for
    the rows r < len(sampled) with state[r, 0] >= 0; a token outside 4..259
    leaves the row as it is (JsonByteMachine.feed_token), a byte the state
    does not allow makes it GUIDED_DEAD."""
    R = sampled.numel()
    st = state[:R].cpu()
    tok = sampled.cpu().tolist()
    changed = False
    for r in torch.nonzero(st[:, 0] >= 0).flatten().tolist():
        t = tok[r]
        if t < 4 or t >= GUIDED_BYTE_IDS:
            continue
        w = [x & 0xFFFFFFFF if i >= 3 else x
             for i, x in enumerate(st[r].tolist())]
        _guided_feed(w, t - 4)
        st[r] = torch.tensor([_guided_i32(x) for x in w], dtype=torch.int32)
        changed = True
    if changed:
        state[:R] = st.to(state.device)


def moe_route(hidden: torch.Tensor, router_w: torch.Tensor, top_k: int):
    """Softmax-topk routing: returns (weights [T,K], expert_ids [T,K])."""
    logits = hidden.float() @ router_w.float().t()
    probs = logits.softmax(-1)
    w, ids = probs.topk(top_k, dim=-1)
    w = w / w.sum(-1, keepdim=True)
    return w, ids

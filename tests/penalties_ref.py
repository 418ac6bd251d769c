"""Independent numpy reference for the penalty ops (csrc/penalties.hip,
hyperspot.ops.torch_ref): counts from np.bincount over the history, the
arithmetic in np.float32 one operation per line, bf16 rounding by bit
manipulation.  Loaded by path from the test modules."""

import numpy as np
import torch


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    """bf16 tensor -> its bit patterns as uint16 (a copy)."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy() \
        .astype(np.uint16)


def from_bits(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(bits.astype(np.uint16).view(np.int16).copy()) \
        .view(torch.bfloat16)


def bits_to_f32(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16_bits(q: np.ndarray) -> np.ndarray:
    """Round to nearest even: add 0x7fff + lsb, keep the high half.  NaN is
    passed through (its high half, quiet bit set)."""
    u = np.ascontiguousarray(q, dtype=np.float32).view(np.uint32)
    lsb = (u >> np.uint32(16)) & np.uint32(1)
    r = ((u + np.uint32(0x7fff) + lsb) >> np.uint32(16)).astype(np.uint16)
    nan = ((u >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16)
    return np.where(np.isnan(q), nan, r)


def counts(history, prompt_len, vocab):
    """(c, s): c[t] = occurrences of t among history[prompt_len:], s[t] =
    t occurs anywhere in history.  Ids outside [0, vocab) are skipped."""
    h = np.asarray(history, dtype=np.int64).reshape(-1)
    ok = (h >= 0) & (h < vocab)
    pos = np.arange(h.size)
    c = np.bincount(h[ok & (pos >= prompt_len)], minlength=vocab)
    a = np.bincount(h[ok], minlength=vocab)
    return c.astype(np.int64), a > 0


def table_row(history, prompt_len, vocab) -> np.ndarray:
    """The table encoding of a history: 2 * c[t] + (t is in the prompt)."""
    h = np.asarray(history, dtype=np.int64).reshape(-1)
    c, _ = counts(h, prompt_len, vocab)
    _, in_prompt = counts(h[:prompt_len], prompt_len, vocab)
    return (2 * c + in_prompt).astype(np.int32)


def penalise_row(bits, history, prompt_len, r, p, f) -> np.ndarray:
    """bf16 bit patterns of one logits row -> the penalised row's."""
    bits = np.asarray(bits, dtype=np.uint16)
    c, s = counts(history, prompt_len, bits.size)
    r, p, f = np.float32(r), np.float32(p), np.float32(f)
    with np.errstate(all="ignore"):
        l = bits_to_f32(bits)
        quo = l / r
        pro = l * r
        q = np.where(l > 0, quo, pro).astype(np.float32)
        cf = c.astype(np.float32)
        fc = (f * cf).astype(np.float32)
        q = (q - fc).astype(np.float32)
        pp = np.where(c > 0, p, np.float32(0)).astype(np.float32)
        q = (q - pp).astype(np.float32)
    new = f32_to_bf16_bits(q)
    # unseen tokens keep their bits; so does a NaN logit
    return np.where(s & ~np.isnan(l), new, bits).astype(np.uint16)


def reference(logits: torch.Tensor, slot, rep, pres, freq, histories):
    """logits bf16 [R, V]; slot[i] < 0 = the row is left alone, otherwise
    histories[slot[i]] = (tokens, prompt_len).  Returns uint16 bits [R, V]."""
    bits = bf16_bits(logits)
    out = bits.copy()
    for i, sl in enumerate(np.asarray(slot).tolist()):
        if sl < 0:
            continue
        h, n = histories[sl]
        out[i] = penalise_row(bits[i], h, n, float(rep[i]), float(pres[i]),
                              float(freq[i]))
    return out


# Hand-computed, dyadic values (exact in any precision):
#   (logit, r, f, c, p, seen only in the prompt, expected)
HAND_CASES = [
    (2.0, 2.0, 0.5, 3, 0.25, False, -0.75),     # 2/2 - 0.5*3 - 0.25
    (-1.5, 2.0, 0.5, 3, 0.25, False, -4.75),    # -1.5*2 - 1.5 - 0.25
    (2.0, 2.0, 0.5, 0, 0.25, True, 1.0),        # prompt only: r alone
    (-1.5, 2.0, 0.5, 0, 0.25, True, -3.0),
    (4.0, 1.0, -0.5, 2, -1.0, False, 6.0),      # negative penalties reward
    (0.0, 4.0, 1.0, 1, 0.5, False, -1.5),
]


def make_case(rows, vocab, seed, max_slots=None):
    """Random penalty problem: bf16 logits with special values sprinkled in,
    histories of length 0, 1 and a few hundred (repeats, out-of-range ids,
    prompt-only / output-only / both), shuffled slots, some rows slot -1.
    Returns (logits, slot i32, rep, pres, freq f32, histories by slot)."""
    g = np.random.default_rng(seed)
    logits = torch.from_numpy(
        (g.standard_normal((rows, vocab)) * 4).astype(np.float32)) \
        .to(torch.bfloat16)
    special = [float("inf"), float("-inf"), float("nan"), 0.0, -0.0]
    for i in range(rows):
        for j, v in enumerate(special):
            logits[i, (7 * i + 13 * j) % vocab] = v
    nslots = max_slots or rows
    perm = g.permutation(nslots)
    slot = np.full(rows, -1, dtype=np.int32)
    histories = {}
    k = 0
    for i in range(rows):
        if i % 5 == 3:
            continue                             # not a penalty row
        sl = int(perm[k]); k += 1
        slot[i] = sl
        kind = i % 4
        n = [0, 1, 300, 200 + 17 * i][kind]
        pool = g.integers(0, vocab, size=max(1, min(vocab, 40)))
        h = g.choice(pool, size=n) if n else np.zeros(0, dtype=np.int64)
        h = h.astype(np.int64)
        if n > 4:
            h[1] = -3
            h[n // 2] = vocab
            h[n - 1] = vocab + 12345
            # the specials get penalised too
            h[2] = (7 * i) % vocab
            h[3] = (7 * i + 13 * 2) % vocab
            h[4] = (7 * i + 13 * 4) % vocab
        plen = [0, n, n // 2][i % 3]             # output-only, prompt-only, both
        histories[sl] = (h, plen)
    rep = g.choice(np.array([1.0, 1.1, 1.3, 0.7, 2.0], dtype=np.float32),
                   size=rows)
    pres = g.uniform(-2, 2, size=rows).astype(np.float32)
    freq = g.uniform(-2, 2, size=rows).astype(np.float32)
    return logits, slot, rep, pres, freq, histories


def flat_histories(histories, order):
    """(slots, tokens, offsets, prompt_len) int32 arrays for penalty_build,
    histories taken in the given slot order.  Out-of-int32 ids are kept out
    of range."""
    toks, off, plen = [], [0], []
    for sl in order:
        h, n = histories[sl]
        toks.extend(int(t) for t in h)
        off.append(len(toks))
        plen.append(n)
    return (np.asarray(order, dtype=np.int32),
            np.asarray(toks, dtype=np.int32).reshape(-1),
            np.asarray(off, dtype=np.int32),
            np.asarray(plen, dtype=np.int32))

"""Shared by the fp8 numerics tests (test_quant_gpu.py, test_kv_append_gpu.py,
test_paged_attn_gpu.py): e4m3fn code helpers and float64 references of the
three fp8 producers in csrc/quant.hip and of the fused RoPE.

Every reference follows the kernel's definition of the op, on CPU tensors:
  scale        s = max(amax / 448, 1e-8), one per row
  codes        e4m3fn(value / s): the float64 quotient rounded once to fp32
               and then converted (torch's convert is round-to-nearest-even)
  fused norm   normalises the unrounded fp32 sum x + res and stores
               bf16(x + res) as the new residual
Each op also has an fp32 twin written with plain torch ops.  The CPU tests
compare twin and float64 codes on the GPU tests' own inputs, which is what
licenses the cap the GPU tests put on the share of differing codes.
"""

import torch

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
CODE_MAX_POS, CODE_MAX_NEG, CODE_NAN = 0x7e, 0xfe, 0x7f
CHUNK = 2048            # elements one pass of 256 threads x 8 covers


def codes(t):
    """uint8 view of an e4m3fn tensor."""
    return t.contiguous().view(torch.uint8)


def to_codes(x):
    """float (any width) -> e4m3fn codes, rounding once to fp32 first."""
    return codes(x.float().to(FP8))


def ordinal(c):
    """Signed ordinal of e4m3fn codes: neighbours on the number line are
    one apart, and +0 / -0 are both 0."""
    c = c.to(torch.int16)
    mag = c & 0x7f
    return torch.where((c & 0x80) != 0, -mag, mag)


def is_nan_code(c):
    return (c & 0x7f) == CODE_NAN


def compare_codes(got, want, what, cap):
    """Every element within one ordinal, at most `cap` of them not
    identical; prints and returns the measured share."""
    assert got.shape == want.shape, (got.shape, want.shape)
    assert not is_nan_code(got).any(), f"{what}: NaN code written"
    dist = (ordinal(got) - ordinal(want)).abs()
    share = (got != want).float().mean().item()
    print(f"{what}: {int((got != want).sum())} of {got.numel()} codes "
          f"differ (share {share:.2e}), max ordinal distance "
          f"{int(dist.max())}")
    assert int(dist.max()) <= 1, f"{what}: ordinal distance {int(dist.max())}"
    assert share <= cap, f"{what}: share {share:.3e} above {cap:.0e}"
    return share


# ---- inputs -------------------------------------------------------------

def planted_cols(width):
    """Column of each row's planted maximum: row 0 the first column, row 1
    the last, row 2 inside the final (for most widths partially filled)
    2048-wide chunk."""
    last = (width - 1) // CHUNK * CHUNK
    return [0, width - 1, last + (width - last) // 2]


PLANT_SIGN = [1.0, -1.0, 1.0]


def quant_input(rows, width, seed=0):
    """bf16 [rows, width], |x| <= 2.5 except one planted +-251/32 per row.

    value / scale is x * 448 / planted.  251 is the largest prime a bf16
    significand holds: only x = 251 / 2^k cancels it, and that lands on a
    code, so no element sits exactly on an e4m3 rounding midpoint (with a
    planted 9, every x = 27 / 2^k would)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, width, generator=g).clamp_(-2.5, 2.5)
    for r, c in enumerate(planted_cols(width)[:rows]):
        x[r, c] = 251.0 / 32 * PLANT_SIGN[r]
    return x.bfloat16()


def norm_input(rows, width, seed=0):
    """x, res, w (bf16).  |x + res| <= 3 and 0.5 <= w <= 1 except at the
    planted column of each row, where x + res = +-(17.375 + 15/1024) and
    w = 1.

    The rsqrt cancels out of value / scale, which leaves
    (x + res) * w * 448 / planted.  With a planted value of few
    significant bits (16, or 139/8) that product of short mantissas sits
    exactly on an e4m3 rounding midpoint for a visible share of the
    elements, and the last fp32 bit then decides their codes.  The planted
    sum is 17807/1024 with 17807 prime, which the numerators of x + res
    and w cannot cancel."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, width, generator=g).clamp_(-2, 2)
    res = torch.randn(rows, width, generator=g).clamp_(-1, 1)
    w = torch.rand(width, generator=g) * 0.5 + 0.5
    for r, c in enumerate(planted_cols(width)[:rows]):
        x[r, c] = 17.375 * PLANT_SIGN[r]
        res[r, c] = 15.0 / 1024 * PLANT_SIGN[r]
        w[c] = 1.0
    return x.bfloat16(), res.bfloat16(), w.bfloat16()


GATE_EDGES = [(1, 100.0), (2, -100.0), (3, 0.0)]    # (column, gate)


def silu_input(rows, inter, seed=0):
    """gate|up bf16 [rows, 2*inter]: |g|, |u| <= 2 (|silu(g)*u| < 3.6), the
    planted column has g = 8, u = +-4 (|f| ~ 32), and columns 1..3 carry the
    gates +100, -100 and 0 against a small up value."""
    g = torch.Generator().manual_seed(seed)
    gate = torch.randn(rows, inter, generator=g).clamp_(-2, 2)
    up = torch.randn(rows, inter, generator=g).clamp_(-2, 2)
    for c, gv in GATE_EDGES:
        gate[:, c] = gv
        up[:, c] = 0.0625
    for r, c in enumerate(planted_cols(inter)[:rows]):
        gate[r, c] = 8.0
        up[r, c] = 4.0 * PLANT_SIGN[r]
    return torch.cat([gate, up], dim=-1).bfloat16()


# ---- float64 references: the value each op quantises ---------------------

def quant_values64(x):
    return x.double()


def norm_values64(x, res, w, eps):
    f = (x.float() + res.float()).double()
    rs = 1.0 / torch.sqrt(f.pow(2).mean(-1, keepdim=True) + eps)
    return f * rs * w.double()


def norm_residual(x, res):
    return (x.float() + res.float()).bfloat16()


def silu_values64(gate_up):
    i = gate_up.shape[-1] // 2
    g, u = gate_up[..., :i].double(), gate_up[..., i:].double()
    return g / (1.0 + torch.exp(-g)) * u


def scale64(values):
    return (values.abs().amax(-1) / FP8_MAX).clamp_min(1e-8)


def ref_codes(values64, scale):
    """Reference codes under a given per-row scale (the kernel's own, so
    that a last-bit difference in the scale does not count as code error)."""
    return to_codes(values64 / scale.double()[:, None])


# ---- fp32 twins: the same ops in plain torch fp32 ------------------------

def _quantize32(v):
    s = (v.abs().amax(-1) / FP8_MAX).clamp_min(1e-8)
    inv = 1.0 / s
    return codes((v * inv[:, None]).to(FP8)), s


def quant_twin32(x):
    return _quantize32(x.float())


def norm_twin32(x, res, w, eps):
    f = x.float() + res.float()
    rs = torch.rsqrt(f.pow(2).sum(-1, keepdim=True) / f.shape[-1] + eps)
    return _quantize32(f * rs * w.float())


def silu_twin32(gate_up):
    i = gate_up.shape[-1] // 2
    g, u = gate_up[..., :i].float(), gate_up[..., i:].float()
    return _quantize32(g / (1.0 + torch.exp(-g)) * u)


# ---- RoPE ----------------------------------------------------------------

def rope64(x, cos_sin, positions):
    """NeoX rotation of x [T, heads, D] (any float dtype) in float64 with
    the kernel's own fp32 cos|sin table; returns float64."""
    d2 = x.shape[-1] // 2
    cs = cos_sin[positions.long()].double()
    c, s = cs[:, None, :d2], cs[:, None, d2:]
    x1, x2 = x[..., :d2].double(), x[..., d2:].double()
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def rope32(x, cos_sin, positions):
    """fp32 twin of rope64."""
    d2 = x.shape[-1] // 2
    cs = cos_sin[positions.long()].float()
    c, s = cs[:, None, :d2], cs[:, None, d2:]
    x1, x2 = x[..., :d2].float(), x[..., d2:].float()
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)

"""The three fp8 producers of csrc/quant.hip (quant_fp8,
fused_add_rmsnorm_fp8, silu_mul_fp8 in both its templates) against the
float64 references in fp8_ref.py: row scales, the code of a planted row
maximum, every code under the kernel's own scale, and what is written
outside the outputs.

The CPU tests at the top need no GPU: they hold the float64 reference and
its fp32 twin together on the inputs the GPU tests use, so the cap on
differing codes there can only be reached by the kernel.
"""

import importlib.util
import math
import pathlib

import pytest
import torch

import hyperspot.ops as ops

_spec = importlib.util.spec_from_file_location(
    "fp8_ref", pathlib.Path(__file__).with_name("fp8_ref.py"))
F = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(F)

gpu = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
SCALE_RTOL = 1e-4   # a few fp32 ops + rsqrtf/__expf, each good to ~1e-6
CODE_CAP = 1e-3     # share of codes allowed to differ from the reference
TWIN_CAP = 1e-4     # same, fp32 twin against float64, on CPU
SENTINEL = 0xa5
PAD = 256           # sentinel bytes on either side of an output

QUANT_WIDTHS = [8, 264, 2048, 2056, 4096, 16384]
NORM_WIDTHS = [8, 2056, 4096, 16384]
SILU_INTERS = [8, 1024, 16384, 16392, 28672]


def _twin_check(twin, values64, what):
    got, s = twin
    share = F.compare_codes(got, F.ref_codes(values64, s), what, TWIN_CAP)
    rel = ((s.double() - F.scale64(values64)).abs()
           / F.scale64(values64)).max().item()
    assert rel < 1e-6, (what, rel)
    return share


@pytest.mark.parametrize("width", QUANT_WIDTHS)
def test_cpu_quant_twin_matches_fp64(width):
    x = F.quant_input(3, width)
    _twin_check(F.quant_twin32(x), F.quant_values64(x), f"quant {width}")


@pytest.mark.parametrize("width", NORM_WIDTHS)
def test_cpu_norm_twin_matches_fp64(width):
    x, res, w = F.norm_input(3, width)
    _twin_check(F.norm_twin32(x, res, w, EPS),
                F.norm_values64(x, res, w, EPS), f"norm {width}")


@pytest.mark.parametrize("inter", SILU_INTERS)
def test_cpu_silu_twin_matches_fp64(inter):
    x = F.silu_input(3, inter)
    _twin_check(F.silu_twin32(x), F.silu_values64(x), f"silu {inter}")


def test_cpu_planted_maximum_dominates_and_saturates():
    """The inputs do what the GPU tests rely on: the planted element is at
    least 3x everything else in its row, and the reference encodes it to
    +-448 although the scaled value can exceed 448 by an ulp."""
    for width, vals in (
            (2056, F.quant_values64(F.quant_input(3, 2056))),
            (2056, F.norm_values64(*F.norm_input(3, 2056), EPS)),
            (16392, F.silu_values64(F.silu_input(3, 16392)))):
        a = vals.abs()
        for r, c in enumerate(F.planted_cols(width)):
            rest = a[r].clone()
            rest[c] = 0
            assert a[r, c] >= 3 * rest.max(), (width, r)
        want = F.ref_codes(vals, F.scale64(vals).float())
        for r, c in enumerate(F.planted_cols(width)):
            assert int(want[r, c]) == (F.CODE_MAX_POS if F.PLANT_SIGN[r] > 0
                                       else F.CODE_MAX_NEG)


# ---- GPU -------------------------------------------------------------------

def _native():
    assert ops.have_native(), \
        "hyperspot._C must be built on GPU boxes (python csrc/build.py)"
    from hyperspot import _C
    return _C


class _Guarded:
    """An output tensor inside a larger buffer of sentinel bytes."""

    def __init__(self, shape, dtype):
        n = math.prod(shape) * torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.uint8,
                              device=DEV)
        self.n = n
        self.t = self.buf[PAD:PAD + n].view(dtype).view(shape)

    def check(self, what):
        b = self.buf.cpu()
        assert (b[:PAD] == SENTINEL).all(), f"{what}: write before the start"
        assert (b[PAD + self.n:] == SENTINEL).all(), \
            f"{what}: write past the end"


def _outputs(rows, width):
    return (_Guarded((rows, width), torch.float8_e4m3fn),
            _Guarded((rows,), torch.float32))


def _check(out, scales, values64, what, rows, width, exact_scale=False):
    out.check(what + " out")
    scales.check(what + " scales")
    got = F.codes(out.t).cpu()
    s = scales.t.cpu()
    want_s = F.scale64(values64)
    if exact_scale:
        # bf16 -> fp32 is exact and the kernel divides in IEEE fp32
        amax = values64.abs().amax(-1).float()
        assert torch.equal(s, (amax / 448.0).clamp_min(1e-8)), (s, want_s)
    rel = ((s.double() - want_s).abs() / want_s).max().item()
    print(f"{what}: scale max rel err {rel:.2e}")
    assert rel <= SCALE_RTOL, (what, rel)
    for r, c in enumerate(F.planted_cols(width)[:rows]):
        want = F.CODE_MAX_POS if F.PLANT_SIGN[r] > 0 else F.CODE_MAX_NEG
        assert int(got[r, c]) == want, \
            f"{what}: planted max row {r} col {c} -> {int(got[r, c]):#x}"
    F.compare_codes(got, F.ref_codes(values64, s), what, CODE_CAP)


@gpu
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("width", QUANT_WIDTHS)
def test_quant_fp8(rows, width):
    """x is a row-strided view of a wider NaN-filled buffer, as the o_proj
    input is."""
    _C = _native()
    x = F.quant_input(rows, width)
    wide = torch.full((rows, width + 64), float("nan"),
                      dtype=torch.bfloat16, device=DEV)
    wide[:, 32:32 + width] = x.to(DEV)
    xv = wide[:, 32:32 + width]
    assert xv.stride(0) == width + 64 and (rows == 1 or
                                           not xv.is_contiguous())
    out, scales = _outputs(rows, width)
    _C.quant_fp8(out.t, scales.t, xv)
    _check(out, scales, F.quant_values64(x), f"quant_fp8 {rows}x{width}",
           rows, width, exact_scale=True)


@gpu
def test_quant_fp8_zero_and_subnormal_rows():
    """An all-zero row takes the 1e-8 floor and all-zero codes; so does a
    row of bf16 subnormals, whose amax / 448 is far below the floor (codes
    are signed zeros there)."""
    _C = _native()
    width = 2056
    x = F.quant_input(3, width)
    x[0] = 0
    sub = (torch.arange(width) % 127 + 1).to(torch.int16)
    sub[1::2] |= -0x8000                     # every other one negative
    x[2] = sub.view(torch.bfloat16)
    assert (x[2].float().abs() < 1.2e-38).all() and (x[2] != 0).all()
    out, scales = _outputs(3, width)
    _C.quant_fp8(out.t, scales.t, x.to(DEV))
    out.check("out")
    scales.check("scales")
    got, s = F.codes(out.t).cpu(), scales.t.cpu()
    floor = torch.tensor(1e-8, dtype=torch.float32)
    assert s[0] == floor and s[2] == floor, s
    assert not got[0].any()
    assert not (got[2] & 0x7f).any()
    F.compare_codes(got, F.ref_codes(x.double(), s), "zero/subnormal rows",
                    CODE_CAP)


@gpu
@pytest.mark.parametrize("width", NORM_WIDTHS)
def test_fused_add_rmsnorm_fp8(width):
    _C = _native()
    rows = 3
    x, res, w = F.norm_input(rows, width)
    out, scales = _outputs(rows, width)
    new_res = _Guarded((rows, width), torch.bfloat16)
    new_res.t.copy_(res)
    xd = x.to(DEV)
    _C.fused_add_rmsnorm_fp8(out.t, scales.t, xd, new_res.t, w.to(DEV), EPS)
    new_res.check("residual")
    assert torch.equal(xd.cpu().view(torch.int16), x.view(torch.int16))
    assert torch.equal(new_res.t.cpu().view(torch.int16),
                       F.norm_residual(x, res).view(torch.int16))
    _check(out, scales, F.norm_values64(x, res, w, EPS),
           f"fused_add_rmsnorm_fp8 {width}", rows, width)


@gpu
@pytest.mark.parametrize("inter", SILU_INTERS)
def test_silu_mul_fp8(inter):
    """inter <= 16384 runs the 8-chunk template, above it the 16-chunk
    one; 16392 is its first width, 28672 the Llama-70B MLP."""
    _C = _native()
    rows = 3
    x = F.silu_input(rows, inter)
    out, scales = _outputs(rows, inter)
    _C.silu_mul_fp8(out.t, scales.t, x.to(DEV))
    vals = F.silu_values64(x)
    _check(out, scales, vals, f"silu_mul_fp8 {inter}", rows, inter)
    # the gate edges: silu(100) = 100, silu(-100) = -0, silu(0) = 0
    got = F.codes(out.t).cpu()
    want = F.ref_codes(vals, scales.t.cpu())
    for c, _ in F.GATE_EDGES:
        assert torch.equal(F.ordinal(got[:, c]), F.ordinal(want[:, c])), c


@gpu
def test_bad_widths_raise():
    _C = _native()

    def bf(*shape):
        return torch.zeros(*shape, dtype=torch.bfloat16, device=DEV)

    def outs(rows, width):
        return (torch.zeros(rows, width, dtype=torch.float8_e4m3fn,
                            device=DEV),
                torch.zeros(rows, dtype=torch.float32, device=DEV))

    for width in (16392, 12):
        with pytest.raises(RuntimeError):
            _C.quant_fp8(*outs(1, width), bf(1, width))
    with pytest.raises(RuntimeError):
        _C.fused_add_rmsnorm_fp8(*outs(1, 16392), bf(1, 16392),
                                 bf(1, 16392), bf(16392), EPS)
    with pytest.raises(RuntimeError):
        _C.silu_mul_fp8(*outs(1, 32776), bf(1, 2 * 32776))
    torch.cuda.synchronize()

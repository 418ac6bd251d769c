"""Op dispatch layer.

On GPU (ROCm) every hot op runs a hand-written CDNA4 HIP kernel from the
in-tree extension ``hyperspot._C`` (csrc/, built for gfx950 only).  On CPU the
pure-PyTorch references in :mod:`hyperspot.ops.torch_ref` run instead (CI has
no GPU).  There is no CUDA path, no Triton, no multi-backend dispatch — a CUDA
device without the extension is a hard error, never a silent eager fallback.
"""

from __future__ import annotations

from typing import NamedTuple

import torch

from . import torch_ref

_C = None
_C_ERR: Exception | None = None
try:  # built by `python csrc/setup.py build_ext --inplace` (gfx950)
    from hyperspot import _C as _C  # type: ignore
except Exception as e:  # pragma: no cover - exercised only on GPU boxes
    _C_ERR = e


def have_native() -> bool:
    return _C is not None


def _native():
    if _C is None:
        raise RuntimeError(
            "hyperspot._C (gfx950 HIP extension) is not built but a GPU tensor "
            "reached the op layer. Build it in-tree with "
            "`python csrc/setup.py build_ext --inplace` "
            f"(import error: {_C_ERR!r})")
    return _C


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    if x.is_cuda:
        out = torch.empty_like(x)
        _native().rmsnorm(out, x, weight, eps)
        return out
    return torch_ref.rmsnorm(x, weight, eps)


def fused_add_rmsnorm(x: torch.Tensor, residual: torch.Tensor,
                      weight: torch.Tensor, eps: float):
    """residual += x (in place); x_out = rmsnorm(residual) (in place on x)."""
    if x.is_cuda:
        _native().fused_add_rmsnorm(x, residual, weight, eps)
        return x, residual
    out, res = torch_ref.fused_add_rmsnorm(x, residual, weight, eps)
    return out, res


def rope_kv_append(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                   positions: torch.Tensor, cos_sin: torch.Tensor,
                   slot_mapping: torch.Tensor,
                   k_cache: torch.Tensor, v_cache: torch.Tensor) -> None:
    """Fused: NeoX RoPE on q,k (in place) + scatter k,v into the paged cache.

    q [T,H,D], k/v [T,KV,D]; cos_sin [max_pos, D] fp32 (cos half | sin half);
    slot_mapping [T] int64 (-1 = skip append, e.g. sliding-window drop).
    """
    if q.is_cuda:
        _native().rope_kv_append(q, k, v, positions, cos_sin, slot_mapping,
                                 k_cache, v_cache)
        return
    d = q.shape[-1]
    cs = cos_sin[positions.long()]
    cos, sin = cs[:, : d // 2], cs[:, d // 2:]
    q.copy_(torch_ref._rotate_neox(q, cos, sin))
    k.copy_(torch_ref._rotate_neox(k, cos, sin))
    mask = slot_mapping >= 0
    if mask.any():
        torch_ref.kv_cache_append(k[mask], v[mask], k_cache, v_cache,
                                  slot_mapping[mask])


import os

_ATTN_SPLIT_TARGET = int(os.environ.get("HYPERSPOT_ATTN_SPLIT_TARGET", "256"))


def _attn_split(rows: int, kvh: int) -> int:
    """Flash-decode page-split factor: bring the workgroup count up to
    ~_ATTN_SPLIT_TARGET when rows*kvh alone cannot fill the 256 CUs (small
    batch, or the kvh=1 GQA shard of 70B at TP=8).  Measured (MI355X, profiles/
    r01_decode_v3.md): splitting at >=256 WGs already loses — the fp32
    partial round trip + merge launch cost more than the occupancy buys —
    so only genuinely tiny grids (rows*kvh < 256, e.g. batch<32 at TP=8)
    split.  Static in (rows, kvh) => capture-safe."""
    s = max(1, min(16, _ATTN_SPLIT_TARGET // max(1, rows * kvh)))
    return 1 if s <= 1 else s


def paged_attn_decode(q: torch.Tensor, k_cache: torch.Tensor,
                      v_cache: torch.Tensor, block_tables: torch.Tensor,
                      seq_lens: torch.Tensor, scale: float) -> torch.Tensor:
    if q.is_cuda:
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        kvh = k_cache.shape[1]
        split = _attn_split(q.shape[0], kvh) if q.shape[-1] == 128 else 1
        ws = None
        if split > 1:
            ws = torch.empty(q.shape[0] * kvh * split
                             * (q.shape[1] // kvh) * 130,
                             dtype=torch.float32, device=q.device)
        _native().paged_attn(out, q, k_cache, v_cache, block_tables,
                             seq_lens, None, scale, ws, split)
        return out
    return torch_ref.paged_attn_decode(q, k_cache, v_cache, block_tables,
                                       seq_lens, scale)


# Short-chunk rule for prefill over the paged cache.  A step whose longest
# chunk is a handful of rows over a long context is decode-shaped: the MFMA
# kernel runs one workgroup per (sequence, head) serially over the context,
# the per-row kernel one per (row, kv head).  Measured on MI355X, H=32 KV=8,
# us/layer (profiles/r03_prefill_paged.md, bf16; fp8 within 10%):
#   chunk rows   1 seq, ctx 8192      8 seqs, ctx 8192
#                mfma   per-row       mfma   per-row
#        1        591     212          597     232
#       16        593     227          600     508
#       64        597     271          617    1657
#      256        612     862          691    6516
# At <= 16 rows the per-row kernel wins every measured shape; at 64 it
# depends on the sequence count (loses 2.7x at 8 sequences, wins 2.2x at
# one); from 256 on the MFMA kernel wins everywhere.  The gate reads the
# host integer meta.max_seqlen only: shapes-only, capture-safe.
_PAGED_MFMA_MAX_PER_ROW = 16


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
              k_cache: torch.Tensor, v_cache: torch.Tensor, meta,
              scale: float) -> torch.Tensor:
    """Attention for one layer, prefill or decode.

    Three gfx950 kernels, picked from shapes and step metadata only (no
    device read, so every choice is hipGraph-capture-safe):

    - decode: ``paged_attn``, one workgroup per (row, kv head) streaming
      the sequence's pages; rows attend over ctx=seq_len cache slots.
    - fresh prefill (every row of the step starts at position 0), head
      dim 128: ``attn_prefill_mfma``, MFMA flash attention reading K/V
      straight from the qkv projection.
    - any other head-dim-128 prefill step (a chunked-prefill continuation,
      the remainder after a prefix-cache hit, and whatever fresh requests
      are packed beside them), when ``meta.paged_mfma`` is set
      (``EngineConfig.prefill_paged_mfma``): ``attn_prefill_paged_mfma``,
      the same flash structure reading K/V from the paged cache, bf16 or
      fp8.  The fused RoPE kernel has appended the step's own k/v just
      before, so rows attend over slots 0..pos.  Steps whose longest chunk
      is at most ``_PAGED_MFMA_MAX_PER_ROW`` rows are decode-shaped and
      stay on ``paged_attn`` (measurement beside the constant).

    Without ``meta.paged_mfma`` (the default: the two kernels round
    differently, and a serving default must not change what a deployment
    computes) and for other head dims, such steps run ``paged_attn`` with
    per-row ctx_lens.
    """
    if meta.mode == "decode":
        return paged_attn_decode(q, k_cache, v_cache, meta.block_tables,
                                 meta.seq_lens, scale)
    if q.is_cuda:
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        if q.shape[-1] == 128 and getattr(meta, "fresh_prefill", True):
            # MFMA flash prefill (K/V straight from the qkv projection)
            _native().attn_prefill_mfma(out, q, k, v, meta.seq_start,
                                        meta.max_seqlen, scale)
        elif q.shape[-1] == 128 and getattr(meta, "paged_mfma", False) \
                and meta.max_seqlen > _PAGED_MFMA_MAX_PER_ROW:
            # MFMA flash prefill over the (freshly appended) paged cache
            if meta.ctx_start is None:
                raise RuntimeError(
                    "prefill over the paged cache needs meta.ctx_start")
            _native().attn_prefill_paged_mfma(
                out, q, k_cache, v_cache, meta.block_tables, meta.seq_start,
                meta.ctx_start, meta.max_seqlen, scale)
        else:
            # per-row attention over the paged cache: the default for
            # continuation steps, odd head dims, and decode-shaped steps
            # (short-chunk rule above)
            _native().paged_attn(out, q, k_cache, v_cache,
                                 meta.block_tables, meta.ctx_lens,
                                 meta.row_seq, scale, None, 1)
        return out
    if getattr(meta, "fresh_prefill", True):
        return torch_ref.prefill_attn(q, k, v, meta.seq_start, scale)
    return torch_ref.prefill_attn_paged(q, k_cache, v_cache,
                                        meta.block_tables, meta.ctx_lens,
                                        meta.row_seq, scale)


def silu_mul(gate_up: torch.Tensor) -> torch.Tensor:
    if gate_up.is_cuda:
        i = gate_up.shape[-1] // 2
        out = torch.empty(*gate_up.shape[:-1], i, dtype=gate_up.dtype,
                          device=gate_up.device)
        _native().silu_mul(out, gate_up)
        return out
    return torch_ref.silu_mul(gate_up)


class QTensor(NamedTuple):
    """Per-token-scaled fp8 activation: data e4m3fn [T,K], scale fp32 [T].

    Produced on GPU by the fused quant kernels (csrc/quant.hip) so fp8
    GEMM inputs never take an extra elementwise pass; consumed by the TP
    linear layers via torch._scaled_mm (hipBLASLt fp8 MFMA)."""

    data: torch.Tensor
    scale: torch.Tensor


def quant_fp8(x: torch.Tensor) -> QTensor:
    """[T,K] bf16 -> QTensor (GPU; row-per-workgroup amax+scale+pack)."""
    assert x.is_cuda
    T, K = x.shape
    out = torch.empty(T, K, dtype=torch.float8_e4m3fn, device=x.device)
    scales = torch.empty(T, dtype=torch.float32, device=x.device)
    _native().quant_fp8(out, scales, x)
    return QTensor(out, scales)


def fused_add_rmsnorm_q(x: torch.Tensor, residual: torch.Tensor,
                        weight: torch.Tensor, eps: float):
    """residual += x (in place); returns (QTensor of rmsnorm(residual)*w,
    residual).  GPU-only fused producer for the fp8 GEMM path."""
    assert x.is_cuda
    T, K = x.shape
    out = torch.empty(T, K, dtype=torch.float8_e4m3fn, device=x.device)
    scales = torch.empty(T, dtype=torch.float32, device=x.device)
    _native().fused_add_rmsnorm_fp8(out, scales, x, residual, weight, eps)
    return QTensor(out, scales), residual


def silu_mul_q(gate_up: torch.Tensor) -> QTensor:
    """silu(g)*u -> fp8 QTensor (GPU fused producer)."""
    assert gate_up.is_cuda
    i = gate_up.shape[-1] // 2
    out = torch.empty(*gate_up.shape[:-1], i, dtype=torch.float8_e4m3fn,
                      device=gate_up.device)
    scales = torch.empty(gate_up.shape[0], dtype=torch.float32,
                         device=gate_up.device)
    _native().silu_mul_fp8(out, scales, gate_up)
    return QTensor(out, scales)


MOE_BM = 256  # sorted-pair tile granularity of the MoE kernels (csrc/moe.hip)


def _moe_splitk(nblocks: int, nchunks: int, out_numel: int, dev):
    """Split-K degree + fp32 workspace for a grouped GEMM launch.

    The w2 GEMM at Mixtral decode shapes has ~288 blocks for 256 CUs —
    its ragged second wave idles most of the chip; splitting K into up
    to 8 segments (each must keep >= 3 k-chunks for the LDS ring and
    divide the chunk count) multiplies the block count back above ~4
    per CU.  Shapes-only decision: hipGraph-capture-safe.
    HS_MOE_SPLITK forces a degree (0 = auto)."""
    forced = int(os.environ.get("HS_MOE_SPLITK", "0"))
    s = 1
    if forced and nblocks >= 1024:
        forced = 0          # forcing never touches saturated launches
    while (s < 8 and nchunks % (s * 2) == 0 and nchunks // (s * 2) >= 3
           and (nblocks * s < 1024 if not forced else s * 2 <= forced)):
        s *= 2
    if forced == 1:
        s = 1
    if s == 1:
        return 1, None
    return s, torch.empty(s * out_numel, dtype=torch.float32, device=dev)


def moe_ffn(x: torch.Tensor, w13: torch.Tensor, w2: torch.Tensor,
            weights: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """Grouped expert SwiGLU FFN (GPU, hipGraph-capture-safe).

    x [T,H]; w13 [E_local, 2I, H]; w2 [E_local, H, I]; weights [T,K] fp32/bf16
    routing weights; ids [T,K] LOCAL expert indices.  Token->expert sorting,
    the two grouped MFMA GEMMs and the weighted combine all run on-device
    with grids that depend only on (T, K, E) — no host sync, no dynamic
    shapes (MoE dispatch/combine + grouped GEMM).

    Every id must lie in [0, E_local): the kernels index LDS counters and
    the weight tensor with it, and checking that would take a host sync,
    so ids outside the range are outside the contract.  T == 0 (an EP rank
    that received nothing) returns an empty [0, H] tensor, no launch.
    """
    T, H = x.shape
    if T == 0:
        return torch.empty(0, H, dtype=torch.bfloat16, device=x.device)
    K = ids.shape[1]
    E = w13.shape[0]
    TK = T * K
    ntiles = (TK + E * (MOE_BM - 1) + MOE_BM - 1) // MOE_BM
    P = ntiles * MOE_BM
    dev = x.device
    flat = ids.reshape(-1).to(torch.int32)
    sorted_ids = torch.empty(P, dtype=torch.int32, device=dev)
    tile_expert = torch.empty(ntiles, dtype=torch.int32, device=dev)
    inv_pos = torch.empty(TK, dtype=torch.int32, device=dev)
    n = _native()
    n.moe_align(sorted_ids, tile_expert, inv_pos, flat, E)
    I2 = w13.shape[1]
    h1 = torch.empty(P, I2, dtype=torch.bfloat16, device=dev)
    s1, ws1 = _moe_splitk(ntiles * (I2 // 128), H // 64, P * I2, dev)
    n.moe_gemm(h1, x, w13, sorted_ids, tile_expert, K, s1, ws1)
    a = silu_mul(h1)
    y = torch.empty(P, H, dtype=torch.bfloat16, device=dev)
    I = w2.shape[2]
    s2, ws2 = _moe_splitk(ntiles * (H // 128), I // 64, P * H, dev)
    n.moe_gemm(y, a, w2, sorted_ids, tile_expert, 0, s2, ws2)
    out = torch.empty(T, H, dtype=torch.bfloat16, device=dev)
    n.moe_combine(out, y, weights.float().contiguous(), inv_pos, K)
    return out


def moe_ffn_fp8(xq: "QTensor", w13q: torch.Tensor, w13s: torch.Tensor,
                w2q: torch.Tensor, w2s: torch.Tensor,
                weights: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """fp8 grouped expert FFN: e4m3fn activations (QTensor from the fused
    norm producer) x e4m3fn expert weights through
    v_mfma_f32_32x32x16_fp8_fp8; the silu stage re-quantizes via the fused
    silu_mul_fp8 kernel so no extra passes appear.  ~2x the bf16 MoE
    weight bandwidth (the binding constraint, profiles/r01).

    As for moe_ffn, ids outside [0, E_local) are outside the contract (no
    check without a host sync), and T == 0 returns an empty [0, H] tensor
    without a launch."""
    T, H = xq.data.shape
    if T == 0:
        return torch.empty(0, H, dtype=torch.bfloat16,
                           device=xq.data.device)
    K = ids.shape[1]
    E = w13q.shape[0]
    TK = T * K
    ntiles = (TK + E * (MOE_BM - 1) + MOE_BM - 1) // MOE_BM
    P = ntiles * MOE_BM
    dev = xq.data.device
    flat = ids.reshape(-1).to(torch.int32)
    sorted_ids = torch.empty(P, dtype=torch.int32, device=dev)
    tile_expert = torch.empty(ntiles, dtype=torch.int32, device=dev)
    inv_pos = torch.empty(TK, dtype=torch.int32, device=dev)
    n = _native()
    n.moe_align(sorted_ids, tile_expert, inv_pos, flat, E)
    I2 = w13q.shape[1]
    h1 = torch.empty(P, I2, dtype=torch.bfloat16, device=dev)
    s1, ws1 = _moe_splitk(ntiles * (I2 // 128), H // 128, P * I2, dev)
    n.moe_gemm_fp8(h1, xq.data, xq.scale, w13q, w13s, sorted_ids,
                   tile_expert, K, s1, ws1)
    a = silu_mul_q(h1)
    y = torch.empty(P, H, dtype=torch.bfloat16, device=dev)
    I = w2q.shape[2]
    s2, ws2 = _moe_splitk(ntiles * (H // 128), I // 128, P * H, dev)
    n.moe_gemm_fp8(y, a.data, a.scale, w2q, w2s, sorted_ids, tile_expert,
                   0, s2, ws2)
    out = torch.empty(T, H, dtype=torch.bfloat16, device=dev)
    n.moe_combine(out, y, weights.float().contiguous(), inv_pos, K)
    return out


def greedy_sample(logits: torch.Tensor,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """Row-wise argmax; `out` (int64 [rows]) is written in place when given
    (the captured decode graph samples into its persistent buffer)."""
    if logits.is_cuda:
        if out is None:
            out = torch.empty(logits.shape[0], dtype=torch.long,
                              device=logits.device)
        _native().greedy_sample(out, logits)
        return out
    res = logits.float().argmax(-1)
    if out is not None:
        out.copy_(res)
        return out
    return res


def sample_fused(logits: torch.Tensor, temperature: torch.Tensor,
                 top_p: torch.Tensor, top_k: torch.Tensor,
                 uniform: torch.Tensor,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """Per-row temperature / top-k / top-p sampling in one kernel
    (csrc/sampling_fused.hip), straight from the bf16 logits: no fp32 copy,
    no sort, no host decision, so it can be captured into a graph.

    temperature, top_p float32 [rows]; top_k int32 [rows] (0 or >= vocab =
    off); uniform float32 [rows] in [0, 1).  temperature == 0 rows take the
    argmax.  Tokens of equal logit are kept or dropped together at either
    cut (torch_ref.sample_fused spells the semantics out).  `out` (int64
    [rows]) is written in place when given.  bf16 GPU logits go to the
    kernel, anything else to the torch twin."""
    if logits.is_cuda and logits.dtype == torch.bfloat16:
        if out is None:
            out = torch.empty(logits.shape[0], dtype=torch.long,
                              device=logits.device)
        _native().sample_fused(out, logits, temperature, top_p, top_k,
                               uniform)
        return out
    res = torch_ref.sample_fused(logits, temperature, top_p, top_k, uniform)
    if out is not None:
        out.copy_(res)
        return out
    return res


def token_logprobs(logits: torch.Tensor, chosen: torch.Tensor,
                   n_top: torch.Tensor, out_val: torch.Tensor | None = None,
                   out_id: torch.Tensor | None = None):
    """Log-probability of each row's chosen token and of its n_top[r] most
    likely tokens, in one kernel (csrc/logprobs.hip) straight from the bf16
    logits: no fp32 copy, no sort, no host decision, so it can be captured
    into a graph behind the sampler.

    chosen int64 [rows]; n_top int32 [rows]: < 0 = the row did not ask (its
    outputs stay untouched), 0 = the chosen token only, 1..20 = plus that
    many alternatives (values above 20 are outside the contract).  Returns
    (val float32 [rows, 21], id int32 [rows, 21]); column 0 is the chosen
    token, columns 1..n the alternatives by (-logit, id), the rest
    (-inf, -1).  torch_ref.token_logprobs spells the semantics out.
    `out_val` / `out_id` are written in place when given.  bf16 GPU logits
    go to the kernel, anything else to the torch twin."""
    if logits.is_cuda and logits.dtype == torch.bfloat16:
        rows = logits.shape[0]
        if out_val is None:
            out_val = torch.full((rows, torch_ref.LOGPROB_COLS),
                                 float("-inf"), dtype=torch.float32,
                                 device=logits.device)
        if out_id is None:
            out_id = torch.full((rows, torch_ref.LOGPROB_COLS), -1,
                                dtype=torch.int32, device=logits.device)
        _native().token_logprobs(out_val, out_id, logits, chosen, n_top)
        return out_val, out_id
    return torch_ref.token_logprobs(logits, chosen, n_top, out_val, out_id)


def penalty_build(table: torch.Tensor, slots: torch.Tensor,
                  tokens: torch.Tensor, offsets: torch.Tensor,
                  prompt_len: torch.Tensor) -> None:
    """Make rows of the penalty table encode whole histories
    (csrc/penalties.hip).

    table int32 [slots, vocab]; slots int32 [n] (distinct); tokens int32
    [total], the histories back to back; offsets int32 [n + 1]; prompt_len
    int32 [n]: how many of history i's first tokens are prompt.  A word is
    2 * (count among the generated tokens) + (occurs in the prompt); ids
    outside the vocabulary are skipped, and the row's earlier content is
    gone.  The grid depends on n: not for capture."""
    if table.is_cuda:
        _native().penalty_build(table, slots, tokens, offsets, prompt_len)
        return
    torch_ref.penalty_build(table, slots, tokens, offsets, prompt_len)


def penalty_apply(logits: torch.Tensor, slot: torch.Tensor,
                  rep: torch.Tensor, pres: torch.Tensor, freq: torch.Tensor,
                  table: torch.Tensor) -> None:
    """Repetition / frequency / presence penalties in place on logits
    [rows, vocab], from the counts in `table` (csrc/penalties.hip).

    slot int32, rep / pres / freq float32, each at least [rows] and read on
    the device, so the launch depends on rows and vocab alone and can be
    captured.  slot[r] < 0 = not a penalty row, left untouched, as is every
    logit whose token the row has not seen.  torch_ref.penalty_apply spells
    the arithmetic out; the kernel matches it bit for bit.  bf16 GPU logits
    go to the kernel, anything else to the torch twin."""
    if logits.is_cuda and logits.dtype == torch.bfloat16:
        _native().penalty_apply(logits, slot, rep, pres, freq, table)
        return
    torch_ref.penalty_apply(logits, slot, rep, pres, freq, table)


def penalty_note(table: torch.Tensor, slot: torch.Tensor,
                 sampled: torch.Tensor) -> None:
    """Count the token each penalty row has just sampled: table[slot[r],
    sampled[r]] += 2 for r < len(sampled) with slot[r] >= 0 and the token
    inside the vocabulary.  sampled int64 [rows]; capturable."""
    if table.is_cuda:
        _native().penalty_note(table, slot, sampled)
        return
    torch_ref.penalty_note(table, slot, sampled)


def guided_json_mask(logits: torch.Tensor, state: torch.Tensor) -> None:
    """JSON-mode grammar mask in place on logits [rows, vocab], from the
    per-row automaton state (csrc/guided.hip).

    state int32 [at least rows, torch_ref.GUIDED_WORDS], read on the device,
    so the launch depends on rows and vocab alone and can be captured.
    state[r, 0] < 0 = not a guided row, left untouched; in a guided row every
    token the state does not allow becomes -inf and the others keep their
    bits.  A vocabulary below the byte tokenizer's 260 ids is refused.
    torch_ref.guided_json_mask spells the semantics out.  bf16 GPU logits go
    to the kernel, anything else to the torch twin."""
    if logits.shape[-1] < torch_ref.GUIDED_BYTE_IDS:
        raise ValueError(
            f"guided_json_mask: the vocabulary must hold the "
            f"{torch_ref.GUIDED_BYTE_IDS} ids of the byte tokenizer, got "
            f"{logits.shape[-1]}")
    if logits.is_cuda and logits.dtype == torch.bfloat16:
        _native().guided_json_mask(logits, state)
        return
    torch_ref.guided_json_mask(logits, state)


def guided_json_advance(state: torch.Tensor, sampled: torch.Tensor) -> None:
    """Feed each guided row the token it has just sampled: state[r] :=
    state[r] after byte sampled[r] - 4, for r < len(sampled) with
    state[r, 0] >= 0 (csrc/guided.hip).  Tokens outside 4..259 are ignored.
    sampled int64 [rows]; capturable."""
    if state.is_cuda:
        _native().guided_json_advance(state, sampled)
        return
    torch_ref.guided_json_advance(state, sampled)


def decode_advance(input_ids: torch.Tensor, positions: torch.Tensor,
                   seq_lens: torch.Tensor, slot_mapping: torch.Tensor,
                   block_tables: torch.Tensor, sampled_prev: torch.Tensor,
                   ctl: torch.Tensor, page: int) -> None:
    """Derive one decode step's inputs on the device (csrc/decode_state.hip).

    In place on the per-row state (positions i64, seq_lens i32, block_tables
    i32 [rows, max_blocks]) and the forward's inputs (input_ids, slot_mapping
    i64).  ctl is int32 [4*rows + 4]: src_idx | new_blk | host_ids | host_pos
    | n_live — see the kernel's header for the row semantics."""
    if input_ids.is_cuda:
        _native().decode_advance(input_ids, positions, seq_lens, slot_mapping,
                                 block_tables, sampled_prev, ctl, page)
        return
    torch_ref.decode_advance(input_ids, positions, seq_lens, slot_mapping,
                             block_tables, sampled_prev, ctl, page)


def sample(logits: torch.Tensor, temperature: torch.Tensor,
           top_p: torch.Tensor, top_k: torch.Tensor,
           uniform: torch.Tensor) -> torch.Tensor:
    """Batch sampling. Greedy rows (temperature==0) take the argmax kernel;
    stochastic rows go through filtering + an inverse-CDF draw."""
    if not logits.is_cuda:
        return torch_ref.sample(logits, temperature, top_p, top_k, uniform)
    if bool((temperature == 0).all()):
        return greedy_sample(logits)
    # Stochastic path: torch does the (sort-based) top-k/top-p filtering,
    # the HIP kernel does temperature softmax + inverse-CDF in one pass.
    lf = logits.float()
    B, V = lf.shape
    t = temperature.clamp_min(1e-6)[:, None]
    row = lf / t
    if bool((top_k > 0).any()):
        k = top_k.clamp(0, V)
        kth = torch.where(
            k > 0,
            row.topk(int(k.max().clamp(min=1)), dim=-1).values.gather(
                1, (k.clamp(min=1) - 1)[:, None]).squeeze(1),
            torch.full_like(row[:, 0], float("-inf")))
        row = torch.where(row < kth[:, None], float("-inf"), row)
    if bool((top_p < 1.0).any()):
        sp, idx = row.softmax(-1).sort(descending=True)
        cum = sp.cumsum(-1)
        drop = (cum - sp) >= top_p[:, None]
        row = row.masked_fill(drop.gather(1, idx.argsort(-1)), float("-inf"))
    out = torch.empty(B, dtype=torch.long, device=logits.device)
    _native().inv_cdf_sample(out, row, uniform)
    greedy = temperature == 0
    if bool(greedy.any()):
        out = torch.where(greedy, greedy_sample(logits), out)
    return out

#!/usr/bin/env python3
"""Isolated kernel microbenchmarks (GPU only) — us/call + achieved GB/s.

Usage: python bench_kernels.py [--which attn|gemm|fp8|prefill_paged|sample|logprobs|penalties|all]
                               [--iters N]

Shapes mirror the flagship bench (Llama-3-8B bf16, bs=256 ctx=512 decode):
the numbers here are the per-kernel budget lines behind bench.py's step
time, compared against the HBM3E stream roofline (~8 TB/s).
"""

from __future__ import annotations

import argparse
import json

import torch


def timed(fn, iters, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters  # us/call


def bench_attn(iters):
    import hyperspot.ops as ops
    from hyperspot.ops import torch_ref
    torch.manual_seed(0)
    dev = "cuda:0"
    for (bs, ctx, kvh, group, D) in [(256, 512, 8, 4, 128),
                                     (256, 2048, 8, 4, 128),
                                     (64, 512, 8, 4, 128),
                                     (256, 512, 1, 8, 128),
                                     (64, 8192, 8, 4, 128),
                                     (16, 32768, 8, 4, 128)]:
        BS = 16
        nblk = (ctx + BS - 1) // BS
        tot_blocks = bs * nblk + 7
        k_cache = torch.randn(tot_blocks, kvh, BS, D, dtype=torch.bfloat16,
                              device=dev) * 0.3
        v_cache = torch.randn_like(k_cache) * 0.3
        q = torch.randn(bs, kvh * group, D, dtype=torch.bfloat16,
                        device=dev) * 0.5
        perm = torch.randperm(bs * nblk, device=dev, dtype=torch.int32)
        block_tables = perm.view(bs, nblk).contiguous()
        seq_lens = torch.full((bs,), ctx, dtype=torch.int32, device=dev)
        scale = D ** -0.5

        out = ops.paged_attn_decode(q, k_cache, v_cache, block_tables,
                                    seq_lens, scale)
        ref = torch_ref.paged_attn_decode(
            q.float().cpu(), k_cache.float().cpu(), v_cache.float().cpu(),
            block_tables.cpu(), seq_lens.cpu(), scale)
        err = (out.float().cpu() - ref).abs().max().item()
        us = timed(lambda: ops.paged_attn_decode(
            q, k_cache, v_cache, block_tables, seq_lens, scale), iters)
        kv_bytes = bs * ctx * kvh * D * 2 * 2
        roof_us = kv_bytes / 8e12 * 1e6
        print(json.dumps({
            "kernel": "paged_attn_decode",
            "shape": f"bs{bs}_ctx{ctx}_kvh{kvh}_g{group}_d{D}",
            "us": round(us, 1), "GBps": round(kv_bytes / us / 1e3, 0),
            "roofline_us": round(roof_us, 1),
            "x_roofline": round(us / roof_us, 2),
            "max_abs_err": round(err, 5)}), flush=True)


def bench_gemm(iters):
    dev = "cuda:0"
    for (m, k, n, tag) in [(256, 4096, 6144, "qkv"),
                           (256, 4096, 4096, "o"),
                           (256, 4096, 28672, "gate_up"),
                           (256, 14336, 4096, "down"),
                           (64, 4096, 6144, "qkv_bs64"),
                           (8192, 4096, 28672, "prefill_gate_up")]:
        x = torch.randn(m, k, dtype=torch.bfloat16, device=dev)
        w = torch.randn(n, k, dtype=torch.bfloat16, device=dev)
        us = timed(lambda: torch.nn.functional.linear(x, w), iters)
        bytes_ = (m * k + n * k + m * n) * 2
        flops = 2 * m * k * n
        print(json.dumps({
            "kernel": f"linear_{tag}", "shape": f"{m}x{k}x{n}",
            "us": round(us, 1),
            "GBps": round(bytes_ / us / 1e3, 0),
            "TFs": round(flops / us / 1e6, 0),
            "roofline_us": round(max(bytes_ / 8e12, flops / 2.5e15) * 1e6,
                                 1)}), flush=True)


def bench_fp8_gemm(iters):
    from hyperspot.parallel.layers import quant_fp8_rowwise, quantize_weight_fp8
    dev = "cuda:0"
    for (m, k, n, tag) in [(1024, 4096, 6144, "qkv"),
                           (1024, 4096, 28672, "gate_up"),
                           (1024, 14336, 4096, "down"),
                           (256, 4096, 28672, "gate_up_bs256")]:
        x = torch.randn(m, k, dtype=torch.bfloat16, device=dev)
        w = torch.randn(n, k, dtype=torch.bfloat16, device=dev) * 0.02
        wq, ws = quantize_weight_fp8(w)
        ws_row = ws[None, :].contiguous()
        us_bf16 = timed(lambda: torch.nn.functional.linear(x, w), iters)

        def fp8_full():
            xq, xs = quant_fp8_rowwise(x)
            return torch._scaled_mm(xq, wq.t(), scale_a=xs[:, None],
                                    scale_b=ws_row, out_dtype=torch.bfloat16)
        us_fp8 = timed(fp8_full, iters)
        xq, xs = quant_fp8_rowwise(x)
        xs_col = xs[:, None].contiguous()
        us_fp8_mm = timed(lambda: torch._scaled_mm(
            xq, wq.t(), scale_a=xs_col, scale_b=ws_row,
            out_dtype=torch.bfloat16), iters)
        print(json.dumps({
            "kernel": f"fp8_{tag}", "shape": f"{m}x{k}x{n}",
            "us_bf16": round(us_bf16, 1), "us_fp8_withquant": round(us_fp8, 1),
            "us_fp8_mm_only": round(us_fp8_mm, 1)}), flush=True)


def _paged_prefill_inputs(seqs, ctx, n, kvh, group, fp8, dev, gen_seed=0):
    """One step of `seqs` sequences, each `n` rows at positions ctx..ctx+n-1
    over a randomly paged cache that already holds positions 0..ctx+n-1."""
    D, BS = 128, 16
    torch.manual_seed(gen_seed)
    nblk = (ctx + n + BS - 1) // BS
    tot = seqs * nblk + 3
    kc = torch.randn(tot, kvh, BS, D, device=dev)
    vc = torch.randn(tot, kvh, BS, D, device=dev) * 0.5
    dt = torch.float8_e4m3fn if fp8 else torch.bfloat16
    kc, vc = kc.to(dt), vc.to(dt)
    q = (torch.randn(seqs * n, kvh * group, D, device=dev) * 0.5).bfloat16()
    bt = torch.randperm(seqs * nblk, device=dev, dtype=torch.int32) \
        .view(seqs, nblk).contiguous()
    seq_start = torch.arange(seqs + 1, dtype=torch.int32, device=dev) * n
    ctx_start = torch.full((seqs,), ctx, dtype=torch.int32, device=dev)
    pos = torch.arange(ctx, ctx + n, dtype=torch.int32, device=dev)
    ctx_lens = (pos + 1).repeat(seqs).contiguous()
    row_seq = torch.arange(seqs, dtype=torch.int32, device=dev) \
        .repeat_interleave(n).contiguous()
    return dict(q=q, kc=kc, vc=vc, bt=bt, seq_start=seq_start,
                ctx_start=ctx_start, ctx_lens=ctx_lens, row_seq=row_seq,
                n=n, scale=D ** -0.5)


def bench_prefill_paged(iters):
    """MFMA flash prefill over the paged cache vs the per-row paged kernel
    (unchanged code = the baseline it replaces on continuation steps), on
    identical tensors in one process.  Llama-3-8B heads (H=32, KV=8).

    Per shape: both kernels warmed, then REPS windows of each, alternating
    (new, per-row, new, ...) so clock drift and neighbours hit both; the
    window length adapts to ~WINDOW_S of device time (the per-row kernel
    spans 4 orders of magnitude over these shapes).  Prints the median and
    the min..max spread of the windows."""
    from hyperspot import _C
    from hyperspot.ops import torch_ref
    dev = "cuda:0"
    KVH, GROUP = 8, 4
    REPS, WINDOW_S = 3, 0.2

    def run_new(t, out):
        _C.attn_prefill_paged_mfma(out, t["q"], t["kc"], t["vc"], t["bt"],
                                   t["seq_start"], t["ctx_start"], t["n"],
                                   t["scale"])

    def run_row(t, out):
        _C.paged_attn(out, t["q"], t["kc"], t["vc"], t["bt"], t["ctx_lens"],
                      t["row_seq"], t["scale"], None, 1)

    # one correctness check per cache dtype against the fp32 reference
    for fp8 in (False, True):
        t = _paged_prefill_inputs(2, 200, 300, KVH, GROUP, fp8, dev)
        out = torch.empty_like(t["q"])
        run_new(t, out)
        ref = torch_ref.prefill_attn_paged(
            t["q"].float().cpu(), t["kc"].float().cpu(),
            t["vc"].float().cpu(), t["bt"].cpu(), t["ctx_lens"].cpu(),
            t["row_seq"].cpu(), t["scale"])
        err = (out.float().cpu() - ref).abs().max().item()
        print(json.dumps({"kernel": "attn_prefill_paged_mfma", "check":
                          "torch_ref", "kv": "fp8" if fp8 else "bf16",
                          "max_abs_err": round(err, 5)}), flush=True)
        assert err < 2.5e-2, err

    def window(fn, k):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(k):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / k  # us/call

    for fp8 in (False, True):
        for seqs in (1, 8):
            for ctx in (0, 2048, 8192):
                for n in (1, 16, 64, 256, 2048):
                    t = _paged_prefill_inputs(seqs, ctx, n, KVH, GROUP, fp8,
                                              dev)
                    o_new = torch.empty_like(t["q"])
                    o_row = torch.empty_like(t["q"])
                    fns = {"new": lambda: run_new(t, o_new),
                           "row": lambda: run_row(t, o_row)}
                    k = {}
                    for name, fn in fns.items():
                        window(fn, 3)                      # warm-up
                        est = window(fn, 3)
                        k[name] = int(min(max(WINDOW_S * 1e6 / est, 5),
                                          max(iters, 5) * 200))
                    diff = (o_new.float() - o_row.float()).abs().max().item()
                    us = {"new": [], "row": []}
                    for _ in range(REPS):
                        for name, fn in fns.items():
                            us[name].append(window(fn, k[name]))
                    med = {a: sorted(v)[len(v) // 2] for a, v in us.items()}
                    print(json.dumps({
                        "kernel": "prefill_paged",
                        "kv": "fp8" if fp8 else "bf16",
                        "shape": f"seqs{seqs}_ctx{ctx}_n{n}",
                        "us_mfma": round(med["new"], 1),
                        "us_per_row": round(med["row"], 1),
                        "per_row_over_mfma": round(med["row"] / med["new"],
                                                   2),
                        "spread_mfma": [round(min(us["new"]), 1),
                                        round(max(us["new"]), 1)],
                        "spread_per_row": [round(min(us["row"]), 1),
                                           round(max(us["row"]), 1)],
                        "iters": [k["new"], k["row"]],
                        "max_abs_diff": round(diff, 5)}), flush=True)
                    del t, o_new, o_row


def bench_sample(iters):
    """Sampling at the decode graph's tail: sample_fused (one kernel on the
    bf16 logits) against today's ops.sample (fp32 copy, topk, sort, cumsum,
    argsort, inv_cdf kernel, with its host syncs) and the greedy argmax.
    GB/s counts one read of the bf16 logits, whatever the op really moves."""
    import hyperspot.ops as ops
    dev = "cuda:0"
    vocab = 128256
    for rows in (2048, 64):
        g = torch.Generator().manual_seed(rows)
        logits = torch.empty(rows, vocab, dtype=torch.bfloat16, device=dev)
        for r0 in range(0, rows, 256):          # bounded host memory
            n = min(256, rows - r0)
            logits[r0:r0 + n] = (torch.randn(n, vocab, generator=g) * 3).to(
                torch.bfloat16).to(dev)
        u = torch.rand(rows, generator=g).to(dev)
        out = torch.empty(rows, dtype=torch.long, device=dev)
        nbytes = rows * vocab * 2

        def params(t, k, p):
            return (torch.full((rows,), t, dtype=torch.float32, device=dev),
                    torch.full((rows,), p, dtype=torch.float32, device=dev),
                    torch.full((rows,), k, dtype=torch.int32, device=dev))

        cases = [("greedy_sample", None),
                 ("sample_fused", (0.0, 0, 1.0)),
                 ("sample_fused", (0.8, 0, 1.0)),
                 ("sample_fused", (0.8, 40, 0.95)),
                 ("ops.sample", (0.8, 0, 1.0)),
                 ("ops.sample", (0.8, 40, 0.95))]
        for name, tkp in cases:
            if tkp is None:
                fn = lambda: ops.greedy_sample(logits, out=out)
            else:
                t, p, k = params(*tkp)
                if name == "sample_fused":
                    fn = lambda: ops.sample_fused(logits, t, p, k, u, out=out)
                else:
                    fn = lambda: ops.sample(logits, t, p, k, u)
            n_it = iters if name != "ops.sample" else max(iters // 10, 5)
            us = timed(fn, n_it, warmup=5)
            print(json.dumps({
                "kernel": name, "shape": f"{rows}x{vocab}",
                "t_k_p": tkp, "us": round(us, 1),
                "GBps_logits": round(nbytes / us / 1e3, 0)}), flush=True)
        del logits


def bench_logprobs(iters, repeats=5):
    """token_logprobs behind the sampler: every row asking for the chosen
    token only (n_top 0), 5 and 20 alternatives, and no row asking (-1,
    the launch floor), next to greedy_sample on the same logits, which
    reads the row once.  Each case is timed `repeats` times, the cases
    taking turns, and reported as the median with its range.  GB/s counts
    one read of the bf16 logits, whatever the kernel really moves."""
    import hyperspot.ops as ops
    dev = "cuda:0"
    vocab = 128256
    for rows in (64, 512, 2048):
        g = torch.Generator().manual_seed(rows)
        logits = torch.empty(rows, vocab, dtype=torch.bfloat16, device=dev)
        for r0 in range(0, rows, 256):          # bounded host memory
            n = min(256, rows - r0)
            logits[r0:r0 + n] = (torch.randn(n, vocab, generator=g) * 3).to(
                torch.bfloat16).to(dev)
        out = torch.empty(rows, dtype=torch.long, device=dev)
        ops.greedy_sample(logits, out=out)
        val = torch.empty(rows, 21, dtype=torch.float32, device=dev)
        idx = torch.empty(rows, 21, dtype=torch.int32, device=dev)
        nbytes = rows * vocab * 2

        def lp_case(n):
            n_top = torch.full((rows,), n, dtype=torch.int32, device=dev)
            return lambda: ops.token_logprobs(logits, out, n_top, val, idx)

        cases = [("greedy_sample", None,
                  lambda: ops.greedy_sample(logits, out=out))]
        cases += [("token_logprobs", n, lp_case(n)) for n in (-1, 0, 5, 20)]
        times = {i: [] for i in range(len(cases))}
        for rep in range(repeats):
            for i, (_, _, fn) in enumerate(cases):
                times[i].append(timed(fn, iters, warmup=20 if rep == 0 else 3))
        base = sorted(times[0])[repeats // 2]
        for i, (name, n, _) in enumerate(cases):
            t = sorted(times[i])
            us = t[repeats // 2]
            print(json.dumps({
                "kernel": name, "shape": f"{rows}x{vocab}", "n_top": n,
                "us": round(us, 1), "us_min": round(t[0], 1),
                "us_max": round(t[-1], 1),
                "x_greedy": round(us / base, 2),
                "GBps_logits": round(nbytes / us / 1e3, 0)}), flush=True)
        del logits


def bench_penalties(iters, repeats=5):
    """penalty_apply in place on [rows, 128256] bf16 logits: 256 penalty
    rows with ~1k tokens of history each, alone and among 2048 rows, and
    launches in which no row has a slot (what device_penalties adds to a
    decode graph without penalty rows), with penalty_note beside them.
    The floor counts what a penalty row must move, 2 bytes of logit and 4
    of state per token read plus 2 per seen token written, at the 6.29
    TB/s measured for a float4 copy on this GPU.  Each call penalises the
    logits the last one left, so seen logits end at -inf and are no longer
    written; the written share is under 1 % of the floor either way."""
    import hyperspot.ops as ops
    dev = "cuda:0"
    vocab, nslots, hist_len = 128256, 256, 1024
    g = torch.Generator().manual_seed(3)
    table = torch.zeros(nslots, vocab, dtype=torch.int32, device=dev)
    toks = torch.randint(0, vocab, (nslots * hist_len,), generator=g,
                         dtype=torch.int32).to(dev)
    off = (torch.arange(nslots + 1, dtype=torch.int32) * hist_len).to(dev)
    plen = torch.full((nslots,), hist_len // 2, dtype=torch.int32, device=dev)
    ops.penalty_build(table, torch.arange(nslots, dtype=torch.int32,
                                          device=dev), toks, off, plen)
    seen = int((table != 0).sum())
    for rows in (256, 2048):
        logits = torch.empty(rows, vocab, dtype=torch.bfloat16, device=dev)
        for r0 in range(0, rows, 256):
            n = min(256, rows - r0)
            logits[r0:r0 + n] = (torch.randn(n, vocab, generator=g) * 3).to(
                torch.bfloat16).to(dev)
        sampled = torch.randint(0, vocab, (rows,), generator=g).to(dev)
        rep = torch.full((rows,), 1.1, device=dev)
        pres = torch.full((rows,), 0.5, device=dev)
        freq = torch.full((rows,), 0.25, device=dev)
        none = torch.full((rows,), -1, dtype=torch.int32, device=dev)
        slot = none.clone()
        # the penalty rows spread over the batch, slots in shuffled order
        where = torch.arange(nslots) * (rows // nslots)
        slot[where] = torch.randperm(nslots, generator=g).to(
            torch.int32).to(dev)
        floor_us = (nslots * vocab * 6 + seen * 2) / 6.29e6
        cases = [
            ("penalty_apply", "no row", lambda: ops.penalty_apply(
                logits, none, rep, pres, freq, table)),
            ("penalty_apply", "256 rows", lambda: ops.penalty_apply(
                logits, slot, rep, pres, freq, table)),
            ("penalty_note", "no row", lambda: ops.penalty_note(
                table, none, sampled)),
            ("penalty_note", "256 rows", lambda: ops.penalty_note(
                table, slot, sampled)),
        ]
        times = {i: [] for i in range(len(cases))}
        for r in range(repeats):
            for i, (_, _, fn) in enumerate(cases):
                times[i].append(timed(fn, iters, warmup=20 if r == 0 else 3))
        for i, (name, what, _) in enumerate(cases):
            t = sorted(times[i])
            us = t[repeats // 2]
            rec = {"kernel": name, "shape": f"{rows}x{vocab}",
                   "penalty_rows": what, "us": round(us, 1),
                   "us_min": round(t[0], 1), "us_max": round(t[-1], 1)}
            if i == 1:
                # the 197 MB a call touches fit the 256 MB Infinity Cache,
                # and back-to-back calls find them there; in a decode step
                # 16 GB of weights have streamed past since the last call.
                # So also time single calls behind a 1 GiB fill.
                flush = torch.empty(1 << 28, dtype=torch.int32, device=dev)
                cold = []
                for k in range(21):
                    flush.fill_(k)
                    s = torch.cuda.Event(enable_timing=True)
                    e = torch.cuda.Event(enable_timing=True)
                    s.record()
                    cases[1][2]()
                    e.record()
                    torch.cuda.synchronize()
                    cold.append(s.elapsed_time(e) * 1e3)
                del flush
                cold = sorted(cold[1:])
                rec.update(floor_us=round(floor_us, 1),
                           x_floor=round(us / floor_us, 2),
                           cold_us=round(cold[len(cold) // 2], 1),
                           cold_us_min=round(cold[0], 1),
                           cold_us_max=round(cold[-1], 1),
                           x_floor_cold=round(
                               cold[len(cold) // 2] / floor_us, 2),
                           seen_tokens=seen)
            print(json.dumps(rec), flush=True)
        del logits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", default="attn")
    ap.add_argument("--iters", type=int, default=100)
    args = ap.parse_args()
    assert torch.cuda.is_available()
    if args.which in ("attn", "all"):
        bench_attn(args.iters)
    if args.which in ("gemm", "all"):
        bench_gemm(args.iters)
    if args.which in ("fp8", "all"):
        bench_fp8_gemm(args.iters)
    if args.which in ("prefill_paged", "all"):
        bench_prefill_paged(args.iters)
    if args.which in ("sample", "all"):
        bench_sample(args.iters)
    if args.which in ("logprobs", "all"):
        bench_logprobs(args.iters)
    if args.which in ("penalties", "all"):
        bench_penalties(args.iters)


if __name__ == "__main__":
    main()

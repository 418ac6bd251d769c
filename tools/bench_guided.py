#!/usr/bin/env python3
"""Engine-direct timings for JSON-mode rows (profiles/r11_device_guided.md).

  step    decode step time of llama3-8b at one batch size with 0, 1 and
          batch / 8 of the running rows in JSON mode, through
          step_pipelined(), with or without --device-guided.  Without the
          flag a batch with a JSON row takes the synchronous step and the
          host-built mask (the parent's behaviour, the baseline); with it
          the batch stays pipelined.  One engine serves the three row counts
          in turn, forwards and then backwards (the rows' response_format is
          switched in place and the device state re-seeded): contexts grow
          with every step, and the mean of a case's two windows cancels
          that.  Run the two flag values alternately, one process each, and
          compare.
  mask    ops.guided_json_mask alone on bf16 [rows, vocab] logits with every
          8th row guided: kernel time from device events over back-to-back
          launches, the bytes it stores and the store bandwidth.

Prints one JSON line.  Needs a GPU."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _sync(args):
    if args.device != "cpu":
        import torch
        torch.cuda.synchronize()


def _engine(args):
    import torch
    from hyperspot.engine import EngineConfig, LLMEngine, SamplingParams
    assert args.device == "cpu" or torch.cuda.is_available(), "needs a GPU"
    extra = 2 * 3 * (args.warmup + args.steps) + 64   # two rounds of three
    cfg = EngineConfig(
        model=args.model, max_num_seqs=args.batch,
        max_num_batched_tokens=max(8192, args.prompt_len),
        max_model_len=args.prompt_len + extra, seed=1234,
        graph_batch_sizes=(args.batch,), device_guided=args.device_guided)
    eng = LLMEngine(cfg, device=args.device, eos_token_id=2)
    g = torch.Generator().manual_seed(7)
    vocab = cfg.spec().vocab_size
    for i in range(args.batch):
        # ignore_eos: a JSON row whose document has closed goes on sampling
        # the one token its mask leaves, so the batch keeps its size
        sp = SamplingParams(temperature=0.0, max_tokens=10 ** 9,
                            ignore_eos=True)
        eng.add_request(torch.randint(4, vocab, (args.prompt_len,),
                                      generator=g).tolist(), sp,
                        request_id=f"r{i}")
    while eng.num_waiting > 0:
        eng.step()
    _sync(args)
    eng.capture_graphs()
    return eng


def run_step(args):
    from hyperspot.engine.guided import JsonByteMachine
    eng = _engine(args)
    reqs = list(eng.scheduler.running)
    out = {"mode": "step", "device_guided": args.device_guided,
           "batch": args.batch, "model": args.model}
    cases = (0, 1, max(args.batch // 8, 1))
    # every step lengthens every context, so a later window is slower
    # whatever it holds: the second round runs the cases in reverse order,
    # and a case's two windows lie symmetrically around the middle of the run
    for order in (cases, cases[::-1]):
        for n_json in order:
            eng.drain()
            stride = len(reqs) // n_json if n_json else 0
            chosen = set(range(0, stride * n_json, stride)) if n_json \
                else set()
            for i, r in enumerate(reqs):
                r.sampling.response_format = "json" if i in chosen else None
                # a fresh document that starts behind the tokens so far
                r._guided = JsonByteMachine()
                r._guided.consumed = len(r.output_token_ids)
            eng.runner.pipe_invalidate()
            for _ in range(args.warmup):
                eng.step_pipelined()
            eng.drain()
            _sync(args)
            piped = 0
            t0 = time.monotonic()
            for _ in range(args.steps):
                eng.step_pipelined()
                piped += eng._inflight is not None
            eng.drain()
            _sync(args)
            ms = (time.monotonic() - t0) / args.steps * 1000
            out.setdefault(f"ms_per_step_json{n_json}", []).append(
                round(ms, 3))
            out[f"pipelined_json{n_json}"] = piped == args.steps
    for n_json in cases:
        ms = out[f"ms_per_step_json{n_json}"]
        out[f"ms_mean_json{n_json}"] = round(sum(ms) / len(ms), 3)
    print(json.dumps(out), flush=True)


def run_mask(args):
    import torch
    from hyperspot import ops
    from hyperspot.engine.guided import JsonByteMachine
    from hyperspot.ops import torch_ref
    assert torch.cuda.is_available(), "needs a GPU"
    rows, vocab = args.batch, args.vocab
    m = JsonByteMachine()
    for b in b'{"k":[1,':
        m.feed(b)
    st = torch.full((rows, torch_ref.GUIDED_WORDS), -1, dtype=torch.int32)
    st[::args.every] = torch.tensor(m.pack(), dtype=torch.int32)
    guided = int((st[:, 0] >= 0).sum())
    st = st.cuda()
    lg = torch.randn(rows, vocab, device="cuda").to(torch.bfloat16)
    allowed = len(m.allowed()[0])
    # the kernel only stores: every logit of a guided row but the allowed
    stored = guided * (vocab - allowed) * 2
    for _ in range(args.warmup):
        ops.guided_json_mask(lg, st)
    torch.cuda.synchronize()
    samples = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), \
            torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            ops.guided_json_mask(lg, st)
        e1.record()
        torch.cuda.synchronize()
        samples.append(e0.elapsed_time(e1) / args.steps * 1000)   # us
    none = torch.full_like(st, -1)
    e0, e1 = torch.cuda.Event(enable_timing=True), \
        torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        ops.guided_json_mask(lg, none)
    e1.record()
    torch.cuda.synchronize()
    us = sorted(samples)[len(samples) // 2]
    print(json.dumps({
        "mode": "mask", "rows": rows, "vocab": vocab, "guided_rows": guided,
        "us_per_launch": round(us, 2),
        "us_range": [round(min(samples), 2), round(max(samples), 2)],
        "us_no_guided_row": round(e0.elapsed_time(e1) / args.steps * 1000, 2),
        "bytes_stored": stored,
        "store_TBps": round(stored / us / 1e6, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["step", "mask"])
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--device-guided", action="store_true")
    ap.add_argument("--device", default="cuda:0",
                    help="cpu only rehearses the script: its times mean "
                         "nothing")
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--every", type=int, default=8,
                    help="mask mode: every n-th row is guided")
    args = ap.parse_args()
    (run_step if args.mode == "step" else run_mask)(args)


if __name__ == "__main__":
    main()

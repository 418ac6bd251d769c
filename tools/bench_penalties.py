#!/usr/bin/env python3
"""Engine-direct timings for the penalty path (profiles/r09_penalties.md).

  step    decode step time at the flagship shape (bench.py --engine-direct:
          llama3-8b, 2048 greedy streams of 512 prompt tokens, no penalty
          row), with or without --device-penalties.  Run the two
          alternately, one process each, and compare.
  reseed  time of ModelRunner._pipe_seed over the running rows with 256
          penalty rows of ~1k tokens of history, and over the same rows
          with their penalties set to neutral.

Prints one JSON line.  Needs a GPU."""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _sync(args):
    if args.device != "cpu":
        import torch
        torch.cuda.synchronize()


def _engine(args, prompt_len, extra_len, device_penalties):
    import torch
    from hyperspot.engine import EngineConfig, LLMEngine, SamplingParams
    assert args.device == "cpu" or torch.cuda.is_available(), "needs a GPU"
    cfg = EngineConfig(
        model=args.model, max_num_seqs=args.batch,
        max_num_batched_tokens=max(8192, prompt_len),
        max_model_len=prompt_len + extra_len + 64, seed=1234,
        device_penalties=device_penalties)
    eng = LLMEngine(cfg, device=args.device)
    g = torch.Generator().manual_seed(7)
    vocab = cfg.spec().vocab_size
    for i in range(args.batch):
        sp = SamplingParams(temperature=0.0, max_tokens=10 ** 9)
        eng.add_request(torch.randint(0, vocab, (prompt_len,),
                                      generator=g).tolist(), sp,
                        request_id=f"r{i}")
    while eng.num_waiting > 0:
        eng.step()
    _sync(args)
    eng.capture_graphs()
    return eng


def run_step(args):
    eng = _engine(args, args.prompt_len, 3 * (args.warmup + args.steps),
                  args.device_penalties)
    out = {"mode": "step", "device_penalties": args.device_penalties,
           "batch": args.batch}
    for name, step in (("step", eng.step),
                       ("step_pipelined", eng.step_pipelined)):
        for _ in range(args.warmup):
            step()
        eng.drain()
        _sync(args)
        t0 = time.monotonic()
        for _ in range(args.steps):
            step()
        eng.drain()
        _sync(args)
        out[f"ms_per_{name}"] = round(
            (time.monotonic() - t0) / args.steps * 1000, 3)
    print(json.dumps(out), flush=True)


def run_reseed(args):
    import torch
    eng = _engine(args, args.history, 64, True)
    rn = eng.runner
    reqs = list(eng.scheduler.running)
    pen = reqs[::max(1, len(reqs) // args.penalty_rows)][:args.penalty_rows]

    def timed(n=9):
        ts = []
        for _ in range(n):
            _sync(args)
            t0 = time.monotonic()
            with torch.inference_mode():     # as pipe_launch calls it
                rn._pipe_seed(reqs)
            _sync(args)
            ts.append((time.monotonic() - t0) * 1000)
        rn.pipe_invalidate()
        return ts

    res = {}
    for rnd in range(2):                       # the two cases take turns
        for name, f in (("with", 0.5), ("without", 0.0)):
            for r in pen:
                r.sampling.frequency_penalty = f
            res.setdefault(name, []).extend(timed()[1:])
    print(json.dumps({
        "mode": "reseed", "batch": len(reqs), "penalty_rows": len(pen),
        "history": args.history,
        "ms_with": round(statistics.median(res["with"]), 3),
        "ms_with_range": [round(min(res["with"]), 3),
                          round(max(res["with"]), 3)],
        "ms_without": round(statistics.median(res["without"]), 3),
        "ms_without_range": [round(min(res["without"]), 3),
                             round(max(res["without"]), 3)]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["step", "reseed"])
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--prompt-len", type=int, default=512)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--device-penalties", action="store_true")
    ap.add_argument("--device", default="cuda:0",
                    help="cpu only rehearses the script: its times mean "
                         "nothing")
    ap.add_argument("--penalty-rows", type=int, default=256)
    ap.add_argument("--history", type=int, default=1024)
    args = ap.parse_args()
    (run_step if args.mode == "step" else run_reseed)(args)


if __name__ == "__main__":
    main()

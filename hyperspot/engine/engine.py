"""LLMEngine — the in-node inference engine facade.

This is what the reference's spec-only llm-gateway calls "the provider":
requests come from the C++ host plane (or directly in tests/bench), the
scheduler places them into the paged KV pool, and step() advances every
running sequence by one token.
"""

from __future__ import annotations

import itertools
import logging
import time
from typing import List, Optional

from .config import EngineConfig, SamplingParams
from .model_runner import ModelRunner
from .request import FinishReason, Request, StepOutput
from .scheduler import Scheduler

log = logging.getLogger(__name__)


class LLMEngine:
    def __init__(self, config: EngineConfig, device: Optional[str] = None,
                 eos_token_id: Optional[int] = None):
        t0 = time.monotonic()
        self.config = config
        self.runner = ModelRunner(config, device=device)
        self.scheduler = Scheduler(config, self.runner.block_manager)
        self.eos_token_id = eos_token_id
        self._id_counter = itertools.count()
        self._inflight = None           # enqueued, uncollected PipeStep
        log.info("engine up: model=%s blocks=%d device=%s (%.1fs)",
                 config.model, self.runner.num_blocks, self.runner.device,
                 time.monotonic() - t0)

    def add_request(self, prompt_token_ids: List[int],
                    sampling: Optional[SamplingParams] = None,
                    request_id: Optional[str] = None,
                    tenant_id: str = "default") -> str:
        rid = request_id or f"req-{next(self._id_counter)}"
        lp = sampling.logprobs if sampling is not None else None
        if lp is not None and not (isinstance(lp, int) and 0 <= lp <= 20):
            raise ValueError(
                f"SamplingParams.logprobs must be None or 0..20, got {lp!r}")
        if sampling is not None:
            sampling.check_penalties()
        req = Request(request_id=rid,
                      prompt_token_ids=list(prompt_token_ids),
                      sampling=sampling or SamplingParams(),
                      tenant_id=tenant_id)
        self.scheduler.add(req)
        return rid

    def abort_request(self, request_id: str) -> None:
        h = self._inflight
        if h is not None and h.runs(request_id):
            # the enqueued step may still write this row's pages: they go
            # back to the pool when that step has been collected
            self.scheduler.abort(request_id, free=False)
            h.deferred_free.append(request_id)
        else:
            self.scheduler.abort(request_id)
        self.runner.pipe_drop(request_id)

    def has_work(self) -> bool:
        return self.scheduler.has_work() or self._inflight is not None

    @property
    def num_running(self) -> int:
        return len(self.scheduler.running)

    @property
    def num_waiting(self) -> int:
        return len(self.scheduler.waiting)

    def step(self) -> List[StepOutput]:
        """Run one step synchronously and return its outputs (after those
        of a pipelined step still in flight, if there is one)."""
        outputs: List[StepOutput] = self.drain()
        batch = self.scheduler.schedule()
        if batch.empty:
            return outputs
        tokens = self.runner.execute(batch)
        # the synchronous path fills the decode inputs from the host; the
        # next pipelined step re-seeds the device state
        self.runner.pipe_invalidate()
        bm = self.runner.block_manager
        lps = self.runner.last_logprobs
        for i, (req, tok) in enumerate(zip(batch.requests, tokens.tolist())):
            if batch.mode == "prefill" and bm.enable_prefix_caching:
                # the chunk's full prompt blocks are now computed and
                # shareable with later prompts
                bm.commit_hashes(req.request_id, req.num_computed_tokens)
            if batch.mode == "prefill" and \
                    req.num_computed_tokens < req.num_prompt_tokens:
                continue     # mid-prompt chunk: no token is sampled yet
            req.append_output(int(tok), self.eos_token_id)
            outputs.append(StepOutput(req.request_id, int(tok), req.finished,
                                      req.finish_reason,
                                      lps[i] if lps is not None else None))
        self.scheduler.finish_step()
        return outputs

    # ---- pipelined stepping (depth one) ----

    def _pipe_eligible(self) -> bool:
        """Every running row unguided unless it is in plain JSON mode and
        the decode graphs run that grammar (EngineConfig.device_guided;
        schema and tool-call rows never, nor a machine nested deeper than
        the device state holds), greedy unless the device samples
        (EngineConfig.device_sampling), without logprobs unless the
        decode graphs compute them (EngineConfig.device_logprobs), and
        without penalties unless the graphs apply them and keep the counts
        (EngineConfig.device_penalties; at most max_penalty_seqs such
        rows): the next decode step's inputs then depend on the in-flight
        tokens only through input_ids, those counts and the grammar state,
        which the device already holds."""
        stochastic_ok = self.config.device_sampling
        logprobs_ok = self.config.device_logprobs
        penalties_ok = self.config.device_penalties
        guided_ok = self.config.device_guided
        npen = 0
        for r in self.scheduler.running:
            sp = r.sampling
            if (sp.temperature != 0 and not stochastic_ok) \
                    or (sp.logprobs is not None and not logprobs_ok) \
                    or sp.response_schema is not None \
                    or sp.response_format == "tool_call":
                return False
            if sp.response_format == "json" and not (
                    guided_ok and self.runner.guided_fits_device(r)):
                return False
            if sp.penalized:
                npen += 1
                if not penalties_ok or npen > self.config.max_penalty_seqs:
                    return False
        return True

    def step_pipelined(self) -> List[StepOutput]:
        """Enqueue decode step n+1, then wait for and return the outputs
        of step n ([] while the pipeline fills).  Whatever the fast path
        does not cover (a prefill, a stochastic or guided row without its
        device flag, preemption, tensor parallelism) first drains, then
        takes step().  A row that
        reaches max_tokens in the in-flight step is left out of the next
        one; EOS / stop tokens are seen one step late, and the token of
        that extra step is dropped, so streams and finish reasons are
        those of step().

        With device_sampling stochastic rows take the fast path too: the
        graph's tail is sample_fused, fed one uniform per launched row.  A
        row with `seed` draws from its own generator once per sampled
        token in either path, so it gets the same tokens and finish reason
        as from step() (the extra draw of a step launched past its EOS
        comes after its last token).  Rows without a seed share one
        generator, which that extra draw, and the order of draws, shift:
        for them only the distribution is that of step()."""
        cfg = self.config
        sch = self.scheduler
        rn = self.runner
        fast = (cfg.pipeline_decode and cfg.tp_size == 1
                and not sch.waiting and bool(sch.running))
        seed = None
        if fast and (not rn.pipe_valid() or rn.pipe_stale()):
            if self._inflight is not None:
                return self.drain()
            fast = self._pipe_eligible()
            seed = sch.running
        if fast:
            h = rn.pipe_launch(seed)
            if h is not None:
                prev, self._inflight = self._inflight, h
                return self._collect(prev) if prev is not None else []
        if self._inflight is not None:
            return self.drain()
        return self.step()

    def drain(self) -> List[StepOutput]:
        """Outputs of the step in flight, if any; the pipeline is empty
        afterwards."""
        h, self._inflight = self._inflight, None
        return self._collect(h) if h is not None else []

    def _collect(self, h) -> List[StepOutput]:
        outputs: List[StepOutput] = []
        done = []
        eos = self.eos_token_id
        pairs = self.runner.pipe_collect(h)
        lps = h.records
        for i, (req, tok) in enumerate(pairs):
            if req.finished:
                # stopped one step earlier, or aborted: dropped, with its
                # logprob record
                continue
            req.append_output(tok, eos)
            outputs.append(StepOutput(req.request_id, tok, req.finished,
                                      req.finish_reason,
                                      lps[i] if lps is not None else None))
            if req.finished:
                done.append(req)
        bm = self.runner.block_manager
        if done:
            nxt = self._inflight
            for r in done:
                self.runner.pipe_drop(r.request_id)
                if nxt is not None and nxt.runs(r.request_id):
                    nxt.deferred_free.append(r.request_id)
                else:
                    bm.free(r.request_id)
            self.scheduler.running = [r for r in self.scheduler.running
                                      if not r.finished]
        for rid in h.deferred_free:
            bm.free(rid)
        return outputs

    def capture_graphs(self) -> None:
        self.runner.capture_all_graphs()

    def embed(self, prompts):
        """Mean-pooled embeddings; caller must not be mid-step."""
        return self.runner.embed(prompts)

    def swap_weights(self, checkpoint_path: str) -> float:
        """Live weight hot-swap (same architecture); KV pool and captured
        decode graphs survive (in-place parameter copy)."""
        return self.runner.swap_weights(checkpoint_path)

    def save_checkpoint(self, path: str) -> None:
        from .checkpoint import save_checkpoint
        save_checkpoint(self.runner.model, path,
                        {"model": self.config.model})

    def generate(self, prompts: List[List[int]],
                 sampling: Optional[SamplingParams] = None):
        """Synchronous batch generation helper (tests / offline)."""
        ids = [self.add_request(p, sampling) for p in prompts]
        results = {i: [] for i in ids}
        while self.has_work():
            for out in self.step():
                if out.request_id in results:
                    results[out.request_id].append(out.token_id)
        return [results[i] for i in ids]

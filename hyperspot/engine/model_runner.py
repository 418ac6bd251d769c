"""ModelRunner: device-side execution of scheduled batches.

Decode steps are captured into hipGraphs per batch-size bucket (torch's CUDA
graph API is hipGraph on ROCm).  The capture includes the whole transformer
forward — custom CDNA4 kernels, hipBLASLt GEMMs and (at TP>1) the RCCL
all-reduces — so steady-state decode replays with one graph launch instead
of ~1k kernel launches (MI355X boundary cost ≈1.2-1.9 us each, see
/opt/skills/guides/MI355X_MICROARCH.md 'boundary').
"""

from __future__ import annotations

import logging
from typing import Dict, List, Optional

import torch

from hyperspot import ops
from hyperspot.models import build_model
from hyperspot.models.llama import ForwardMeta

from .config import EngineConfig
from .kv_cache import (BlockManager, allocate_kv_caches,
                       compute_num_gpu_blocks)
from .request import Request, TokenLogprobs
from .scheduler import ScheduledBatch

log = logging.getLogger(__name__)

_TUNABLEOP_LOADED = False


def _load_tunableop_results() -> None:
    """Load committed hipBLASLt algo selections (profiles/tunableop_gfx950.csv).

    The default hipBLASLt heuristic picks ~1.5-3x-off-roofline kernels for
    the skinny decode GEMMs (M=64..256); offline tuning (tools/tune_gemms.py
    on an MI355X) selects per-shape algorithms which TunableOp then replays.
    No tuning happens at serve time — results are read-only.
    """
    global _TUNABLEOP_LOADED
    if _TUNABLEOP_LOADED:
        return
    _TUNABLEOP_LOADED = True
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(
        os.path.dirname(os.path.abspath(__file__)))),
        "profiles", "tunableop_gfx950.csv")
    if not os.path.exists(path):
        return
    try:
        t = torch.cuda.tunable
        t.enable(True)
        t.tuning_enable(False)   # replay only; never tune in the hot path
        t.record_untuned_enable(False)
        t.read_file(path)
        log.info("TunableOp: loaded %s", path)
    except Exception as e:  # pragma: no cover
        log.warning("TunableOp load failed: %s", e)


def _logprob_records(val, idx, n_top) -> List[Optional[TokenLogprobs]]:
    """Host records from ops.token_logprobs' outputs (numpy [rows, 21]);
    n_top[i] < 0 = row i did not ask."""
    ninf = float("-inf")
    out: List[Optional[TokenLogprobs]] = []
    for i, n in enumerate(n_top):
        if n < 0:
            out.append(None)
            continue
        ids = idx[i, 1:1 + n].tolist()
        vals = val[i, 1:1 + n].tolist()
        out.append(TokenLogprobs(
            int(idx[i, 0]), float(val[i, 0]),
            [(t, v) for t, v in zip(ids, vals) if v > ninf]))
    return out


class PipeStep:
    """One enqueued pipelined decode step: the rows it runs (slot order),
    the staging slot its tokens land in, and the sequences whose pages may
    only be freed once it has been collected.  lp_n: logprobs asked per
    launched row (None = the step copied no logprob records back);
    records: what pipe_collect made of them."""

    __slots__ = ("reqs", "slots", "ring", "deferred_free", "_rids", "lp_n",
                 "records")

    def __init__(self, reqs, slots, ring):
        self.reqs = reqs
        self.slots = slots
        self.ring = ring
        self.deferred_free: List[str] = []
        self._rids = None
        self.lp_n = None
        self.records = None

    def runs(self, request_id: str) -> bool:
        if self._rids is None:
            self._rids = {r.request_id for r in self.reqs}
        return request_id in self._rids


class ModelRunner:
    def __init__(self, config: EngineConfig, device: Optional[str] = None):
        self.config = config
        self.spec = config.spec()
        if config.max_model_len > self.spec.max_position:
            # the rope table is sized for max_position; admitting longer
            # prompts crashed the stepping thread with an index OOB
            log.warning("max_model_len %d clamped to the model's "
                        "max_position %d", config.max_model_len,
                        self.spec.max_position)
            config.max_model_len = self.spec.max_position
        self.device = torch.device(
            device if device is not None
            else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.dtype = torch.bfloat16 if self.device.type == "cuda" \
            else torch.float32
        torch.manual_seed(config.seed)
        if self.device.type == "cuda":
            _load_tunableop_results()
        from hyperspot.parallel.layers import set_init_device, set_quant_mode
        set_init_device(self.device)
        set_quant_mode(config.quant)
        self.model = build_model(self.spec, dtype=self.dtype).to(self.device)
        self.model.eval()
        self.num_blocks = compute_num_gpu_blocks(self.spec, config, self.device)
        kv_heads_local = self.spec.num_kv_heads // max(config.tp_size, 1)
        assert config.kv_dtype in ("bfloat16", "fp8"), config.kv_dtype
        kv_dt = torch.float8_e4m3fn if config.kv_dtype == "fp8"             else self.dtype
        self.kv_caches = allocate_kv_caches(
            self.spec.num_layers, self.num_blocks, kv_heads_local,
            config.block_size, self.spec.head_dim, kv_dt, self.device)
        self.max_blocks_per_seq = (config.max_model_len + config.block_size - 1) \
            // config.block_size
        self.block_manager = BlockManager(
            self.num_blocks, config.block_size,
            capacity=max(config.max_num_seqs * 2, 64),
            max_blocks_per_seq=self.max_blocks_per_seq,
            enable_prefix_caching=config.enable_prefix_caching)
        self._gen = torch.Generator().manual_seed(config.seed)
        # pinned staging for the decode hot path (vectorized input prep)
        pin = self.device.type == "cuda"
        cap = self.block_manager.capacity
        self._st_ids = torch.empty(cap, dtype=torch.long, pin_memory=pin)
        self._st_pos = torch.empty(cap, dtype=torch.long, pin_memory=pin)
        self._st_slots = torch.empty(cap, dtype=torch.long, pin_memory=pin)
        self._st_lens = torch.empty(cap, dtype=torch.int32, pin_memory=pin)
        self._st_bt_flat = torch.empty(cap * self.max_blocks_per_seq,
                                       dtype=torch.int32, pin_memory=pin)
        # guided-decoding logit-mask rows keyed by machine state
        self._guided_mask_cache: Dict[tuple, torch.Tensor] = {}
        self._graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self._graph_io: Dict[int, dict] = {}
        self._pgraphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self._pgraph_io: Dict[int, dict] = {}
        self._graph_pool = None
        # pipelined decode: device state of the current bucket (None = the
        # next pipelined step re-seeds it from the host), io tensors of the
        # eager twin, and a ring of pinned staging slots.  A slot is read
        # (ctl H2D) and written (token D2H) when the copy EXECUTES; with a
        # depth-one pipeline at most two steps are uncollected, so four
        # slots keep the host off anything a queued copy still touches.
        self._pipe: Optional[dict] = None
        self._pipe_eager_io: Optional[dict] = None
        self._pipe_seq = 0
        # With device_sampling a slot's control block is followed by one
        # float32 uniform per row, so both go up in a single copy.
        ctl_len = (5 if config.device_sampling else 4) * cap + 4
        self._pipe_ring = [
            {"ctl": torch.empty(ctl_len, dtype=torch.int32, pin_memory=pin),
             "tok": torch.empty(cap, dtype=torch.long, pin_memory=pin),
             "event": torch.cuda.Event() if pin else None}
            for _ in range(4)]
        if config.device_logprobs:
            cols = ops.torch_ref.LOGPROB_COLS
            for slot in self._pipe_ring:
                slot["lp_val"] = torch.empty(cap, cols, dtype=torch.float32,
                                             pin_memory=pin)
                slot["lp_id"] = torch.empty(cap, cols, dtype=torch.int32,
                                            pin_memory=pin)
        # penalty count table int32 [max_penalty_seqs, vocab] (csrc/
        # penalties.hip).  With device_penalties it is part of the decode
        # graphs and allocated here, behind the KV pool; without, the first
        # step that has a penalty row allocates it
        self._pen_table: Optional[torch.Tensor] = None
        if config.device_penalties:
            self._penalty_table()
        # logprob records of the last execute(), one per batch row (None =
        # the row did not ask), or None when no row asked
        self.last_logprobs: Optional[List[Optional[TokenLogprobs]]] = None

    # ---------------- input preparation ----------------

    def _prefill_inputs(self, batch: ScheduledBatch):
        ids: List[int] = []
        pos: List[int] = []
        slots: List[int] = []
        starts = [0]
        logit_rows = []
        import numpy as np
        row_seq: List[int] = []
        tables = []
        bm = self.block_manager
        bs = bm.block_size
        fresh = True
        ctx_start: List[int] = []
        for si, req in enumerate(batch.requests):
            cs = req.chunk_start
            n = req.chunk_len or req.num_prompt_tokens
            ctx_start.append(cs)
            if cs > 0:
                fresh = False      # continuation chunk attends over cache
            ids.extend(req.prompt_token_ids[cs:cs + n])
            pos.extend(range(cs, cs + n))
            row = bm.row_of[req.request_id]
            p = np.arange(cs, cs + n)
            s = bm.tables_np[row, p // bs].astype(np.int64) * bs + p % bs
            slots.extend(s.tolist())
            starts.append(starts[-1] + n)
            logit_rows.append(starts[-1] - 1)
            row_seq.extend([si] * n)
            tables.append(bm.table(req.request_id))
        max_t = max(len(t) for t in tables)
        bt = torch.zeros(len(tables), max_t, dtype=torch.int32)
        for i, t in enumerate(tables):
            bt[i, :len(t)] = torch.tensor(t, dtype=torch.int32)
        d = self.device
        positions = torch.tensor(pos, dtype=torch.long, device=d)
        meta = ForwardMeta(
            mode="prefill",
            positions=positions,
            slot_mapping=torch.tensor(slots, dtype=torch.long, device=d),
            seq_start=torch.tensor(starts, dtype=torch.int32, device=d),
            max_seqlen=max((r.chunk_len or r.num_prompt_tokens)
                           for r in batch.requests),
            fresh_prefill=fresh,
            ctx_start=torch.tensor(ctx_start, dtype=torch.int32, device=d),
            paged_mfma=self.config.prefill_paged_mfma,
            row_seq=torch.tensor(row_seq, dtype=torch.int32, device=d),
            ctx_lens=(positions + 1).to(torch.int32),
            block_tables=bt.to(d),
            logits_indices=torch.tensor(logit_rows, dtype=torch.long, device=d),
        )
        input_ids = torch.tensor(ids, dtype=torch.long, device=d)
        return input_ids, meta

    def _decode_inputs(self, batch: ScheduledBatch):
        """Vectorized decode-step prep: numpy state + pinned staging (the
        per-sequence Python loop cost more than the GPU step at batch 256)."""
        import numpy as np
        bm = self.block_manager
        reqs = batch.requests
        B = len(reqs)
        rows = np.fromiter((bm.row_of[r.request_id] for r in reqs),
                           dtype=np.int64, count=B)
        ids = np.fromiter((r.last_token_id for r in reqs),
                          dtype=np.int64, count=B)
        pos = bm.tokens_np[rows].copy()             # next position index
        slots = bm.append_slots_batch(rows)
        max_nt = int(bm.ntables_np[rows].max())
        bt = bm.tables_np[rows[:, None], np.arange(max_nt)[None, :]]
        self._st_ids.numpy()[:B] = ids
        self._st_pos.numpy()[:B] = pos
        self._st_slots.numpy()[:B] = slots
        self._st_lens.numpy()[:B] = pos + 1
        bt_stage = self._st_bt_flat[:B * max_nt].view(B, max_nt)
        bt_stage.numpy()[:] = bt
        d = self.device
        nb = d.type == "cuda"
        meta = ForwardMeta(
            mode="decode",
            positions=self._st_pos[:B].to(d, non_blocking=nb),
            slot_mapping=self._st_slots[:B].to(d, non_blocking=nb),
            block_tables=bt_stage.to(d, non_blocking=nb),
            seq_lens=self._st_lens[:B].to(d, non_blocking=nb),
        )
        input_ids = self._st_ids[:B].to(d, non_blocking=nb)
        return input_ids, meta

    # ---------------- execution ----------------

    @torch.inference_mode()
    def execute(self, batch: ScheduledBatch) -> torch.Tensor:
        """Run one step; returns sampled token ids [num_seqs] (cpu)."""
        if batch.mode == "prefill":
            logits = self._prefill_graph_forward(batch)
            if logits is None:
                input_ids, meta = self._prefill_inputs(batch)
                logits = self.model(input_ids, meta, self.kv_caches)
        else:
            input_ids, meta = self._decode_inputs(batch)
            logits = self._decode_forward(input_ids, meta)
        return self._sample(logits, batch.requests)

    # ---- TTFT fast path: single-request whole-prompt prefill graphs ----

    def _prefill_bucket(self, n: int) -> Optional[int]:
        for s in self.config.prefill_graph_sizes:
            if s >= n and s <= self.config.max_num_batched_tokens:
                return s
        return None

    def _prefill_graph_forward(self, batch: ScheduledBatch):
        """Replay a padded single-sequence prefill graph (eager prefill
        costs ~350 kernel launches + the Python layer loop — several ms
        of the TTFT).  Pad tokens sit AFTER the real prompt, so causal
        attention keeps real rows exact; padded slots are -1 (no KV
        write) and the single logit row indexes the real last token."""
        if (self.device.type != "cuda" or self.config.enforce_eager
                or len(batch.requests) != 1):
            return None
        req = batch.requests[0]
        n = req.chunk_len or req.num_prompt_tokens
        if req.chunk_start != 0 or n != req.num_prompt_tokens:
            return None              # chunked / continued prompt
        T = self._prefill_bucket(n)
        if T is None:
            return None
        if T not in self._pgraphs:
            self._capture_prefill(T)
        import numpy as np
        bm = self.block_manager
        row = bm.row_of[req.request_id]
        p = np.arange(n)
        slots = bm.tables_np[row, p // bm.block_size].astype(np.int64)             * bm.block_size + p % bm.block_size
        io = self._pgraph_io[T]
        d = self.device
        io["input_ids"][:n] = torch.tensor(req.prompt_token_ids[:n],
                                           dtype=torch.long, device=d)
        io["input_ids"][n:] = 0
        io["positions"][:n] = torch.arange(n, dtype=torch.long, device=d)
        io["positions"][n:] = 0
        io["slot_mapping"][:n] = torch.from_numpy(slots).to(d)
        io["slot_mapping"][n:] = -1
        io["lidx"][0] = n - 1
        self._pgraphs[T].replay()
        return io["logits"]

    def _capture_prefill(self, T: int) -> None:
        d = self.device
        log.info("capturing prefill hipGraph for tokens=%d", T)
        io = {
            "input_ids": torch.zeros(T, dtype=torch.long, device=d),
            "positions": torch.zeros(T, dtype=torch.long, device=d),
            "slot_mapping": torch.full((T,), -1, dtype=torch.long,
                                       device=d),
            "lidx": torch.zeros(1, dtype=torch.long, device=d),
        }
        meta = ForwardMeta(
            mode="prefill", positions=io["positions"],
            slot_mapping=io["slot_mapping"],
            seq_start=torch.tensor([0, T], dtype=torch.int32, device=d),
            max_seqlen=T, fresh_prefill=True,
            logits_indices=io["lidx"])
        for _ in range(2):
            self.model(io["input_ids"], meta, self.kv_caches)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=self._graph_pool):
            io["logits"] = self.model(io["input_ids"], meta,
                                      self.kv_caches)
        if self._graph_pool is None:
            self._graph_pool = g.pool()
        self._pgraphs[T] = g
        self._pgraph_io[T] = io

    def _decode_forward(self, input_ids, meta):
        B = input_ids.shape[0]
        bucket = self._bucket_for(B)
        if bucket is None or self.device.type != "cuda" \
                or self.config.enforce_eager:
            return self.model(input_ids, meta, self.kv_caches)
        if bucket not in self._graphs:
            self._capture(bucket)
        io = self._graph_io[bucket]
        if not io["passthrough"]:
            # the graph's head kernel leaves host-filled inputs alone
            io["ctl"][4 * bucket:].fill_(-1)
            if self.config.device_sampling:
                io["temperature"].zero_()     # the tail is a plain argmax
            if self.config.device_logprobs:
                io["lp_n"].fill_(-1)          # and computes no logprobs
            if self.config.device_penalties:
                io["pen_slot"].fill_(-1)      # and penalises no row
            if self.config.device_guided:
                io["gd_state"].fill_(-1)      # and masks none
            io["passthrough"] = True
        io["input_ids"][:B] = input_ids
        io["input_ids"][B:] = 0
        io["positions"][:B] = meta.positions
        io["positions"][B:] = 0
        io["slot_mapping"][:B] = meta.slot_mapping
        io["slot_mapping"][B:] = -1          # padded rows write nothing
        io["block_tables"].zero_()
        io["block_tables"][:B, :meta.block_tables.shape[1]] = meta.block_tables
        io["seq_lens"][:B] = meta.seq_lens
        io["seq_lens"][B:] = 1
        self._graphs[bucket].replay()
        return io["logits"][:B]

    def _bucket_for(self, b: int) -> Optional[int]:
        for s in self.config.graph_batch_sizes:
            if s >= b:
                return s
        return None

    def _capture(self, bucket: int) -> None:
        d = self.device
        log.info("capturing decode hipGraph for batch=%d", bucket)
        io = {
            "input_ids": torch.zeros(bucket, dtype=torch.long, device=d),
            "positions": torch.zeros(bucket, dtype=torch.long, device=d),
            "slot_mapping": torch.full((bucket,), -1, dtype=torch.long, device=d),
            "block_tables": torch.zeros(bucket, self.max_blocks_per_seq,
                                        dtype=torch.int32, device=d),
            "seq_lens": torch.ones(bucket, dtype=torch.int32, device=d),
            # pipelined stepping: the previous step's argmax and the
            # per-step control block of decode_advance (n_live < 0 =
            # pass-through, the synchronous path fills the inputs itself)
            "sampled": torch.zeros(bucket, dtype=torch.long, device=d),
            "passthrough": True,
        }
        io.update(self._pipe_ctl_io(bucket, d))
        meta = ForwardMeta(mode="decode", positions=io["positions"],
                           slot_mapping=io["slot_mapping"],
                           block_tables=io["block_tables"],
                           seq_lens=io["seq_lens"])
        # warmup outside capture (allocator, hipBLASLt heuristics, RCCL)
        for _ in range(2):
            self._pipe_head(io)
            self._pipe_tail(
                io, self.model(io["input_ids"], meta, self.kv_caches))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=self._graph_pool):
            # head: per-step inputs derived on the device; tail: the
            # sampled token (argmax, or sample_fused with device_sampling)
            # into the buffer the next replay's head reads
            self._pipe_head(io)
            io["logits"] = self.model(io["input_ids"], meta, self.kv_caches)
            self._pipe_tail(io, io["logits"])
        if self._graph_pool is None:
            self._graph_pool = g.pool()
        self._graphs[bucket] = g
        self._graph_io[bucket] = io

    @torch.inference_mode()
    def capture_all_graphs(self) -> None:
        # inference_mode matches the lazy in-step captures: every graph
        # io tensor is an inference tensor regardless of capture origin
        # (mixing modes trips "inplace update to inference tensor")
        if self.device.type != "cuda" or self.config.enforce_eager:
            return
        for b in self.config.graph_batch_sizes:
            if b <= self.config.max_num_seqs and b not in self._graphs:
                self._capture(b)
        for t in self.config.prefill_graph_sizes:
            if (t <= self.config.max_num_batched_tokens
                    and t <= self.config.max_model_len
                    and t not in self._pgraphs):
                self._capture_prefill(t)

    # ---------------- pipelined decode ----------------
    #
    # A decode step whose inputs do not depend on the tokens still in flight
    # is enqueued from lengths alone: decode_advance (head of the graph)
    # derives ids / positions / slots / table updates on the device from
    # the previous step's token (tail of the graph: the argmax, or with
    # device_sampling sample_fused on per-row parameters uploaded at the
    # re-seed and one uniform per row and step).  Rows keep their slot
    # in the bucket for as long as the device state lives; a row that leaves
    # becomes a padding row in place, and the state is re-seeded from the
    # host (every row on the host-id path, rows compacted) after any
    # synchronous step or when the live rows fit a smaller bucket.

    def _pipe_head(self, io: dict) -> None:
        ops.decode_advance(io["input_ids"], io["positions"], io["seq_lens"],
                           io["slot_mapping"], io["block_tables"],
                           io["sampled"], io["ctl"], self.config.block_size)

    def _pipe_ctl_io(self, rows: int, d) -> dict:
        """Device control block of a `rows`-row state.  With
        device_sampling the per-row sampling parameters come with it, and
        the uniforms sit right behind the block (one H2D for both)."""
        io = {}
        if self.config.device_logprobs:
            cols = ops.torch_ref.LOGPROB_COLS
            # lp_n -1 = the row asks for none: padding rows, pass-through
            # replays, rows without SamplingParams.logprobs
            io["lp_n"] = torch.full((rows,), -1, dtype=torch.int32, device=d)
            io["lp_val"] = torch.full((rows, cols), float("-inf"),
                                      dtype=torch.float32, device=d)
            io["lp_id"] = torch.full((rows, cols), -1, dtype=torch.int32,
                                     device=d)
        if self.config.device_penalties:
            # pen_slot -1 = not a penalty row: padding rows, pass-through
            # replays, rows whose three penalties are neutral
            io["pen_slot"] = torch.full((rows,), -1, dtype=torch.int32,
                                        device=d)
            io["pen_rep"] = torch.ones(rows, dtype=torch.float32, device=d)
            io["pen_pres"] = torch.zeros(rows, dtype=torch.float32, device=d)
            io["pen_freq"] = torch.zeros(rows, dtype=torch.float32, device=d)
        if self.config.device_guided:
            # word 0 = -1 = not a guided row: padding rows, pass-through
            # replays, rows that are not in JSON mode
            io["gd_state"] = torch.full(
                (rows, ops.torch_ref.GUIDED_WORDS), -1, dtype=torch.int32,
                device=d)
        if not self.config.device_sampling:
            io["ctl"] = torch.full((4 * rows + 4,), -1, dtype=torch.int32,
                                   device=d)
            return io
        buf = torch.full((5 * rows + 4,), -1, dtype=torch.int32, device=d)
        uni = buf[4 * rows + 4:].view(torch.float32)
        uni.zero_()
        io.update({
            "ctl_uniform": buf, "ctl": buf[:4 * rows + 4], "uniform": uni,
            # temperature 0 = argmax: padding rows, pass-through replays
            "temperature": torch.zeros(rows, dtype=torch.float32, device=d),
            "top_p": torch.ones(rows, dtype=torch.float32, device=d),
            "top_k": torch.zeros(rows, dtype=torch.int32, device=d),
        })
        return io

    def _pipe_tail(self, io: dict, logits: torch.Tensor) -> None:
        pen = self.config.device_penalties
        if pen:
            # first, so that the sampler and the logprobs see the
            # penalised logits
            ops.penalty_apply(logits, io["pen_slot"], io["pen_rep"],
                              io["pen_pres"], io["pen_freq"],
                              self._pen_table)
        guided = self.config.device_guided
        if guided:
            # behind the penalties and in front of the sampler, the order of
            # _sample: the logprobs describe the masked logits
            ops.guided_json_mask(logits, io["gd_state"])
        if self.config.device_sampling:
            ops.sample_fused(logits, io["temperature"], io["top_p"],
                             io["top_k"], io["uniform"], out=io["sampled"])
        else:
            ops.greedy_sample(logits, out=io["sampled"])
        if guided:
            # the next step's mask is that of the state behind this token.
            # EOS is no byte and leaves the state alone, so the extra step of
            # a row whose EOS is seen one step late is masked like the last
            ops.guided_json_advance(io["gd_state"], io["sampled"])
        if pen:
            # the next step's penalty_apply counts this token.  A row that
            # runs a step past its end (EOS seen one step late, dropped,
            # aborted) or idles as a padding row in place still notes a
            # token into its own slot: nothing reads that slot again before
            # the next re-seed rebuilds it
            ops.penalty_note(self._pen_table, io["pen_slot"], io["sampled"])
        if self.config.device_logprobs:
            ops.token_logprobs(logits, io["sampled"], io["lp_n"],
                               io["lp_val"], io["lp_id"])

    def pipe_invalidate(self) -> None:
        self._pipe = None

    def pipe_valid(self) -> bool:
        return self._pipe is not None

    def pipe_drop(self, request_id: str) -> None:
        """The row takes part in no further pipelined step."""
        p = self._pipe
        if p is not None:
            s = p["slot_of"].get(request_id)
            if s is not None:
                p["alive"][s] = False

    def pipe_stale(self) -> bool:
        """Enough rows left that the rest fit a smaller bucket."""
        p = self._pipe
        if p is None:
            return False
        n = int(p["alive"].sum())
        if n == 0:
            return False
        if p["graph"]:
            return self._bucket_for(n) != p["bucket"]
        return n * 2 <= len(p["reqs"])

    def _pipe_seed(self, reqs: List[Request]) -> None:
        import numpy as np
        bm = self.block_manager
        B = len(reqs)
        bucket = self._bucket_for(B)
        graph = (bucket is not None and self.device.type == "cuda"
                 and not self.config.enforce_eager)
        if graph:
            if bucket not in self._graphs:
                self._capture(bucket)
            io = self._graph_io[bucket]
            nrows = bucket
        else:
            full = self._pipe_eager_io
            if full is None:
                cap, d = bm.capacity, self.device
                full = self._pipe_eager_io = {
                    "input_ids": torch.zeros(cap, dtype=torch.long, device=d),
                    "positions": torch.zeros(cap, dtype=torch.long, device=d),
                    "slot_mapping": torch.full((cap,), -1, dtype=torch.long,
                                               device=d),
                    "block_tables": torch.zeros(cap, self.max_blocks_per_seq,
                                                dtype=torch.int32, device=d),
                    "seq_lens": torch.ones(cap, dtype=torch.int32, device=d),
                    "sampled": torch.zeros(cap, dtype=torch.long, device=d),
                }
                full.update(self._pipe_ctl_io(cap, d))
            nrows = B
            whole = ("ctl", "ctl_uniform", "uniform")
            io = {k: v[:nrows] for k, v in full.items() if k not in whole}
            if self.config.device_sampling:
                buf = full["ctl_uniform"][:5 * nrows + 4]
                io["ctl_uniform"] = buf
                io["ctl"] = buf[:4 * nrows + 4]
                io["uniform"] = buf[4 * nrows + 4:].view(torch.float32)
            else:
                io["ctl"] = full["ctl"][:4 * nrows + 4]
        self._pipe = {
            "graph": graph, "bucket": bucket, "io": io, "nrows": nrows,
            "reqs": list(reqs), "fresh": True,
            "slot_of": {r.request_id: i for i, r in enumerate(reqs)},
            "rows": np.fromiter((bm.row_of[r.request_id] for r in reqs),
                                dtype=np.int64, count=B),
            "alive": np.ones(B, dtype=bool),
            # steps the row may still be launched for
            "remaining": np.fromiter(
                (r.sampling.max_tokens - r.num_generated for r in reqs),
                dtype=np.int64, count=B),
        }
        if self.config.device_sampling:
            self._pipe_seed_sampling(reqs, io, nrows)
        if self.config.device_logprobs:
            # once per re-seed; rows past the live ones ask for none
            lp = torch.full((nrows,), -1, dtype=torch.int32)
            lp[:B] = torch.tensor(
                [-1 if r.sampling.logprobs is None else r.sampling.logprobs
                 for r in reqs], dtype=torch.int32)
            io["lp_n"].copy_(lp)
            self._pipe["lp_n"] = lp[:B].numpy()
        if self.config.device_penalties:
            self._pipe_seed_penalties(reqs, io, nrows)
        if self.config.device_guided:
            self._pipe_seed_guided(reqs, io, nrows)

    def _pipe_seed_penalties(self, reqs: List[Request], io: dict,
                             nrows: int) -> None:
        """Give each penalty row a table slot, build the slots from the
        histories and upload the four per-row vectors (once per re-seed).
        Nothing is in flight at a re-seed, so the host knows every history
        completely, the last token included: that one goes into this step
        through decode_advance's host-id path and is in the built counts
        already, so penalty_note only ever counts newly sampled tokens.
        _pipe_eligible has seen to it that the slots suffice."""
        rows = [i for i, r in enumerate(reqs) if r.sampling.penalized]
        slot, par = self._penalty_rows(reqs, rows, nrows)
        io["pen_slot"].copy_(slot)
        io["pen_rep"].copy_(par[0])
        io["pen_pres"].copy_(par[1])
        io["pen_freq"].copy_(par[2])

    def _pipe_seed_sampling(self, reqs: List[Request], io: dict,
                            nrows: int) -> None:
        """Upload the rows' sampling parameters (once per re-seed; rows
        past the live ones are argmax rows) and note which rows draw."""
        import numpy as np
        B = len(reqs)
        par = torch.zeros(3, nrows, dtype=torch.float32)
        par[1].fill_(1.0)
        par[0, :B] = torch.tensor([r.sampling.temperature for r in reqs],
                                  dtype=torch.float32)
        par[1, :B] = torch.tensor([r.sampling.top_p for r in reqs],
                                  dtype=torch.float32)
        topk = torch.zeros(nrows, dtype=torch.int32)
        topk[:B] = torch.tensor([r.sampling.top_k for r in reqs],
                                dtype=torch.int32)
        io["temperature"].copy_(par[0])
        io["top_p"].copy_(par[1])
        io["top_k"].copy_(topk)
        p = self._pipe
        p["stoch"] = par[0, :B].numpy() != 0
        p["seeded"] = np.fromiter((r.sampling.seed is not None for r in reqs),
                                  dtype=bool, count=B)

    def _seed_gen_of(self, r: Request) -> torch.Generator:
        g = getattr(r, "_seed_gen", None)
        if g is None:
            g = torch.Generator().manual_seed(r.sampling.seed)
            r._seed_gen = g
        return g

    def _pipe_draw(self, p: dict, idx, uni: torch.Tensor) -> None:
        """One uniform per launched row into the ring slot's pinned tail
        (uni, float32 [nrows]): a seeded row takes one torch.rand(1) from
        its own generator per sampled token, exactly as _sample does, the
        others share self._gen."""
        seeded = p["seeded"][idx]
        plain = idx[~seeded]
        if plain.size:
            uni[torch.from_numpy(plain)] = torch.rand(
                plain.size, generator=self._gen)
        reqs = p["reqs"]
        for i in idx[seeded]:
            uni[int(i)] = torch.rand(
                1, generator=self._seed_gen_of(reqs[i]))[0]

    @torch.inference_mode()
    def pipe_launch(self, seed_reqs: Optional[List[Request]] = None):
        """Enqueue one decode step without waiting for the previous one.

        seed_reqs: re-seed the device state from these requests first (only
        with nothing in flight).  Returns a handle for pipe_collect, or None
        when no step was enqueued: no row has a token left to produce, or
        the pool cannot give every page-starting row its page (the caller
        falls back to the synchronous step, which may preempt)."""
        import numpy as np
        bm = self.block_manager
        bs = bm.block_size
        if seed_reqs is not None:
            self._pipe_seed(seed_reqs)
        p = self._pipe
        idx = np.nonzero(p["alive"] & (p["remaining"] > 0))[0]
        if idx.size == 0:
            return None
        rows = p["rows"][idx]
        n = bm.tokens_np[rows].copy()            # this step's positions
        boundary = n % bs == 0
        if int(boundary.sum()) > bm.num_free:
            if p["fresh"]:
                self._pipe = None
            return None
        bm.append_slots_batch(rows)
        R = p["nrows"]
        io = p["io"]
        ring = self._pipe_ring[self._pipe_seq % len(self._pipe_ring)]
        self._pipe_seq += 1
        ctl = ring["ctl"].numpy()[:4 * R + 4]
        c = ctl[:4 * R].reshape(4, R)
        c[0].fill(-2)
        c[1].fill(-1)
        d = self.device
        nb = d.type == "cuda"
        if p["fresh"]:
            reqs = p["reqs"]
            c[0][idx] = -1
            c[2][idx] = np.fromiter((reqs[i].last_token_id for i in idx),
                                    dtype=np.int64, count=idx.size)
            c[3][idx] = n
            max_nt = int(bm.ntables_np[rows].max())
            bt_stage = self._st_bt_flat[:idx.size * max_nt].view(
                idx.size, max_nt)
            bt_stage.numpy()[:] = bm.tables_np[
                rows[:, None], np.arange(max_nt)[None, :]]
            # a fresh state holds every row, in order: idx == arange(B)
            io["block_tables"][:idx.size, :max_nt] = \
                bt_stage.to(d, non_blocking=nb)
            p["fresh"] = False
        else:
            c[0][idx] = idx
            c[1][idx[boundary]] = bm.tables_np[rows[boundary],
                                               n[boundary] // bs]
        ctl[4 * R] = int(idx[-1]) + 1
        if self.config.device_sampling and p["stoch"][idx].any():
            # the step is certain to launch: only now consume the draws
            self._pipe_draw(p, idx,
                            ring["ctl"][4 * R + 4:5 * R + 4].view(
                                torch.float32))
            io["ctl_uniform"].copy_(ring["ctl"][:5 * R + 4], non_blocking=nb)
        else:
            io["ctl"].copy_(ring["ctl"][:4 * R + 4], non_blocking=nb)
        if p["graph"]:
            io["passthrough"] = False
            self._graphs[p["bucket"]].replay()
        else:
            self._pipe_head(io)
            meta = ForwardMeta(mode="decode", positions=io["positions"],
                               slot_mapping=io["slot_mapping"],
                               block_tables=io["block_tables"],
                               seq_lens=io["seq_lens"])
            self._pipe_tail(
                io, self.model(io["input_ids"], meta, self.kv_caches))
        # token D2H behind the step on the same stream, outside the graph
        ring["tok"][:R].copy_(io["sampled"], non_blocking=nb)
        step = PipeStep([p["reqs"][i] for i in idx], idx, ring)
        if self.config.device_logprobs and (p["lp_n"][idx] >= 0).any():
            # the records follow the tokens, only when a launched row asks
            ring["lp_val"][:R].copy_(io["lp_val"], non_blocking=nb)
            ring["lp_id"][:R].copy_(io["lp_id"], non_blocking=nb)
            step.lp_n = p["lp_n"][idx]
        if nb:
            ring["event"].record()
        p["remaining"][idx] -= 1
        return step

    def pipe_collect(self, step: "PipeStep"):
        """Wait for the step's tokens (its own event, never a device-wide
        sync); returns [(request, token_id)] in slot order.  The logprob
        records of the same rows, if the step carries any, are left in
        step.records."""
        ev = step.ring["event"]
        if ev is not None:
            ev.synchronize()
        toks = step.ring["tok"].numpy()[step.slots].tolist()
        if step.lp_n is not None:
            step.records = _logprob_records(
                step.ring["lp_val"].numpy()[step.slots],
                step.ring["lp_id"].numpy()[step.slots], step.lp_n.tolist())
        return zip(step.reqs, toks)

    # ---------------- embeddings ----------------

    @torch.inference_mode()
    def embed(self, prompts: List[List[int]]) -> torch.Tensor:
        """Mean-pooled final hidden state per prompt -> [N, hidden] fp32.

        Runs outside the scheduler on temporary KV pages (freed at the end);
        serves the llm-gateway /embeddings contract."""
        from .request import Request
        from .config import SamplingParams
        bm = self.block_manager
        fake = []
        try:
            for i, p in enumerate(prompts):
                rid = f"__embed_{i}"
                bm.allocate(rid, len(p))
                fake.append(Request(request_id=rid, prompt_token_ids=list(p),
                                    sampling=SamplingParams()))
            batch = ScheduledBatch(mode="prefill", requests=fake,
                                   num_tokens=sum(len(p) for p in prompts))
            input_ids, meta = self._prefill_inputs(batch)
            meta.return_hidden = True
            hidden = self.model(input_ids, meta, self.kv_caches).float()
            out = torch.empty(len(prompts), hidden.shape[-1],
                              dtype=torch.float32, device=hidden.device)
            ss = meta.seq_start
            for i in range(len(prompts)):
                out[i] = hidden[int(ss[i]):int(ss[i + 1])].mean(0)
        finally:
            for i in range(len(prompts)):
                bm.free(f"__embed_{i}")
        return out.cpu()

    def swap_weights(self, checkpoint_path: str) -> float:
        from .checkpoint import load_checkpoint_into
        return load_checkpoint_into(self.model, checkpoint_path)

    # ---------------- sampling ----------------

    def _guided_machine(self, r: Request):
        """The request's grammar machine, created on first use and fed
        every output token it has not seen yet.  Shared by the host mask
        (_apply_guided) and the device state's re-seed (_pipe_seed_guided),
        so both stand on the same machine.  After a preemption has folded
        the outputs into the prompt the machine has consumed more than
        output_token_ids holds and a fresh one takes its place."""
        from .guided import (JsonByteMachine, SchemaMachine,
                             ToolCallMachine)
        m = getattr(r, "_guided", None)
        if m is None or m.consumed > len(r.output_token_ids):
            if r.sampling.response_format == "tool_call":
                m = ToolCallMachine(tuple(r.sampling.tool_names))
            elif r.sampling.response_schema is not None:
                try:
                    # untrusted schema: any compile failure degrades
                    # to plain JSON-grammar enforcement
                    m = SchemaMachine(r.sampling.response_schema)
                except Exception:
                    m = JsonByteMachine()
            else:
                m = JsonByteMachine()
            r._guided = m
        for t in r.output_token_ids[m.consumed:]:
            m.feed_token(t)
        return m

    def guided_fits_device(self, r: Request) -> bool:
        """A JSON-mode row whose machine, caught up with its outputs, fits
        the device state's 256-level stack (LLMEngine._pipe_eligible asks
        with nothing in flight, so the outputs are complete)."""
        m = self._guided_machine(r)
        return len(m.stack) <= ops.torch_ref.GUIDED_MAX_DEPTH

    def _pipe_seed_guided(self, reqs: List[Request], io: dict,
                          nrows: int) -> None:
        """Upload the automaton state of the JSON-mode rows (once per
        re-seed; every other row is -1).  Nothing is in flight at a
        re-seed, so the host machine has been fed every output token, the
        last one included: that one goes into this step through
        decode_advance's host-id path, and guided_json_advance only ever
        sees newly sampled tokens.  Nothing comes back from the device: the
        host machine catches up from output_token_ids at the next
        synchronous step or re-seed."""
        st = torch.full((nrows, ops.torch_ref.GUIDED_WORDS), -1,
                        dtype=torch.int32)
        for i, r in enumerate(reqs):
            if r.sampling.response_format == "json" \
                    and r.sampling.response_schema is None:
                st[i] = torch.tensor(self._guided_machine(r).pack(),
                                     dtype=torch.int32)
        io["gd_state"].copy_(st)

    def _apply_guided(self, logits: torch.Tensor,
                      requests: List[Request]) -> None:
        """Structured-output mask (SamplingParams.response_format="json"):
        only grammar-legal next BYTES (byte tokenizer: id = byte + 4)
        keep their logits; EOS opens up once the JSON value is closed.
        In-place on the [B, vocab] logits; no-op without guided seqs."""
        gis = [i for i, r in enumerate(requests)
               if r.sampling.response_format in ("json", "tool_call")
               or r.sampling.response_schema is not None]
        if not gis:
            return
        NB = 4 + 256                       # specials + byte ids
        neg = float("-inf")
        rows: List[torch.Tensor] = []
        cache = self._guided_mask_cache
        for k, i in enumerate(gis):
            r = requests[i]
            m = self._guided_machine(r)
            # cache mask rows by machine state (mask_key): avoids a
            # ~230-iteration Python loop per guided sequence per step
            key = m.mask_key() if hasattr(m, "mask_key") else None
            row = cache.get(key) if key is not None else None
            if row is None:
                allow, eos_ok = m.allowed()
                row = torch.full((NB,), neg, dtype=torch.float32)
                for b in allow:
                    row[b + 4] = 0.0
                if eos_ok:
                    row[2] = 0.0           # ByteTokenizer EOS
                if key is not None:
                    cache[key] = row
            rows.append(row)
        small = torch.stack(rows)
        d = logits.device
        gidx = torch.tensor(gis, device=d)
        logits[gidx, NB:] = neg
        logits[gidx, :NB] += small.to(device=d, dtype=logits.dtype)

    # ---------------- penalties ----------------

    def _penalty_table(self) -> torch.Tensor:
        if self._pen_table is None:
            self._pen_table = torch.zeros(
                max(self.config.max_penalty_seqs, 1), self.spec.vocab_size,
                dtype=torch.int32, device=self.device)
        return self._pen_table

    def _penalty_build(self, reqs: List[Request]) -> None:
        """Table slots 0..len(reqs)-1 := the requests' histories, uploaded
        as one flat int32 tensor.  The generated tokens are the last
        num_generated of prompt + output, not output_token_ids: preemption
        folds the outputs into the prompt, and num_generated survives."""
        import numpy as np
        n = len(reqs)
        off = np.zeros(n + 1, dtype=np.int32)
        plen = np.empty(n, dtype=np.int32)
        hist: List[int] = []
        for i, r in enumerate(reqs):
            hist.extend(r.prompt_token_ids)
            hist.extend(r.output_token_ids)
            off[i + 1] = len(hist)
            plen[i] = r.num_tokens - r.num_generated
        d = self.device
        # ids that do not fit int32 lie outside any vocabulary: -1 skips
        toks = np.asarray(hist, dtype=np.int64)
        toks[(toks < 0) | (toks > 0x7fffffff)] = -1
        ops.penalty_build(
            self._penalty_table(),
            torch.arange(n, dtype=torch.int32).to(d),
            torch.from_numpy(toks.astype(np.int32)).to(d),
            torch.from_numpy(off).to(d), torch.from_numpy(plen).to(d))

    def _penalty_rows(self, requests: List[Request], rows: List[int],
                      nrows: int):
        """Rows `rows` of the batch take table slots 0..len(rows)-1, built
        from their histories.  Returns the per-row vectors of an
        `nrows`-row launch on the host: slot int32 (-1 elsewhere) and
        float32 [3, nrows] = repetition (1 elsewhere) | presence |
        frequency (0 elsewhere)."""
        par = torch.zeros(3, nrows, dtype=torch.float32)
        par[0].fill_(1.0)
        slot = torch.full((nrows,), -1, dtype=torch.int32)
        for k, i in enumerate(rows):
            sp = requests[i].sampling
            slot[i] = k
            par[0, i] = sp.repetition_penalty
            par[1, i] = sp.presence_penalty
            par[2, i] = sp.frequency_penalty
        if rows:
            self._penalty_build([requests[i] for i in rows])
        return slot, par

    def _apply_penalties(self, logits: torch.Tensor,
                         requests: List[Request]) -> None:
        """Penalties of the synchronous step, in place on its logits and
        before anything else reads them.  The penalty rows that sample a
        token this step (not a mid-prompt chunk) take scratch slots
        0..k-1 of the table, max_penalty_seqs at a time, rebuilt from the
        host's histories every step; the pipelined state that may live in
        those slots is invalid after a synchronous step anyway.  On a
        request's first prefill every token is prompt, so only
        repetition_penalty acts; a prefill that recomputes a preempted
        request still counts the outputs folded into its prompt as
        generated.  No penalty row: no op is called, no table allocated."""
        rows = [i for i, r in enumerate(requests) if r.sampling.penalized
                and r.num_computed_tokens >= r.num_prompt_tokens]
        if not rows:
            return
        S = self._penalty_table().shape[0]
        R = logits.shape[0]
        d = logits.device
        for k0 in range(0, len(rows), S):
            slot, par = self._penalty_rows(requests, rows[k0:k0 + S], R)
            par = par.to(d)
            ops.penalty_apply(logits, slot.to(d), par[0], par[1], par[2],
                              self._pen_table)

    def _sample(self, logits: torch.Tensor, requests: List[Request]) -> torch.Tensor:
        self._apply_penalties(logits, requests)
        self._apply_guided(logits, requests)
        tokens = self._sample_tokens(logits, requests)
        # after the token is chosen, on the (penalised, guided-masked) logits
        # it was chosen from; the records wait in last_logprobs for LLMEngine.step
        n_top = [-1 if r.sampling.logprobs is None else r.sampling.logprobs
                 for r in requests]
        self.last_logprobs = None
        if max(n_top) >= 0:
            d = logits.device
            val, idx = ops.token_logprobs(
                logits, tokens.to(d),
                torch.tensor(n_top, dtype=torch.int32).to(d))
            self.last_logprobs = _logprob_records(
                val.cpu().numpy(), idx.cpu().numpy(), n_top)
        return tokens.cpu()

    def _sample_tokens(self, logits: torch.Tensor,
                       requests: List[Request]) -> torch.Tensor:
        B = logits.shape[0]
        temps = torch.tensor([r.sampling.temperature for r in requests],
                             dtype=torch.float32)
        if bool((temps == 0).all()):
            return ops.greedy_sample(logits)
        top_p = torch.tensor([r.sampling.top_p for r in requests],
                             dtype=torch.float32)
        top_k = torch.tensor([r.sampling.top_k for r in requests],
                             dtype=torch.int32)
        if any(r.sampling.seed is not None for r in requests):
            # per-request reproducible draws (SamplingParams.seed)
            us = []
            for r in requests:
                if r.sampling.seed is not None:
                    us.append(torch.rand(1, generator=self._seed_gen_of(r)))
                else:
                    us.append(torch.rand(1, generator=self._gen))
            uniform = torch.cat(us)
        else:
            uniform = torch.rand(B, generator=self._gen)
        d = logits.device
        if self.config.device_sampling:
            # one kernel on the logits as they are (no fp32 copy, no sort);
            # the pipelined step runs the same kernel on the same draws
            return ops.sample_fused(logits, temps.to(d), top_p.to(d),
                                    top_k.to(d), uniform.to(d))
        return ops.sample(logits, temps.to(d), top_p.to(d), top_k.to(d),
                          uniform.to(d))

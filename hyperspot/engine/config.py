"""Model and engine configuration.

The reference (cyberfabric/cyberfabric-core) ships no model code; the model set
here is the one named by BASELINE.json: Llama-3-8B (TP=1), Llama-3-70B (TP=8),
Mixtral 8x7B (EP).  Architecture hyper-parameters follow the public
architectures; weights are random-init (no network in this environment).
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional


@dataclass
class ModelSpec:
    """Architecture description for a decoder-only transformer."""

    name: str
    hidden_size: int
    num_layers: int
    num_heads: int
    num_kv_heads: int
    head_dim: int
    intermediate_size: int
    vocab_size: int
    rope_theta: float = 500000.0
    rms_eps: float = 1e-5
    max_position: int = 8192
    tie_embeddings: bool = False
    # MoE (0 experts => dense MLP)
    num_experts: int = 0
    num_experts_per_tok: int = 0
    dtype: str = "bfloat16"

    @property
    def is_moe(self) -> bool:
        return self.num_experts > 0

    def param_count(self) -> int:
        h, l, i, v = self.hidden_size, self.num_layers, self.intermediate_size, self.vocab_size
        qkv = h * (self.num_heads + 2 * self.num_kv_heads) * self.head_dim
        o = self.num_heads * self.head_dim * h
        if self.is_moe:
            mlp = 3 * h * i * self.num_experts + h * self.num_experts
        else:
            mlp = 3 * h * i
        per_layer = qkv + o + mlp + 2 * h
        emb = v * h * (1 if self.tie_embeddings else 2)
        return l * per_layer + emb + h


# Preset registry (keys are the canonical model ids used by the model-registry
# module; reference modules/model-registry/docs/PRD.md:11 canonical id format).
_PRESETS = {
    "llama3-8b": ModelSpec(
        name="llama3-8b", hidden_size=4096, num_layers=32, num_heads=32,
        num_kv_heads=8, head_dim=128, intermediate_size=14336,
        vocab_size=128256, rope_theta=500000.0,
    ),
    "llama3-70b": ModelSpec(
        name="llama3-70b", hidden_size=8192, num_layers=80, num_heads=64,
        num_kv_heads=8, head_dim=128, intermediate_size=28672,
        vocab_size=128256, rope_theta=500000.0,
    ),
    "mixtral-8x7b": ModelSpec(
        name="mixtral-8x7b", hidden_size=4096, num_layers=32, num_heads=32,
        num_kv_heads=8, head_dim=128, intermediate_size=14336,
        vocab_size=32000, rope_theta=1000000.0, num_experts=8,
        num_experts_per_tok=2,
    ),
    # Tiny models for CPU tests / CI (same code paths, small shapes).
    "tiny-llama": ModelSpec(
        name="tiny-llama", hidden_size=256, num_layers=2, num_heads=4,
        num_kv_heads=2, head_dim=64, intermediate_size=512, vocab_size=512,
        rope_theta=10000.0, max_position=1024,
    ),
    # tiny-llama at head_dim 128: engine tests reach the 128-dim attention
    # kernels (MFMA prefill, v3 decode, fp8 KV) without an 8B-shaped model
    "tiny-llama-d128": ModelSpec(
        name="tiny-llama-d128", hidden_size=256, num_layers=2, num_heads=4,
        num_kv_heads=2, head_dim=128, intermediate_size=512, vocab_size=512,
        rope_theta=10000.0, max_position=1024,
    ),
    "tiny-moe": ModelSpec(
        name="tiny-moe", hidden_size=256, num_layers=2, num_heads=4,
        num_kv_heads=2, head_dim=64, intermediate_size=256, vocab_size=512,
        rope_theta=10000.0, max_position=1024, num_experts=4,
        num_experts_per_tok=2,
    ),
}


def get_model_spec(name: str) -> ModelSpec:
    key = name.lower()
    if key not in _PRESETS:
        raise KeyError(f"unknown model preset '{name}' (have: {sorted(_PRESETS)})")
    return _PRESETS[key]


@dataclass
class EngineConfig:
    """Engine/runtime configuration (the serverless-runtime worker side).

    KV sizing targets 288 GB HBM3E per MI355X GPU: after weights, the pool
    takes ``gpu_memory_utilization`` of free memory in BLOCK_SIZE-token pages.
    """

    model: str = "llama3-8b"
    block_size: int = 16                 # tokens per KV page
    max_num_seqs: int = 256              # max concurrent sequences
    max_num_batched_tokens: int = 8192   # per-step token budget (chunked prefill)
    max_model_len: int = 8192
    gpu_memory_utilization: float = 0.90
    num_gpu_blocks: Optional[int] = None  # override (tests / CPU)
    enforce_eager: bool = False           # disable hipGraph decode capture
    tp_size: int = 1
    ep_size: int = 1
    dtype: str = "bfloat16"
    quant: Optional[str] = None          # None (bf16) | "fp8" (e4m3fn weights)
    kv_dtype: str = "bfloat16"           # "bfloat16" | "fp8" (e4m3fn cache)
    enable_prefix_caching: bool = False  # shared-prompt KV block reuse
    # prefill steps that do not start at position 0 (chunked-prefill
    # continuations, prefix-cache hits) on the MFMA flash kernel over the
    # paged cache instead of the per-row kernel.  Off by default: the two
    # kernels round differently (bf16 vs fp32 P), so turning it on changes
    # greedy outputs of such steps by bf16-ulp effects
    prefill_paged_mfma: bool = False
    # enqueue decode step n+1 before step n's tokens reach the host
    # (LLMEngine.step_pipelined); same tokens and finish reasons either way
    pipeline_decode: bool = True
    # sample on the device with the fused top-k/top-p kernel
    # (ops.sample_fused): stochastic rows then stay in the pipelined
    # decode, whose graphs end in that kernel instead of the argmax.  Off
    # by default: where tokens tie at a top-k/top-p cut, or a draw falls on
    # a rounding boundary, it can pick another token than the sort-based
    # ops.sample does for the same seed
    device_sampling: bool = False
    # keep rows that ask for logprobs (SamplingParams.logprobs) in the
    # pipelined decode: every decode graph then ends in ops.token_logprobs
    # behind the sampler, and the records ride the staging ring.  Off by
    # default, so that the default graphs launch what they always did;
    # logprob rows then take the synchronous step
    device_logprobs: bool = False
    # keep rows with presence / frequency / repetition penalties in the
    # pipelined decode: every decode graph then runs ops.penalty_apply in
    # front of the sampler and ops.penalty_note behind it, on a count table
    # int32 [max_penalty_seqs, vocab] allocated with the engine (131 MB at
    # Llama's vocabulary and 256 slots).  Off by default, so that the
    # default graphs launch what they always did; penalty rows then take
    # the synchronous step, and the table is allocated at the first one
    device_penalties: bool = False
    max_penalty_seqs: int = 256          # slots of the penalty count table
    # keep JSON-mode rows (SamplingParams.response_format="json", no
    # response_schema) in the pipelined decode: every decode graph then runs
    # ops.guided_json_mask in front of the sampler and
    # ops.guided_json_advance behind it, on an automaton state int32
    # [rows, 11] per graph.  The device stack holds 256 levels: at that depth
    # '{' and '[' are masked, where the host machine nests without bound.
    # Off by default, so that the default graphs launch what they always
    # did; JSON rows then take the synchronous step, as schema and tool-call
    # rows do either way
    device_guided: bool = False
    seed: int = 0
    # decode hipGraph capture batch buckets (padded up to nearest)
    graph_batch_sizes: tuple = (1, 2, 4, 8, 16, 24, 32, 48, 64, 96, 128,
                                192, 256, 384, 512, 768, 1024, 1536, 2048)
    # single-request whole-prompt prefill graphs (TTFT fast path):
    # tokens pad up to the bucket, padded slots write no KV
    prefill_graph_sizes: tuple = (128, 256, 512, 1024, 2048)

    def spec(self) -> ModelSpec:
        return get_model_spec(self.model)


@dataclass
class SamplingParams:
    """Per-request sampling parameters.

    The reference request schema has *no* sampling fields
    (llm-gateway-sdk/schemas/core/request.v1.schema.json — verified in
    SURVEY.md Appendix B); these are the engine-side extension exposed via the
    v2 request surface.
    """

    temperature: float = 1.0
    top_p: float = 1.0
    top_k: int = 0            # 0 => disabled
    max_tokens: int = 128
    min_tokens: int = 0
    stop_token_ids: tuple = ()
    ignore_eos: bool = False
    seed: Optional[int] = None
    # "json": constrained decoding — the sampler masks every token that
    # would break RFC-8259 validity and only allows EOS once the
    # top-level value closes; "tool_call" forces the ToolCall skeleton
    # (engine/guided.py)
    response_format: Optional[str] = None
    # a JSON Schema dict: SCHEMA-shaped constrained decoding — the
    # object skeleton (known keys, declared value types) is forced
    # byte-exactly (guided.SchemaMachine); overrides response_format
    response_schema: Optional[dict] = None
    # declared tool names: a forced tool call ("tool_call" format)
    # narrows the emitted name to one of these (guided.ToolCallMachine)
    tool_names: tuple = ()
    # per-token log-probabilities: None = off, 0 = the sampled token only,
    # 1..20 = plus that many most likely alternatives.  The distribution
    # is the one the token was chosen from at temperature 1, before top-k
    # and top-p (after the penalties below and the guided-decoding mask):
    # a record describes the penalised logits the token was chosen from
    logprobs: Optional[int] = None
    # OpenAI-style penalties on the tokens the request has seen, applied
    # to the logits before anything else (guided mask, sampler, logprobs).
    # repetition_penalty r divides the positive and multiplies the other
    # logits of every token of prompt or output; frequency_penalty times
    # a token's count among the GENERATED tokens, and presence_penalty
    # once if that count is not zero, are subtracted.  presence and
    # frequency lie in [-2, 2], r > 0; (0, 0, 1) = no penalty
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    repetition_penalty: float = 1.0

    @property
    def greedy(self) -> bool:
        return self.temperature == 0.0

    @property
    def penalized(self) -> bool:
        return not (self.presence_penalty == 0 and self.frequency_penalty == 0
                    and self.repetition_penalty == 1)

    def check_penalties(self) -> None:
        """ValueError unless the three penalties are finite and in range."""
        import math
        for name, lo, hi in (("presence_penalty", -2.0, 2.0),
                             ("frequency_penalty", -2.0, 2.0),
                             ("repetition_penalty", 0.0, math.inf)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) \
                    or not math.isfinite(v):
                raise ValueError(
                    f"SamplingParams.{name} must be a finite number, "
                    f"got {v!r}")
            if name == "repetition_penalty":
                if v <= 0:
                    raise ValueError(
                        f"SamplingParams.repetition_penalty must be > 0, "
                        f"got {v!r}")
            elif not lo <= v <= hi:
                raise ValueError(
                    f"SamplingParams.{name} must lie in [-2, 2], got {v!r}")

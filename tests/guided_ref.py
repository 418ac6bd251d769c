"""Shared ground for the device JSON-mode tests: a corpus of JSON documents,
its byte-by-byte walk through the host machine (JsonByteMachine), and the
host mask row of a machine exactly as ModelRunner._apply_guided builds it.

Not a test module: test_guided_device.py (CPU, torch twins) and
test_guided_gpu.py (kernels against the twins) load it by path."""

import copy
import functools
import json
import random
import types

import torch

from hyperspot.engine.config import SamplingParams
from hyperspot.engine.guided import JsonByteMachine
from hyperspot.engine.model_runner import ModelRunner
from hyperspot.engine.request import Request
from hyperspot.ops import torch_ref as TR

# every scalar form: escapes and \u in strings, raw UTF-8, the three
# literals, every number shape (and so every num_* mode and terminator)
VALUES = ['"a\\n\\u00e9\\\\ \\"q\\" \\/"', '"hé世"', '""', "true",
          "false", "null", "0", "-0", "7", "-12", "0.5", "3.25", "1e5", "0e0",
          "2E+3", "-1.5e-7", "10.01E2", "[]", "{}"]


def _hand_written():
    docs = list(VALUES)
    for v in VALUES:
        docs += [f"[{v}]", f"[{v},{v}]", f'{{"a":{v}}}',
                 f'{{"a\\t\\u0041":{v},"b":{v}}}', f"[[{v}],{{\"k\":[{v}]}}]"]
    docs += ['{"a":{"b":{"c":[1,[2,[3,{"d":null}]]]}},"e":[{},[],{"f":{}}]}',
             "[[[[[[[[[[0]]]]]]]]]]", '[{"x":[{"y":[{"z":-0.0e-0}]}]}]']
    return docs


def _random_value(rng, depth):
    k = rng.randrange(9 if depth < 4 else 6)
    if k == 0:
        return rng.choice([True, False, None])
    if k == 1:
        return rng.randrange(-10 ** rng.randrange(1, 12),
                             10 ** rng.randrange(1, 12))
    if k == 2:
        return rng.choice([0.0, -0.0, rng.uniform(-1, 1),
                           rng.uniform(-1e20, 1e20), rng.uniform(0, 1e-9)])
    if k in (3, 4, 5):
        alphabet = 'ab"\\/\b\f\n\r\t\x01 é世\U0001f600{}[]:,0'
        return "".join(rng.choice(alphabet)
                       for _ in range(rng.randrange(0, 7)))
    if k in (6, 7):
        return [_random_value(rng, depth + 1)
                for _ in range(rng.randrange(0, 4))]
    return {"".join(rng.choice('k"\\é_1') for _ in range(rng.randrange(3))):
            _random_value(rng, depth + 1) for _ in range(rng.randrange(0, 4))}


def _seeded_random(n=60, seed=20240611):
    rng = random.Random(seed)
    return [json.dumps(_random_value(rng, 0), separators=(",", ":"),
                       ensure_ascii=bool(i % 2)) for i in range(n)]


@functools.lru_cache(maxsize=None)
def corpus():
    """The documents, as bytes."""
    return tuple(d.encode("utf-8") for d in _hand_written() + _seeded_random())


@functools.lru_cache(maxsize=None)
def walk():
    """Every prefix of every document: a tuple of (machine, next_byte, fed)
    where `machine` has been fed the prefix, next_byte is the document's
    next byte (None at its end) and `fed` is a machine after that byte too
    (None at the end).  The machines are never touched again: copy one
    before feeding it."""
    out = []
    for doc in corpus():
        m = JsonByteMachine()
        for b in doc:
            nxt = copy.deepcopy(m)
            nxt.feed(b)
            out.append((m, b, nxt))
            m = nxt
        assert m.done, doc
        out.append((m, None, None))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def distinct_steps():
    """The walk's (packed state, token id, packed state after) triples, each
    distinct (state, token) once: what the advance op is held to."""
    seen = {}
    for m, b, nxt in walk():
        if b is None:
            continue
        key = (tuple(m.pack()), b + 4)
        if key not in seen:
            seen[key] = tuple(nxt.pack())
    return tuple((list(s), t, list(a)) for (s, t), a in seen.items())


@functools.lru_cache(maxsize=None)
def distinct_states():
    """Distinct packed states of the walk, with one machine each."""
    seen = {}
    for m, _, _ in walk():
        seen.setdefault(tuple(m.pack()), m)
    return tuple((list(k), m) for k, m in seen.items())


def nested(depth, kind="arr"):
    """A machine `depth` containers deep, the innermost one just opened."""
    m = JsonByteMachine()
    for d in range(depth):
        if kind == "obj" or (kind == "mixed" and d % 3 == 0):
            m.feed(ord("{"))
            if d + 1 < depth:
                for b in b'"k":':
                    m.feed(b)
        else:
            m.feed(ord("["))
    return m


def dead_state():
    return [TR.GUIDED_DEAD] + [0] * (TR.GUIDED_WORDS - 1)


def host_mask(machines, logits):
    """ModelRunner._apply_guided, its own code, on logits [N, V] whose row i
    belongs to a JSON-mode request that stands on machines[i].  In place."""
    reqs = []
    for i, m in enumerate(machines):
        r = Request(request_id=f"g{i}", prompt_token_ids=[1],
                    sampling=SamplingParams(response_format="json"))
        r._guided = m
        reqs.append(r)
    fake = types.SimpleNamespace(_guided_mask_cache={},
                                 _guided_machine=lambda r: r._guided)
    ModelRunner._apply_guided(fake, logits, reqs)


def finite_logits(rows, vocab, seed, dtype=torch.float32):
    """Finite, with both zeros and values that bf16 holds exactly."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, vocab, generator=g) * 4).to(torch.bfloat16)
    x[:, ::37] = 0.0
    x[:, 5::41] = -0.0
    return x.to(dtype)

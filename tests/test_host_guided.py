"""JSON mode through the whole serving plane: REST request -> C++ gateway ->
mux protocol -> engine worker, on a default worker and on one configured
with device_guided.  Requests and responses are the same bytes either way;
only the worker's stepping path differs."""

import json
from pathlib import Path

import pytest

from hyperspot.engine.guided import JsonByteMachine
from hyperspot.sdk import HyperspotClient
from tests.test_host_e2e import _http, BASE
from tests.test_host_logprobs import CPU_WORKER, MSG, _start


@pytest.fixture(scope="module")
def servers(tmp_path_factory):
    """Two CPU servers: the default worker, and one with device_guided."""
    tmp = tmp_path_factory.mktemp("gd")
    started = []
    try:
        started.append(_start(tmp, "plain", "tiny-llama", CPU_WORKER))
        started.append(_start(tmp, "devgd", "tiny-llama",
                              dict(CPU_WORKER, device_guided="true")))
        yield started
    finally:
        for s in started:
            s.stop()


def _chat(srv, **fields):
    body = {"model": "tiny-llama", "messages": MSG, "temperature": 0.0,
            "max_tokens": 48, **fields}
    st, out = _http("POST", BASE.format(srv.port) + "/v1/chat/completions",
                    body, timeout=120)
    assert st == 200, out
    j = json.loads(out)
    for k in ("id", "request_id", "created", "latency_ms", "timing"):
        j.pop(k, None)                 # per-request ids and timings apart
    return j


def _text(j):
    return "".join(p["text"] for p in j["content"] if p["type"] == "text")


def _worker_args(srv):
    """argv of the engine worker the server has spawned."""
    for p in Path("/proc").iterdir():
        if not p.name.isdigit():
            continue
        try:
            stat = (p / "stat").read_text()
            argv = (p / "cmdline").read_bytes().split(b"\0")
        except OSError:
            continue
        ppid = int(stat.rsplit(")", 1)[1].split()[1])
        if ppid == srv.proc.pid and b"hyperspot.serving.worker" in argv:
            return [a.decode() for a in argv]
    raise AssertionError("no worker process under the server")


def test_the_config_key_reaches_the_worker(servers):
    assert "--device-guided" not in _worker_args(servers[0])
    assert "--device-guided" in _worker_args(servers[1])


@pytest.mark.parametrize("fields", [
    dict(),
    dict(max_tokens=200, temperature=1.0, seed=11),
    dict(ignore_eos=True, max_tokens=24),
])
def test_json_request_returns_the_same_from_both_workers(servers, fields):
    a = _chat(servers[0], response_format="json", **fields)
    b = _chat(servers[1], response_format="json", **fields)
    assert a == b                      # content, usage, finish reason if any
    assert _text(a)
    m = JsonByteMachine()
    for byte in _text(b).encode():
        m.feed(byte)                   # a grammar-legal prefix always
    stopped = b["usage"]["output_tokens"] < fields.get("max_tokens", 48)
    if stopped:                        # EOS opens only on a whole document
        assert m.done
        json.loads(_text(b))
    assert stopped != bool(fields.get("ignore_eos"))


def test_sse_json_request_returns_the_same(servers):
    def stream(srv):
        c = HyperspotClient(BASE.format(srv.port))
        chunks = list(c.chat_stream_events(
            MSG, model="tiny-llama", temperature=0.0, max_tokens=32,
            response_format="json"))
        return [ch["delta"].get("content") for ch in chunks[1:-1]], \
            chunks[-1]["finish_reason"]
    assert stream(servers[1]) == stream(servers[0])


def test_request_without_response_format_is_unchanged(servers):
    for fields in (dict(), dict(ignore_eos=True, max_tokens=24),
                   dict(temperature=0.8, seed=5)):
        assert _chat(servers[1], **fields) == _chat(servers[0], **fields)
    # and differs from the JSON-mode reply: the mask did act
    assert _text(_chat(servers[1])) != \
        _text(_chat(servers[1], response_format="json"))


def test_schema_request_returns_the_same(servers):
    """Schema rows keep the synchronous path on either worker."""
    schema = {"type": "object", "properties": {"a": {"type": "integer"}}}
    a = _chat(servers[0], response_schema=schema)
    b = _chat(servers[1], response_schema=schema)
    assert a == b and _text(a).startswith('{"a":')

"""Presence / frequency / repetition penalties through the whole serving
plane: REST request -> C++ gateway -> mux protocol -> engine worker, on a
default worker and on one with device_penalties."""

import json

import pytest

from hyperspot.sdk import HyperspotClient
from tests.test_host_e2e import _http, BASE
from tests.test_host_logprobs import CPU_WORKER, MSG, _start


@pytest.fixture(scope="module")
def servers(tmp_path_factory):
    """Two CPU servers: the default worker, and one with device_penalties."""
    tmp = tmp_path_factory.mktemp("pen")
    started = []
    try:
        started.append(_start(tmp, "plain", "tiny-llama", CPU_WORKER))
        started.append(_start(tmp, "devpen", "tiny-llama",
                              dict(CPU_WORKER, device_penalties="true")))
        yield started
    finally:
        for s in started:
            s.stop()


def _chat(srv, **fields):
    body = {"model": "tiny-llama", "messages": MSG, "temperature": 0.0,
            "max_tokens": 24, "ignore_eos": True, **fields}
    return _http("POST", BASE.format(srv.port) + "/v1/chat/completions",
                 body, timeout=120)


def _stream(srv, **fields):
    c = HyperspotClient(BASE.format(srv.port))
    chunks = list(c.chat_stream_events(
        MSG, model="tiny-llama", temperature=0.0, max_tokens=24,
        ignore_eos=True, **fields))
    assert chunks[-1]["finish_reason"] in ("stop", "length")
    assert chunks[-1]["usage"]["output_tokens"] == 24
    return [ch["delta"]["content"] for ch in chunks[1:-1]
            if "content" in ch["delta"]]


def _ids(srv, **fields):
    """Token ids of a blocking completion (through logprobs.content)."""
    st, body = _chat(srv, logprobs=True, **fields)
    assert st == 200, body
    j = json.loads(body)
    assert j["usage"]["output_tokens"] == 24
    return [e["token_id"] for e in j["logprobs"]["content"]], j


def test_blocking_request_with_a_penalty_differs(servers):
    base, _ = _ids(servers[0])
    pen, _ = _ids(servers[0], frequency_penalty=1.5)
    assert pen != base
    rep, _ = _ids(servers[0], repetition_penalty=1.8, presence_penalty=1.0)
    assert rep != base


def test_sse_request_with_a_penalty_differs(servers):
    base = _stream(servers[0])
    pen = _stream(servers[0], frequency_penalty=1.5)
    assert pen != base
    # the stream and the blocking response are one completion
    st, body = _chat(servers[0], frequency_penalty=1.5)
    assert st == 200, body
    assert json.loads(body)["content"][0]["text"] == "".join(pen)


def test_device_penalties_worker_returns_the_same(servers):
    for fields in (dict(frequency_penalty=1.5),
                   dict(repetition_penalty=1.3, presence_penalty=-0.5),
                   dict()):
        a, ja = _ids(servers[0], **fields)
        b, jb = _ids(servers[1], **fields)
        assert a == b, fields
        assert ja["content"] == jb["content"]
        assert ja["logprobs"] == jb["logprobs"]
    assert _stream(servers[1], frequency_penalty=1.5) == \
        _stream(servers[0], frequency_penalty=1.5)


def test_neutral_values_are_absent_fields(servers):
    for srv in servers:
        st0, b0 = _chat(srv)
        st1, b1 = _chat(srv, presence_penalty=0, frequency_penalty=0.0,
                        repetition_penalty=1.0)
        assert st0 == st1 == 200, (b0, b1)
        j0, j1 = json.loads(b0), json.loads(b1)
        for j in (j0, j1):             # per-request ids and timings apart
            for k in ("id", "request_id", "created", "latency_ms", "timing"):
                j.pop(k, None)
        assert j1 == j0


def test_bad_requests_are_refused(servers):
    for fields in (dict(presence_penalty=2.5), dict(presence_penalty=-3),
                   dict(frequency_penalty=2.0001),
                   dict(frequency_penalty="1"),
                   dict(repetition_penalty=0), dict(repetition_penalty=-1.5),
                   dict(repetition_penalty=True),
                   dict(presence_penalty=[1])):
        for srv in servers:
            st, body = _chat(srv, **fields)
            assert st == 400, (fields, body)
            assert json.loads(body)["code"] == "validation_error"
    # the edges are inside
    st, body = _chat(servers[0], presence_penalty=2, frequency_penalty=-2,
                     repetition_penalty=0.01)
    assert st == 200, body


def test_worker_refuses_what_the_gateway_did_not_see(servers):
    """`params` goes to the worker as it is: its own check answers, as an
    event and not as an exception in the stepping thread, and the worker
    keeps serving."""
    st, body = _chat(servers[0], params={"frequency_penalty": 9})
    assert st != 200, body
    assert "frequency_penalty" in body
    st, body = _chat(servers[0])
    assert st == 200, body


def test_sdk_chat_passes_the_fields(servers):
    c = HyperspotClient(BASE.format(servers[1].port))
    kw = dict(model="tiny-llama", temperature=0.0, max_tokens=24,
              ignore_eos=True)
    base = c.chat(MSG, **kw)
    pen = c.chat(MSG, frequency_penalty=1.5, **kw)
    assert pen["content"] != base["content"]
    assert pen["usage"]["output_tokens"] == 24

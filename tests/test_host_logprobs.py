"""Per-token logprobs through the whole serving plane: REST request ->
C++ gateway -> mux protocol -> engine worker -> `logprobs.content` entries
in the blocking response and beside every SSE content chunk."""

import json
import tempfile
from pathlib import Path

import pytest

from hyperspot.sdk import HyperspotClient
from tests.test_host_e2e import ServerProc, _free_port, _http, BASE

MSG = [{"role": "user", "content": [{"type": "text", "text": "hello"}]}]


def _config(home, port, sock, model, worker):
    lines = "\n".join(f"        {k}: {v}" for k, v in worker.items())
    return f"""
server:
  home_dir: "{home}"
logging:
  default:
    console_level: warn
modules:
  api-gateway:
    config:
      bind_addr: "127.0.0.1:{port}"
      auth_disabled: true
  llm-gateway:
    config:
      model: "{model}"
      worker_socket: "{sock}"
      auto_start_worker: true
      worker:
{lines}
"""


def _start(tmp, name, model, worker, timeout=120):
    home = tmp / name
    home.mkdir()
    port = _free_port()
    cfg_path = home / "cfg.yaml"
    cfg_path.write_text(_config(home, port, tempfile.mktemp(
        suffix=".sock", prefix="hs-lp-"), model, worker))
    srv = ServerProc(cfg_path, port)
    try:
        srv.wait_ready()
        srv.wait_worker(timeout=timeout)
    except Exception:
        srv.stop()
        raise
    return srv


CPU_WORKER = {"device": '"cpu"', "eager": "true", "max_num_seqs": 8,
              "num_gpu_blocks": 256}


@pytest.fixture(scope="module")
def servers(tmp_path_factory):
    """Two CPU servers: the default worker, and one with device_logprobs."""
    tmp = tmp_path_factory.mktemp("lp")
    started = []
    try:
        started.append(_start(tmp, "plain", "tiny-llama", CPU_WORKER))
        started.append(_start(tmp, "devlp", "tiny-llama",
                              dict(CPU_WORKER, device_logprobs="true")))
        yield started
    finally:
        for s in started:
            s.stop()


def _chat(srv, model="tiny-llama", **fields):
    body = {"model": model, "messages": MSG, "temperature": 0.0,
            "max_tokens": 8, "ignore_eos": True, **fields}
    return _http("POST", BASE.format(srv.port) + "/v1/chat/completions",
                 body, timeout=120)


def _check_entries(entries, n_tokens, n_top, greedy=True):
    assert len(entries) == n_tokens
    for e in entries:
        assert set(e) == {"token", "token_id", "bytes", "logprob",
                          "top_logprobs"}
        assert e["logprob"] <= 0.0
        top = e["top_logprobs"]
        assert len(top) == n_top
        lps = [t["logprob"] for t in top]
        assert lps == sorted(lps, reverse=True)
        if greedy and n_top:
            assert e["token_id"] == top[0]["token_id"]
            assert e["logprob"] == top[0]["logprob"]
        for t in [e] + top:
            tid = t["token_id"]
            assert t["bytes"] == ([tid - 4] if 4 <= tid < 260 else [])
            want = chr(tid - 4) if 4 <= tid < 4 + 0x80 else ""
            assert t["token"] == want


def _text_of(entries):
    """The content text from the entries alone: the UTF-8 of the
    concatenated `bytes`, a token outside the byte range (the random
    tiny model emits them) showing as <id>, BOS / EOS as nothing."""
    text, run = "", b""
    for e in entries:
        if e["bytes"]:
            run += bytes(e["bytes"])
            continue
        text += run.decode("utf-8", errors="replace")
        run = b""
        if e["token_id"] not in (1, 2):
            text += f"<{e['token_id']}>"
    return text + run.decode("utf-8", errors="replace")


def test_blocking_completion_carries_one_entry_per_token(servers):
    st, body = _chat(servers[0], logprobs=True, top_logprobs=3)
    assert st == 200, body
    j = json.loads(body)
    assert j["usage"]["output_tokens"] == 8
    entries = j["logprobs"]["content"]
    _check_entries(entries, 8, 3)
    assert _text_of(entries) == j["content"][0]["text"]
    # logprobs without alternatives
    st, body = _chat(servers[0], logprobs=True)
    assert st == 200, body
    _check_entries(json.loads(body)["logprobs"]["content"], 8, 0)


def test_sse_chunks_carry_one_entry_each(servers):
    c = HyperspotClient(BASE.format(servers[0].port))
    chunks = list(c.chat_stream_events(
        MSG, model="tiny-llama", temperature=0.0, max_tokens=8,
        ignore_eos=True, logprobs=True, top_logprobs=3))
    assert chunks[0]["delta"].get("role") == "assistant"
    final = chunks[-1]
    assert final["finish_reason"] in ("stop", "length")
    content = [ch for ch in chunks[1:-1] if "content" in ch["delta"]]
    assert len(content) == final["usage"]["output_tokens"] == 8
    entries = []
    for ch in content:
        assert len(ch["logprobs"]["content"]) == 1
        entries.append(ch["logprobs"]["content"][0])
    _check_entries(entries, 8, 3)
    assert "logprobs" not in chunks[0] and "logprobs" not in final
    # the stream and the blocking response report the same records
    st, body = _chat(servers[0], logprobs=True, top_logprobs=3)
    assert json.loads(body)["logprobs"]["content"] == entries


def test_bad_requests_are_refused(servers):
    for fields in (dict(logprobs=True, top_logprobs=21),
                   dict(logprobs=True, top_logprobs=-1),
                   dict(top_logprobs=2),
                   dict(logprobs=False, top_logprobs=2)):
        st, body = _chat(servers[0], **fields)
        assert st == 400, (fields, body)
        assert json.loads(body)["code"] == "validation_error"


def test_request_without_the_fields_has_no_logprobs_key(servers):
    st, body = _chat(servers[0])
    assert st == 200, body
    assert "logprobs" not in json.loads(body)
    c = HyperspotClient(BASE.format(servers[0].port))
    chunks = list(c.chat_stream_events(MSG, model="tiny-llama",
                                       temperature=0.0, max_tokens=4))
    assert chunks and all("logprobs" not in ch for ch in chunks)


def test_device_logprobs_worker_returns_the_same_entries(servers):
    st0, b0 = _chat(servers[0], logprobs=True, top_logprobs=3)
    st1, b1 = _chat(servers[1], logprobs=True, top_logprobs=3)
    assert st0 == st1 == 200, (b0, b1)
    j0, j1 = json.loads(b0), json.loads(b1)
    assert j1["content"] == j0["content"]
    assert j1["logprobs"] == j0["logprobs"]


@pytest.mark.gpu
def test_rest_logprobs_on_gpu(tmp_path):
    import torch
    assert torch.cuda.is_available()
    srv = _start(tmp_path, "gpu", "tiny-llama-d128",
                 {"max_num_seqs": 8, "num_gpu_blocks": 512,
                  "device_logprobs": "true", "device_sampling": "true"},
                 timeout=300)
    try:
        st, body = _chat(srv, model="tiny-llama-d128", logprobs=True,
                         top_logprobs=5)
        assert st == 200, body
        j = json.loads(body)
        _check_entries(j["logprobs"]["content"], 8, 5)
        c = HyperspotClient(BASE.format(srv.port))
        chunks = list(c.chat_stream_events(
            MSG, model="tiny-llama-d128", temperature=0.8, seed=3,
            max_tokens=8, ignore_eos=True, logprobs=True, top_logprobs=5))
        content = [ch for ch in chunks[1:-1] if "content" in ch["delta"]]
        assert len(content) == chunks[-1]["usage"]["output_tokens"] == 8
        _check_entries([ch["logprobs"]["content"][0] for ch in content],
                       8, 5, greedy=False)
    finally:
        srv.stop()

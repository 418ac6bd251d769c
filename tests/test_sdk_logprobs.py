"""HyperspotClient.chat_stream_events: the parsed SSE chunks, logprobs
included; chat_stream keeps yielding the content strings."""

import contextlib
import json

from hyperspot.sdk import HyperspotClient


def _entry(tid, lp):
    return {"token": chr(tid - 4), "token_id": tid, "bytes": [tid - 4],
            "logprob": lp, "top_logprobs": [
                {"token": chr(tid - 4), "token_id": tid, "bytes": [tid - 4],
                 "logprob": lp}]}


CHUNKS = [
    {"id": "c", "model": "m", "delta": {"role": "assistant"}},
    {"id": "c", "model": "m", "delta": {"content": "h"},
     "logprobs": {"content": [_entry(108, -0.25)]}},
    {"id": "c", "model": "m", "delta": {"content": ""},
     "logprobs": {"content": [_entry(109, -1.5)]}},
    {"id": "c", "model": "m", "delta": {"content": "i"},
     "logprobs": {"content": [_entry(110, -0.5)]}},
    {"id": "c", "model": "m", "delta": {}, "finish_reason": "length",
     "usage": {"input_tokens": 5, "output_tokens": 3}},
]


def _client(monkeypatch, seen):
    c = HyperspotClient("http://127.0.0.1:1", model="m")
    feed = []
    for ch in CHUNKS:
        feed += [b"data: " + json.dumps(ch).encode() + b"\n", b"\n"]
    feed += [b"data: [DONE]\n", b"\n", b"data: {\"late\": 1}\n", b"\n"]

    @contextlib.contextmanager
    def fake_req(method, path, body=None, stream=False, **kw):
        seen.append((method, path, body, stream))
        yield iter(feed)

    monkeypatch.setattr(c, "_req", fake_req)
    return c


def test_chat_stream_events_yields_parsed_chunks(monkeypatch):
    seen = []
    c = _client(monkeypatch, seen)
    evs = list(c.chat_stream_events([{"role": "user", "content": "x"}],
                                    logprobs=True, top_logprobs=1,
                                    max_tokens=3))
    assert evs == CHUNKS                       # [DONE] ends the stream
    method, path, body, stream = seen[0]
    assert (method, path, stream) == ("POST", "/v1/chat/completions", True)
    assert body["stream"] is True and body["logprobs"] is True
    assert body["top_logprobs"] == 1 and body["max_tokens"] == 3
    entries = [e for ev in evs for e in
               ev.get("logprobs", {}).get("content", [])]
    assert [e["token_id"] for e in entries] == [108, 109, 110]
    assert len(entries) == evs[-1]["usage"]["output_tokens"]


def test_chat_stream_still_yields_strings(monkeypatch):
    c = _client(monkeypatch, [])
    assert list(c.chat_stream([{"role": "user", "content": "x"}])) == \
        ["h", "i"]

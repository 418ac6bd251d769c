"""The device form of JSON-mode guided decoding on the CPU: pack / unpack of
JsonByteMachine and the torch twins of csrc/guided.hip (ops.guided_json_mask,
ops.guided_json_advance) against the host machine, over every prefix of a
corpus of JSON documents.

Everything is exact: the state is integers and the mask either keeps a
logit's value or makes it -inf.  Logits are finite and are compared by value
(torch.equal): _apply_guided adds 0.0, which turns -0.0 into +0.0."""

import copy
import importlib.util
import json
import pathlib

import pytest
import torch

from hyperspot import ops
from hyperspot.engine.guided import JsonByteMachine
from hyperspot.ops import torch_ref as TR

_spec = importlib.util.spec_from_file_location(
    "guided_ref", pathlib.Path(__file__).with_name("guided_ref.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

W = TR.GUIDED_WORDS
V = 264


def _state(rows):
    return torch.tensor(rows, dtype=torch.int32).view(-1, W)


def test_corpus_is_json_and_covers_every_mode_in_every_context():
    for doc in G.corpus():
        json.loads(doc.decode("utf-8"))
    seen = {(m.mode, m.stack[-1] if m.stack else None)
            for m, _, _ in G.walk()}
    everywhere = ("value", "string", "escape", "hex", "lit", "num_minus",
                  "num_zero", "num_int", "num_dot", "num_frac", "num_esign",
                  "num_e", "num_exp", "end")
    want = {(m, top) for m in everywhere for top in (None, "arr", "obj")}
    want |= {("value_first", "arr"), ("key", "obj"), ("key_first", "obj"),
             ("colon", "obj")}
    assert seen == want
    # and these are all the modes allowed() knows, each with a number
    assert {m for m, _ in want} == set(TR.GUIDED_MODES)
    assert TR.GUIDED_DEAD == len(TR.GUIDED_MODES) and W == 11


def test_pack_unpack_round_trip_at_every_prefix():
    for m, _, _ in G.walk():
        words = m.pack()
        assert len(words) == W
        assert all(-2 ** 31 <= w < 2 ** 31 for w in words) and words[0] >= 0
        u = JsonByteMachine.unpack(words)
        assert u.mask_key() == m.mask_key()
        assert u.allowed() == m.allowed()
        assert (u.stack, u.mode, bytes(u.lit), u.in_key, u.hex_left) == \
            (m.stack, m.mode, bytes(m.lit), m.in_key, m.hex_left)
        assert u.pack() == words


def test_twin_mask_is_the_host_mask_at_every_prefix():
    states = G.distinct_states()
    n = len(states)
    assert n > 150
    base = G.finite_logits(n, V, seed=1)
    want = base.clone()
    G.host_mask([copy.deepcopy(m) for _, m in states], want)
    got = base.clone()
    ops.guided_json_mask(got, _state([w for w, _ in states]))
    assert torch.equal(got, want)
    # what survives is allowed() and has its value; EOS only when done
    for i, (_, m) in enumerate(states):
        ok, eos = m.allowed()
        keep = sorted(b + 4 for b in ok) + ([2] if eos else [])
        assert torch.nonzero(got[i] > float("-inf")).flatten().tolist() \
            == sorted(keep)
        assert eos == m.done
        assert torch.equal(got[i, keep], base[i, keep])


def test_twin_advance_is_feed_at_every_prefix():
    steps = G.distinct_steps()
    assert len(steps) > 300
    st = _state([s for s, _, _ in steps])
    ops.guided_json_advance(st, torch.tensor([t for _, t, _ in steps]))
    assert torch.equal(st, _state([a for _, _, a in steps]))


def test_whole_documents_through_the_twins():
    """Mask, pick the document's byte, advance: the byte is always allowed
    and the state ends done, EOS open."""
    docs = G.corpus()[::7]
    st = _state([JsonByteMachine().pack() for _ in docs])
    for pos in range(max(len(d) for d in docs) + 1):
        lg = torch.zeros(len(docs), V)
        ops.guided_json_mask(lg, st)
        tok = torch.tensor([d[pos] + 4 if pos < len(d) else 2 for d in docs])
        assert bool((lg[torch.arange(len(docs)), tok] == 0).all()), pos
        ops.guided_json_advance(st, tok)
    for row in st.tolist():
        assert JsonByteMachine.unpack(row).done


def test_depth_cap():
    cap = TR.GUIDED_MAX_DEPTH
    assert cap == 256
    for kind in ("arr", "obj", "mixed"):
        for depth in (cap - 1, cap):
            m = G.nested(depth, kind)
            words = m.pack()
            assert words[2] == depth
            assert JsonByteMachine.unpack(words).stack == m.stack
            lg = G.finite_logits(1, V, seed=depth)
            want = lg.clone()
            G.host_mask([copy.deepcopy(m)], want)
            ops.guided_json_mask(lg, _state(words))
            opens = [ord("{") + 4, ord("[") + 4]
            value = m.mode in ("value", "value_first")
            if depth < cap or not value:
                assert torch.equal(lg, want)         # the host's mask
                if value:
                    assert bool(torch.isfinite(lg[0, opens]).all())
            else:
                # the one difference: no deeper; everything else as the host
                assert bool((lg[0, opens] == float("-inf")).all())
                assert bool(torch.isfinite(want[0, opens]).all())
                lg[0, opens] = want[0, opens]
                assert torch.equal(lg, want)
    # mode "value" at the cap (behind a comma): the same
    m = G.nested(cap)
    for b in b"1,":
        m.feed(b)
    lg = torch.zeros(1, V)
    ops.guided_json_mask(lg, _state(m.pack()))
    ok = {b for b in m.allowed()[0]} - set(b"{[")
    assert torch.nonzero(lg[0] == 0).flatten().tolist() == \
        sorted(b + 4 for b in ok)
    # closing from the cap works and the stack bits go back to zero
    m = G.nested(cap, "mixed")
    st = _state(m.pack())
    while m.stack:
        b = ord("]") if m.stack[-1] == "arr" else ord("}")
        m.feed(b)
        ops.guided_json_advance(st, torch.tensor([b + 4]))
        assert st[0].tolist() == m.pack()
    assert st[0, 2:].tolist() == [0] * (W - 2) and m.done
    # deeper than the cap does not pack
    with pytest.raises(ValueError):
        G.nested(cap + 1).pack()


def test_dead_mode():
    dead = G.dead_state()
    lg = G.finite_logits(1, V, seed=3)
    base = lg.clone()
    ops.guided_json_mask(lg, _state(dead))
    assert torch.nonzero(lg[0] > float("-inf")).flatten().tolist() == [2]
    assert lg[0, 2] == base[0, 2]
    # sticky under every byte, and entered on a byte the state refuses
    st = _state([dead] * 256)
    ops.guided_json_advance(st, torch.arange(256) + 4)
    assert torch.equal(st, _state([dead] * 256))
    for m, refused in ((JsonByteMachine(), ord("}")),
                       (G.nested(1, "obj"), ord("1")),
                       (G.nested(TR.GUIDED_MAX_DEPTH), ord("["))):
        st = _state(m.pack())
        ops.guided_json_advance(st, torch.tensor([refused + 4]))
        assert st[0, 0] == TR.GUIDED_DEAD
    with pytest.raises(ValueError):
        JsonByteMachine.unpack(dead)
    # words no machine packs read as DEAD instead of indexing anywhere
    for bad in ([99] + [0] * 10, [0, 0, 257] + [0] * 8, [0, 0, -5] + [0] * 8,
                [17, 0, 2 ** 31 - 1] + [-1] * 8, [8, 0, 0] + [0] * 8,
                [8, (3 << 4) | (7 << 6), 0] + [0] * 8):
        lg = torch.zeros(1, V)
        ops.guided_json_mask(lg, _state(bad))
        assert torch.nonzero(lg[0] == 0).flatten().tolist() == [2], bad
        st = _state(bad)
        ops.guided_json_advance(st, torch.tensor([ord("1") + 4]))
        assert st[0, 0] == TR.GUIDED_DEAD


def test_tokens_outside_the_bytes_are_ignored():
    states = [w for w, _ in G.distinct_states()][::5]
    for tok in (0, 1, 2, 3, 260, 261, 511, 128255, 1 << 40, -1):
        st = _state(states)
        ops.guided_json_advance(st, torch.full((len(states),), tok))
        assert torch.equal(st, _state(states))


def test_unguided_rows_are_untouched():
    states = [w for w, _ in G.distinct_states()][:6]
    rows = []
    for i, w in enumerate(states):
        rows += [w, [-1] * W, [-1 - i] + [12345] * (W - 1)]
    st = _state(rows)
    lg = G.finite_logits(len(rows), V, seed=4)
    lg[1, 7] = float("nan")
    lg[2, 9] = float("inf")
    before = lg.clone()
    ops.guided_json_mask(lg, st)
    un = (st[:, 0] < 0)
    assert before[un].view(torch.int32).equal(lg[un].view(torch.int32))
    assert not torch.equal(lg[~un], before[~un])
    # a state tensor longer than the batch: the rows past it are not read
    short = before[:2].clone()
    ops.guided_json_mask(short, st)
    assert torch.equal(short[0], lg[0])
    ops.guided_json_advance(st, torch.full((len(rows),), ord("1") + 4))
    assert torch.equal(st[un], _state(rows)[un])
    assert not torch.equal(st[~un], _state(rows)[~un])


def test_small_vocabulary_is_refused():
    st = _state(JsonByteMachine().pack())
    for vocab in (259, 64):
        with pytest.raises(ValueError, match="260"):
            ops.guided_json_mask(torch.zeros(1, vocab), st)
        with pytest.raises(ValueError, match="260"):
            TR.guided_json_mask(torch.zeros(1, vocab), st)
    ops.guided_json_mask(torch.zeros(1, 260), st)

"""Memcached sessions without a GPU: the C-ABI entry points are exported, a
host-only engine answers hipErrorNoDevice for each of them and stays usable,
and the Python model the GPU tests compare against (tests/mc_sessions_py.py)
reproduces the reference's 31 recorded op sequences
(tests/golden/reference_kats.json "memcache_ops") -- ops, results and injected
bytes -- and the points of the parsers that are easy to get wrong."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np

import cilium_amd
from cilium_amd import _lib, gen
import mc_sessions_py as model
from mc_sessions_py import MORE, PASS, DROP, INJECT, ERROR, OK, PARSER_ERROR, ALLOW, DENY

HIP_ERROR_NO_DEVICE = 100

SYMBOLS = ("l7g_mc_sessions_enable", "l7g_mc_forward", "l7g_mc_replies", "l7g_mc_forward_host", "l7g_mc_replies_host",
           "l7g_mc_session_reset", "l7g_mc_session_stats", "l7g_mc_denied_message")
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_kats.json")


def test_session_symbols_exported():
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(rf"\bT {name}\b", out), name
        assert name in _lib.EXPORTS


def test_denied_messages_live_once():
    assert _lib.mc_denied_message(False) == model.DENIED_TEXT and len(model.DENIED_TEXT) == 28
    assert _lib.mc_denied_message(True) == model.DENIED_BINARY and len(model.DENIED_BINARY) == 37
    assert _lib.MC_SESS_WINDOW == 64
    # the other templates are where they were
    assert _lib.deny_reply_template(_lib.PROTO_R2D2) == b"ERROR\r\n"


def test_host_only_engine_answers_no_device():
    e = cilium_amd.Engine(-1)
    try:
        e.mc_sessions(64)
    except RuntimeError as ex:
        assert f"HIP error {HIP_ERROR_NO_DEVICE}" in str(ex), ex
    else:
        raise AssertionError("a host-only engine enabled sessions")
    L, h = e._lib, e._h
    arena = np.frombuffer(b"get a\r\n" + bytes(9), np.uint8).copy()
    off, ln, conn = np.zeros(1, np.uint64), np.full(1, 7, np.uint32), np.zeros(1, np.uint32)
    verdict, act = np.ones(1, np.uint8), np.zeros(1, np.uint8)
    kind, opn, aux = np.zeros(4, np.uint8), np.zeros(4, np.uint32), np.zeros(4, np.uint64)
    nops, res, taken = np.zeros(1, np.uint32), np.zeros(1, np.uint8), np.zeros(1, np.uint64)
    p = lambda a: a.ctypes.data
    assert L.l7g_mc_sessions_enable(h, 0, None, 0) == HIP_ERROR_NO_DEVICE
    for host in (False, True):
        fwd = L.l7g_mc_forward_host if host else L.l7g_mc_forward
        rep = L.l7g_mc_replies_host if host else L.l7g_mc_replies
        tail = () if host else (None,)
        assert fwd(h, p(arena), 7, p(off), p(ln), p(conn), p(verdict), None, 1, p(act), *tail) == HIP_ERROR_NO_DEVICE
        assert fwd(h, p(arena), 7, p(off), p(ln), p(conn), p(verdict), None, 0, p(act), *tail) == HIP_ERROR_NO_DEVICE
        assert rep(h, p(arena), 7, p(off), p(ln), p(conn), 1, 4, p(kind), p(opn), p(aux), p(nops), p(res), p(taken),
                   *tail) == HIP_ERROR_NO_DEVICE
    assert L.l7g_mc_session_reset(h, p(conn), 1) == HIP_ERROR_NO_DEVICE
    assert e.mc_session_stats() == dict.fromkeys(e.MC_SESSION_STATS, 0)
    assert len(e.MC_SESSION_STATS) == 8 and e.MC_SESSION_STATS == model.Sessions.STATS
    # still a working rule compiler
    e.update_policy(gen.mc_policy())
    e.set_connections(gen.make_conns(2, 0, gen.MC_PORT, True, gen.PROTO_MEMCACHE, [3005, 7]))
    assert e.nrules > 0
    e.close()


# ---------------------------------------------------------------- the reference's op sequences

def one_conn(flags=0, cap=64):
    conns = gen.make_conns(1, 0, gen.MC_PORT, True, gen.PROTO_MEMCACHE, [3005])
    conns["flags"] = flags
    return model.Sessions(conns, cap)


def golden_request_frames(call):
    """The frames and verdicts of a recorded request call, read off its PASS / DROP ops."""
    data = b"".join(bytes.fromhex(b) for b in call["data"])
    frames, verdicts, at = [], [], 0
    for op, n in call["ops"]:
        if op in (PASS, DROP):
            frames.append(data[at:at + n])
            verdicts.append(ALLOW if op == PASS else DENY)
            at += n
    return frames, verdicts


def replay_golden(forward, replies):
    """The 31 sequences through forward(frames, verdicts) -> (act, injected
    bytes) and replies(data, max_ops) -> (ops [(kind, n)], result, injected).
    The recording's "inject" is what the reference's test compares its inject
    buffer with after the call (helpers_test.go:52-144): the buffer holds
    "inject_buf" bytes at most and must equal the expectation's prefix of its
    own length -- so a message still queued after a request call shows as an
    empty buffer against the expectation of the reply call that sends it."""
    doc = json.load(open(KATS))["memcache_ops"]
    calls, buf_cap = doc["calls"], doc["connection"]["inject_buf"]
    assert len(calls) == 31 and buf_cap == 30
    sent = 0
    seen_reply_calls = 0
    for name, seq in calls.items():
        fwd, rep = forward(name), replies(name)
        for k in seq:
            want_inj = bytes.fromhex(k["inject"])
            if not k["reply"]:
                frames, verdicts = golden_request_frames(k)
                act, inj = fwd(frames, verdicts)
                # PASS / DROP from the acts, as a caller would rebuild them
                got = [(PASS if a in (1, 2) else DROP, len(f)) for a, f in zip(act, frames)]
                assert got == [tuple(o) for o in k["ops"] if o[0] in (PASS, DROP)], (name, k, act)
                assert all(a in ((1, 2) if v == ALLOW else (3, 4, 5)) for a, v in zip(act, verdicts)), (name, act)
                assert inj[:buf_cap] == want_inj[:len(inj[:buf_cap])], (name, k, inj)
                assert k["result"] == "OK"
                sent += len(inj)
            else:
                seen_reply_calls += 1
                data = b"".join(bytes.fromhex(b) for b in k["data"])
                ops, result, inj = rep(data, 1 + 2 * len(k["ops"]))
                assert ops == [tuple(o) for o in k["ops"]], (name, k, ops)
                assert result == (OK if k["result"] == "OK" else PARSER_ERROR), (name, k, result)
                assert inj[:buf_cap] == want_inj[:len(inj[:buf_cap])], (name, k, inj)
                assert len(inj) == sum(n for o, n in ops if o == INJECT), (name, k)
                sent += len(inj)
    assert seen_reply_calls >= 5 and sent > 0


def test_model_reproduces_the_reference_sequences():
    state = {}

    def forward(name):
        state[name] = one_conn()

        def f(frames, verdicts):
            act, inj = state[name].forward(frames, [0] * len(frames), verdicts)
            return act.tolist(), b"".join(inj)
        return f

    def replies(name):
        def r(data, max_ops):
            ops, result, _, inj = state[name].replies([data], [0], max_ops)[0]
            return [(o, n) for o, n, _ in ops], result, inj
        return r

    replay_golden(forward, replies)


# ---------------------------------------------------------------- directed cases

def text_session(requests, cap=64):
    """A text connection after `requests` [(line, verdict)]; -> (sessions, acts)."""
    s = one_conn(cap=cap)
    act, _ = s.forward([r for r, _ in requests], [0] * len(requests), [v for _, v in requests],
                       tags=list(range(100, 100 + len(requests))))
    return s, act.tolist()


def run(s, data, max_ops=8):
    ops, result, taken, inj = s.replies([data], [0], max_ops)[0]
    return ops, result, taken, inj


def test_end_miss_waits_for_the_next_end():
    s, act = text_session([(b"get a\r\n", ALLOW), (b"get b\r\n", ALLOW)])
    assert act == [1, 1]
    assert run(s, b"END\r\n") == ([(MORE, 1, 0)], OK, 0, b"")   # bytes.Index > 0: a hit at 0 does not count
    # ... and passes together with what follows, up to the next END
    two = b"END\r\nVALUE b 0 1\r\nx\r\nEND\r\n"
    assert run(s, two) == ([(PASS, len(two), 100)], OK, len(two), b"")
    assert s.stats()["queued"] == 1


def test_blank_reply_line_and_empty_queue_panic():
    s, _ = text_session([(b"delete a\r\n", ALLOW)])
    assert run(s, b"\r\nDELETED\r\n") == ([], PARSER_ERROR, 0, b"")          # tokens[0] of a blank line
    assert run(s, b" \t \r\n") == ([], PARSER_ERROR, 0, b"")                   # ... of an all-space line
    assert run(s, b"DELETED\r\nDELETED\r\n") == ([(PASS, 9, 100)], PARSER_ERROR, 9, b"")   # replyQueue[0], queue empty
    e = one_conn(flags=1)
    assert run(e, b"STORED") == ([(MORE, 2, 0)], OK, 0, b"")                   # no CRLF comes before the queue
    assert run(e, b"STORED\r") == ([(MORE, 1, 0)], OK, 0, b"")
    assert run(e, b"STORED\r\n") == ([], PARSER_ERROR, 0, b"")
    assert run(e, b"") == ([], OK, 0, b"")
    assert e.stats()["errors"] == 1


def test_watch_passes_lines_and_pops_nothing():
    for verdict in (ALLOW, DENY):
        s, act = text_session([(b"get a\r\n", ALLOW), (b"watch fetchers\r\n", verdict)])
        assert act == [1, 1 if verdict == ALLOW else 4]
        lines = b"OK\r\nts=1 gid=2\r\n\r\nEND\r\n"
        ops, result, taken, _ = run(s, lines)
        assert ops == [(PASS, 4, 0), (PASS, 12, 0), (PASS, 2, 0), (PASS, 5, 0)] and result == OK and taken == 23
        assert s.stats()["queued"] == 2
    # watching with an empty queue still panics first
    s, act = text_session([(b"watch\r\n", DENY)])
    assert act == [3] and run(s, b"OK\r\n")[1] == PARSER_ERROR


def test_error_lines_are_one_line_for_every_class():
    for req in (b"get a\r\n", b"gats 1 a\r\n", b"stats\r\n", b"lru_crawler metadump all\r\n", b"set a 0 0 1\r\n",
                b"version\r\n", b"verbosity 1\r\n"):
        for err in (b"ERROR\r\n", b"CLIENT_ERROR bad data chunk\r\n", b"SERVER_ERROR out of memory\r\n"):
            s, _ = text_session([(req, ALLOW)])
            assert run(s, err + b"END\r\n")[0][0] == (PASS, len(err), 100), (req, err)
    # a class without a rule: ERROR, 0
    s, _ = text_session([(b"verbosity 1\r\n", ALLOW)])
    assert run(s, b"OK\r\n") == ([], PARSER_ERROR, 0, b"")


def test_lru_crawler_both_ways():
    for word in (b"OK", b"BUSY currently processing", b"BADCLASS invalid class id"):
        s, _ = text_session([(b"lru_crawler crawl 1\r\n", ALLOW)])
        assert run(s, word + b"\r\nEND\r\n")[0][0] == (PASS, len(word) + 2, 100)
    s, _ = text_session([(b"lru_crawler metadump all\r\n", ALLOW)])
    dump = b"key=a exp=-1\r\nkey=b exp=-1\r\nEND\r\n"
    assert run(s, dump[:20]) == ([(MORE, 1, 0)], OK, 0, b"")
    assert run(s, dump) == ([(PASS, len(dump), 100)], OK, len(dump), b"")


def test_noreply_forms_and_denied_order():
    reqs = [(b"set a 0 0 1 noreply\r\n", ALLOW), (b"cas a 0 0 1 5 noreply\r\n", DENY), (b"delete a noreply\r\n", ALLOW),
            (b"incr a 1 noreply\r\n", DENY), (b"touch a 1 noreply\r\n", ALLOW), (b"flush_all noreply\r\n", DENY),
            (b"cache_memlimit 5 noreply\r\n", ALLOW), (b"quit\r\n", ALLOW),
            (b"flush_all 0\r\n", DENY),                 # reply owed, queue empty: now
            (b"get\xe2\x80\x83a\xc2\xa0\r\n", ALLOW),   # multi-byte White_Space separators
            (b"delete b\r\n", DENY), (b"delete c\r\n", DENY), (b"set d 0 0 1\r\n", ALLOW)]
    s, act = text_session(reqs)
    assert act == [2, 5, 2, 5, 2, 5, 2, 2, 3, 1, 4, 4, 1]
    assert [q[0] for q in s.parsers[0].reply_queue] == [b"get", b"delete", b"delete", b"set"]
    # the two denied ones leave once the get's reply has passed: in the same call, before the next frame
    ops, result, taken, inj = run(s, b"END\r\nEND\r\nSTORED\r\n")
    assert ops == [(PASS, 10, 109), (INJECT, 56, 0), (PASS, 8, 112)] and result == OK and taken == 18
    assert inj == model.DENIED_TEXT * 2


def test_binary_double_append_and_the_stuck_queue():
    conns = one_conn()
    b = lambda magic=0x80: bytes([magic, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1]) + bytes(12) + b"k"
    act, inj = conns.forward([b(), b(), b()], [0, 0, 0], [ALLOW, DENY, DENY])
    p = conns.parsers[0]
    assert act.tolist() == [1, 4, 4] and inj == [b"", b"", b""]
    assert p.inject_queue == [(0x81, 2), (0x81, 2), (0x81, 3), (0x81, 3)] and (p.request_count, p.reply_count) == (3, 0)
    reply = bytes([0x81, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]) + bytes(12)
    ops, result, taken, inj = run(conns, reply)
    assert ops == [(PASS, 24, 0), (INJECT, 37, 0x81)] and inj == model.DENIED_BINARY
    # the second copy of request 2 heads the queue now: request 3's message is never sent
    assert p.inject_queue[0] == (0x81, 2) and p.reply_count == 2
    assert run(conns, b"") == ([], OK, 0, b"")
    assert run(conns, reply + reply)[0] == [(PASS, 24, 0), (PASS, 24, 0)]


def test_unsolicited_binary_reply_then_deny():
    conns = one_conn(flags=2)
    reply = bytes([0x81, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2]) + bytes(12) + b"xy"
    assert run(conns, reply) == ([(PASS, 26, 0)], OK, 26, b"")              # replyCount 1, requestCount 0
    req = bytes([0x80, 0, 0, 0]) + bytes(20)
    act, inj = conns.forward([req, req, req], [0, 0, 0], [DENY, DENY, DENY])
    # request 1: 1 != 1 + 1, queued twice (and can never fire); request 2 == replyCount + 1: now; request 3 too
    assert act.tolist() == [4, 3, 3]
    assert inj[1] == model.DENIED_BINARY and inj[1] == inj[2]
    assert conns.parsers[0].inject_queue[0] == (0x81, 1) and conns.parsers[0].reply_count == 3


def test_binary_error_fills_the_ops_and_short_frames():
    conns = one_conn(flags=2)
    bad = bytes([0x01, 0, 0, 0]) + bytes(20)
    assert run(conns, bad, max_ops=5) == ([(ERROR, 2, 0)] * 5, OK, 0, b"")
    assert run(conns, bad[:10]) == ([(MORE, 14, 0)], OK, 0, b"")            # short header first
    keyed = bytes([0x01, 0, 0, 9, 2, 0, 0, 0]) + bytes(16)
    assert run(conns, keyed) == ([(MORE, 11, 0)], OK, 0, b"")               # then the missing key bytes
    good = bytes([0x81, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 100]) + bytes(12)
    assert run(conns, good + bad, max_ops=3) == ([(PASS, 124, 0)], OK, 124, b"")   # a PASS past the bytes present


def test_max_ops_continues_from_taken():
    reqs = [(b"get k%d\r\n" % i, ALLOW) if i % 3 else (b"delete k%d\r\n" % i, DENY if i % 2 else ALLOW)
            for i in range(1, 41)]
    stream = b"".join(b"VALUE k 0 1\r\nx\r\nEND\r\n" if r.startswith(b"get") else b"DELETED\r\n"
                      for r, v in reqs if v == ALLOW)
    whole, _ = text_session(reqs)
    want = run(whole, stream, max_ops=200)
    for max_ops in (1, 3):
        s, _ = text_session(reqs)
        ops, at = [], 0
        while True:
            o, result, taken, _ = run(s, stream[at:], max_ops=max_ops)
            assert result == OK
            ops += o
            at += taken
            if len(o) < max_ops:
                break
        assert ops == want[0] and at == want[2]


def test_ring_capacity_in_the_model():
    s, act = text_session([(b"get a\r\n", ALLOW)] * 3 + [(b"delete a\r\n", DENY), (b"set a 0 0 1 noreply\r\n", ALLOW),
                                                         (b"get b\r\n", ALLOW), (b"get c\r\n", ALLOW)], cap=4)
    assert act == [1, 1, 1, 4, 2, 6, 6]
    assert s.stats()["full"] == 2 and s.stats()["queued"] == 4

"""Kafka sessions without a GPU: the C-ABI entry points are exported, a
host-only engine refuses to keep sessions and stays usable, the script
generator is deterministic and produces every kind of frame it promises, and
the Python model the GPU tests compare against (tests/kafka_sessions_py.py)
agrees with the host correlation cache (_lib.KafkaCorrelationCache) and with
the reference's own test vectors (tests/golden/kafka_correlation_kats.json)."""
import json
import os
import re
import subprocess

import numpy as np

import cilium_amd
from cilium_amd import _lib, gen
import kafka_sessions_py as model

HIP_ERROR_NO_DEVICE = 100

SYMBOLS = ("l7g_kafka_sessions_enable", "l7g_kafka_forward", "l7g_kafka_responses", "l7g_kafka_forward_host",
           "l7g_kafka_responses_host", "l7g_kafka_session_gc", "l7g_kafka_session_reset", "l7g_kafka_session_stats")
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kafka_correlation_kats.json")


def test_session_symbols_exported():
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(rf"\bT {name}\b", out), name
        assert name in _lib.EXPORTS


def test_host_only_engine_refuses_sessions():
    e = cilium_amd.Engine(-1)
    try:
        e.kafka_sessions(1024)
    except RuntimeError as ex:
        assert f"HIP error {HIP_ERROR_NO_DEVICE}" in str(ex), ex
    else:
        raise AssertionError("a host-only engine enabled sessions")
    assert e.kafka_session_stats() == dict.fromkeys(e.KAFKA_SESSION_STATS, 0)
    assert len(e.KAFKA_SESSION_STATS) == 7
    # still a working rule compiler
    e.update_policy(gen.cfg3_policy())
    e.set_connections(gen.make_conns(2, 0, 9092, True, gen.PROTO_KAFKA, [100, 7]))
    assert e.nrules > 0
    e.close()


def _same_script(a, b):
    return (np.array_equal(a[0], b[0]) and a[1] == b[1] and len(a[2]) == len(b[2]) and all(
        ra["requests"] == rb["requests"] and ra["responses"] == rb["responses"] and ra["now_ms"] == rb["now_ms"]
        and all(np.array_equal(ra[k], rb[k]) for k in ("req_conn", "rep_conn", "verdict", "tags"))
        for ra, rb in zip(a[2], b[2])))


def test_script_is_deterministic():
    a = gen.kafka_session_script(nconns=16, rounds=4, nreq=64, nrep=24, seed=77)
    b = gen.kafka_session_script(nconns=16, rounds=4, nreq=64, nrep=24, seed=77)
    c = gen.kafka_session_script(nconns=16, rounds=4, nreq=64, nrep=24, seed=78)
    assert _same_script(a, b) and not _same_script(a, c)
    d1, d2 = gen.kafka_session_script(rounds=1), gen.kafka_session_script(rounds=1)
    assert _same_script(d1, d2)   # the default seed is the generator's own


def test_script_has_every_kind():
    """Replayed through the model: what each request and response turns out to be."""
    conns, policy, script = gen.kafka_session_script()
    assert len(conns) == 64 and len(script) == 30
    assert set(conns["proto"].tolist()) == {0, gen.PROTO_KAFKA}
    m = model.Sessions(conns)
    issued = [set() for _ in conns]
    kinds, api_keys, aligns = set(), set(), set()
    off = 0
    for r in script:
        assert len(r["requests"]) == len(r["req_conn"]) == len(r["verdict"]) == len(r["tags"]) == 256
        assert len(r["responses"]) == len(r["rep_conn"]) == 96
        for f, c, v in zip(r["requests"], r["req_conn"].tolist(), r["verdict"].tolist()):
            aligns.add((off + 8) & 3)
            off += len(f)
            kinds.add("req-v%d" % v)
            kinds.add("req-noconn" if c >= 64 else "req-kafka" if m.kafka[c] else "req-other-proto")
            if len(f) < 12:
                kinds.add("req-short")
            elif len(f) >= 6:
                api_keys.add(int.from_bytes(f[4:6], "big"))
        fwd, new_id, _ = m.forward(r["requests"], r["req_conn"], r["verdict"], r["tags"], r["now_ms"])
        for c, w, i in zip(r["req_conn"].tolist(), fwd.tolist(), new_id.tolist()):
            if w:
                issued[c].add(i)
        seen = set()
        for f, c in zip(r["responses"], r["rep_conn"].tolist()):
            cid = int.from_bytes(f[4:8], "big") if len(f) >= 8 else None
            if cid is None:
                kinds.add("rep-short")
            elif (c, cid) in seen:
                kinds.add("rep-duplicate")
            elif m.kafka[c] and cid in m.caches[c].cache:
                kinds.add("rep-live")
            elif cid in issued[c]:
                kinds.add("rep-answered")
            else:
                kinds.add("rep-never")
            seen.add((c, cid))
        found = m.responses(r["responses"], r["rep_conn"])[0]
        assert 0 < int(found.sum()) < 96
    assert kinds == {"req-v0", "req-v1", "req-v2", "req-v3", "req-v4", "req-noconn", "req-kafka", "req-other-proto",
                     "req-short", "rep-short", "rep-duplicate", "rep-live", "rep-answered", "rep-never"}
    assert {0, 1, 2, 3, 8, 18} <= api_keys      # several kinds of real frames
    assert aligns == {0, 1, 2, 3}               # packed back to back: ids at every alignment
    assert m.stats()["live"] <= 4096            # the shape the GPU test enables sessions for


def test_model_equals_host_cache():
    """Connection by connection: the model's new ids, rewritten request bytes,
    restored response bytes and found flags are the host cache's."""
    conns, _, script = gen.kafka_session_script(nconns=16, rounds=8, nreq=128, nrep=64, seed=5)
    m = model.Sessions(conns)
    host = [_lib.KafkaCorrelationCache() for _ in conns]
    for r in script:
        fwd, new_id, after = m.forward(r["requests"], r["req_conn"], r["verdict"], r["tags"], r["now_ms"])
        for c in range(len(conns)):
            idx = [i for i in range(len(fwd)) if fwd[i] and int(r["req_conn"][i]) == c]
            if not idx:
                continue
            arena, offs, lens = gen.pack([r["requests"][i] for i in idx])
            ids = host[c].requests(arena, offs, lens)
            assert ids.tolist() == new_id[idx].tolist(), c
            assert arena.tobytes() == b"".join(after[i] for i in idx), c
        found, _, _, _, _, rafter = m.responses(r["responses"], r["rep_conn"])
        for c in range(len(conns)):
            idx = [i for i in range(len(found)) if int(r["rep_conn"][i]) == c]
            if not idx:
                continue
            if not m.kafka[c]:
                assert not found[idx].any()
                continue
            arena, offs, lens = gen.pack([r["responses"][i] for i in idx])
            got = host[c].responses(arena, offs, lens)
            assert got.tolist() == found[idx].astype(bool).tolist(), c
            assert arena.tobytes() == b"".join(rafter[i] for i in idx), c
        for c in range(len(conns)):
            assert len(host[c]) == len(m.caches[c].cache), c


def replay_kats(make):
    """The reference's two assertion sequences through `make()`'s object:
    request(frame, now) -> (new id, frame after), response(frame) -> (found,
    orig id, frame after), gc(now, lifetime) -> (expired, live)."""
    doc = json.load(open(KATS))
    assert [c["name"] for c in doc["cases"]] == ["TestCorrelation", "TestCorrelationGC"]
    assert len(doc["request1"]) == 18 and len(doc["request2"]) == 20   # correlation_cache_test.go:24-25
    for case in doc["cases"]:
        o = make()
        prev = None
        for s in case["steps"]:
            if s["op"] == "request":
                nid, after = o.request(bytes(s["frame"]), s["now_ms"])
                assert nid == s["want_id"], s
                assert after[8:12] == s["want_id"].to_bytes(4, "big") and after[:8] == bytes(s["frame"][:8]), s
            elif s["op"] == "response":
                f = prev if s["frame"] == "prev" else bytes(s["frame"])
                found, orig, prev = o.response(f)
                assert found == s["want_found"], s
                if found:
                    assert orig == s["want_orig"] and prev[4:8] == orig.to_bytes(4, "big"), s
                else:
                    assert prev == f, s
            else:
                assert o.gc(s["now_ms"], case["lifetime_ms"]) == (s["want_expired"], s["want_live"]), s


class _ModelKat:
    def __init__(self):
        self.c = model.Cache()

    def request(self, frame, now):
        f = bytearray(frame)
        return self.c.handle_request(f, 0, now), bytes(f)

    def response(self, frame):
        f = bytearray(frame)
        ent = self.c.correlate_response(f)
        return ent is not None, ent[0] if ent else 0, bytes(f)

    def gc(self, now, lifetime):
        return self.c.gc(now, lifetime), len(self.c.cache)


def test_reference_kats_through_the_model():
    replay_kats(_ModelKat)

"""Cassandra sessions without a GPU: the C-ABI entry points are exported, a
host-only engine refuses to keep sessions and stays usable, and the session
script generator is deterministic and stays inside the device tables' caps
(so the randomized GPU test can take the oracle's answer for every frame)."""
import re
import subprocess

import numpy as np

import cilium_amd
from cilium_amd import _lib, gen

HIP_ERROR_NO_DEVICE = 100

SYMBOLS = ("l7g_cass_sessions_enable", "l7g_cass_replies", "l7g_cass_replies_host", "l7g_cass_session_reset",
           "l7g_cass_session_stats")


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
        e.cass_sessions(1024)
    except RuntimeError as ex:
        assert f"HIP error {HIP_ERROR_NO_DEVICE}" in str(ex), ex
    else:
        raise AssertionError("a host-only engine enabled sessions")
    assert e.cass_session_stats() == dict.fromkeys(e.SESSION_STATS, 0)
    # still a working rule compiler
    e.update_policy(gen.cassandra_policy())
    e.set_connections(gen.make_conns(2, 0, gen.CASS_PORT, True, gen.PROTO_CASSANDRA, [100, 7]))
    assert e.nrules > 0
    e.close()


def _frames(script):
    for r in script:
        for f in r["requests"]:
            yield False, f
        for f in r["replies"]:
            yield True, f


def test_script_is_deterministic():
    a = gen.cassandra_session_script(nconns=16, rounds=4, nreq=64, nrep=24, seed=77)
    b = gen.cassandra_session_script(nconns=16, rounds=4, nreq=64, nrep=24, seed=77)
    c = gen.cassandra_session_script(nconns=16, rounds=4, nreq=64, nrep=24, seed=78)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    for ra, rb in zip(a[2], b[2]):
        assert ra["requests"] == rb["requests"] and ra["replies"] == rb["replies"]
        assert np.array_equal(ra["req_conn"], rb["req_conn"]) and np.array_equal(ra["rep_conn"], rb["rep_conn"])
    assert [r["requests"] for r in a[2]] != [r["requests"] for r in c[2]]
    # the default seed is the generator's own
    d1, d2 = gen.cassandra_session_script(rounds=1), gen.cassandra_session_script(rounds=1)
    assert d1[2][0]["requests"] == d2[2][0]["requests"]


def test_script_shape_and_caps():
    conns, policy, script = gen.cassandra_session_script()
    assert len(conns) == 64 and len(script) == 30
    kinds = set()
    for r in script:
        assert len(r["requests"]) == len(r["req_conn"]) == 256
        assert len(r["replies"]) == len(r["rep_conn"]) == 96
        assert int(r["req_conn"].max()) < 64 and int(r["rep_conn"].max()) < 64
    for reply, f in _frames(script):
        if len(f) < 9:
            kinds.add("short")
            continue
        op, body = f[4], f[9:]
        if not reply and op in (0x07, 0x09) and len(body) >= 4:
            q = body[4:4 + int.from_bytes(body[:4], "big")]
            kinds.add("prepare" if op == 0x09 else "query")
            # every token (so every table and keyspace) is at most 64 bytes: "<keyspace>.<table>"
            # stays under the table cap even if lower-casing grew every rune (2 -> 3 bytes at most)
            assert 2 * (64 * 3 // 2) + 1 <= gen.CASS_TABLE_MAX and 64 <= gen.CASS_KS_MAX
            for tok in q.split():
                assert len(tok) <= 64, tok
            if q.lower().startswith(b"use "):
                kinds.add("use")
        elif not reply and op == 0x0A and len(body) >= 2:
            il = int.from_bytes(body[:2], "big")
            kinds.add("execute")
            assert il <= gen.CASS_ID_MAX
        elif not reply and op == 0x0D:
            kinds.add("batch")
        elif reply and op == 0x08 and (f[0] & 0x80) and len(body) >= 6 and int.from_bytes(body[:4], "big") == 4:
            kinds.add("prepared-reply")
            assert int.from_bytes(body[4:6], "big") <= gen.CASS_ID_MAX
        else:
            kinds.add("other")
    assert kinds == {"short", "prepare", "query", "use", "execute", "batch", "prepared-reply", "other"}

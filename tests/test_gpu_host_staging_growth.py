"""The per-thread staging of the host-buffer calls (HostCtx in engine_state.h,
host_call.cc) regrown between calls: on one fresh engine, from one thread, the
same call over the first 32, then 2048, then 32 requests of a workload.  The
sizes come from the code: the pinned output staging starts at 16 KiB and a
call needs CallOutCap(n) = 9 n + 64 bytes of it, so 2048 requests outgrow it
and 32 do not; the input staging starts at 64 KiB, which 2048 requests of the
mixed workload exceed; the log, reply and Kafka-session pairs start empty and
grow to need + need / 4, so the first and the second call both grow them and
the third reuses what the second left.  Every call's outputs equal those of
the device-pointer call over the same prefix."""
import types

import numpy as np
import pytest
import torch

import test_gpu_cassandra_sessions as CS
import test_gpu_deny_replies as DR
import test_gpu_generic_log as GL
import test_gpu_kafka_sessions as KS
from cilium_amd import Engine, gen
from cilium_amd._lib import ALLOW, DENY

pytestmark = pytest.mark.gpu

SIZES = (32, 2048, 32)
SPAN_STRIDE, TEXT_STRIDE = 4, 32


def test_the_sizes_cross_the_floors():
    def out_cap(n):  # call_layout.h CallOutCap
        return 9 * n + 64

    def in_cap(n, arena_len):  # CallInCap
        return ((16 * n + 255) & ~255) + arena_len + 64

    assert out_cap(32) < (1 << 14) < out_cap(2048)
    w = gen.mixed_workload(2048)
    assert in_cap(32, _prefix(w, 32).arena.nbytes) < (1 << 16) < in_cap(2048, w.arena.nbytes)


def _prefix(w, n):
    """The first n requests of w over no more arena than they use."""
    end = int((w.offsets[:n] + w.lengths[:n]).max())
    return gen.Workload(w.name, w.arena[:end], w.offsets[:n], w.lengths[:n], w.conn_ids[:n], w.conns, w.policy)


@pytest.fixture
def fresh():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def mixed():
    w = gen.mixed_workload(2048)
    return {n: _prefix(w, n) for n in set(SIZES)}


def _mixed_engine(fresh, mixed):
    fresh.update_policy(mixed[2048].policy)
    fresh.set_connections(mixed[2048].conns)
    return fresh


def _live(v):
    return (v == ALLOW) | (v == DENY)


def _has_both(v):
    assert (v == ALLOW).any() and (v == DENY).any()


def _same_vrc(got, D):
    assert np.array_equal(got[0], D.v) and np.array_equal(got[1], D.r) and np.array_equal(got[2], D.c)


def test_classify(fresh, mixed):
    e = _mixed_engine(fresh, mixed)
    want = {n: GL._run(e, w, call="plain") for n, w in mixed.items()}
    _has_both(want[32].v)
    for n in SIZES:
        w = mixed[n]
        _same_vrc(e.classify(w.arena, w.offsets, w.lengths, w.conn_ids), want[n])


def test_classify_logged(fresh, mixed):
    e = _mixed_engine(fresh, mixed)
    want = {n: GL._run(e, w, SPAN_STRIDE, 0, call="logged") for n, w in mixed.items()}
    _has_both(want[32].v)
    for n in SIZES:
        w, D = mixed[n], want[n]
        rows = np.full((n, SPAN_STRIDE, 2), GL.SPAN_FILL, np.uint32)
        got = e.classify_logged(w.arena, w.offsets, w.lengths, w.conn_ids, SPAN_STRIDE,
                                rows.view([("off", "<u4"), ("len", "<u4")]).reshape(n, SPAN_STRIDE))
        _same_vrc(got, D)
        live = _live(D.v)
        assert np.array_equal(np.frombuffer(got[3].tobytes(), np.uint32).reshape(n, 8)[live], D.raw[live])
        assert np.array_equal(got[4].view(np.uint32).reshape(n, SPAN_STRIDE, 2), D.spans)


def test_classify_logged_all(fresh, mixed):
    e = _mixed_engine(fresh, mixed)
    want = {n: GL._run(e, w, SPAN_STRIDE, TEXT_STRIDE) for n, w in mixed.items()}
    _has_both(want[32].v)
    for n in SIZES:
        w, D = mixed[n], want[n]
        rows = np.full((n, SPAN_STRIDE, 2), GL.SPAN_FILL, np.uint32)
        text = np.full((n, TEXT_STRIDE), GL.TEXT_FILL, np.uint8)
        got = e.classify_logged_all(w.arena, w.offsets, w.lengths, w.conn_ids, SPAN_STRIDE, TEXT_STRIDE,
                                    rows.view([("off", "<u4"), ("len", "<u4")]).reshape(n, SPAN_STRIDE), text)
        _same_vrc(got, D)
        live = _live(D.v)
        assert np.array_equal(np.frombuffer(got[3].tobytes(), np.uint32).reshape(n, 8)[live], D.raw[live])
        assert np.array_equal(got[4].view(np.uint32).reshape(n, SPAN_STRIDE, 2), D.spans)
        assert np.array_equal(got[5], D.text)


def test_deny_replies(fresh, mixed):
    """deny_replies_arrays with a cap that holds every reply."""
    e = _mixed_engine(fresh, mixed)
    want = {}
    for n, w in mixed.items():
        d = DR._Dev(w.arena, w.offsets, w.lengths, w.conn_ids)
        d_v, (v, _, _, _) = DR._classify(e, d)
        want[n] = (v, DR._replies(e, d, d_v))
    _has_both(want[32][0])
    for n in SIZES:
        w, (v, (buf, off, ln, tot)) = mixed[n], want[n]
        cap = int(tot[0])
        assert cap > 0 and int(tot[1]) > 0
        got = e.deny_replies_arrays(w.arena, w.offsets, w.lengths, w.conn_ids, v, cap)
        assert np.array_equal(got[0], buf[:cap])
        assert np.array_equal(got[1], off) and np.array_equal(got[2], ln) and np.array_equal(got[3], tot)


def test_kafka_forward_then_responses(fresh):
    conns, policy, script = gen.kafka_session_script(rounds=1, nreq=2048, nrep=2048)
    r = script[0]
    fresh.update_policy(policy)
    conn, verdict = np.asarray(r["req_conn"], np.uint32), np.asarray(r["verdict"], np.uint8)
    tags, rconn = np.asarray(r["tags"], np.uint64), np.asarray(r["rep_conn"], np.uint32)
    _has_both(verdict[:32])

    def run(n, device):
        """Both calls over the first n frames, on sessions that start empty."""
        fresh.kafka_sessions(4096)
        fresh.set_connections(conns)
        d = types.SimpleNamespace(e=fresh, device=device)
        f = KS.Dev._forward(d, r["requests"][:n], conn[:n], verdict[:n], tags[:n], r["now_ms"])
        return f, KS.Dev._responses(d, r["responses"][:n], rconn[:n])

    want = {n: run(n, True) for n in set(SIZES)}
    assert (want[32][0][0] == 1).any() and want[2048][1][0].any()      # some forwarded, some responses found
    for n in SIZES:
        got = run(n, False)
        for g, w in zip(got[0] + got[1], want[n][0] + want[n][1]):      # (the rewritten arenas with them)
            assert np.array_equal(g, w)


def test_cass_replies(fresh, oracle):
    """A reply has no DENY (it is ALLOW, INCOMPLETE or PARSE_ERROR): the
    requests that precede the replies hold the ALLOW and the DENY."""
    conns, policy, script = gen.cassandra_session_script(rounds=1, nreq=2048, nrep=2048)
    r = script[0]
    fresh.update_policy(policy)
    req_conn, rep_conn = np.asarray(r["req_conn"], np.uint32), np.asarray(r["rep_conn"], np.uint32)

    def run(n, device):
        """The first n requests, then the first n replies, on sessions that start empty."""
        fresh.cass_sessions(CS.MAX_STATEMENTS)
        fresh.set_connections(conns)
        arena, offs, lens = gen.pack(r["requests"][:n])
        v = fresh.classify(arena, offs, lens, req_conn[:n])[0]
        if device:
            g = CS.Sessions._device_call(types.SimpleNamespace(e=fresh), r["replies"][:n], rep_conn[:n], True)
            return v, g[0], g[2]
        arena, offs, lens = gen.pack(r["replies"][:n])
        return (v,) + tuple(fresh.cass_replies(arena, offs, lens, rep_conn[:n]))

    want = {n: run(n, True) for n in set(SIZES)}
    _has_both(want[32][0])
    assert (want[32][1] == ALLOW).any() and (want[32][1] != ALLOW).any()
    for n in SIZES:
        for g, w in zip(run(n, False), want[n]):
            assert np.array_equal(g, w)

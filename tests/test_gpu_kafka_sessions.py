"""Kafka sessions on the GPU (l7g_kafka_sessions_enable): l7g_kafka_forward,
l7g_kafka_responses and the table's upkeep against the Python model of the
reference's correlation cache (tests/kafka_sessions_py.py, pinned to the host
cache by tests/test_kafka_sessions_host.py).  Every comparison is exact; device
results are never compared with device results, except where a test is about
two runs agreeing (batch order), and there both are held to the model too.

The engine of this file is its own: the session-scoped engine of conftest.py
never has sessions on."""
import numpy as np
import pytest

from cilium_amd import gen
import kafka_sessions_py as model
from test_kafka_sessions_host import replay_kats

pytestmark = pytest.mark.gpu

DENY, ALLOW = 0, 1
HIP_ERROR_NOT_READY = 600
CONN_KEYS = ("policy", "port", "ingress", "proto", "src_id", "dst_id")


@pytest.fixture(scope="module")
def sengine():
    from cilium_amd import Engine
    e = Engine(0)
    e.update_policy(gen.cfg3_policy())
    yield e
    e.close()


def kafka_conns(n, other=()):
    conns = gen.make_conns(n, 0, 9092, True, gen.PROTO_KAFKA, ([7, 8, 100, 101] * (n // 4 + 1))[:n])
    for c in other:
        conns["proto"][c] = 0
    return conns


def req(corr, key=3, ver=1, extra=b""):
    """A request frame: size, api key, version, correlation id, an empty client id."""
    body = key.to_bytes(2, "big") + ver.to_bytes(2, "big") + (corr & 0xFFFFFFFF).to_bytes(4, "big") + b"\x00\x00" + extra
    return len(body).to_bytes(4, "big") + body


rsp = gen.kafka_response_frame


class Dev:
    """The engine and the model, kept in step; every call is compared in full."""

    def __init__(self, engine, conns, max_inflight, device=False):
        self.e, self.device = engine, device
        self.e.kafka_sessions(max_inflight)
        self.conns = conns
        self.e.set_connections(conns)
        self.m = model.Sessions(conns)

    # ---- the two ways to call
    def _forward(self, frames, conn, verdict, tags, now):
        arena, offs, lens = gen.pack(frames)
        if not self.device:
            fwd, nid = self.e.kafka_forward(arena, offs, lens, conn, verdict, now, tags)
            return fwd, nid, arena
        import torch
        dev = torch.device("cuda", 0)
        d = [torch.from_numpy(a).to(dev) for a in (arena, offs.view(np.int64), lens.view(np.int32), conn.view(np.int32),
                                                   verdict, tags.view(np.int64))]
        n = len(frames)
        o = [torch.full((n,), 7, dtype=t, device=dev) for t in (torch.uint8, torch.int32)]
        self.e.kafka_forward_device(d[0].data_ptr(), d[0].numel(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                    d[4].data_ptr(), d[5].data_ptr(), n, now, o[0].data_ptr(), o[1].data_ptr(),
                                    stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return o[0].cpu().numpy(), o[1].cpu().numpy().view(np.uint32), d[0].cpu().numpy()

    def _responses(self, frames, conn):
        arena, offs, lens = gen.pack(frames)
        if not self.device:
            return self.e.kafka_responses(arena, offs, lens, conn) + (arena,)
        import torch
        dev = torch.device("cuda", 0)
        d = [torch.from_numpy(a).to(dev) for a in (arena, offs.view(np.int64), lens.view(np.int32), conn.view(np.int32))]
        n = len(frames)
        o = [torch.full((n,), 7, dtype=t, device=dev) for t in (torch.uint8, torch.int32, torch.int16, torch.int16,
                                                                torch.int64)]
        self.e.kafka_responses_device(d[0].data_ptr(), d[0].numel(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                      n, *[t.data_ptr() for t in o], stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        g = [t.cpu().numpy() for t in o]
        return g[0], g[1].view(np.uint32), g[2], g[3], g[4].view(np.uint64), d[0].cpu().numpy()

    # ---- the compared calls
    def forward(self, frames, conn, verdict=None, tags=None, now=0, may_drop=False):
        n = len(frames)
        conn = np.asarray(conn, np.uint32)
        verdict = np.full(n, ALLOW, np.uint8) if verdict is None else np.asarray(verdict, np.uint8)
        tags = np.arange(1, n + 1, dtype=np.uint64) * 1000003 if tags is None else np.asarray(tags, np.uint64)
        fwd, nid, arena = self._forward(frames, conn, verdict, tags, now)
        # the model is told which inserts the table dropped (it cannot know the table's occupancy)
        dropped = np.nonzero(fwd == 2)[0] if may_drop else ()
        wf, wi, after = self.m.forward(frames, conn, verdict, tags, now, dropped)
        assert fwd.tolist() == wf.tolist()
        assert nid.tolist() == wi.tolist()
        assert arena.tobytes() == b"".join(after)       # the whole arena
        self.check_stats()
        return fwd, nid, after

    def responses(self, frames, conn):
        conn = np.asarray(conn, np.uint32)
        got = self._responses(frames, conn)
        want = self.m.responses(frames, conn)
        for name, g, w in zip(("found", "orig_id", "api_key", "api_version", "tag"), got, want):
            assert g.tolist() == w.tolist(), name
        assert got[5].tobytes() == b"".join(want[5])    # the whole arena
        self.check_stats()
        return got[0]

    def gc(self, now, lifetime):
        got = self.e.kafka_session_gc(now, lifetime)
        assert got == self.m.gc(now, lifetime)
        st = self.check_stats()
        assert st["used_slots"] == st["live"]
        return got

    def check_stats(self):
        st = self.e.kafka_session_stats()
        want = self.m.stats()
        assert {k: st[k] for k in want} == want
        assert st["used_slots"] >= st["live"]
        return st


# ------------------------------------------------------------------ the reference's own vectors
class _DevKat:
    def __init__(self, engine):
        self.e = engine
        engine.kafka_sessions(16)
        engine.set_connections(kafka_conns(1))

    def request(self, frame, now):
        arena, offs, lens = gen.pack([frame])
        fwd, nid = self.e.kafka_forward(arena, offs, lens, [0], [ALLOW], now)
        assert fwd.tolist() == [1]
        return int(nid[0]), arena.tobytes()

    def response(self, frame):
        arena, offs, lens = gen.pack([frame])
        found, orig, _, _, _ = self.e.kafka_responses(arena, offs, lens, [0])
        return bool(found[0]), int(orig[0]), arena.tobytes()

    def gc(self, now, lifetime):
        return self.e.kafka_session_gc(now, lifetime), self.e.kafka_session_stats()["live"]


def test_reference_kats_on_the_device(sengine):
    replay_kats(lambda: _DevKat(sengine))


# ------------------------------------------------------------------ scripted parity
@pytest.mark.parametrize("device", [False, True], ids=["host-twins", "device-pointers"])
def test_scripted_parity(sengine, device):
    """64 connections, 30 rounds of 256 requests + 96 responses; frames packed
    back to back, so ids land at every alignment mod 4."""
    conns, policy, script = gen.kafka_session_script()
    d = Dev(sengine, conns, 4096, device)
    for r in script:
        d.forward(r["requests"], r["req_conn"], r["verdict"], r["tags"], r["now_ms"])
        d.responses(r["responses"], r["rep_conn"])
    st = d.check_stats()
    # (7680 requests, 6 of 11 verdicts ALLOW, 7 of 8 connections Kafka: about 3600 forwarded)
    assert st["dropped"] == 0 and st["found"] > 500 and st["missed"] > 500 and st["forwarded"] > 3000


def test_batch_order(sengine):
    """The same per-connection sequences under two interleavings: every request
    gets the same id.  (Both runs are also held to the model.)"""
    rng = np.random.default_rng(11)
    per = {c: [req(1000 * c + k, extra=b"x" * (k % 3)) for k in range(int(rng.integers(1, 40)))] for c in range(12)}
    ids = []
    for seed in (1, 2):
        order = np.random.default_rng(seed).permutation([c for c, fs in per.items() for _ in fs])
        at = dict.fromkeys(per, 0)
        frames, who = [], []
        for c in order.tolist():
            frames.append(per[c][at[c]])
            who.append((c, at[c]))
            at[c] += 1
        d = Dev(sengine, kafka_conns(12), 1024)
        _, nid, _ = d.forward(frames, order)
        ids.append({w: int(i) for w, i in zip(who, nid)})
    assert ids[0] == ids[1]
    assert all(ids[0][(c, k)] == k + 1 for c, fs in per.items() for k in range(len(fs)))


def test_forced_chains_and_deletes(sengine):
    """max_inflight 4 = 8 slots: chains whatever the hash."""
    d = Dev(sengine, kafka_conns(2), 4)
    d.forward([req(10 + k) for k in range(6)], [0, 1, 0, 1, 0, 1])      # ids 1..3 on both connections
    assert d.check_stats()["used_slots"] == 6
    assert d.responses([rsp(2), rsp(2)], [0, 1]).tolist() == [1, 1]       # the ones in the middle
    st = d.check_stats()
    assert (st["live"], st["used_slots"]) == (4, 6)
    # 2 never-used slots are left: 4 more fit only if both answered slots are claimed again
    fwd, _, _ = d.forward([req(20 + k) for k in range(4)], [0, 0, 1, 1])
    assert fwd.tolist() == [1, 1, 1, 1]
    st = d.check_stats()
    assert (st["live"], st["used_slots"], st["dropped"]) == (8, 8, 0)
    # answered ids miss; everything else is still found, past answered slots in its chain
    assert d.responses([rsp(2), rsp(2)], [0, 1]).tolist() == [0, 0]
    assert d.responses([rsp(k) for k in (5, 1, 3, 4)] * 2, [0] * 4 + [1] * 4).tolist() == [1] * 8
    st = d.check_stats()
    assert (st["live"], st["used_slots"]) == (0, 8)
    # a table with no never-used slot: inserts claim answered slots, [1] does not grow
    assert d.forward([req(30 + k) for k in range(8)], [0, 1] * 4)[0].tolist() == [1] * 8
    assert d.check_stats()["used_slots"] == 8


def test_full_table(sengine):
    d = Dev(sengine, kafka_conns(2), 4)
    assert d.forward([req(k) for k in range(8)], [0, 1] * 4)[0].tolist() == [1] * 8
    frames = [req(100 + k, extra=b"y" * k) for k in range(3)]
    fwd, nid, after = d.forward(frames, [0, 1, 0], may_drop=True)
    assert fwd.tolist() == [2, 2, 2] and nid.tolist() == [0, 0, 0] and after == frames   # bytes untouched
    assert d.check_stats()["dropped"] == 3
    # the dropped numbers (5 and 6 on connection 0, 5 on connection 1) are spent and resolve to nothing
    assert d.responses([rsp(5), rsp(6), rsp(5)], [0, 0, 1]).tolist() == [0, 0, 0]
    assert d.responses([rsp(1), rsp(2), rsp(1)], [0, 0, 1]).tolist() == [1, 1, 1]
    assert d.gc(0, 10) == 0                                                # (nothing is old; the table is compacted)
    assert d.check_stats()["used_slots"] == 5
    fwd, nid, _ = d.forward([req(200), req(201), req(202)], [0, 0, 1], may_drop=True)
    assert fwd.tolist() == [1, 1, 1] and nid.tolist() == [7, 8, 6]
    assert d.responses([rsp(7), rsp(3), rsp(6), rsp(4)], [0, 0, 1, 1]).tolist() == [1, 1, 1, 1]


def test_gc_boundary(sengine):
    d = Dev(sengine, kafka_conns(3), 64)
    for now in (100, 200, 300):
        d.forward([req(now + c, key=c, ver=now // 100) for c in range(3)], [0, 1, 2], now=now,
                  tags=[now * 10 + c for c in range(3)])
    assert d.gc(400, 201) == 3         # ages 300, 200, 100: only 300 >= 201
    assert d.gc(400, 200) == 3         # now 200 >= 200 goes too: the >= boundary
    st = d.check_stats()
    assert (st["live"], st["used_slots"], st["expired"]) == (3, 3, 6)
    # the survivors (id 3 of every connection) with their payload, the expired ones miss
    got = d.responses([rsp(k) for k in (1, 2, 3)] * 3, [0] * 3 + [1] * 3 + [2] * 3)
    assert got.tolist() == [0, 0, 1] * 3
    assert d.gc(10 ** 9, 1) == 0


def test_resets(sengine):
    conns = kafka_conns(4)
    d = Dev(sengine, conns, 64)
    d.forward([req(k) for k in range(8)], [0, 1, 2, 3] * 2)               # ids 1, 2 everywhere
    # the new-connection event: connection 1 restarts at 1 and its old responses are orphans
    d.e.conn_update(1, tuple(conns[1][k] for k in CONN_KEYS))
    d.m.reset(1)
    d.e.update_policy(gen.cfg3_policy())                                   # a policy update changes nothing
    assert d.responses([rsp(1), rsp(1), rsp(1)], [0, 1, 2]).tolist() == [1, 0, 1]
    _, nid, _ = d.forward([req(50), req(51)], [1, 0])
    assert nid.tolist() == [1, 3]
    # the named connections
    d.e.kafka_session_reset([2, 3])
    d.m.reset(2)
    d.m.reset(3)
    assert d.responses([rsp(2), rsp(2), rsp(2), rsp(1)], [0, 2, 3, 1]).tolist() == [1, 0, 0, 1]
    assert d.forward([req(60), req(61)], [2, 3])[1].tolist() == [1, 1]
    # every connection
    d.e.set_connections(conns)
    d.m.set_connections(conns)
    assert d.check_stats()["live"] == 0
    assert d.responses([rsp(3), rsp(1), rsp(1)], [0, 2, 3]).tolist() == [0, 0, 0]
    assert d.forward([req(70 + c) for c in range(4)], [0, 1, 2, 3])[1].tolist() == [1, 1, 1, 1]


# ------------------------------------------------------------------ the multi-workgroup paths
def test_large_batch(sengine):
    """The grids are capped at 4096 workgroups of 256 lanes and stride only
    above 1,048,576 frames, so the batch is just above that size (not the
    70,000 a smaller cap would need): 300 connections, connection 5 owning half
    of the requests -- its segment spans most workgroups and its rank crosses
    65,536 -- then as many responses in a shuffled order.  The model is
    vectorised: rank = position in a stable argsort by connection."""
    n, nconns = 4096 * 256 + 1234, 300
    rng = np.random.default_rng(23)
    conns = kafka_conns(nconns, other=(17,))
    sengine.kafka_sessions(n)
    sengine.set_connections(conns)
    conn = rng.integers(0, nconns, size=n).astype(np.uint32)
    conn[rng.random(n) < 0.5] = 5
    verdict = np.where(rng.random(n) < 0.9, ALLOW, DENY).astype(np.uint8)
    corr = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    tags = rng.integers(1, 1 << 63, size=n, dtype=np.uint64)
    lens = (14 + np.arange(n) % 3).astype(np.uint32)                       # ids at every alignment
    offs = np.zeros(n, np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    arena = np.zeros(int(lens.sum()), np.uint8)
    o = offs.astype(np.int64)

    def put_be32(a, at, v):
        for k in range(4):
            a[at + k] = (v >> (24 - 8 * k)).astype(np.uint8)

    put_be32(arena, o, lens - 4)
    arena[o + 5] = (np.arange(n) % 11).astype(np.uint8)                    # api key
    arena[o + 7] = (np.arange(n) % 5).astype(np.uint8)                     # version
    put_be32(arena, o + 8, corr)
    # the model
    go = (verdict == ALLOW) & (conns["proto"][conn] == gen.PROTO_KAFKA)
    idx = np.nonzero(go)[0]
    order = idx[np.argsort(conn[idx], kind="stable")]
    sc = conn[order]
    start = np.searchsorted(sc, sc, side="left")
    want_id = np.zeros(n, np.uint32)
    want_id[order] = (np.arange(len(order)) - start + 1).astype(np.uint32)
    assert int(want_id.max()) > 65536 * 4
    want_arena = arena.copy()
    put_be32(want_arena, o[go] + 8, want_id[go])

    got_arena = arena.copy()
    fwd, nid = sengine.kafka_forward(got_arena, offs, lens, conn, verdict, 5, tags)
    assert np.array_equal(fwd, go.astype(np.uint8))
    assert np.array_equal(nid, want_id)
    assert np.array_equal(got_arena, want_arena)
    st = sengine.kafka_session_stats()
    assert (st["live"], st["used_slots"], st["forwarded"], st["dropped"]) == (len(idx), len(idx), len(idx), 0)

    # every request answered, in a shuffled order: 12-byte frames carrying the new id (0 for the ones not forwarded,
    # an id no connection has issued)
    p = rng.permutation(n)
    rlen = np.full(n, 12, np.uint32)
    roff = np.arange(n, dtype=np.uint64) * 12
    rarena = np.zeros(12 * n, np.uint8)
    ro = roff.astype(np.int64)
    rarena[ro + 3] = 8
    put_be32(rarena, ro + 4, want_id[p])
    want_r = rarena.copy()
    put_be32(want_r, ro[go[p]] + 4, corr[p][go[p]])
    found, orig, key, ver, tag = sengine.kafka_responses(rarena, roff, rlen, conn[p])
    assert np.array_equal(found, go[p].astype(np.uint8))
    assert np.array_equal(orig, np.where(go[p], corr[p], 0).astype(np.uint32))
    assert np.array_equal(key, np.where(go[p], p % 11, 0).astype(np.int16))
    assert np.array_equal(ver, np.where(go[p], p % 5, 0).astype(np.int16))
    assert np.array_equal(tag, np.where(go[p], tags[p], 0).astype(np.uint64))
    assert np.array_equal(rarena, want_r)
    st = sengine.kafka_session_stats()
    assert (st["live"], st["found"], st["missed"]) == (0, len(idx), n - len(idx))


# ------------------------------------------------------------------ off
def test_sessions_off(sengine):
    w = gen.kafka_workload(2000, nconns=16, seed=9)
    sengine.kafka_sessions(0)
    sengine.set_connections(w.conns)
    before = sengine.classify(w.arena, w.offsets, w.lengths, w.conn_ids)
    assert 0 < int((before[0] == ALLOW).sum()) < w.n
    arena = w.arena.copy()
    for call in (lambda: sengine.kafka_forward(arena, w.offsets, w.lengths, w.conn_ids, before[0], 0),
                 lambda: sengine.kafka_responses(arena, w.offsets, w.lengths, w.conn_ids),
                 lambda: sengine.kafka_session_gc(0, 1),
                 lambda: sengine.kafka_session_reset([0])):
        with pytest.raises(RuntimeError, match=f"HIP error {HIP_ERROR_NOT_READY}"):
            call()
    assert np.array_equal(arena, w.arena)
    assert sengine.kafka_session_stats() == dict.fromkeys(sengine.KAFKA_SESSION_STATS, 0)
    # and a classify on the same engine does not care whether sessions are on
    sengine.kafka_sessions(4096)
    sengine.kafka_forward(arena, w.offsets, w.lengths, w.conn_ids, before[0], 0)
    on = sengine.classify(w.arena, w.offsets, w.lengths, w.conn_ids)
    sengine.kafka_sessions(0)
    off = sengine.classify(w.arena, w.offsets, w.lengths, w.conn_ids)
    for a, b, c in zip(before, on, off):
        assert np.array_equal(a, b) and np.array_equal(a, c)

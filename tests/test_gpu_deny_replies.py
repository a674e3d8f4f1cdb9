"""Deny replies on the device (include/l7gpu.h: l7g_deny_replies,
l7g_deny_replies_host).  Every comparison is bit-exact.

Expected bytes: a Kafka reply is what the host function gives for the same
request (_lib.kafka_deny_response, pinned by tests/test_kafka_response.py;
"none" is an empty reply); the fixed replies are restated below from the
reference lines they cite."""
import struct

import numpy as np
import pytest
import torch

from cilium_amd import _lib, api, gen
from cilium_amd._lib import (ALLOW, DENY, INCOMPLETE, PARSE_ERROR, PROTO_CASSANDRA, PROTO_HTTP, PROTO_KAFKA,
                             PROTO_MEMCACHE, PROTO_R2D2)

pytestmark = pytest.mark.gpu

# envoy/cilium_l7policy.cc:90-96,171-177: sendLocalReply(Forbidden, "Access denied\r\n")
DENIED_403 = (b"HTTP/1.1 403 Forbidden\r\ncontent-length: 15\r\ncontent-type: text/plain\r\n\r\n"
              b"Access denied\r\n")
# proxylib/cassandra/cassandraparser.go:269-278 unauthMsgBase
CASS_UNAUTH = bytes([0, 0, 0, 0, 0, 0, 0, 0, 0x1a, 0, 0, 0x21, 0, 0, 0x14]) + b"Request Unauthorized"
R2D2_ERROR = b"ERROR\r\n"

CANARY = 0xA5
GUARD = 64
TOPICS = [("alpha", [0, 3]), ("", [7]), ("gamma", [])]
R2_DENIED = b"READ /priv/b\r\n"  # no r2d2 rule of gen.r2d2_policy() admits it


# ------------------------------------------------------------------ running
class _Dev:
    """A batch resident on the device."""

    def __init__(self, arena, offs, lens, cids, d_arena=None):
        dev = torch.device("cuda", 0)
        if d_arena is None:
            d_arena = torch.from_numpy(np.ascontiguousarray(arena, np.uint8)).to(dev)
        self.arena, self.arena_len = d_arena, d_arena.numel()
        self.ins = [torch.from_numpy(np.ascontiguousarray(x)).to(dev)
                    for x in (np.asarray(offs, np.uint64).view(np.int64), np.asarray(lens, np.uint32).view(np.int32),
                              np.asarray(cids, np.uint32).view(np.int32))]
        self.n = len(offs)

    def args(self):
        return (self.arena.data_ptr(), self.arena_len, *[t.data_ptr() for t in self.ins], self.n)


def _classify(engine, D):
    dev = D.arena.device
    o = [torch.full((D.n,), 7, dtype=t, device=dev) for t in (torch.uint8, torch.int32, torch.int32)]
    cnt = torch.zeros(engine.nrules + 8, dtype=torch.int64, device=dev)
    engine.classify_device(*D.args(), *[t.data_ptr() for t in o], counters_ptr=cnt.data_ptr())
    torch.cuda.synchronize()
    return o[0], [t.cpu().numpy() for t in o] + [cnt.cpu().numpy()]


def _replies(engine, D, d_v, cap=None, null_buf=False):
    """One l7g_deny_replies call: (buf with GUARD bytes past cap, off, len,
    total); every output pre-filled with a canary.  cap=None: sized first."""
    dev = D.arena.device
    ro = torch.full((max(D.n, 1),), -2, dtype=torch.int64, device=dev)
    rl = torch.full((max(D.n, 1),), -2, dtype=torch.int32, device=dev)
    tot = torch.full((2,), -2, dtype=torch.int64, device=dev)
    if cap is None:
        engine.deny_replies_device(*D.args(), d_v.data_ptr(), 0, 0, ro.data_ptr(), rl.data_ptr(), tot.data_ptr())
        torch.cuda.synchronize()
        cap = int(tot.cpu().numpy().view(np.uint64)[0])
        tot.fill_(-2)
    buf = torch.full((cap + GUARD,), CANARY, dtype=torch.uint8, device=dev)
    engine.deny_replies_device(*D.args(), d_v.data_ptr(), 0 if null_buf else buf.data_ptr(), 0 if null_buf else cap,
                               ro.data_ptr(), rl.data_ptr(), tot.data_ptr())
    torch.cuda.synchronize()
    return (buf.cpu().numpy(), ro.cpu().numpy().view(np.uint64)[:D.n], rl.cpu().numpy().view(np.uint32)[:D.n],
            tot.cpu().numpy().view(np.uint64))


def _expect_one(req, proto, verdict, ok=True):
    if verdict != DENY or not ok:
        return b""
    if proto == PROTO_KAFKA:
        return _lib.kafka_deny_response(req) or b""
    if proto == PROTO_HTTP:
        return DENIED_403
    if proto == PROTO_CASSANDRA:
        return b"" if len(req) < 4 else bytes([0x80 | (req[0] & 7), 0, req[2], req[3]]) + CASS_UNAUTH[4:]
    if proto == PROTO_R2D2:
        return R2D2_ERROR
    return b""


def _check(exp, out, cap):
    """out = (buf, off, len, total) of a call with `cap` against the expected
    replies: sizes complete, exactly the fitting replies written, every other
    byte (the guard included) untouched."""
    buf, off, ln, tot = out
    lens = np.array([len(e) for e in exp], np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64) if len(exp) else lens
    assert ln.tolist() == lens.tolist()
    assert off.tolist() == offs.tolist()
    assert tot.tolist() == [int(lens.sum()), int((lens > 0).sum())]
    want = np.full(len(buf), CANARY, np.uint8)
    for e, o in zip(exp, offs.tolist()):
        if e and o + len(e) <= cap:
            want[o:o + len(e)] = np.frombuffer(e, np.uint8)
    bad = np.nonzero(buf != want)[0]
    assert len(bad) == 0, ("first differing byte", int(bad[0]), len(bad))


def _reqs(arena, offs, lens):
    raw = np.ascontiguousarray(arena).tobytes()
    return [raw[int(o):int(o) + int(n)] for o, n in zip(offs, lens)]


# ------------------------------------------------------------------ the small engine set-up
def _kafka_deny_policy(name="k-deny"):
    # (no request below names this topic: every Kafka request is denied)
    return api.network_policy(name, 3, ingress=[(9092, [api.port_rule(
        kafka=[api.PortRuleKafka(api_key="produce", topic="zz-nomatch")])])])


K_CONN, R2_CONN, CS_CONN, H_CONN = 0, 1, 2, 3


def _install_small(engine):
    pol = {"policies": [_kafka_deny_policy(), dict(gen.r2d2_policy()["policies"][0], name="r2"),
                        dict(gen.cassandra_policy()["policies"][0], name="cs"),
                        dict(gen.cfg1_policy()["policies"][0], name="h1")]}
    conns = np.concatenate([gen.make_conns(1, 0, 9092, True, PROTO_KAFKA, [2000]),
                            gen.make_conns(1, 1, gen.R2D2_PORT, True, PROTO_R2D2, [100]),
                            gen.make_conns(1, 2, gen.CASS_PORT, True, PROTO_CASSANDRA, [100]),
                            gen.make_conns(1, 3, 80, True, PROTO_HTTP, [1])])
    engine.update_policy(pol)
    engine.set_connections(conns)
    return conns


def _run_small(engine, reqs, cids, supplied=None, offs=None, arena=None):
    """Requests on the small set-up's connections; verdicts from l7g_classify
    unless supplied.  Returns (D, verdicts, replies)."""
    conns = _install_small(engine)
    if arena is None:
        arena, offs, lens = gen.pack(reqs)
    else:
        lens = np.array([len(r) for r in reqs], np.uint32)
    D = _Dev(arena, offs, lens, cids)
    if supplied is None:
        d_v, (v, _, _, _) = _classify(engine, D)
    else:
        v = np.asarray(supplied, np.uint8)
        d_v = torch.from_numpy(v).to(D.arena.device)
    out = _replies(engine, D, d_v)
    return D, v, out, conns


# ------------------------------------------------------------------ 1. every kind and version
def _all_kinds():
    reqs = []
    for v in range(4):
        t = [(n, [(p, [gen.k_message(b"x" * 10, version=v)]) for p in ps]) for n, ps in TOPICS]
        reqs.append(gen.k_produce(v, 11, "c", t, txn="t" if v >= 3 else None))
    reqs += [gen.k_fetch(v, 12, "c", TOPICS) for v in range(6)]
    reqs += [gen.k_offset(v, 13, "c", TOPICS) for v in range(3)]
    reqs += [gen.k_metadata(v, 14, "c", names) for v in range(6) for names in (None, [], ["a", "", "a"])]
    reqs += [gen.k_offset_commit(v, 15, "c", "g", TOPICS) for v in range(4)]
    reqs += [gen.k_offset_fetch(v, 16, "c", "g", t) for v in range(4) for t in (TOPICS, None)]
    reqs += [gen.k_consumer_metadata(v, 17, "c", "g") for v in range(2)]
    reqs.append(gen.k_request(18, 0, 1, "c", b""))  # ApiVersions: untyped, no response
    return reqs


def test_every_kafka_kind_and_version(engine):
    reqs = _all_kinds()
    D, v, out, _ = _run_small(engine, reqs, np.full(len(reqs), K_CONN, np.uint32))
    assert (v == DENY).all(), v.tolist()
    exp = [_expect_one(r, PROTO_KAFKA, DENY) for r in reqs]
    assert exp[-1] == b"" and all(exp[:-1])
    _check(exp, out, int(out[3][0]))


# ------------------------------------------------------------------ 2. produce edge cases
def _produce_raw(version, corr, topics):
    """topics: [(name, [(partition, set size field, set bytes)])]"""
    b = struct.pack(">hi", -1, 1000) + struct.pack(">i", len(topics))
    for name, parts in topics:
        b += gen.k_str(name) + struct.pack(">i", len(parts))
        for pid, size, ms in parts:
            b += struct.pack(">ii", pid, size) + ms
    return gen.k_request(0, version, corr, "c", b)


def test_produce_edge_cases(engine):
    good = lambda n=20, v=0: gen.k_message(b"g" * n, version=v)  # noqa: E731
    bad = lambda n=20, v=0: gen.k_message(b"b" * n, version=v, bad_crc=True)  # noqa: E731
    inner = good(30) + good(40)
    tiny = struct.pack(">qi", 0, 4) + b"\x01\x02\x03\x04"  # msize <= 4
    reqs = [
        gen.k_produce(0, 5, "c", [("t", [(1, [bad(), good()])]), ("u", [(2, [good()])])]),
        gen.k_produce(0, 6, "c", [("t", [(1, [good(), bad()])]), ("u", [(2, [good()])])]),
        gen.k_produce(1, 7, "c", [("t", [(1, [good(v=1)]), (2, [bad(v=1), good(v=1)])]), ("u", [(3, [good(v=1)])])]),
        gen.k_produce(2, 8, "c", [("t", [(1, [good(300, 2), bad(300, 2)]), (4, [good(64, 2)])])]),
        gen.k_produce(0, 9, "c", [("z", [(1, [gen.k_compressed(inner, 1)]), (2, [good()])])]),
        gen.k_produce(0, 10, "c", [("z", [(1, [gen.k_compressed(inner, 2)]), (2, [good()])])]),
        gen.k_produce(1, 11, "c", [("z", [(1, [gen.k_compressed(inner, 2, version=1, xerial=True), good(v=1)])])]),
        gen.k_produce(0, 12, "c", [("t", [(1, [tiny, good()]), (2, [good()])])]),
        _produce_raw(0, 13, [("t", [(1, -1, b""), (2, len(good()), good())]), ("u", [(3, -1, b"")])]),
        _produce_raw(2, 14, [("t", [(1, -1, b"")])]),
    ]
    # (whatever the classifier makes of them: the reply decoder is what is under test)
    D, v, out, _ = _run_small(engine, reqs, np.full(len(reqs), K_CONN, np.uint32), supplied=[DENY] * len(reqs))
    exp = [_expect_one(r, PROTO_KAFKA, DENY) for r in reqs]
    assert sum(1 for e in exp if e) >= 6  # (most still decode; the others must answer nothing)
    _check(exp, out, int(out[3][0]))


# ------------------------------------------------------------------ 3. alignment
def test_every_source_and_destination_alignment(engine):
    """A Fetch with topic names of every length 0..40 at each of the 16 arena
    alignments, behind as many denied r2d2 requests (7-byte replies) as put its
    reply at each of the 16 destination alignments: all 256 pairs."""
    names = [bytes((97 + (i + j) % 26) for j in range(i)) for i in range(41)]
    fetch = gen.k_fetch(5, 77, "client", [(nm, [i, i + 1]) for i, nm in enumerate(names)])
    reply = _lib.kafka_deny_response(fetch)
    arena = bytearray()
    offs, lens, cids, protos = [], [], [], []
    r2_at = None
    total = 0
    pairs = set()
    for a in range(16):
        for d in range(16):
            k = ((d - total) * 7) % 16  # 7 k = d - total (mod 16): 7 is its own inverse
            assert 0 <= k <= 15
            for _ in range(k):
                if r2_at is None:
                    r2_at = len(arena)
                    arena += R2_DENIED
                offs.append(r2_at); lens.append(len(R2_DENIED)); cids.append(R2_CONN); protos.append(PROTO_R2D2)
                total += len(R2D2_ERROR)
            arena += b"\x00" * ((a - len(arena)) % 16)
            offs.append(len(arena)); lens.append(len(fetch)); cids.append(K_CONN); protos.append(PROTO_KAFKA)
            arena += fetch
            pairs.add((offs[-1] % 16, total % 16))
            total += len(reply)
    assert len(pairs) == 256
    reqs = [R2_DENIED if p == PROTO_R2D2 else fetch for p in protos]
    D, v, out, _ = _run_small(engine, reqs, np.array(cids, np.uint32), offs=np.array(offs, np.uint64),
                              arena=np.frombuffer(bytes(arena), np.uint8).copy())
    assert D.arena.data_ptr() % 16 == 0
    assert (v == DENY).all()
    exp = [R2D2_ERROR if p == PROTO_R2D2 else reply for p in protos]
    assert int(out[3][0]) == total
    _check(exp, out, total)


# ------------------------------------------------------------------ 4. mixed verdicts
def _cass_requests(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        q = gen._CASS_QUERIES[int(rng.integers(0, len(gen._CASS_QUERIES)))].encode("utf-8", "surrogateescape")
        body = len(q).to_bytes(4, "big") + q + b"\x00\x01\x00"
        f = gen.cass_frame(0x07, body, stream=(0, 0x7FFF, 0xFFFF)[i % 3], version=3 + (i // 3) % 2)
        out.append(f[:int(rng.integers(0, len(f)))] if i % 23 == 22 else f)
    return out


class _Mixed:
    pass


def _build_mixed():
    """4,200 requests over the five protocols, interleaved; one connection index out of range."""
    parts = [gen.http_workload(2, 1200, seed=gen.SEED_BASE + 301), gen.kafka_workload(1000, seed=gen.SEED_BASE + 302,
                                                                                     all_kinds=True),
             gen.memcache_workload(600, seed=gen.SEED_BASE + 303), gen.r2d2_workload(700, seed=gen.SEED_BASE + 304),
             gen.cassandra_workload(1, seed=gen.SEED_BASE + 305)]
    cs = _cass_requests(700, 306)
    M = _Mixed()
    M.policy = {"policies": [dict(w.policy["policies"][0], name=f"p{i}") for i, w in enumerate(parts)]}
    # every other connection is under a policy without L7 restrictions, so that about half is allowed
    ports = sorted({int(p) for w in parts for p in w.conns["port"]})
    wide = [(p, [api.port_rule(kafka=[api.PortRuleKafka()]) if p == 9092 else api.port_rule()]) for p in ports]
    M.policy["policies"].append(api.network_policy("open", 21, ingress=wide, egress=wide))
    conns, reqs, cids = [], [], []
    base = 0
    for i, w in enumerate(parts):
        c = w.conns.copy()
        c["policy"] = i
        c["policy"][1::2] = len(parts)
        conns.append(c)
        if i == 4:
            r = cs
            ci = np.random.default_rng(307).integers(0, len(c), len(cs))
        else:
            r, ci = _reqs(w.arena, w.offsets, w.lengths), w.conn_ids
        reqs += r
        cids += (np.asarray(ci, np.int64) + base).tolist()
        base += len(c)
    M.conns = np.concatenate(conns)
    perm = np.random.default_rng(308).permutation(len(reqs))
    M.reqs = [reqs[i] for i in perm]
    M.cids = np.array([cids[i] for i in perm], np.uint32)
    M.cids[1234] = len(M.conns) + 5  # outside the table
    M.arena, M.offs, M.lens = gen.pack(M.reqs)
    ok = M.cids < len(M.conns)
    M.proto = np.where(ok, M.conns["proto"][np.minimum(M.cids, len(M.conns) - 1)], 0)
    M.ok = ok
    assert len(M.reqs) == 4200
    return M


@pytest.fixture(scope="module")
def mixed():
    return _build_mixed()


def _mixed_expect(M, v, sel=slice(None)):
    return [_expect_one(r, p, x, k) for r, p, x, k in zip(M.reqs[sel], M.proto[sel], v[sel], M.ok[sel])]


@pytest.fixture(scope="module")
def mixed_run(engine, mixed):
    """Batch 4 classified and answered once: shared, read-only."""
    M = mixed
    engine.update_policy(M.policy)
    engine.set_connections(M.conns)
    D = _Dev(M.arena, M.offs, M.lens, M.cids)
    d_v, outs = _classify(engine, D)
    full = _replies(engine, D, d_v)
    return D, d_v, outs, full


def _use_mixed(engine, M):
    engine.update_policy(M.policy)
    engine.set_connections(M.conns)


def test_mixed_batch(engine, mixed, mixed_run):
    M = mixed
    D, d_v, (v, _, _, _), full = mixed_run
    counts = np.bincount(v, minlength=5)
    assert 0.35 * D.n < counts[ALLOW] < 0.65 * D.n and counts[DENY] >= 1000, counts.tolist()  # (about half allowed)
    assert counts[PARSE_ERROR] > 0 and counts[INCOMPLETE] > 0, counts.tolist()
    for p in (PROTO_HTTP, PROTO_KAFKA, PROTO_MEMCACHE, PROTO_R2D2, PROTO_CASSANDRA):
        assert ((M.proto == p) & (v == DENY)).any(), p
    exp = _mixed_expect(M, v)
    ln = full[2]
    # len is 0 exactly off DENY -- but for what a DENY is answered nothing with
    silent = np.array([len(e) == 0 for e in exp])
    assert (ln[v != DENY] == 0).all() and ((ln == 0) == silent).all()
    assert (ln[(v == DENY) & (M.proto == PROTO_HTTP)] == 87).all()
    assert (ln[(v == DENY) & (M.proto == PROTO_MEMCACHE)] == 0).all()
    _check(exp, full, int(full[3][0]))


def test_mixed_batch_without_denials_and_small_n(engine, mixed, mixed_run):
    M = mixed
    D, d_v, (v, _, _, _), full = mixed_run
    _use_mixed(engine, M)
    none = torch.from_numpy(np.where(v == DENY, ALLOW, v).astype(np.uint8)).to(d_v.device)
    out = _replies(engine, D, none, cap=256)
    assert out[3].tolist() == [0, 0] and (out[2] == 0).all() and (out[1] == 0).all()
    assert (out[0] == CANARY).all()
    first_deny = int(np.nonzero((v == DENY) & (full[2] > 0))[0][0])
    for n in (0, 1, 64, 65):
        for start in (0, first_deny):
            sel = slice(start, start + n)
            Dn = _Dev(M.arena, M.offs[sel], M.lens[sel], M.cids[sel], d_arena=D.arena)
            d_vn = d_v[sel].clone()
            out = _replies(engine, Dn, d_vn)
            _check(_mixed_expect(M, v, sel), out, int(out[3][0]))


# ------------------------------------------------------------------ 5. small cap
def test_small_cap(engine, mixed, mixed_run):
    M = mixed
    D, d_v, (v, _, _, _), full = mixed_run
    _use_mixed(engine, M)
    exp = _mixed_expect(M, v)
    total = int(full[3][0])
    for cap in (total - 1, total // 2, 0):
        out = _replies(engine, D, d_v, cap=cap)
        assert np.array_equal(out[1], full[1]) and np.array_equal(out[2], full[2]) and np.array_equal(out[3], full[3])
        _check(exp, out, cap)
    out = _replies(engine, D, d_v, cap=total, null_buf=True)  # buf NULL, cap 0: sizes only
    assert np.array_equal(out[1], full[1]) and np.array_equal(out[2], full[2]) and np.array_equal(out[3], full[3])
    assert (out[0] == CANARY).all()


def test_bad_arguments(engine, mixed, mixed_run):
    D, d_v, _, full = mixed_run
    _use_mixed(engine, mixed)
    ro, rl, tot = (torch.zeros(D.n, dtype=torch.int64, device=d_v.device) for _ in range(3))
    for buf, cap, a, b, c in ((0, 16, ro, rl, tot), (0, 0, None, rl, tot), (0, 0, ro, None, tot), (0, 0, ro, rl, None)):
        with pytest.raises(RuntimeError, match="HIP error 1$"):
            engine.deny_replies_device(*D.args(), d_v.data_ptr(), buf, cap, *[t.data_ptr() if t is not None else 0
                                                                              for t in (a, b, c)])


# ------------------------------------------------------------------ 6. caller-supplied verdicts
def test_caller_supplied_verdicts(engine):
    fetch = gen.k_fetch(0, 1, "c", TOPICS)
    reqs = [fetch[:20], b"\x00\x00\x00\x02\x00\x00", fetch, fetch, R2_DENIED, fetch]
    arena, offs, lens = gen.pack(reqs)
    offs = offs.copy()
    offs[2] = len(arena) + 4096  # outside the arena
    offs[5] = len(arena) - 8     # starts inside, ends outside
    cids = np.array([K_CONN, K_CONN, K_CONN, H_CONN, 99, K_CONN], np.uint32)  # (99: outside the table)
    D, v, out, _ = _run_small(engine, reqs, cids, supplied=[DENY] * len(reqs), offs=offs, arena=arena)
    exp = [b"", b"", b"", DENIED_403, b"", b""]
    assert _lib.kafka_deny_response(reqs[0]) is None and _lib.kafka_deny_response(reqs[1]) is None
    _check(exp, out, int(out[3][0]))
    # and any byte as a verdict: only L7G_DENY is answered
    for code in (1, 2, 3, 4, 5, 0x80, 0xFF):
        d_v = torch.full((D.n,), code, dtype=torch.uint8, device=D.arena.device)
        o = _replies(engine, D, d_v, cap=128)
        assert o[3].tolist() == [0, 0] and (o[0] == CANARY).all()


# ------------------------------------------------------------------ 7. one large reply
def test_one_large_reply(engine):
    big = gen.k_offset_fetch(1, 9, "c", "g", [("bigtopic", list(range(5000)))])
    reqs = [R2_DENIED, big, R2_DENIED, gen.k_fetch(2, 3, "c", TOPICS)]
    D, v, out, _ = _run_small(engine, reqs, np.array([R2_CONN, K_CONN, R2_CONN, K_CONN], np.uint32))
    assert (v == DENY).all()
    exp = [R2D2_ERROR, _lib.kafka_deny_response(big), R2D2_ERROR, _lib.kafka_deny_response(reqs[3])]
    assert len(exp[1]) > 3.9 * len(big)
    _check(exp, out, int(out[3][0]))


# ------------------------------------------------------------------ 8. host twin
def test_host_twin(engine, mixed, mixed_run):
    M = mixed
    D, d_v, (v, _, _, _), full = mixed_run
    _use_mixed(engine, M)
    total = int(full[3][0])
    for cap in (total, total // 3, 0):
        mine = np.full(cap + GUARD, CANARY, np.uint8)
        buf, off, ln, tot = engine.deny_replies_arrays(M.arena, M.offs, M.lens, M.cids, v, cap, buf=mine)
        assert np.array_equal(off, full[1]) and np.array_equal(ln, full[2]) and np.array_equal(tot, full[3])
        _check(_mixed_expect(M, v), (buf, off, ln, tot), cap)
    got = engine.deny_replies(M.arena, M.offs, M.lens, M.cids, v)
    assert got == _mixed_expect(M, v)


# ------------------------------------------------------------------ 9. scale
def _one_percent_policy():
    """cfg3's generator names 1000 topics and, one time in ten, one of 1000
    "other-" topics: every topic allowed but the last 40 others, and the
    topic-less kinds it sends."""
    rules = [api.PortRuleKafka(topic=t) for t in gen.kafka_topics()]
    rules += [api.PortRuleKafka(topic=f"other-{j:04d}") for j in range(960)]
    rules += [api.PortRuleKafka(api_key=k) for k in ("metadata", "apiversions", "heartbeat")]
    return api.policy_set(api.network_policy("k1", 3, ingress=[(9092, [api.port_rule(kafka=rules)])]))


def _build_scale():
    """2^17 Kafka requests: 2^13 of cfg3's generator, 16 copies (gen.tile_offsets)."""
    w = gen.kafka_workload(1 << 13, seed=gen.SEED_BASE + 310)
    offs, lens, cids = gen.tile_offsets(w, 16)
    return w, offs, lens, cids


@pytest.fixture(scope="module")
def scale_batch():
    return _build_scale()


@pytest.mark.parametrize("leg", ["one_percent", "all"])
def test_scale(engine, scale_batch, leg):
    w, offs, lens, cids = scale_batch
    engine.update_policy(_one_percent_policy() if leg == "one_percent" else {"policies": [_kafka_deny_policy()]})
    engine.set_connections(w.conns)
    d_arena = torch.from_numpy(w.arena).to(torch.device("cuda", 0)).repeat(16)
    D = _Dev(None, offs, lens, cids, d_arena=d_arena)
    d_v, (v, _, _, _) = _classify(engine, D)
    frac = float((v == DENY).mean())
    if leg == "one_percent":
        assert 0.003 < frac < 0.03, frac
    else:
        assert frac > 0.99, frac  # (but for the few requests that do not parse)
    buf, off, ln, tot = _replies(engine, D, d_v)
    # sizes: every request's, from the unique part (a Kafka reply does not depend on where the request lies)
    u = w.n
    ureqs = _reqs(w.arena, w.offsets, w.lengths)
    vu = v.reshape(16, u)
    assert (vu == vu[0]).all()
    ulen = np.array([len(_expect_one(r, PROTO_KAFKA, x)) for r, x in zip(ureqs, vu[0])], np.uint64)
    want_len = np.tile(ulen, 16)
    assert np.array_equal(ln.astype(np.uint64), want_len)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(want_len)[:-1]]).astype(np.uint64))
    assert tot.tolist() == [int(want_len.sum()), int((want_len > 0).sum())]
    assert (buf[int(tot[0]):] == CANARY).all()
    # bytes: a fixed seeded sample of 2,000 denied requests against the host function
    denied = np.nonzero(v == DENY)[0]
    pick = np.random.default_rng(311).choice(denied, size=min(2000, len(denied)), replace=False)
    for i in pick.tolist():
        e = _expect_one(ureqs[i % u], PROTO_KAFKA, DENY)
        assert buf[int(off[i]):int(off[i]) + int(ln[i])].tobytes() == e, i


# ------------------------------------------------------------------ 10. classification untouched
def test_classification_untouched(engine, mixed, mixed_run):
    M = mixed
    D, d_v, before, full = mixed_run
    _use_mixed(engine, M)
    d_v1, first = _classify(engine, D)
    out = _replies(engine, D, d_v1)
    d_v2, second = _classify(engine, D)
    for a, b, c in zip(before, first, second):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert all(np.array_equal(x, y) for x, y in zip(out, full))

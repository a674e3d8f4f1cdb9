"""Access-log records of the logged classification calls (include/l7gpu.h:
l7g_classify_logged, l7g_classify_logged_host) on the device.

1. HTTP records against the oracle's ref_http_parse, Kafka records against
   tests/kafka_topics_py.py (pinned to the oracle by test_kafka_topics_py.py),
   wherever the device's verdict is ALLOW or DENY.
2. The logged calls give l7g_classify's verdict, rule, consumed and counters,
   and l7g_classify_logged_host gives l7g_classify_host's.
3. One batch of 2^20 requests (partition lists, both Kafka grids, the grouped
   HTTP path, the post-pass), records checked on a 20k sample."""
import ctypes as C

import numpy as np
import pytest
import torch

import kafka_topics_py
from cilium_amd import gen
from cilium_amd._lib import ALLOW, DENY, PROTO_HTTP, PROTO_KAFKA
from cilium_amd.engine import LOGREC_DTYPE, SPAN_DTYPE

pytestmark = pytest.mark.gpu

STRIDE = 4
CANARY = 0xC0FFEE11
BESIDE_MIN = 1 << 20  # engine_state.h kBesideMin


# ------------------------------------------------------------------ running
class _Out:
    pass


def _run_device(engine, w, stride=STRIDE, logged=True, arena=None, idx=None):
    """One device call over workload w (idx: these request indices, in this
    order); the outputs pre-filled, the topic rows with a canary."""
    dev = torch.device("cuda", 0)
    d_arena = torch.from_numpy(w.arena).to(dev) if arena is None else arena
    sel = slice(None) if idx is None else idx
    ins = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
           for a in (w.offsets[sel].view(np.int64), w.lengths[sel].view(np.int32), w.conn_ids[sel].view(np.int32))]
    n = ins[0].numel()
    o = [torch.full((n,), 7, dtype=t, device=dev) for t in (torch.uint8, torch.int32, torch.int32)]
    cnt = torch.zeros(engine.nrules + 8, dtype=torch.int64, device=dev)
    R = _Out()
    args = (d_arena.data_ptr(), d_arena.numel(), *[t.data_ptr() for t in ins], n, *[t.data_ptr() for t in o])
    if logged:
        rec = torch.full((n, 8), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        top = torch.full((n, max(stride, 1), 2), CANARY - (1 << 32), dtype=torch.int32, device=dev)
        engine.classify_logged_device(*args, rec.data_ptr(), top.data_ptr() if stride else 0, stride,
                                      counters_ptr=cnt.data_ptr())
        torch.cuda.synchronize()
        R.raw = rec.cpu().numpy().view(np.uint32)  # the records as 8 words each
        R.rec = R.raw.view(LOGREC_DTYPE).reshape(n)
        R.topics = top.cpu().numpy().view(np.uint32).reshape(n, max(stride, 1), 2)
    else:
        engine.classify_device(*args, counters_ptr=cnt.data_ptr())
        torch.cuda.synchronize()
    R.v, R.r, R.c = o[0].cpu().numpy(), o[1].cpu().numpy(), o[2].cpu().numpy().view(np.uint32)
    R.cnt = cnt.cpu().numpy()
    return R


def _install(engine, w):
    engine.update_policy(w.policy)
    engine.set_connections(w.conns)


def _req(w, i):
    o, n = int(w.offsets[i]), int(w.lengths[i])
    return w.arena[o:o + n].tobytes()


def _wl(reqs, base, seed, name):
    arena, offs, lens = gen.pack(reqs)
    cids = np.random.default_rng(seed).integers(0, len(base.conns), len(reqs)).astype(np.uint32)
    return gen.Workload(name, arena, offs, lens, cids, base.conns, base.policy)


# ------------------------------------------------------------------ HTTP reference
class _HttpInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("method_off", C.c_int32), ("method_len", C.c_int32), ("path_off", C.c_int32),
                ("path_len", C.c_int32), ("host_off", C.c_int32), ("host_len", C.c_int32), ("consumed", C.c_uint32),
                ("nheaders", C.c_int32)]


@pytest.fixture(scope="module")
def http_parse(oracle):
    lib = oracle.load()
    lib.ref_http_parse.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(_HttpInfo)]

    def parse(data):
        info = _HttpInfo()
        lib.ref_http_parse(data, len(data), C.byref(info))
        return info
    return parse


def _check_http(http_parse, data, rec, where):
    info = http_parse(data)
    assert info.status == ALLOW, where  # ("ok": the device answered ALLOW / DENY, so the head frames)
    assert rec["kind"] == 1, where
    assert (rec["method_len"], rec["path_len"]) == (info.method_len, info.path_len), where
    assert info.method_off == 0 and info.path_off == info.method_len + 1
    assert bool(rec["flags"] & 1) == (info.host_off >= 0), where
    if info.host_off >= 0:
        assert (rec["host_off"], rec["host_len"]) == (info.host_off, info.host_len), where
    assert rec["nheaders"] == info.nheaders, where
    assert rec["head_len"] == data.find(b"\r\n\r\n") + 4, where
    ver = data[info.path_off + info.path_len + 1:][5:8]
    assert rec["api_key"] == ((ver[0] - 48) << 4 | (ver[2] - 48)), where


def _check_http_workload(engine, http_parse, w, need=1):
    _install(engine, w)
    R = _run_device(engine, w)
    hit = np.nonzero((R.v == ALLOW) | (R.v == DENY))[0]
    assert len(hit) >= need, (w.name, len(hit))
    for i in hit:
        _check_http(http_parse, _req(w, i), R.rec[i], (w.name, int(i)))
    return R


@pytest.mark.parametrize("cfg", [1, 2])
def test_http_records_cfg(engine, http_parse, cfg):
    _check_http_workload(engine, http_parse, gen.http_workload(cfg, 3000, seed=gen.SEED_BASE + 90 + cfg), 3000)


@pytest.mark.parametrize("kind", ["adversarial", "chunked"])
def test_http_records_adversarial_and_chunked(engine, http_parse, kind):
    reqs = gen.http_adversarial(4000, 4243) if kind == "adversarial" else gen.http_chunked(4000, 2025)
    _check_http_workload(engine, http_parse, _wl(reqs, gen.http_workload(2, 1), 5, kind), 500)


# ---- the hand-built edge set
def _http(lines, method=b"GET", target=b"/x", version=b"HTTP/1.1", body=b""):
    return method + b" " + target + b" " + version + b"\r\n" + b"".join(x + b"\r\n" for x in lines) + b"\r\n" + body


def _host_at(x, host_line=b"Host: svc-1.ns.svc.cluster.local", after=(b"Accept: */*",)):
    """A request whose Host line starts at head offset x (a padding header slides it)."""
    k = x - 24  # "GET /x HTTP/1.1\r\n" is 17 bytes, "X-P: " + pad + CRLF is 7 + k
    assert k >= 0
    r = _http([b"X-P: " + b"a" * k, host_line, *after])
    assert r.find(host_line) == x
    return r


def _edge_requests():
    out = []
    # the Host line's name, colon, value and CRLF across every 16-byte chunk edge,
    # and across the 256-byte window edges
    for x in list(range(24, 66)) + list(range(230, 276)) + list(range(486, 532)):
        out.append(_host_at(x))
    variants = [
        [b"Accept: */*"],                                       # no Host
        [b"Host: first.example", b"Host: second.example"],      # twice: the first wins
        [b"HOST: upper.example"], [b"hOsT: mixed.example"],
        [b"hostx: not.host"], [b"x-host: not.host"], [b"hostx: a", b"x-host: b", b"Host: real.example"],
        [b"Host:"], [b"Host: "], [b"Host: \t a \t"], [b"Host:a"], [b"Host: \t \t"],
        [b"Accept: */*", b"X-Q: 1", b"Host: last.example"],     # Host as the last line
        [b"H: h", b"Ho: ho", b"Hos: hos", b"Hosts: x"],
        [b"X-V: host: inside.a.value", b"Host: after.example"],
    ]
    for lines in variants:
        out.append(_http(lines))
        for x in (40, 250, 251, 252, 253, 254, 255, 256, 257, 258, 506, 510, 512):  # the same, slid
            out.append(_http([b"X-P: " + b"b" * (x - 24)] + lines))
    out.append(_http([b"Host: m.example"], method=b"G"))               # a one-byte method
    for tl in (1, 300, 1500):                                           # short and long targets
        out.append(_http([b"Host: t.example"], target=b"/" + b"p" * (tl - 1)))
        out.append(_http([b"Accept: */*", b"Host: t.example"], method=b"DELETE", target=b"/" + b"q" * (tl - 1)))
    out.append(_http([b"Host: old.example"], version=b"HTTP/1.0"))
    out.append(_http([]))                                               # no header lines
    out.append(_http([], target=b"/" + b"r" * 236))                     # ... the empty line across the window edge
    for tl in range(233, 243):
        out.append(_http([], target=b"/" + b"s" * tl))
    out.append(_http([b"X-%d: v%d" % (k, k) for k in range(69)] + [b"Host: seventy.example"]))  # 70 header lines
    out.append(_http([b"X-%d: v%d" % (k, k) for k in range(70)]))
    # a body that looks like a head
    out.append(_http([b"Host: b.example", b"Content-Length: 21"], method=b"POST", body=b"\r\n\r\nHost: body\r\n\r\n \r\n"))
    return out


def _pack_aligned(reqs):
    """Every request at every arena alignment 0-15; the gaps are filled with
    CRs, LFs, SPs and colons; the last request ends on the arena's last byte."""
    filler = b"\r\n\r\n \r:\r\n\r\nhost: gap\r\n\r\n" * 2
    buf, offs, lens = bytearray(), [], []
    for a in range(16):
        for r in reqs:
            buf += filler[:(a - len(buf)) % 16]
            offs.append(len(buf))
            lens.append(len(r))
            buf += r
    return (np.frombuffer(bytes(buf), np.uint8).copy(), np.asarray(offs, np.uint64), np.asarray(lens, np.uint32))


def test_http_records_edge_set(engine, http_parse):
    reqs = _edge_requests()
    ok = sum(http_parse(r).status == ALLOW for r in reqs)
    assert ok >= 0.9 * len(reqs), (ok, len(reqs))  # (checked on the CPU: the comparison cannot run empty)
    base = gen.http_workload(2, 1)
    arena, offs, lens = _pack_aligned(reqs)
    assert int(offs[-1]) + int(lens[-1]) == len(arena)
    assert sorted(set((offs % 16).tolist())) == list(range(16))
    cids = np.random.default_rng(11).integers(0, len(base.conns), len(offs)).astype(np.uint32)
    w = gen.Workload("edges", arena, offs, lens, cids, base.conns, base.policy)
    R = _check_http_workload(engine, http_parse, w, int(0.9 * len(offs)))
    # spot checks of what the reference comparison implies
    i = reqs.index(_http([b"Host: first.example", b"Host: second.example"]))
    r = R.rec[i]
    assert reqs[i][r["host_off"]:r["host_off"] + r["host_len"]] == b"first.example"
    i = reqs.index(_http([b"Host: \t a \t"]))
    assert (R.rec[i]["host_len"], R.rec[i]["flags"] & 1) == (1, 1)
    i = reqs.index(_http([b"Host:"]))
    assert (R.rec[i]["host_len"], R.rec[i]["flags"] & 1) == (0, 1)
    i = reqs.index(_http([b"hostx: not.host"]))
    assert R.rec[i]["flags"] & 1 == 0


# ------------------------------------------------------------------ Kafka
def _check_kafka(data, rec, row, stride, where):
    p = kafka_topics_py.parse(data)
    assert p is not None, where
    assert rec["kind"] == 2, where
    assert (rec["api_key"], rec["api_version"], rec["correlation_id"]) == \
        (p["api_key"], p["api_version"], p["correlation_id"]), where
    nt = len(p["topics"])
    assert rec["ntopics"] == nt, where
    assert (rec["flags"] & 1) == (nt > stride), where
    k = min(nt, stride)
    if stride:
        assert [tuple(x) for x in row[:k].tolist()] == p["topics"][:k], where
        assert (row[k:] == CANARY).all(), where  # the rest of the row is not written
    return p


def _kafka_base():
    return gen.kafka_workload(16, seed=gen.SEED_BASE + 75)


KAFKA_GENS = {
    "all_kinds": lambda: gen.kafka_all_kinds(2000, gen.SEED_BASE + 81),
    "requests": lambda: gen.kafka_requests(2000, gen.SEED_BASE + 82),
    "adversarial": lambda: gen.kafka_adversarial(2000, gen.SEED_BASE + 83),
    "compressed": lambda: gen.kafka_compressed_requests(500, gen.SEED_BASE + 84),
}


@pytest.mark.parametrize("name", list(KAFKA_GENS))
def test_kafka_records_generators(engine, name):
    w = _wl(KAFKA_GENS[name](), _kafka_base(), 12, name)
    _install(engine, w)
    R = _run_device(engine, w)
    hit = np.nonzero((R.v == ALLOW) | (R.v == DENY))[0]
    assert len(hit) >= w.n // 4, (name, len(hit))
    for i in hit:
        _check_kafka(_req(w, i), R.rec[i], R.topics[i], STRIDE, (name, int(i)))


def _msg(v=b"value", **kw):
    return gen.k_message(v, **kw)


def _kafka_hand_built():
    T = [f"topic-{i:04d}" for i in range(300)]
    parts = [0]
    reqs = {
        "no_topics": gen.k_metadata(1, 1, "c", []),
        "null_metadata": gen.k_metadata(1, 2, "c", None),
        "null_offset_fetch": gen.k_offset_fetch(2, 3, "c", "grp", None),
        "consumer_metadata": gen.k_consumer_metadata(0, 4, "c", "grp"),
        "stride": gen.k_fetch(2, 5, "c", [(t, parts) for t in T[:STRIDE]]),
        "stride_plus_1": gen.k_fetch(2, 6, "c", [(t, parts) for t in T[:STRIDE + 1]]),
        "many": gen.k_metadata(0, 7, "c", T),
        "duplicates_and_empty": gen.k_offset(1, 8, "c", [("dup", parts), ("", parts), ("dup", parts)]),
        "negative_correlation": gen.k_metadata(0, -5, "c", ["topic-0001"]),
        "unknown_key": gen.k_request(77, 1, 9, "c", b"\x00" * 6),
        # the first topic's second partition stops at a bad CRC: mid-set (the
        # outer decoder resumes inside the set) and at the set's end
        "bad_crc_mid": gen.k_produce(1, 10, "c", [("topic-0001", [(0, [_msg(version=1)]),
                                                                 (1, [_msg(version=1, bad_crc=True), _msg(version=1)])]),
                                                  ("topic-0002", [(0, [_msg(version=1)])])]),
        "bad_crc_last": gen.k_produce(1, 11, "c", [("topic-0001", [(0, [_msg(version=1)]),
                                                                  (1, [_msg(version=1), _msg(version=1, bad_crc=True)])]),
                                                   ("topic-0002", [(0, [_msg(version=1)])])]),
    }
    return reqs


def test_kafka_records_hand_built(engine):
    named = _kafka_hand_built()
    names = list(named)
    base = _kafka_base()
    arena, offs, lens = gen.pack([named[k] for k in names])
    cids = np.zeros(len(names), np.uint32)
    # behind the request with one topic too many: a request no classifier owns, whose row stays as it was
    at = names.index("stride_plus_1") + 1
    names.insert(at, "unowned")
    offs, lens = np.insert(offs, at, offs[at - 1]), np.insert(lens, at, lens[at - 1])
    cids = np.insert(cids, at, len(base.conns) + 5).astype(np.uint32)
    w = gen.Workload("hand", arena, offs, lens, cids, base.conns, base.policy)
    _install(engine, w)
    R = _run_device(engine, w)
    P = {}
    for i, k in enumerate(names):
        if k == "unowned":
            assert R.v[i] not in (ALLOW, DENY) and (R.topics[i] == CANARY).all()
            continue
        data = _req(w, i)
        if k.startswith("bad_crc"):
            # the helper and the device agree on whether the request decodes
            assert (kafka_topics_py.parse(data) is not None) == (R.v[i] in (ALLOW, DENY)), (k, R.v[i])
            if R.v[i] not in (ALLOW, DENY):
                continue
        assert R.v[i] in (ALLOW, DENY), (k, R.v[i])
        P[k] = _check_kafka(data, R.rec[i], R.topics[i], STRIDE, k)
    rec = dict(zip(names, R.rec))
    for k in ("no_topics", "null_metadata", "null_offset_fetch", "consumer_metadata", "unknown_key"):
        assert rec[k]["ntopics"] == 0 and rec[k]["flags"] & 1 == 0, k
    assert rec["unknown_key"]["api_key"] == 77 and rec["negative_correlation"]["correlation_id"] == -5
    assert (rec["stride"]["ntopics"], rec["stride"]["flags"] & 1) == (STRIDE, 0)
    assert (rec["stride_plus_1"]["ntopics"], rec["stride_plus_1"]["flags"] & 1) == (STRIDE + 1, 1)
    assert (rec["many"]["ntopics"], rec["many"]["flags"] & 1) == (300, 1)
    assert rec["duplicates_and_empty"]["ntopics"] == 3
    assert R.topics[names.index("duplicates_and_empty")][1].tolist() == [0, 0]
    assert "bad_crc_last" in P and len(P["bad_crc_last"]["topics"]) == 2
    # the request with 300 topics again, alone, with a stride of its ntopics
    i = names.index("many")
    one = gen.Workload("many", arena, offs[i:i + 1], lens[i:i + 1], cids[i:i + 1], base.conns, base.policy)
    R1 = _run_device(engine, one, stride=300)
    p = _check_kafka(_req(one, 0), R1.rec[0], R1.topics[0], 300, "many alone")
    assert len(p["topics"]) == 300 and R1.rec[0]["flags"] & 1 == 0
    # and the whole set once without topic rows
    R0 = _run_device(engine, w, stride=0)
    for i, k in enumerate(names):
        if R0.v[i] in (ALLOW, DENY):
            _check_kafka(_req(w, i), R0.rec[i], None, 0, (k, "stride 0"))
    assert (R0.v == R.v).all()


# ------------------------------------------------------------------ same answers
def _workload(name):
    if name in ("cfg1", "cfg2"):
        return gen.http_workload(int(name[3]), 3000, seed=gen.SEED_BASE + 95)
    if name == "http_adversarial":
        return _wl(gen.http_adversarial(3000, 4244), gen.http_workload(2, 1), 5, name)
    if name == "http_chunked":
        return _wl(gen.http_chunked(3000, 2026), gen.http_workload(2, 1), 6, name)
    if name.startswith("kafka_"):
        return _wl(KAFKA_GENS[name[6:]](), _kafka_base(), 13, name)
    if name == "r2d2":
        return gen.r2d2_workload(2000)
    if name == "cassandra":
        return gen.cassandra_workload(2000)
    assert name == "mixed"
    return gen.mixed_workload(20000)


@pytest.mark.parametrize("name", ["cfg1", "cfg2", "http_adversarial", "http_chunked"] +
                         ["kafka_" + k for k in KAFKA_GENS] + ["mixed", "r2d2", "cassandra"])
def test_logged_calls_answer_as_the_plain_ones(engine, name):
    w = _workload(name)
    _install(engine, w)
    A = _run_device(engine, w, logged=False)
    B = _run_device(engine, w)
    for f in ("v", "r", "c", "cnt"):
        assert np.array_equal(getattr(A, f), getattr(B, f)), (name, f)
    # the host twins
    hv, hr, hc = engine.classify(w.arena, w.offsets, w.lengths, w.conn_ids)
    canary = np.empty((w.n, STRIDE), SPAN_DTYPE)
    canary["off"] = canary["len"] = CANARY
    lv, lr, lc, rec, topics = engine.classify_logged(w.arena, w.offsets, w.lengths, w.conn_ids, STRIDE, topics=canary)
    assert np.array_equal(hv, lv) and np.array_equal(hr, lr) and np.array_equal(hc, lc), name
    assert np.array_equal(hv, A.v) and np.array_equal(hr, A.r) and np.array_equal(hc, A.c), name
    done = (lv == ALLOW) | (lv == DENY)
    assert np.array_equal(rec.view(np.uint32).reshape(w.n, 8)[done], B.raw[done]), name
    proto = w.conns["proto"][np.minimum(w.conn_ids, len(w.conns) - 1)]
    other = done & (proto != PROTO_HTTP) & (proto != PROTO_KAFKA)
    assert (rec["kind"][other] == 0).all() and (B.rec["kind"][other] == 0).all(), name
    assert (rec["kind"][done & (proto == PROTO_HTTP)] == 1).all() and (rec["kind"][done & (proto == PROTO_KAFKA)] == 2).all()
    # rows of requests that are not Kafka come back as they went in
    t = topics.view(np.uint32).reshape(w.n, STRIDE, 2)
    assert (t[proto != PROTO_KAFKA] == CANARY).all() and (B.topics[proto != PROTO_KAFKA] == CANARY).all(), name
    assert np.array_equal(t[done], B.topics[done]), name
    if name in ("r2d2", "cassandra", "mixed"):
        assert other.any(), name


# ------------------------------------------------------------------ the big paths
def test_one_batch_of_2_20_requests(engine, http_parse):
    """A mixed batch tiled to kBesideMin requests: the partition lists, the
    Kafka grid beside memcached and the helper grid behind it (logged
    instantiations), HTTP requests on two rule sets (the grouped path), and the
    post-pass over all of it."""
    h2 = gen.http_workload(2, 4000, seed=gen.SEED_BASE + 71)
    h1 = gen.http_workload(1, 2000, nconns=64, seed=gen.SEED_BASE + 70)
    kreqs = (gen.kafka_requests(2500, gen.SEED_BASE + 72) + gen.kafka_compressed_requests(600, gen.SEED_BASE + 73) +
             gen.kafka_adversarial(900, gen.SEED_BASE + 74))
    k = _wl(kreqs, _kafka_base(), 76, "k")
    m = gen.memcache_workload(5000, seed=gen.SEED_BASE + 77)
    parts = [h2, k, m, h1]
    pol = {"policies": [dict(p.policy["policies"][0], name=f"10.0.0.{j + 1}") for j, p in enumerate(parts)]}
    conns = np.concatenate([p.conns for p in parts])
    arena = np.concatenate([p.arena for p in parts])
    offs, cids, a0, c0 = [], [], 0, 0
    for j, p in enumerate(parts):
        conns["policy"][c0:c0 + len(p.conns)] = j
        offs.append(p.offsets + np.uint64(a0))
        cids.append(p.conn_ids + np.uint32(c0))
        a0 += len(p.arena)
        c0 += len(p.conns)
    w = gen.Workload("big", arena, np.concatenate(offs), np.concatenate([p.lengths for p in parts]),
                     np.concatenate(cids), conns, pol)
    _install(engine, w)
    n = BESIDE_MIN + 4321
    idx = np.tile(np.arange(w.n), -(-n // w.n))[:n]
    np.random.default_rng(3).shuffle(idx)
    d_arena = torch.from_numpy(w.arena).to(torch.device("cuda", 0))
    A = _run_device(engine, w, logged=False, arena=d_arena, idx=idx)
    B = _run_device(engine, w, arena=d_arena, idx=idx)
    for f in ("v", "r", "c", "cnt"):
        assert np.array_equal(getattr(A, f), getattr(B, f)), f
    proto = w.conns["proto"][w.conn_ids[idx]]
    done = (B.v == ALLOW) | (B.v == DENY)
    assert (B.rec["kind"][done & (proto == PROTO_HTTP)] == 1).all()
    assert (B.rec["kind"][done & (proto == PROTO_KAFKA)] == 2).all()
    assert (B.rec["kind"][done & (proto != PROTO_HTTP) & (proto != PROTO_KAFKA)] == 0).all()
    assert (B.topics[proto != PROTO_KAFKA] == CANARY).all()
    # every copy of a request has the record of its first copy; the first copies of a 20k sample are checked
    first = np.full(w.n, -1, np.int64)
    first[idx[::-1]] = np.arange(n)[::-1]
    same = done & done[first[idx]]
    assert np.array_equal(B.raw[same], B.raw[first[idx]][same])
    ks = proto == PROTO_KAFKA
    assert np.array_equal(B.topics[same & ks], B.topics[first[idx]][same & ks])
    sample = np.random.default_rng(4).choice(n, 20000, replace=False)
    seen = set()
    for j in sample:
        u = int(idx[j])
        if u in seen or not done[j]:
            continue
        seen.add(u)
        if proto[j] == PROTO_HTTP:
            _check_http(http_parse, _req(w, u), B.rec[j], ("big", u))
        elif proto[j] == PROTO_KAFKA:
            _check_kafka(_req(w, u), B.rec[j], B.topics[j], STRIDE, ("big", u))
    assert len(seen) > 5000

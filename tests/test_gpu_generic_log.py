"""Access-log records of memcached, r2d2 and cassandra requests on the device
(include/l7gpu.h: l7g_classify_logged_all, l7g_classify_logged_all_host).

Wherever the device's verdict is ALLOW or DENY the record, the span row and the
text row are compared with tests/generic_log_py.py (the parsers' Go restated;
pinned by tests/test_generic_log_py.py) and, for cassandra, with the oracle's
parser walked over each connection's requests in batch order (refpy.Cassandra).
Every comparison is exact.  Rows are pre-filled: what no kernel owns, and every
byte past a row's written prefix, must keep the fill.

Limits of the feature that the session test pins as documented (l7gpu.h): a
resolved EXECUTE whose stored statement's table was cut at a '/' is logged with
the cut table, and one whose stored action is outside queryActionMap has flags
bit2 instead of an action word.

The last test drives requests through the proxylib shim's OnData as well and
compares log_entries() with the LogEntry records the shim sends (the socket
helpers of tests/test_gpu_accesslog.py, imported unchanged)."""
import ctypes as C

import numpy as np
import pytest
import torch

import generic_log_py as G
from cilium_amd import _lib, gen
from cilium_amd._lib import ALLOW, DENY, PROTO_CASSANDRA, PROTO_HTTP, PROTO_KAFKA, PROTO_MEMCACHE, PROTO_R2D2
from cilium_amd.engine import LOGREC_DTYPE, SPAN_DTYPE, log_entries

pytestmark = pytest.mark.gpu

SPAN_STRIDE, TEXT_STRIDE = 4, 24
SPAN_FILL, TEXT_FILL, REC_FILL = 0xC0FFEE11, 0xA5, 0x5A5A5A5A
SPACES = [chr(c).encode() for c in [0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000] +
          list(range(0x2000, 0x200B))]


# ------------------------------------------------------------------ running
class _Out:
    pass


def _run(engine, w, span_stride=SPAN_STRIDE, text_stride=TEXT_STRIDE, call="all", arena=None):
    """One device call over workload w: "all" l7g_classify_logged_all, "logged"
    l7g_classify_logged, "plain" l7g_classify; every output pre-filled."""
    dev = torch.device("cuda", 0)
    d_arena = torch.from_numpy(w.arena).to(dev) if arena is None else arena
    ins = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
           for a in (w.offsets.view(np.int64), w.lengths.view(np.int32), w.conn_ids.view(np.int32))]
    n = ins[0].numel()
    o = [torch.full((n,), 7, dtype=t, device=dev) for t in (torch.uint8, torch.int32, torch.int32)]
    cnt = torch.zeros(engine.nrules + 8, dtype=torch.int64, device=dev)
    R = _Out()
    args = (d_arena.data_ptr(), d_arena.numel(), *[t.data_ptr() for t in ins], n, *[t.data_ptr() for t in o])
    if call == "plain":
        engine.classify_device(*args, counters_ptr=cnt.data_ptr())
    else:
        rec = torch.full((n, 8), REC_FILL, dtype=torch.int32, device=dev)
        spans = torch.full((n, max(span_stride, 1), 2), SPAN_FILL - (1 << 32), dtype=torch.int32, device=dev)
        text = torch.full((n, max(text_stride, 1)), TEXT_FILL, dtype=torch.uint8, device=dev)
        if call == "all":
            engine.classify_logged_all_device(*args, rec.data_ptr(), spans.data_ptr() if span_stride else 0, span_stride,
                                              text.data_ptr() if text_stride else 0, text_stride,
                                              counters_ptr=cnt.data_ptr())
        else:
            engine.classify_logged_device(*args, rec.data_ptr(), spans.data_ptr() if span_stride else 0, span_stride,
                                          counters_ptr=cnt.data_ptr())
        torch.cuda.synchronize()
        R.raw = rec.cpu().numpy().view(np.uint32)
        R.rec = R.raw.view(LOGREC_DTYPE).reshape(n)
        R.spans = spans.cpu().numpy().view(np.uint32).reshape(n, max(span_stride, 1), 2)
        R.text = text.cpu().numpy()
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


@pytest.fixture(scope="module")
def base():
    """Connections and policies of the three parsers in one table: memcached
    (text / binary by first byte), r2d2, cassandra, each with an allowing and a
    denying remote."""
    m, r, c = gen.memcache_workload(8, nconns=8), gen.r2d2_workload(8, nconns=7), gen.cassandra_workload(8, nconns=7)
    conns = np.concatenate([m.conns, r.conns, c.conns])
    conns["policy"][8:15] = 1
    conns["policy"][15:] = 2
    pol = {"policies": [m.policy["policies"][0], r.policy["policies"][0], c.policy["policies"][0]]}
    b = _Out()
    b.conns, b.policy = conns, pol
    b.mc, b.r2, b.cs = list(range(0, 8)), list(range(8, 15)), list(range(15, 22))
    return b


def _wl(base, reqs, cids, align=None):
    """A workload over base's connections; align: every request starts at this
    offset mod 16 (the arena padded between requests)."""
    if align is None:
        arena, offs, lens = gen.pack(reqs)
    else:
        buf, offs = bytearray(), []
        for q in reqs:
            while len(buf) % 16 != align:
                buf.append(0x20)
            offs.append(len(buf))
            buf += q
        arena = np.frombuffer(bytes(buf), np.uint8).copy()
        offs = np.array(offs, np.uint64)
        lens = np.array([len(q) for q in reqs], np.uint32)
    return gen.Workload("generic-log", arena, offs, lens, np.asarray(cids, np.uint32), base.conns, base.policy)


# ------------------------------------------------------------------ expectations
def _cass_paths(oracle, w):
    """The oracle's parser per connection over the batch in order: the path of
    every cassandra request the parser passes or drops (else None)."""
    pol = oracle.Policy(w.policy)
    refs, out = {}, [None] * w.n
    for i in range(w.n):
        ci = int(w.conn_ids[i])
        if ci >= len(w.conns) or w.conns[ci]["proto"] != PROTO_CASSANDRA:
            continue
        if ci not in refs:
            refs[ci] = oracle.Cassandra(pol, w.conns[ci:ci + 1])
        op, _, _, path, _ = refs[ci].request(_req(w, i))
        out[i] = (op, path)
    return out


def _want(w, i, cass):
    conn = w.conns[int(w.conn_ids[i])]
    data = _req(w, i)
    if conn["proto"] == PROTO_MEMCACHE:
        return G.memcached(data, int(conn["flags"]))
    if conn["proto"] == PROTO_R2D2:
        return G.r2d2(data)
    if conn["proto"] == PROTO_CASSANDRA:
        op, path = cass[i]
        assert op in (1, 2), (i, op, data)  # the oracle passes or drops what the device allowed or denied
        assert b"\x00" not in (path or b"")
        return {"proto": "cassandra", "entry": G.cassandra_path(path)}
    return None


def _check(oracle, w, R, span_stride=SPAN_STRIDE, text_stride=TEXT_STRIDE, need=()):
    """Every record and row of R against the restatement; returns how many
    records of each kind were checked.  need: kinds that must occur."""
    cass = _cass_paths(oracle, w)
    seen = {3: 0, 4: 0, 5: 0, 6: 0, "cass_logged": 0}
    S = max(span_stride, 1)
    entries = None
    trunc = (R.rec["flags"] & 1).astype(bool) & (R.rec["kind"] >= 3)
    for i in range(w.n):
        ci = int(w.conn_ids[i])
        proto = int(w.conns[ci]["proto"]) if ci < len(w.conns) else 0
        rec, where = R.rec[i], (i, _req(w, i)[:80])
        live = R.v[i] in (ALLOW, DENY)
        spans, text = R.spans[i], R.text[i]
        nspan = ntext = 0  # the prefix of each row the request may have written
        if live and proto in (PROTO_MEMCACHE, PROTO_R2D2, PROTO_CASSANDRA):
            want = _want(w, i, cass)
            assert want is not None, where
            assert int(R.raw[i][5]) == 0 and int(R.raw[i][6]) == 0 and int(R.raw[i][7]) == 0, where
            if want["proto"] == "textmemcached":
                assert rec["kind"] == 3 and rec["api_key"] == 0, where
                assert (rec["mc_cmd_off"], rec["mc_cmd_len"]) == want["cmd"], where
                assert rec["mc_nkeys"] == len(want["keys"]), where
                assert rec["flags"] == (1 if len(want["keys"]) > span_stride else 0), where
                nspan = min(len(want["keys"]), span_stride)
                assert [tuple(int(x) for x in s) for s in spans[:nspan]] == want["keys"][:nspan], where
            elif want["proto"] == "binarymemcached":
                assert rec["kind"] == 4 and rec["flags"] == 0 and rec["api_key"] == want["opcode"], where
                assert (rec["mcb_key_off"], rec["mcb_key_len"]) == want["key"], where
            elif want["proto"] == "r2d2":
                assert rec["kind"] == 5 and rec["flags"] == 0 and rec["api_key"] == 0, where
                assert rec["r2_cmd_len"] == want["cmd_len"] and rec["r2_nfields"] == want["nfields"], where
                assert (rec["r2_file_off"], rec["r2_file_len"]) == want["file"], where
            else:
                assert rec["kind"] == 6, where
                e = want["entry"]
                assert bool(rec["flags"] & 2) == (e is not None), (where, cass[i])
                ntext = min(int(rec["cass_table_len"]), text_stride)
                if e is not None:
                    table = e["fields"]["query_table"]
                    assert rec["cass_table_len"] == len(table), (where, table)
                    assert bool(rec["flags"] & 1) == (len(table) > text_stride), where
                    assert text[:ntext].tobytes() == table[:ntext], (where, table)
                    assert not rec["flags"] & 4, where
                    seen["cass_logged"] += 1
            seen[int(rec["kind"])] += 1
            if not trunc[i]:  # the whole entry, through the public helper
                if entries is None:
                    entries = log_entries(R.v, _untruncated(R.rec, trunc), R.spans.view(SPAN_DTYPE).reshape(w.n, S),
                                          R.text, w.arena, w.offsets, w.lengths)
                et = "Request" if R.v[i] == ALLOW else "Denied"
                if want["proto"] == "cassandra":
                    e = want["entry"]
                    assert entries[i] == (None if e is None else (et, "cassandra", e["fields"])), where
                else:
                    assert entries[i] == (et, want["proto"], want["fields"]), where
        elif proto not in (PROTO_HTTP, PROTO_KAFKA):
            assert not live or rec["kind"] == 0, where
        if proto == PROTO_KAFKA:
            continue  # (its rows: tests/test_gpu_access_log.py)
        assert (spans[nspan:] == SPAN_FILL).all() if span_stride else (spans == SPAN_FILL).all(), where
        assert (text[ntext:] == TEXT_FILL).all() if text_stride else (text == TEXT_FILL).all(), where
    for k in need:
        assert seen[k] > 0, (k, seen)
    return seen


def _untruncated(rec, trunc):
    """The records with the truncated ones blanked (log_entries raises on those)."""
    r = rec.copy()
    r["kind"][trunc] = 0
    return r


def _same_answers(a, b):
    assert np.array_equal(a.v, b.v) and np.array_equal(a.r, b.r) and np.array_equal(a.c, b.c)
    assert np.array_equal(a.cnt, b.cnt)


# ------------------------------------------------------------------ 1. generators
@pytest.mark.parametrize("name", ["memcache", "memcache_adversarial", "r2d2", "cassandra"])
def test_generated_workloads(engine, oracle, name):
    w = {"memcache": lambda: gen.memcache_workload(3000),
         "memcache_adversarial": lambda: gen.memcache_workload(3000, adversarial=True),
         "r2d2": lambda: gen.r2d2_workload(2000),
         "cassandra": lambda: gen.cassandra_workload(3000)}[name]()
    _install(engine, w)
    R = _run(engine, w)
    _same_answers(R, _run(engine, w, call="plain"))
    need = {"memcache": (3, 4), "memcache_adversarial": (3, 4), "r2d2": (5,), "cassandra": (6, "cass_logged")}[name]
    seen = _check(oracle, w, R, need=need)
    assert sum(seen[k] for k in (3, 4, 5, 6)) > w.n // 4, seen


def test_mixed_workload_http_and_kafka_as_logged(engine, oracle):
    w = gen.mixed_workload(4000)
    _install(engine, w)
    A, L, P = _run(engine, w), _run(engine, w, call="logged"), _run(engine, w, call="plain")
    _same_answers(A, P)
    _same_answers(L, P)
    proto = w.conns["proto"][w.conn_ids]
    live = (A.v == ALLOW) | (A.v == DENY)
    hk = (proto == PROTO_HTTP) | (proto == PROTO_KAFKA)
    assert (live & hk).sum() > 1000
    assert np.array_equal(A.raw[live & hk], L.raw[live & hk])
    assert np.array_equal(A.spans[hk], L.spans[hk])      # Kafka rows as l7g_classify_logged writes them
    assert (L.rec["kind"][live & ~hk] == 0).all()        # (what the older call answers for memcached)
    assert (A.text == TEXT_FILL).all()
    _check(oracle, w, A, need=(3, 4))


# ------------------------------------------------------------------ 2. alignment, arena end
def test_all_alignments_and_the_arena_end(engine, oracle, base):
    _install(engine, base)
    one = [b"  get user:1 k2 k3\r\n", b"set cache:a 0 0 100\r\nabc", gen.mc_bin(1, b"user:7", bytes(8), b"v" * 5),
           b"READ /pub/a\r\n", gen.cass_query_frame("select * from Ks1.Users"), gen.cass_query_frame("use ks9"),
           gen.cass_query_frame("insert into users (a) values (1)")]
    cids = [base.mc[0], base.mc[1], base.mc[2], base.r2[2], base.cs[2], base.cs[2], base.cs[2]]
    for a in range(16):
        for k in (a % 7, (a + 3) % 7):  # rotated: each request is the arena's last at some alignments
            reqs, ids = one[k:] + one[:k], cids[k:] + cids[:k]
            w = _wl(base, reqs, ids, align=a)
            assert int(w.offsets[-1] + w.lengths[-1]) == len(w.arena)
            R = _run(engine, w)
            seen = _check(oracle, w, R, need=(3, 4, 5, 6))
            assert seen[3] == 2 and seen[6] == 3 and seen["cass_logged"] == 3, (a, seen)
    # every request alone in an arena that ends with its last byte
    for q, ci in zip(one, cids):
        w = _wl(base, [q], [ci], align=5)
        _check(oracle, w, _run(engine, w))


# ------------------------------------------------------------------ 3. memcached text tokens
def test_text_token_boundaries(engine, oracle, base):
    _install(engine, base)
    reqs = []
    for at in (14, 15, 16, 17, 254, 255, 256, 257):
        key = b"k" * (at - 4)
        reqs.append(b"get " + key + b"\r\n")                     # the line's CRLF at `at`
        reqs.append(b"get " + key + b" z\r\n")                   # a token boundary
        for sp in SPACES:
            reqs.append(b"get " + key + sp + b"zz\r\n")          # each multi-byte space
            reqs.append(b"get " + key + sp[:-1] + b"zz\r\n")     # and its truncation: no space
        reqs.append(b"get" + b" " * (at - 3) + b"k\r\n")         # a run of spaces up to `at`
    w = _wl(base, reqs, [base.mc[0]] * len(reqs), align=0)
    R = _run(engine, w)
    assert ((R.v == ALLOW) | (R.v == DENY)).all()
    assert _check(oracle, w, R)[3] == len(reqs)
    w = _wl(base, reqs, [base.mc[1]] * len(reqs), align=9)
    assert _check(oracle, w, _run(engine, w))[3] == len(reqs)


def test_text_commands_and_strides(engine, oracle, base):
    _install(engine, base)
    S = SPAN_STRIDE
    reqs = [b"\t \xc2\xa0get a\r\n", b" \xe3\x80\x80delete tmp\r\n", b" \x0b\x0cversion\r\n"]
    reqs += [b"get " + b" ".join(b"k%d" % j for j in range(k)) + b"\r\n" for k in (1, S - 1, S, S + 1, 3 * S)]
    reqs += [b"gat 10\r\n", b"gat 10 a\r\n", b"gats 5 a bb ccc dddd eeeee\r\n", b"gatx 1 q\r\n", b"getq\r\n"]
    reqs += [b"set k 0 0 3\r\nabc\r\n", b"cas k 0 0 3 9 noreply\r\nabc\r\n", b"append k 0 0 700\r\nab",
             b"incr counter 2\r\n", b"decr counter 2\r\n", b"touch k 9\r\n", b"delete k noreply\r\n", b"stats a b\r\n",
             b"flush_all 5\r\n", b"get a\rb c\nd\r\n", b"get k\xc2\x85\r\n", b"get \xe2\x80\x8bk \xff\r\n"]
    w = _wl(base, reqs, [base.mc[k % 3] for k in range(len(reqs))])
    for stride in (S, 1, 0):
        R = _run(engine, w, span_stride=stride)
        assert ((R.v == ALLOW) | (R.v == DENY)).all()
        seen = _check(oracle, w, R, span_stride=stride)
        assert seen[3] == len(reqs)
    assert (R.rec["flags"][3:8] == 1).all()  # stride 0: every get with keys is truncated, no row is written


def test_binary_headers(engine, oracle, base):
    _install(engine, base)
    reqs = [gen.mc_bin(10, b"", bytes(4)), gen.mc_bin(0, b"user:1"), gen.mc_bin(1, b"session:0000abcd", bytes(20), b"vvv"),
            gen.mc_bin(1, b"k" * 250, bytes(8), b"x"), gen.mc_bin(7, b"", b"", b"", body=0), gen.mc_bin(0xFE, b"q")]
    conns = base.conns.copy()
    conns["flags"][base.mc[3]] = 2  # a connection whose parser was chosen: binary whatever the first byte
    b2 = _Out()
    b2.conns, b2.policy = conns, base.policy
    engine.set_connections(conns)
    w = _wl(b2, reqs + [gen.mc_bin(0, b"user:1")], [base.mc[k % 3] for k in range(len(reqs))] + [base.mc[3]], align=3)
    R = _run(engine, w)
    assert ((R.v == ALLOW) | (R.v == DENY)).all()
    assert _check(oracle, w, R)[4] == len(reqs) + 1
    engine.set_connections(base.conns)


# ------------------------------------------------------------------ 4. r2d2
def test_r2d2_fields(engine, oracle, base):
    _install(engine, base)
    reqs = [b"READ\r\n", b"READ /pub/a\r\n", b"READ /pub/a b\r\n", b"READ  /pub/a\r\n", b" READ\r\n", b"READ \r\n", b"\r\n",
            b"WRITE tmp12\r\nREAD x\r\n", b"READ x\rx\r\n", b"HALT" + b" " * 40 + b"\r\n", b"READ /pub/" + b"a" * 300 + b"\r\n"]
    ids = [base.r2[k % len(base.r2)] for k in range(len(reqs))]
    for a in (0, 11):
        w = _wl(base, reqs, ids, align=a)
        R = _run(engine, w)
        assert ((R.v == ALLOW) | (R.v == DENY)).all()
        assert _check(oracle, w, R)[5] == len(reqs)


# ------------------------------------------------------------------ 5. cassandra
def _action_queries():
    out = []
    for a in range(38):
        name = _lib.cass_action_name(a)
        if name in ("select", "delete"):
            out.append(name + " * from ks1.t%d" % a)
        elif name == "insert":
            out.append("INSERT INTO ks1.users (a) VALUES (1)")
        elif name == "update":
            out.append("Update ks1.t set a = 1")
        elif name == "use":
            out.append("USE ks7")
        elif name.split("-")[0] in ("grant", "revoke"):
            continue  # in the map, but parseQuery takes no such statement (answered PARSE_ERROR)
        else:
            kw, word = name.split("-", 1)
            out.append(kw + " materialized view v" if word == "materialized-view" else "%s %s x%d" % (kw, word, a))
    return out


def test_cassandra_actions_and_tables(engine, oracle, base):
    _install(engine, base)
    T = TEXT_STRIDE
    qs = _action_queries()
    assert len(qs) == 34
    qs += ["truncate foo", "alter materialized view v", "create Foo bar", "list stuff", "DROP thing x y",
           "select * from a/b", "create a/bab c", "use ''", "create role r", "select * from \u00c9T\u00c9",
           "select * from \u0130x.y", "select * from \u212as.t", "update \u00e9t\u00e9 set a = 1"]
    qs += ["select * from ks." + "a" * (k - 3) for k in (T - 1, T, T + 1, 4 * T)]
    qs += ["select * from " + "b" * (k - 1) for k in (T - 1, T, T + 1)]  # ".bbb": the empty keyspace
    reqs = [gen.cass_query_frame(q) for q in qs]
    reqs.append(gen.cass_query_frame("select * from ks1.prep", 0x09, stream=7))  # PREPARE
    reqs.append(gen.cass_query_frame("truncate foo", 0x09, stream=8))
    reqs += [gen.cass_frame(0x05, b""), gen.cass_frame(0x01, b"\x00\x00")]       # OPTIONS, STARTUP: no path entry
    reqs.append(gen.cass_query_frame("grant role r to x"))                       # PARSE_ERROR
    # one connection each, so that no USE reaches another query
    conns = np.concatenate([base.conns, np.repeat(base.conns[base.cs[2]:base.cs[2] + 1], len(reqs))])
    b2 = _Out()
    b2.conns, b2.policy = conns, base.policy
    engine.set_connections(conns)
    ids = [len(base.conns) + k for k in range(len(reqs))]
    for a in (0, 7):
        w = _wl(b2, reqs, ids, align=a)
        R = _run(engine, w)
        live = (R.v == ALLOW) | (R.v == DENY)
        assert live[:-1].all() and not live[-1]
        seen = _check(oracle, w, R)
        assert seen[6] == len(reqs) - 1 and seen["cass_logged"] == len(reqs) - 1 - 4, seen
    # the actions outside the map: id -1, the keyword and the word
    k0 = 34
    assert list(R.rec["api_key"][k0:k0 + 5]) == [-1] * 5
    assert list(R.rec["cass_keyword"][k0:k0 + 5]) == [3, 0, 1, 4, 2]
    assert all(R.rec["api_key"][:34] >= 0)
    # text stride 0 with NULL: the lengths are still told, no row is written
    R0 = _run(engine, w, text_stride=0)
    assert np.array_equal(R0.rec["cass_table_len"][live], R.rec["cass_table_len"][live])
    _check(oracle, w, R0, text_stride=0)
    _check(oracle, w, _run(engine, w, text_stride=T - 1), text_stride=T - 1)  # a stride that is no multiple of 4
    engine.set_connections(base.conns)


def test_cassandra_keyspaces_on_interleaved_connections(engine, oracle, base):
    _install(engine, base)
    a, b, c = base.cs[2], base.cs[3], base.cs[4]
    script = [(a, "select * from t"), (b, "use ks1"), (a, "use ksA"), (b, "select * from t"), (c, "select * from t"),
              (a, "select * from t"), (b, "USE \"Ks2\""), (b, "select * from T"), (a, "use 'KS/B'"),
              (a, "select * from t"), (b, "insert into users (x) values (1)"), (c, "use été"),
              (c, "update T set a = 1"), (a, "select * from dotted.t"), (b, "use ks1"), (b, "drop table tmpx")]
    w = _wl(base, [gen.cass_query_frame(q) for _, q in script], [ci for ci, _ in script], align=13)
    R = _run(engine, w)
    assert ((R.v == ALLOW) | (R.v == DENY)).all()
    seen = _check(oracle, w, R)
    assert seen[6] == len(script) and seen["cass_logged"] == len(script) - 2  # 'KS/B' and the query after it
    tables = [R.text[i][:R.rec["cass_table_len"][i]].tobytes() for i in range(w.n)]
    assert tables[0] == b".t" and tables[3] == b"ks1.t" and tables[5] == b"ksa.t" and tables[7] == b"ks2.t"


# ------------------------------------------------------------------ 6. sessions
@pytest.fixture(scope="module")
def sengine():
    from cilium_amd import Engine
    e = Engine(0)
    e.cass_sessions(1024)
    yield e
    e.close()


class _Session:
    """A sessions engine and one oracle parser per connection, kept in step."""

    def __init__(self, e, oracle, policy, conns):
        self.e, self.conns, self.policy = e, conns, policy
        e.update_policy(policy)
        e.set_connections(conns)
        pol = oracle.Policy(policy)
        self.refs = [oracle.Cassandra(pol, conns[i:i + 1]) for i in range(len(conns))]
        self.pol = pol

    def requests(self, frames, ids):
        w = gen.Workload("sess", *gen.pack(frames), np.asarray(ids, np.uint32), self.conns, self.policy)
        R = _run(self.e, w)
        return w, R, [self.refs[int(c)].request(f) for f, c in zip(frames, ids)]

    def replies(self, frames, ids):
        arena, offs, lens = gen.pack(frames)
        self.e.cass_replies(arena, offs, lens, np.asarray(ids, np.uint32))
        for f, c in zip(frames, ids):
            self.refs[int(c)].reply(f)


def _check_session_batch(w, R, refs, frames):
    """Records of one request batch against the oracle's (op, n, rule, path)."""
    n_exec = n_cut = 0
    for i, (op, n, rule, path, _) in enumerate(refs):
        where = (i, frames[i][:60], path)
        want_v = None if op < 0 or op in (0, 4) else ALLOW if op == 1 else DENY  # (panic, MORE, ERROR; PASS; DROP)
        if want_v is None:
            assert R.v[i] not in (ALLOW, DENY), where
            assert (R.text[i] == TEXT_FILL).all(), where
            continue
        assert R.v[i] == want_v, where
        rec = R.rec[i]
        assert rec["kind"] == 6, where
        parts = path.split(b"/")
        execute = frames[i][4] == 0x0A
        ntext = min(int(rec["cass_table_len"]), TEXT_STRIDE)
        if len(parts) == 4 or (execute and len(parts) > 4):
            # (> 4 parts on an EXECUTE: the stored table was cut at its '/', the documented limit)
            assert rec["flags"] & 2, where
            assert rec["cass_table_len"] == len(parts[3]) and R.text[i][:ntext].tobytes() == parts[3][:ntext], where
            name = _lib.cass_action_name(int(rec["api_key"]))
            if name is not None:
                assert name.encode() == parts[2], where
            elif execute:
                assert rec["flags"] & 4, where  # a statement keeps no action word
            else:
                e = log_entries(R.v[i:i + 1], R.rec[i:i + 1], R.spans.view(SPAN_DTYPE).reshape(len(refs), -1)[i:i + 1],
                                R.text[i:i + 1], w.arena, w.offsets[i:i + 1], w.lengths[i:i + 1])[0]
                assert e[2]["query_action"] == parts[2], where
            n_exec += execute
            n_cut += execute and len(parts) > 4
        else:
            assert not rec["flags"] & 2, where
        assert (R.text[i][ntext:] == TEXT_FILL).all(), where
    return n_exec, n_cut


def test_sessions_script(sengine, oracle):
    conns, policy, rounds = gen.cassandra_session_script(nconns=8, rounds=6, nreq=160, nrep=64)
    S = _Session(sengine, oracle, policy, conns)
    n_exec = 0
    for rd in rounds:
        w, R, refs = S.requests(rd["requests"], rd["req_conn"])
        n_exec += _check_session_batch(w, R, refs, rd["requests"])[0]
        S.replies(rd["replies"], rd["rep_conn"])
    assert n_exec > 20  # EXECUTEs that resolved and were logged
    st = sengine.cass_session_stats()
    assert st["resolved"] > 0 and st["unprepared"] > 0


def test_sessions_directed(sengine, oracle, base):
    q, ex, prepared = gen.cass_query_frame, gen.cass_execute_frame, gen.cass_prepared_reply
    cs = base.conns[base.cs[2]:base.cs[2] + 2].copy()
    S = _Session(sengine, oracle, {"policies": [base.policy["policies"][2]]}, _repolicy(cs))
    S.requests([q("use Ks1")], [0])
    # PREPAREs under the slot's keyspace (connection 0) and under none (connection 1)
    S.requests([q("select * from users", 0x09, stream=1), q("truncate foo", 0x09, stream=2),
                q("select * from a/b", 0x09, stream=3), q("select * from users", 0x09, stream=1)], [0, 0, 0, 1])
    S.replies([prepared(b"id1", 1), prepared(b"id2", 2), prepared(b"id3", 3), prepared(b"id1", 1)], [0, 0, 0, 1])
    frames = [ex(b"id1"), ex(b"id2"), ex(b"id3"), ex(b"nope"), q("select * from t2"), ex(b"id1"), q("use other"),
              q("select * from t3"), ex(b"id1")]
    ids = [0, 0, 0, 0, 0, 1, 0, 0, 0]
    w, R, refs = S.requests(frames, ids)
    n_exec, n_cut = _check_session_batch(w, R, refs, frames)
    assert (n_exec, n_cut) == (5, 1)
    tab = [R.text[i][:R.rec["cass_table_len"][i]].tobytes() for i in range(len(frames))]
    assert tab[0] == b"ks1.users" and tab[4] == b"ks1.t2" and tab[5] == b".users" and tab[7] == b"other.t3"
    assert R.rec["flags"][1] & 4 and R.rec["api_key"][1] == -1  # "truncate-foo": the word is not stored
    assert R.v[3] not in (ALLOW, DENY)                           # unprepared
    want_r = [rule if op == 1 else -1 for op, _, rule, _, _ in refs]
    assert list(R.r) == want_r


def _repolicy(conns):
    conns["policy"] = 0
    return conns


# ------------------------------------------------------------------ 7. whole-call checks
def test_host_twin_equals_the_device_call(engine, oracle, base):
    _install(engine, base)
    m, r, c = gen.memcache_requests(300, 5), gen.r2d2_requests(200, 6), gen.cassandra_requests(300, 7)
    rng = np.random.default_rng(11)
    reqs = m + r + c
    ids = [int(rng.choice(base.mc)) for _ in m] + [int(rng.choice(base.r2)) for _ in r] + \
        [int(rng.choice(base.cs)) for _ in c]
    perm = rng.permutation(len(reqs))
    w = _wl(base, [reqs[k] for k in perm], [ids[k] for k in perm])
    D = _run(engine, w)
    _same_answers(D, _run(engine, w, call="plain"))
    _check(oracle, w, D, need=(3, 4, 5, 6, "cass_logged"))
    spans = np.full((w.n, SPAN_STRIDE, 2), SPAN_FILL, np.uint32)
    text = np.full((w.n, TEXT_STRIDE), TEXT_FILL, np.uint8)
    v, rl, cons, rec, hs, ht = engine.classify_logged_all(
        w.arena, w.offsets, w.lengths, w.conn_ids, SPAN_STRIDE, TEXT_STRIDE,
        spans.view([("off", "<u4"), ("len", "<u4")]).reshape(w.n, SPAN_STRIDE), text)
    assert np.array_equal(v, D.v) and np.array_equal(rl, D.r) and np.array_equal(cons, D.c)
    live = (v == ALLOW) | (v == DENY)
    assert np.array_equal(np.frombuffer(rec.tobytes(), np.uint32).reshape(w.n, 8)[live], D.raw[live])
    assert np.array_equal(hs.view(np.uint32).reshape(w.n, SPAN_STRIDE, 2), D.spans)
    assert np.array_equal(ht, D.text)
    # and with no rows at all
    v0, _, _, rec0, _, _ = engine.classify_logged_all(w.arena, w.offsets, w.lengths, w.conn_ids, 0, 0)
    assert np.array_equal(v0, v)
    k = rec["kind"][live]
    assert np.array_equal(rec0["kind"][live], k) and np.array_equal(rec0["cass_table_len"][live & (rec["kind"] == 6)],
                                                                      rec["cass_table_len"][live & (rec["kind"] == 6)])


def test_device_argument_errors(engine, base):
    _install(engine, base)
    w = _wl(base, [b"get a\r\n"], [base.mc[0]])
    dev = torch.device("cuda", 0)
    rec = torch.zeros((1, 8), dtype=torch.int32, device=dev)
    a = torch.from_numpy(w.arena).to(dev)
    z = torch.zeros(4, dtype=torch.int64, device=dev)
    for lo in (_lib.LogAllOut(rec.data_ptr(), None, 4, None, 0), _lib.LogAllOut(rec.data_ptr(), None, 0, None, 8),
               _lib.LogAllOut(rec.data_ptr() + 8, None, 0, None, 0), _lib.LogAllOut(None, None, 0, None, 0)):
        rc = engine._lib.l7g_classify_logged_all(engine._h, a.data_ptr(), a.numel(), z.data_ptr(), z.data_ptr(),
                                                 z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), None,
                                                 C.byref(lo), None)
        assert rc == 1  # hipErrorInvalidValue
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 8. the shim's LogEntry stream
from test_gpu_accesslog import logsock, read_all  # noqa: E402,F401  (its socket helpers, unchanged)


def test_entries_equal_the_shims_log(engine, oracle, base, logsock):  # noqa: F811
    """About 50 requests per protocol through the proxylib shim's OnData, one
    call each, on a connection of the same identity as the batch's: the
    LogEntry records the shim sends equal log_entries() of the batch call.
    (Requests that the batch answers ALLOW or DENY and whose fields are ASCII:
    a protobuf string field is UTF-8, and after an ERROR the shim's connection
    is done.)"""
    from cilium_amd import proxylib as P
    _install(engine, base)
    srv, path = logsock
    mid = P.open_module([("access-log-path", path), ("node-id", "host~127.0.0.1~glog~localdomain")])
    assert mid
    try:
        P.policy_update(mid, base.policy)
        sock = None
        legs = [("memcache", base.mc[1], [q for q in gen.memcache_requests(120, 21) if q[0] < 0x80][:50]),
                ("memcache", base.mc[1], [q for q in gen.memcache_requests(200, 22) if q[0] >= 0x80][:50]),
                ("r2d2", base.r2[2], [q for q in gen.r2d2_requests(80, 23) if q.endswith(b"\r\n") and b"\rx" not in q][:50]),
                ("cassandra", base.cs[2], [q for q in gen.cassandra_requests(160, 24) if b"\xff" not in q])]
        total = 0
        def entries_of(reqs, ci):
            w = _wl(base, reqs, [ci] * len(reqs))
            R = _run(engine, w, span_stride=8, text_stride=64)
            return R, log_entries(R.v, R.rec, R.spans.view(SPAN_DTYPE).reshape(w.n, 8), R.text, w.arena, w.offsets,
                                  w.lengths)

        for k, (proto, ci, reqs) in enumerate(legs):
            R, ent = entries_of(reqs, ci)
            keep = [i for i in range(len(reqs)) if R.v[i] in (ALLOW, DENY) and
                    (ent[i] is None or all(c < 0x80 for f in ent[i][2].values() for c in f))][:50]
            reqs = [reqs[i] for i in keep]
            R, ent = entries_of(reqs, ci)  # (again: a cassandra keyspace follows the requests that stay)
            assert ((R.v == ALLOW) | (R.v == DENY)).all() and len(reqs) >= 30, (proto, len(reqs))
            want = [e for e in ent if e is not None]
            cn = base.conns[ci]
            names = [p["name"] for p in base.policy["policies"]]
            c = P.Connection(mid, proto, 2000 + k, True, int(cn["src_id"]), int(cn["dst_id"]), "1.1.1.1:%d" % (5000 + k),
                             "10.0.0.5:%d" % int(cn["port"]), names[int(cn["policy"])], 4096)
            assert c.result == P.OK
            if sock is None:
                sock, _ = srv.accept()
                sock.settimeout(20)
            for q in reqs:
                c.on_data(False, [q], 8)
            got = read_all(sock, len(want))
            for g, (et, pname, fields) in zip(got, want):
                assert g.WhichOneof("l7") == "generic_l7" and g.generic_l7.proto == pname
                assert g.entry_type == (0 if et == "Request" else 2)
                assert {a: b.encode() for a, b in dict(g.generic_l7.fields).items()} == fields, (proto, fields)
            total += len(want)
            c.close()
        assert total >= 120
        sock.close()
    finally:
        P.close_module(mid)

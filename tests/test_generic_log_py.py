"""tests/generic_log_py.py (the Python restatement of the generic access-log
fields) against what is already pinned: the literal textmemcached /
binarymemcached expectations of tests/test_gpu_accesslog.py, Go's documented
splitting rules, and, for cassandra, the oracle's path.  No device needed."""
import pytest

import generic_log_py as G
from cilium_amd import gen


def test_text_memcached_literals():
    data = b"get user:1 user:2\r\ndelete tmp\r\nget nope\r\n"
    want = [{"command": b"get", "keys": b"user:1, user:2"}, {"command": b"delete", "keys": b"tmp"},
            {"command": b"get", "keys": b"nope"}]
    for w in want:
        e = G.mc_text(data)
        assert e["proto"] == "textmemcached" and e["fields"] == w
        data = data[data.find(b"\r\n") + 2:]


def test_binary_memcached_literal():
    e = G.mc_binary(gen.mc_bin(0, key=b"user:7"))
    assert e["proto"] == "binarymemcached" and e["fields"] == {"opcode": b"0", "key": b"user:7"}
    assert e["key"] == (24, 6)
    e = G.mc_binary(gen.mc_bin(5, key=b"", extras=bytes(4)))
    assert e["fields"] == {"opcode": b"5", "key": b""} and e["key"] == (0, 0)
    assert G.mc_binary(gen.mc_bin(0, key=b"k", magic=0x01)) is None
    assert G.mc_binary(gen.mc_bin(0, key=b"kkkk")[:26]) is None


def test_fields_is_rune_wise():
    sp = [chr(c) for c in [0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000] + list(range(0x2000, 0x200B))]
    for s in sp:
        b = b"a" + s.encode() + b"b"
        assert [b[x:y] for x, y in G.go_fields(b)] == [b"a", b"b"], s
    # not spaces: U+200B, raw Latin-1 bytes, truncated sequences, an invalid byte is a one-byte non-space
    for junk in (b"\xe2\x80\x8b", b"\x85", b"\xa0", b"\xe2\x80", b"\xc2", b"\xff", b"\xe3\x80"):
        b = b"a" + junk + b"b"
        assert G.go_fields(b) == [(0, len(b))], junk
    assert G.go_fields(b"\xe2\xc2\x85x") == [(0, 1), (3, 4)]
    assert G.go_fields(b"  \t get\x0b\x0ck \r x\n") == [(4, 7), (9, 10), (13, 14)]
    assert G.go_fields(b"") == []


def test_text_key_sets():
    def keys(line):
        e = G.mc_text(line + b"\r\n")
        return None if e is None else (e["fields"]["command"], [line[o:o + n] for o, n in e["keys"]])
    assert keys(b"gets a b c") == (b"gets", [b"a", b"b", b"c"])
    assert keys(b"getx") == (b"getx", [])
    assert keys(b"gat 10 a b") == (b"gat", [b"a", b"b"])
    assert keys(b"gats 10") == (b"gats", [])
    assert keys(b"gat") is None
    assert keys(b"  set k 0 0 5 noreply") == (b"set", [b"k"])
    assert keys(b"set k 0 0 x") is None and keys(b"set k 0 0") is None
    assert keys(b"cas k 0 0 5 77") == (b"cas", [b"k"])
    assert keys(b"delete k noreply") == (b"delete", [b"k"]) and keys(b"delete") is None
    assert keys(b"incr k 5") == (b"incr", [b"k"]) and keys(b"touch k 5") == (b"touch", [b"k"])
    assert keys(b"stats a b") == (b"stats", []) and keys(b"flush_all") == (b"flush_all", [])
    assert keys(b"GET a") is None and keys(b"") is None
    assert G.mc_text(b"get a") is None and G.mc_text(b"get a\r") is None
    e = G.mc_text(b"\xc2\xa0get\xe3\x80\x80k\xe2\x80\xa8\r\nrest")
    assert e["cmd"] == (2, 3) and e["keys"] == [(8, 1)]


def test_memcached_parser_choice():
    assert G.memcached(gen.mc_bin(0, key=b"k"))["proto"] == "binarymemcached"
    assert G.memcached(b"get k\r\n")["proto"] == "textmemcached"
    assert G.memcached(b"get k\r\n", 2) is None           # a text line on a binary connection: a short header
    assert G.memcached(gen.mc_bin(0, key=b"k"), 1) is None  # no "\r\n"
    assert G.memcached(b"") is None


def test_r2d2_split():
    def f(line):
        e = G.r2d2(line)
        return None if e is None else (e["fields"]["cmd"], e["fields"]["file"], e["nfields"])
    assert f(b"READ\r\n") == (b"READ", b"", 1)
    assert f(b"READ /pub/a\r\n") == (b"READ", b"/pub/a", 2)
    assert f(b"READ a b\r\n") == (b"READ", b"", 3)
    assert f(b"READ  a\r\n") == (b"READ", b"", 3)
    assert f(b" READ\r\n") == (b"", b"READ", 2)
    assert f(b"READ \r\n") == (b"READ", b"", 2)
    assert f(b"\r\n") == (b"", b"", 1)
    assert f(b"READ x\rx\r\nmore\r\n") == (b"READ", b"x\rx", 2)
    assert f(b"READ x") is None
    assert G.r2d2(b"READ /pub/a\r\n")["file"] == (5, 6)


CASS = [  # query, keyspace set before it, (action, table) or None
    ("SELECT * FROM ks1.users WHERE id = 1", None, (b"select", b"ks1.users")),
    ("select a from users", "ks1", (b"select", b"ks1.users")),
    ("select a from users", None, (b"select", b".users")),
    ("use \"KS2\"", None, (b"use", b"ks2")),
    ("use ''", None, (b"use", b"")),
    ("create role r", None, (b"create-role", b"")),
    ("truncate foo", None, (b"truncate-foo", b"")),
    ("alter materialized view v", None, (b"alter-materialized-view", b"")),
    ("drop materialized view v", None, (b"drop-materialized-view", b"")),
    ("create custom index j on t (b)", None, (b"create-index", b"")),
    ("select * from a/b", None, None),
    ("create a/bab c", None, None),
    ("select * from t", "ks/x", None),
    ("select * from ÉTÉ", "k", (b"select", "k.été".encode())),
    ("select * from KS1.t", None, (b"select", b"ks1.t")),
]


@pytest.mark.parametrize("query,ks,want", CASS)
def test_cassandra_entry_of_the_oracles_path(oracle, query, ks, want):
    conns = gen.cassandra_workload(4).conns
    ref = oracle.Cassandra(oracle.Policy(gen.cassandra_policy()), conns[2:3])
    if ks:
        ref.request(gen.cass_query_frame("use " + ks))
    op, _, _, path, _ = ref.request(gen.cass_query_frame(query))
    assert op in (1, 2)  # PASS / DROP
    e = G.cassandra_path(path)
    if want is None:
        assert e is None, path
    else:
        assert e["proto"] == "cassandra"
        assert (e["fields"]["query_action"], e["fields"]["query_table"]) == want, path


def test_cassandra_other_opcodes_log_nothing(oracle):
    conns = gen.cassandra_workload(4).conns
    ref = oracle.Cassandra(oracle.Policy(gen.cassandra_policy()), conns[2:3])
    op, _, _, path, _ = ref.request(gen.cass_frame(0x05, b""))
    assert op in (1, 2) and path is not None and G.cassandra_path(path) is None

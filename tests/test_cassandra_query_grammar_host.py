"""The cassandra query parser the kernels and the host shim share
(cilium_amd/csrc/kernels/cass_parse.h), on the host through
tests/native/cass_parse_main.cc, against the oracle's parseQuery
(oracle/cassandra_ref.c, refpy.Cassandra.parse_query) over the corpus of
tests/cass_query_cases.py: the curated branch cases (whose answers are written
down there, read off the Go code) and 20,000 generated queries, each under an
optional USE.  Compared: the status, parts[2] and parts[3] of the path split on
"/" as CassandraRule.Matches splits it, and the action id against parts[2].

The coverage test reads the oracle's answers only; the decoder sweep needs
neither parser to be right about the other: every scalar value that Python's
str.lower() leaves alone and that is no White_Space must come back as the bytes
that went in, from both."""
import subprocess

import pytest

import cass_query_cases as Q
import refpy
from cilium_amd import build as b

N_GENERATED = 20000
# the branches the fixed corpora leave unreached, each with curated cases
BRANCHES = ["create_table_if_short", "drop_if_short", "drop_table_two", "alter_if", "materialized", "custom",
            "slash_in_field1", "trailing_from", "comment_index", "semicolons", "white_space", "lookalikes", "relength",
            "invalid_before_fc", "invalid_after_fc", "observed", "use_prefix"]


def _hex(x):
    return x.hex() if x else "-"


def product(cases):
    """[(status, action id, parts[2], parts[3])] of the header under test."""
    exe = [x for x in b.build_test_natives() if x.endswith("cass_parse_main")][0]
    text = "".join("%s %s\n" % (_hex(c.use), _hex(c.query)) for c in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = []
    for line in r.stdout.splitlines():
        st, aid, a, t = line.split(" ")
        out.append((int(st), int(aid), bytes.fromhex(a.replace("-", "")), bytes.fromhex(t.replace("-", ""))))
    assert len(out) == len(cases)
    return out


def reference(cases):
    """[(status, parts[2], parts[3])] of the oracle, a fresh parser a case."""
    refpy.build()
    out = []
    for c in cases:
        st = refpy.Cassandra()
        if c.use is not None:
            st.parse_query(c.use)
        rc, action, table = st.parse_query(c.query)
        parts = (action + b"/" + table).split(b"/") if rc == 0 else [b"", b""]
        out.append((rc, parts[0], parts[1]))
    return out


@pytest.fixture(scope="module")
def cases():
    return Q.corpus(N_GENERATED)


@pytest.fixture(scope="module")
def ref(cases):
    return reference(cases)


def test_curated_answers_of_the_oracle(cases, ref):
    """Every curated case gets the answer written beside it, so every listed
    branch is reached (by the oracle's own account)."""
    cur = Q.curated()
    assert sorted({br for br, _, _ in cur}) == sorted(BRANCHES)
    for k, (branch, c, want) in enumerate(cur):
        assert cases[k] == c
        got = ref[k] if not isinstance(want, int) else ref[k][0]
        assert got == want, (branch, c.use, c.query, got, want)


def test_product_equals_oracle(cases, ref):
    assert len(cases) >= N_GENERATED + len(Q.curated())
    got = product(cases)
    bad = [(c, g, w) for c, g, w in zip(cases, got, ref) if (g[0], g[2], g[3]) != w]
    assert not bad, (len(bad), bad[:5])
    for c, g in zip(cases, got):  # the id the rule match compares is the one of parts[2]
        if g[0] == 0:
            name = g[2].decode("utf-8", "replace")
            assert g[1] == (Q.ACTIONS.index(name) if name in Q.ACTIONS else -1), (c, g)


def test_corpus_coverage(cases, ref):
    """Conditions on the generator, from the oracle's answers alone."""
    assert {r[0] for r in ref} == {0, 1, 2}
    n = len(ref)
    assert sum(r[0] == 0 for r in ref) > n // 5 and sum(r[0] == 1 for r in ref) > n // 5
    assert sum(r[0] == 2 for r in ref) >= 20
    actions = {r[1] for r in ref if r[0] == 0}
    in_map = {a.encode() for a in Q.ACTIONS if a.split("-")[0] not in ("grant", "revoke")}
    assert len(in_map) == 34 and in_map <= actions, sorted(in_map - actions)
    assert len(actions - {a.encode() for a in Q.ACTIONS}) >= 100
    # a rune that is the query's only separator split it if the answer is a table without it
    split = {s for c, r in zip(cases, ref) for s in c.seps
             if len(c.seps) == 1 and c.invalid is None and r[0] == 0 and r[2] and s not in r[1] + r[2]}
    assert split == set(Q.SPACES) and len(split) == 25
    # invalid bytes on both sides of the first rune ToLower changes: kept, or U+FFFD each
    kept, repl = set(), set()
    for c, r in zip(cases, ref):
        if c.invalid and r[0] == 0:
            form, rest = Q.INVALID[c.invalid], r[2].replace(Q.FFFD, b"")
            if form in rest:
                kept.add(c.invalid)
            elif Q.FFFD * len(form) in r[2]:
                repl.add(c.invalid)
    assert kept == set(Q.INVALID) and repl == set(Q.INVALID), (set(Q.INVALID) - kept, set(Q.INVALID) - repl)
    # keyspaces reach tables
    assert sum(c.use is not None and r[0] == 0 and not r[2].startswith(b".") and b"." in r[2]
               for c, r in zip(cases, ref)) > 500
    assert all(b"\x00" not in c.query for c in cases)


def test_every_scalar_value_through_both_decoders():
    """SELECT * FROM k.<runes>: the 'S' makes ToLower re-encode every rune after
    it, so each rune is decoded and encoded again.  Runes that str.lower()
    leaves alone (the Unicode 10 tables of Go 1.10 change no others) and that
    are not White_Space come back byte for byte; each White_Space rune ends the
    token."""
    keep = [cp for cp in range(0x80, 0x110000)
            if not 0xD800 <= cp <= 0xDFFF and cp not in Q.WHITE_SPACE and chr(cp).lower() == chr(cp)]
    assert len(keep) > 1_100_000
    B = 4096
    names = ["".join(map(chr, keep[k:k + B])).encode() for k in range(0, len(keep), B)]
    cases = [Q.Case(None, b"SELECT * FROM k." + nm, frozenset(), None) for nm in names]
    cases += [Q.Case(None, b"SELECT * FROM k.a" + s + b"b" + s, frozenset(), None) for s in Q.SPACES]
    want = [(0, b"select", b"k." + nm) for nm in names] + [(0, b"select", b"k.a")] * 25
    for who, got in (("oracle", reference(cases)), ("product", [(g[0], g[2], g[3]) for g in product(cases)])):
        for k, (g, w) in enumerate(zip(got, want)):
            if g != w:
                first = next((i for i in range(min(len(g[2]), len(w[2]))) if g[2][i] != w[2][i]), None)
                raise AssertionError("%s: batch %d differs (first byte %s, near %r; lengths %d / %d)" %
                                     (who, k, first, w[2][max((first or 0) - 4, 0):(first or 0) + 8], len(g[2]), len(w[2])))

"""The cassandra query grammar on the GPU over the corpus of
tests/cass_query_cases.py (the curated branch cases and generated queries with
their USE prefixes): verdict, rule and consumed bytes of the classifier, the
access-log records (action id, keyword, word and the lowered table bytes as
the device wrote them) and the session kernels, each against the oracle's
parser walked over the same frames in the same order.  Every comparison is
exact.

The policy adds, to the rules of gen.cassandra_policy(), table regexes that
answer differently when a rune of the new corpus is decoded, lowered or split
wrongly, and one rule per table-less action family."""
import re

import numpy as np
import pytest

import cass_query_cases as Q
from cilium_amd import api, gen
from cilium_amd._lib import ALLOW, DENY, PARSE_ERROR
from cilium_amd.engine import CASS_KEYWORDS
from test_gpu_cassandra_sessions import Sessions
from test_gpu_generic_log import TEXT_FILL, _Out, _check, _run
from test_gpu_http import assert_same, wl_from_reqs

pytestmark = pytest.mark.gpu

N_GENERATED = 3300
NCONNS = 16
REMOTES = [7, 8, 100, 101, 150, 163, 5]
NFA_NAME = "бдббддбдбдбддбдб"  # 16 runes, the 15th from the end a д


def grammar_policy(broad=True):
    """broad=False: without the last two table rules, which allow nearly every table."""
    family = [{"query_action": a} for a in ("create-index", "drop-materialized-view", "create-role", "list-permissions",
                                            "drop-user", "create-function", "drop-aggregate", "alter-type",
                                            "create-trigger")]
    base = [{"query_action": "select", "query_table": "^ks1\\."}, {"query_action": "insert", "query_table": "users$"},
            {"query_action": "use"}, {"query_action": "update", "query_table": "é"},
            {"query_action": "drop-table", "query_table": "^\\.tmp"}]
    # (a rule without an action matches every request whose table is empty: after the family rules)
    tables = [{"query_table": "^system\\.local$"}, {"query_table": "(a|b)*a(a|b){14}"},
              {"query_table": "(д|б)*д(д|б){14}"}, {"query_table": "\\p{Cyrillic}"},
              {"query_table": "[\\x{8000}-\\x{FFFF}]"}, {"query_table": "\\p{Lu}"}]
    if broad:
        tables += [{"query_table": "^\\."}, {"query_table": "^[^.]*\\.[^.]*$"}]
    groups = [api.port_rule(remote_policies=[7, 8], l7proto="cassandra", l7=[{"query_action": "delete"}]),
              api.port_rule(remote_policies=list(range(100, 164)), l7proto="cassandra", l7=family + base + tables)]
    wild = [api.port_rule(l7proto="cassandra", l7=[{"query_action": "select", "query_table": "^wild"}])]
    return api.policy_set(api.network_policy("cs", 11, ingress=[(gen.CASS_PORT, groups), (0, wild)])), \
        1 + len(family + base + tables) + 1


def grammar_frames(nconns, seed=77):
    """(frames, connection ids, index of each case's query frame): every corpus
    case as a QUERY frame (a fifth PREPARE) after its USE frame, on a connection
    drawn per case; the fixed queries of gen.py, which the base rules answer to,
    and the NFA rule's table among them."""
    rng = np.random.default_rng(seed)
    cases = Q.corpus(N_GENERATED)
    extra = [q.encode("utf-8", "surrogateescape") for q in gen._CASS_QUERIES] * 4
    extra += [b"select * from " + NFA_NAME.encode(), b"UPDATE k." + NFA_NAME.upper().encode() + b" set",
              b"select * from k.\xf0\x9d\x90\x80x"]  # U+1D400 is Lu and has no lower case
    extra += [b"select * from k." + b"ab" * 3 + b"a" + b"ab" * 7] * 4  # the base NFA rule, whatever the keyspace
    extra += [b"select * from wild.cat"] * 6          # the port-0 rule, for the remotes no other rule allows
    cases += [Q.Case(None, q, frozenset(), None) for q in extra]
    frames, ids, at = [], [], []
    for c in cases:
        ci = int(rng.integers(0, nconns))
        stream = int(rng.integers(0, 65536))
        if c.use is not None:
            frames.append(gen.cass_query_frame(c.use, 0x07, stream))
            ids.append(ci)
        at.append(len(frames))
        frames.append(gen.cass_query_frame(c.query, 0x09 if rng.random() < 0.2 else 0x07, stream))
        ids.append(ci)
    assert 4000 <= len(frames) <= 5000
    return frames, np.asarray(ids, np.uint32), at


def _conns(nconns):
    return gen.make_conns(nconns, 0, gen.CASS_PORT, True, gen.PROTO_CASSANDRA, (REMOTES * 3)[:nconns])


@pytest.fixture(scope="module")
def workloads():
    policy, nrules = grammar_policy()
    frames, ids, _ = grammar_frames(NCONNS)
    many = wl_from_reqs(frames, policy, _conns(NCONNS), ids)
    one = wl_from_reqs(frames, policy, gen.make_conns(1, 0, gen.CASS_PORT, True, gen.PROTO_CASSANDRA, [100]))
    return many, one, nrules


# ------------------------------------------------------------------ 1. verdicts
@pytest.mark.parametrize("which", ["sixteen_connections", "one_connection"])
def test_verdict_parity(engine, oracle, workloads, which):
    many, one, nrules = workloads
    w = many if which == "sixteen_connections" else one
    engine.update_policy(w.policy)
    engine.set_connections(w.conns)
    want = oracle.classify_workload(w, 1)
    got = engine.classify(w.arena, w.offsets, w.lengths, w.conn_ids)
    assert_same(got, want, w)
    v, r = want[0], want[1]
    assert (v == ALLOW).sum() > 200 and (v == DENY).sum() > 50 and (v == PARSE_ERROR).sum() > 200
    if w is many:  # every rule allows something
        assert len(set(r[v == ALLOW].tolist())) == nrules, sorted(set(r[v == ALLOW].tolist()))
    else:          # (the connection's remote reaches the second group only)
        assert len(set(r[v == ALLOW].tolist())) == nrules - 2


# ------------------------------------------------------------------ 2. access log
_SPACE_RE = re.compile(b"|".join(re.escape(s) for s in sorted(Q.SPACES, key=len, reverse=True)))


def _second_field(frame):
    """fields[1] of a QUERY / PREPARE frame's query, split on the White_Space
    encodings (a UTF-8 lead byte always starts a rune, so the byte patterns are
    exact), and its offset in the frame."""
    ql = int.from_bytes(frame[9:13], "big")
    q = frame[13:13 + ql].rstrip(b";")
    pos, n = 0, 0
    for m in list(_SPACE_RE.finditer(q)) + [None]:
        end = m.start() if m else len(q)
        if end > pos:
            if n == 1:
                return 13 + pos, q[pos:end]
            n += 1
        pos = m.end() if m else end
    return None


def test_access_log_records(engine, oracle, workloads):
    """Each cassandra record against the oracle's path: flags bit1 iff the path
    has four parts, the table bytes and length, the action id, and for an action
    outside queryActionMap the keyword and the raw word.  No row is truncated.
    Then _check of tests/test_gpu_generic_log.py on the requests whose action
    word log_entries() lowers exactly (it lowers ASCII only, as it says)."""
    w = workloads[0]
    engine.update_policy(w.policy)
    engine.set_connections(w.conns)
    pol = oracle.Policy(w.policy)
    refs = [oracle.Cassandra(pol, w.conns[i:i + 1]) for i in range(len(w.conns))]
    frames = [w.arena[int(o):int(o) + int(n)].tobytes() for o, n in zip(w.offsets, w.lengths)]
    paths = [refs[int(c)].request(f) for f, c in zip(frames, w.conn_ids)]
    longest = max(len(p[3].split(b"/")[3]) for p in paths if p[3] is not None and p[3].count(b"/") >= 3)
    stride = (longest + 4) // 4 * 4
    assert longest < stride <= 256
    R = _run(engine, w, text_stride=stride)
    plain = _run(engine, w, call="plain")
    assert np.array_equal(R.v, plain.v) and np.array_equal(R.r, plain.r) and np.array_equal(R.c, plain.c)
    names = [a.encode() for a in Q.ACTIONS]
    n_logged = n_word = 0
    ascii_word = np.ones(w.n, bool)
    for i, (op, _, _, path, _) in enumerate(paths):
        where = (i, frames[i][13:], path)
        if op not in (1, 2):
            assert R.v[i] not in (ALLOW, DENY), where
            continue
        assert R.v[i] == (ALLOW if op == 1 else DENY), where
        rec = R.rec[i]
        parts = path.split(b"/")
        assert rec["kind"] == 6 and not rec["flags"] & 1 and not rec["flags"] & 4, where
        assert bool(rec["flags"] & 2) == (len(parts) == 4), where
        if len(parts) != 4:
            continue
        n_logged += 1
        assert rec["cass_table_len"] == len(parts[3]), where
        assert R.text[i][:len(parts[3])].tobytes() == parts[3], where
        assert (R.text[i][len(parts[3]):] == TEXT_FILL).all(), where
        if parts[2] in names:
            assert rec["api_key"] == names.index(parts[2]), where
        else:
            kw, _, word = parts[2].partition(b"-")
            off, raw = _second_field(frames[i])
            assert rec["api_key"] == -1 and CASS_KEYWORDS[int(rec["cass_keyword"])].encode() == kw, where
            assert (int(rec["cass_word_off"]), int(rec["cass_word_len"])) == (off, len(raw)), where
            ascii_word[i] = all(c < 0x80 for c in raw)
            n_word += 1
    assert n_logged > 1500 and n_word > 200 and (~ascii_word).sum() > 20
    idx = np.nonzero(ascii_word)[0]
    S = _Out()
    S.v, S.rec, S.raw, S.spans, S.text = R.v[idx], R.rec[idx], R.raw[idx], R.spans[idx], R.text[idx]
    seen = _check(oracle, w.subset(idx), S, text_stride=stride, need=(6, "cass_logged"))
    assert seen["cass_logged"] > 1500


# ------------------------------------------------------------------ 3. sessions
@pytest.fixture(scope="module")
def sengine():
    from cilium_amd import Engine
    e = Engine(0)
    e.cass_sessions(1024)
    yield e
    e.close()


def test_sessions_same_answers(sengine, oracle, workloads):
    """The sixteen-connection batch through the session kernels, in three calls
    (the keyspaces carry over between them)."""
    w = workloads[0]
    S = Sessions(sengine, oracle, w.policy, w.conns, device=True)
    frames = [w.arena[int(o):int(o) + int(n)].tobytes() for o, n in zip(w.offsets, w.lengths)]
    cut = [0, len(frames) // 3, 2 * len(frames) // 3, len(frames)]
    n_live = 0
    for a, b in zip(cut, cut[1:]):
        got, _ = S.requests(frames[a:b], w.conn_ids[a:b])
        n_live += int(((got[0] == ALLOW) | (got[0] == DENY)).sum())
    assert n_live > 1500


# statements whose tables hold a name of each decoder range, a rune whose lowering changes its length, or an
# invalid byte on either side of the first lowered rune: (USE before it or None, statement)
STATEMENTS = [
    (None, "select * from Дб"), (None, "select * from a\ub000b"), (None, "select * from a\u0485b"),
    (None, "SELECT * FROM t\ufeff"), (None, "select * from Ⱥ"), (None, "select * from k.ẞx"),
    (None, "select * from \u212a.\u0130"), (None, "select * from \U00010400\U00010427"), ("use Дб", "select * from t"),
    ("use 한", "update Ａ"), ("use \U0010ffff", "delete from \U0001f600"), (b"use k\xffs", "select * from t"),
    (b"USE k\xffs", "select * from t"), (None, b"select * from T\xed\xa0\x80"), (None, b"select * from T\xc0\xa0"),
    (None, b"Select * from t\xf4\x90\x80\x80x"), (None, b"select * from \xc3\x89\xf0\x9f\x98"),
    (None, b"select * from t\x85x"), (None, b"select * from \xe2\x80X"), (None, "insert into ÉTÀ.users (a) values (?)"),
    (None, "select * from " + NFA_NAME), (None, "UPDATE k." + NFA_NAME.upper() + " set a = ?"),
    (None, "drop table if exists 表験"), (None, "select * from k.\U0001d400x"), (None, "create index i on t (a)"),
    ("use ÉTÉ", "update T set a = ?"),
]


def test_prepared_statements_get_the_verdict_of_their_query(sengine, oracle):
    """PREPARE -> RESULT/prepared -> EXECUTE of each statement, one connection
    each: the EXECUTE is answered from the stored statement, whose table the
    session kernel lowered when it stored it, and gets the QUERY form's verdict
    and rule."""
    policy, _ = grammar_policy(broad=False)  # the verdict depends on the table's runes
    n = len(STATEMENTS)
    assert n >= 24
    S = Sessions(sengine, oracle, policy, gen.make_conns(n, 0, gen.CASS_PORT, True, gen.PROTO_CASSANDRA, [100] * n),
                 device=True)
    b = Q._b
    uses = [(k, gen.cass_query_frame(b(u))) for k, (u, _) in enumerate(STATEMENTS) if u is not None]
    S.requests([f for _, f in uses], [k for k, _ in uses])
    ids = np.arange(n, dtype=np.uint32)
    (qv, qr, _), _ = S.requests([gen.cass_query_frame(b(s), 0x07, stream=k) for k, (_, s) in enumerate(STATEMENTS)], ids)
    assert set(qv.tolist()) == {ALLOW, DENY}
    (pv, pr, _), _ = S.requests([gen.cass_query_frame(b(s), 0x09, stream=k) for k, (_, s) in enumerate(STATEMENTS)], ids)
    assert np.array_equal(pv, qv) and np.array_equal(pr, qr)
    S.replies([gen.cass_prepared_reply(b"id%d" % k, stream=k) for k in range(n)], ids)
    ex = [gen.cass_execute_frame(b"id%d" % k, stream=k) for k in range(n)]
    (ev, er, ec), _ = S.requests(ex, ids)
    assert np.array_equal(ev, qv) and np.array_equal(er, qr), (ev.tolist(), qv.tolist(), er.tolist(), qr.tolist())
    assert ec.tolist() == [len(f) for f in ex]
    assert len(set(qr[qv == ALLOW].tolist())) >= 6  # the rules for the runes of each range among them

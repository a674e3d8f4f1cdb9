"""The Kafka kernel's rule matching (kafka_classify.hip: str_lookup,
topic_first, rule_matches, matches_rule) and the compiler's rule-set selection
(kafka_compile.cc: RulesetFor, Compile) over rule-set shapes that
gen.cfg3_policy() does not have, against the oracle: every verdict, rule id and
consumed length, and the per-rule counters.

tests/kafka_rules_stream.py builds the policy family, the connection table and
one stream of about 6,000 unique Kafka requests (and 600 memcached ones for the
large case); the oracle classifies it once.  The rule sets have topics with 1,
2, 3 and 5 rules that differ in apiKey, apiVersion and clientID; topicless
rules before, between and behind the topic rules; a {} rule; an L3-only group
(rule -1); identities admitted by one, two or three groups, or by none; an
exact-port entry beside a port-0 entry, an egress entry, a port without entry,
a connection without policy; proxylib connections.  The names have every length
at which str_lookup takes another path (1 to 255 bytes, around 16 and 32),
pairs that differ in one byte, in case or by a suffix, and two rule topics with
one 32-bit hash and the same first 16 bytes.

test_stream_covers_the_cases states what the stream must contain; it needs no
GPU.  Every other test classifies the stream on the device by another way in:
calls of several sizes, the logged kernel, the host entry point, a call past
kBesideMin (6-wave build, helper grid), an engine that imported the tables, and
engines whose rule sets keep to the sorted directory (L7G_KAFKA_DENSE_BUDGET)."""
import numpy as np
import pytest
import torch

import kafka_match_py as M
import kafka_rules_stream as KS
from cilium_amd import Engine
from cilium_amd._lib import ALLOW, DENY

gpu = pytest.mark.gpu
BESIDE_MIN = 1 << 20  # engine_state.h kBesideMin
SIZES = [1, 63, 64, 65, 4097, None]
# index[] words (kafka_compile.cc): a dense table takes 12 words per interned topic, and the stream's
# policy interns fewer than 64 topics; its first rule sets fit under this budget, its later ones do not
MIXED_BUDGET = 3000


class _Ctx:
    pass


@pytest.fixture(scope="module")
def stream(oracle):
    S = KS.make()
    S.ref = oracle.classify_workload(S.w, 8)
    return S


@pytest.fixture(scope="module")
def ctx(engine, stream):
    c = _Ctx()
    engine.update_policy(stream.w.policy)
    engine.set_connections(stream.w.conns)
    c.dev = torch.device("cuda", 0)
    c.d_arena = torch.from_numpy(stream.w.arena).to(c.dev)
    return c


def test_stream_covers_the_cases(stream):
    """Conditions on the stream, from the Python model's facts
    (kafka_match_py.walk_facts) and the oracle's answers alone.

    Every rule of every rule set in use allows a request; every rule set in use
    allows and, unless it holds a rule that matches every request ({} or the
    L3-only wildcard: such a set cannot deny), denies; at least 50 requests in
    each class of kafka_rules_stream.CLASSES; every request is well-formed, so
    none is left out of the comparisons."""
    S, ref = stream, stream.ref
    answers = KS.model_answers(S)
    assert all(a is not None for a in answers) and np.isin(ref[0][:S.nk], (ALLOW, DENY)).all()
    assert 5000 <= S.nk <= 6500 and not S.unreached
    a, b = S.collision
    assert a != b and len(a) == len(b) and a[:16] == b[:16] and KS.whash(a) == KS.whash(b)
    assert a in S.rule_topics and b in S.rule_topics
    assert sorted({len(t) for t in S.rule_topics} & set(KS.LENGTHS)) == KS.LENGTHS
    sets = {}
    for i, ans in enumerate(answers):
        rules = ans[3]["rules"]
        if rules is None:
            assert ref[0][i] == DENY and ref[1][i] == -1
            continue
        d = sets.setdefault(tuple(r["gid"] for r in rules), {"rules": rules, "allowed_by": set(), "deny": 0})
        if ref[0][i] == ALLOW:
            d["allowed_by"].add(int(ref[1][i]))
        else:
            d["deny"] += 1
    assert len(sets) >= 8 and max(len(k) for k in sets) >= 50
    for key, d in sets.items():
        assert d["allowed_by"] == set(key), (key, sorted(set(key) - d["allowed_by"]))
        catch_all = any(r["keys"] is None and r["version"] is None and not r["topic"] and not r["client"] for r in d["rules"])
        assert catch_all or d["deny"] > 0, key
    # the topic lists of 1, 2, 3 and 5 rules, each rule of them the first to match for some request
    counts = {}
    for r in max(sets.values(), key=lambda d: len(d["rules"]))["rules"]:
        if r["topic"]:
            counts[r["topic"]] = counts.get(r["topic"], 0) + 1
    assert {1, 2, 3, 5} <= set(counts.values())
    seen = {(t, k) for ans in answers if ans[3]["rules"] is not None and ans[0] for t, k in ans[3]["first"].items()}
    for t, n in counts.items():
        assert all((t.encode(), k) in seen for k in range(n)), t
    cls = KS.classes(S, answers)
    for name in KS.CLASSES:
        assert sum(name in c for c in cls) >= 50, name
    ids = np.arange(S.nk)[[("rule_-1" in c) for c in cls]]
    assert (ref[0][ids] == ALLOW).all() and (ref[1][ids] == -1).all()
    # rule_matches' branches: every decoded kind, kinds outside 0..63, ConsumerMetadata allowed by a rule
    # with a topic or a client id, an untyped kind of isTopicAPIKey refused by a topic rule that admits its key
    reqs = [ans[3]["req"] for ans in answers]
    kinds = {r["kind"] for r in reqs}
    assert {0, 1, 2, 3, 8, 9, 10} <= kinds and min(kinds) < 0 and max(kinds) > 63
    for k, vs in KS.TYPED_VERSIONS.items():
        assert {r["version"] for r in reqs if r["kind"] == k} >= set(vs), k
    allowed_by = [ans[3]["rules"][ans[3]["pos"]] if ans[0] else None for ans in answers]
    assert sum(r["typed"] == 2 and bool(a and (a["topic"] or a["client"])) for r, a in zip(reqs, allowed_by)) >= 10
    assert sum(r["typed"] == 0 and r["kind"] in M.TOPIC_API_KEYS and
               any(x["topic"] and x["keys"] is None for x in ans[3]["rules"] or [])
               for r, ans in zip(reqs, answers)) >= 10
    ntopics = [len(r["topics"]) for r in reqs]
    assert set(ntopics) >= set(range(6)) and any(b"" in r["topics"] for r in reqs)
    assert any(len(set(r["topics"])) < len(r["topics"]) for r in reqs)
    # requests on proxylib connections, and on the connections that resolve to no rule set
    flags = S.w.conns["flags"][S.w.conn_ids[:S.nk]]
    assert (flags & 4).astype(bool).sum() >= 300


def test_dense_budget_changes_the_tables_only_when_set(stream, monkeypatch):
    """Compile-only engines: L7G_KAFKA_DENSE_BUDGET gives other tables at 0 and
    at MIXED_BUDGET (some rule sets dense, some not: neither image), and a
    budget every rule set fits under gives the default's."""
    def digest():
        e = Engine(-1)
        e.update_policy(stream.w.policy)
        e.set_connections(stream.w.conns)
        return e.tables_digest
    default = digest()
    got = {}
    for budget in ("0", str(MIXED_BUDGET), str(1 << 20)):
        monkeypatch.setenv("L7G_KAFKA_DENSE_BUDGET", budget)
        got[budget] = digest()
    assert got[str(1 << 20)] == default
    assert len({default, got["0"], got[str(MIXED_BUDGET)]}) == 3, got


# ------------------------------------------------------------------ the device's answers
def _upload(c, w, idx):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(c.dev)
            for a in (w.offsets[idx].view(np.int64), w.lengths[idx].view(np.int32), w.conn_ids[idx].view(np.int32))]


def _classify(c, eng, w, idx, logged=False):
    inputs = _upload(c, w, idx)
    n = len(idx)
    o = [torch.full((n,), 7, dtype=t, device=c.dev) for t in (torch.uint8, torch.int32, torch.int32)]
    cnt = torch.zeros(eng.nrules + 8, dtype=torch.int64, device=c.dev)
    args = [c.d_arena.data_ptr(), c.d_arena.numel(), *[t.data_ptr() for t in inputs], n, *[t.data_ptr() for t in o]]
    torch.cuda.synchronize()
    if logged:
        rec = torch.zeros(n * 32, dtype=torch.uint8, device=c.dev)
        top = torch.zeros(n * 4 * 8, dtype=torch.uint8, device=c.dev)
        eng.classify_logged_device(*args, rec.data_ptr(), top.data_ptr(), 4, counters_ptr=cnt.data_ptr())
    else:
        eng.classify_device(*args, counters_ptr=cnt.data_ptr())
    torch.cuda.synchronize()
    return (o[0].cpu().numpy(), o[1].cpu().numpy(), o[2].cpu().numpy().view(np.uint32)), cnt.cpu().numpy()


def _same(S, idx, got, cnt=None, nrules=None):
    """Verdict, rule id and consumed length bit for bit; the counters: the
    histogram of the oracle's ALLOW rule ids (rule -1 in no bin), then the verdicts."""
    ref = tuple(r[idx] for r in S.ref)
    bad = np.nonzero((got[0] != ref[0]) | (got[1] != ref[1]) | (got[2] != ref[2]))[0]
    if len(bad):
        i = int(idx[bad[0]])
        raise AssertionError(f"{len(bad)} of {len(idx)} differ; request {i} on connection {S.w.conn_ids[i]}: got "
                             f"{[int(g[bad[0]]) for g in got]}, oracle {[int(r[bad[0]]) for r in ref]}; "
                             f"{KS.request_bytes(S.w, i)[:64]!r}")
    if cnt is not None:
        want = np.zeros(nrules + 8, np.int64)
        allowed = ref[1][(ref[0] == ALLOW) & (ref[1] >= 0)]
        want[:nrules] = np.bincount(allowed, minlength=nrules)[:nrules]
        want[nrules:nrules + 5] = np.bincount(ref[0], minlength=5)[:5]
        assert (cnt[:nrules + 5] == want[:nrules + 5]).all(), np.nonzero(cnt[:nrules + 5] != want[:nrules + 5])[0][:8]


@gpu
@pytest.mark.parametrize("n", SIZES, ids=lambda n: "all" if n is None else str(n))
def test_prefix_matches_oracle(engine, stream, ctx, n):
    idx = np.arange(stream.nk if n is None else n)
    got, cnt = _classify(ctx, engine, stream.w, idx)
    _same(stream, idx, got, cnt, engine.nrules)


@gpu
def test_logged_kernel(engine, stream, ctx):
    """l7g_classify_logged: the logged instantiation of the kernel, the same matcher."""
    idx = np.arange(stream.nk)
    got, cnt = _classify(ctx, engine, stream.w, idx, logged=True)
    _same(stream, idx, got, cnt, engine.nrules)


@gpu
def test_host_entry_point(engine, stream, ctx):
    """l7g_classify_host: the whole Kafka stream (one parser: the unpartitioned
    kernel), and calls small enough for the synchronous path."""
    w = stream.w
    for idx in (np.arange(stream.nk), np.arange(100, 117), np.arange(4000, 4001)):
        got = engine.classify(w.arena, w.offsets[idx], w.lengths[idx], w.conn_ids[idx])
        _same(stream, idx, (got[0], got[1], got[2]), None)


@gpu
def test_proxylib_connections(engine, stream, ctx):
    """The requests on L7G_CONN_PROXYLIB connections alone (the proxylib view of RulesetFor)."""
    w = stream.w
    idx = np.nonzero(w.conns["flags"][w.conn_ids[:stream.nk]] & 4)[0]
    assert len(idx) >= 300 and len(np.unique(stream.ref[0][idx])) == 2
    got, cnt = _classify(ctx, engine, w, idx)
    _same(stream, idx, got, cnt, engine.nrules)


@gpu
def test_large_call(engine, stream, ctx):
    """Just past kBesideMin: the stream's indices (Kafka and memcached) repeated
    over the same arena, in a shuffled order.  The Kafka kernel's 6-wave build
    and its helper grid run the matcher."""
    n = BESIDE_MIN + 4321
    idx = np.tile(np.arange(stream.w.n), -(-n // stream.w.n))[:n]
    np.random.default_rng(3).shuffle(idx)
    got, cnt = _classify(ctx, engine, stream.w, idx)
    _same(stream, idx, got, cnt, engine.nrules)


def _second_engine(stream, ctx, prepare):
    """A fresh engine, prepared, classifying the whole Kafka stream."""
    e = Engine(0)
    try:
        prepare(e)
        e.set_connections(stream.w.conns)
        idx = np.arange(stream.nk)
        got, cnt = _classify(ctx, e, stream.w, idx)
        _same(stream, idx, got, cnt, e.nrules)
        return e.tables_digest, e.tables_compiled
    finally:
        e.close()


@gpu
def test_after_export_and_import(engine, stream, ctx):
    """l7g_tables_export / l7g_tables_import: a second engine that installs the
    first one's compiled tables, and compiles none, answers the same."""
    digest, compiled = _second_engine(stream, ctx, lambda e: e.import_tables(engine.export_tables()))
    assert digest == engine.tables_digest and compiled == 0


@gpu
def test_sorted_directory_form(engine, stream, ctx, monkeypatch):
    """L7G_KAFKA_DENSE_BUDGET (read at engine creation): with 0 every rule set
    keeps to its sorted topic directory (topic_first's binary search); with a
    budget between, the first rule sets compiled get the dense table and the
    later ones the directory, both forms in one image.  Same answers."""
    # (fresh engines: the shared engine's image also holds the rule sets that the connections of
    # earlier tests resolved to under this policy)
    fresh = lambda e: e.update_policy(stream.w.policy)  # noqa: E731
    digests = {"default": _second_engine(stream, ctx, fresh)[0]}
    for budget in ("0", str(MIXED_BUDGET)):
        monkeypatch.setenv("L7G_KAFKA_DENSE_BUDGET", budget)
        digests[budget] = _second_engine(stream, ctx, fresh)[0]
    # three different images: all dense, none dense, and some of either
    assert len(set(digests.values())) == 3, digests


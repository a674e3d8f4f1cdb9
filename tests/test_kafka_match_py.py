"""The plain Python model of the Kafka matcher (tests/kafka_match_py.py)
against the reference's known answers and against the C oracle, on the CPU.

The oracle and the device kernel were written by the same hands; the model is
a third, sequential statement of GetRelevantRules and MatchesRule.  Where all
three agree on the stream of tests/kafka_rules_stream.py (the device's part is
tests/test_gpu_kafka_rules.py), a misreading shared by oracle and kernel has
one more chance to show."""
import numpy as np
import pytest

import kafka_match_py as M
import kafka_rules_stream as KS
from cilium_amd._lib import ALLOW, DENY
from test_oracle_kats import kafka_policy


def test_reference_kats(kats):
    """The 11 MatchesRule cases of pkg/kafka/policy_test.go and the proxy cases
    of pkg/proxy/kafka_test.go (tests/golden/reference_kats.json)."""
    K = kats["kafka"]
    assert sum(c["ref"].startswith("pkg/kafka/policy_test.go") for c in K["cases"]) == 11
    for case in K["cases"]:
        req = bytes.fromhex(K["requests"][case["request"]])
        pols = M.load_policy_set(kafka_policy(case["rules"]))
        conn = {"policy": 0, "port": 9092, "ingress": 1, "flags": 0, "src_id": case.get("src_id", 7)}
        allow, gid, consumed, _ = M.classify(pols, conn, req)
        assert allow == (case["expect"] == "ALLOW"), case
        assert consumed == len(req)
        assert (gid >= 0) == allow


def test_hash_restatement_and_collision():
    """kafka_rules_stream.whash is the compiler's hash (the interned strings of
    an exported image carry it), and the two colliding names collide."""
    a, b = KS.find_collision()
    assert a != b and len(a) == len(b) == 24 and a[:16] == b[:16]
    assert KS.whash(a) == KS.whash(b)
    # known answers of l7_whash, worked by hand from device_tables.h: the empty string, one word
    h = (0x811C9DC5 * 0x85EBCA6B) & 0xFFFFFFFF
    assert KS.whash(b"") == h ^ (h >> 13)
    h = ((0x811C9DC5 ^ 0x64636261) * 0x9E3779B1) & 0xFFFFFFFF
    h ^= h >> 15
    h = ((h ^ 4) * 0x85EBCA6B) & 0xFFFFFFFF
    assert KS.whash(b"abcd") == h ^ (h >> 13)


@pytest.fixture(scope="module")
def stream(oracle):
    S = KS.make()
    return S, oracle.classify_workload(S.w, 8), KS.model_answers(S)


def test_model_agrees_with_oracle_on_the_stream(stream):
    S, ref, answers = stream
    assert not S.unreached, S.unreached
    nwell = 0
    for i, a in enumerate(answers):
        got = (int(ref[0][i]), int(ref[1][i]), int(ref[2][i]))
        if a is None:
            assert got[0] not in (ALLOW, DENY), (i, got)
            continue
        nwell += 1
        assert (ALLOW if a[0] else DENY, a[1], a[2]) == got, (i, a[:3], got, KS.request_bytes(S.w, i)[:48])
    assert nwell >= 5000


def test_proxylib_view_differs_where_it_should(stream):
    """The proxylib view of RulesetFor is a view of its own: on the entry
    without L7 rules it admits an identity that the other view refuses."""
    S, ref, _ = stream
    conns = S.w.conns
    px = [i for i, c in enumerate(KS.CONNS) if c[:4] == (999, 9095, 1, 0) and c[4] & M.PROXYLIB]
    plain = [i for i, c in enumerate(KS.CONNS) if c[:4] == (999, 9095, 1, 0) and not c[4]]
    assert len(px) == 1 and len(plain) == 1 and conns["flags"][px[0]] == M.PROXYLIB
    k = np.arange(S.nk)
    on_px, on_plain = k[S.w.conn_ids[:S.nk] == px[0]], k[S.w.conn_ids[:S.nk] == plain[0]]
    assert len(on_px) >= 10 and (ref[0][on_px] == ALLOW).all() and (ref[1][on_px] == -1).all()
    assert len(on_plain) >= 10 and (ref[0][on_plain] == DENY).all()

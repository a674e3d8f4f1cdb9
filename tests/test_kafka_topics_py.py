"""tests/kafka_topics_py.py (the Python restatement of where a Kafka request's
topic names lie, which the access-log GPU tests compare the device's topic
spans with) pinned to the oracle on the CPU.

The oracle exports verdicts, not topics, so the helper's decoded names are
checked through MatchesRule (pkg/kafka/policy.go:200-225): a request is allowed
by a list of topic rules exactly when every distinct topic it names is covered.
For every request the oracle answers ALLOW or DENY under an allow-all Kafka
policy, whose key is a topic API key and whose decoded names are all non-empty
(and spellable in a policy: KafkaTopicValidChar, at most 255 bytes), a policy
with one topic rule per distinct decoded name must make the oracle ALLOW, and
dropping any single one of those rules must make it DENY.  A name missed,
invented or cut at the wrong byte fails one of the two."""
import re

import numpy as np
import pytest

import kafka_topics_py
from cilium_amd import api, gen
from cilium_amd._lib import ALLOW, DENY, PROTO_KAFKA

TOPIC_OK = re.compile(rb"^[a-zA-Z0-9\\._\-]{1,255}$")
PORT = 9092
CHUNK = 400  # requests per oracle call


def _policy(rule_lists):
    """One network policy per rule list (its index = its position)."""
    return api.policy_set(*[api.network_policy(f"p{i}", i + 1, ingress=[(PORT, [api.port_rule(kafka=rules)])])
                            for i, rules in enumerate(rule_lists)])


def _classify(oracle, reqs, policies_of):
    """policies_of[i]: the rule lists request i is classified under; returns a
    list of verdict lists in the same shape (one oracle call)."""
    rule_lists, which = [], []
    for i, lists in enumerate(policies_of):
        for rules in lists:
            which.append(i)
            rule_lists.append(rules)
    if not rule_lists:
        return [[] for _ in policies_of]
    arena, offs, lens = gen.pack(reqs)
    which = np.asarray(which)
    conns = gen.make_conns(len(rule_lists), 0, PORT, True, PROTO_KAFKA, 2000)
    conns["policy"] = np.arange(len(rule_lists))
    v, _, _ = oracle.Policy(_policy(rule_lists)).classify(conns, arena, offs[which], lens[which],
                                                           np.arange(len(rule_lists), dtype=np.uint32), 4)
    out = [[] for _ in policies_of]
    for k, i in enumerate(which):
        out[i].append(int(v[k]))
    return out


def _requests():
    well = (gen.kafka_all_kinds(2000, gen.SEED_BASE + 81) + gen.kafka_requests(2000, gen.SEED_BASE + 82) +
            gen.kafka_compressed_requests(500, gen.SEED_BASE + 84))
    return well, gen.kafka_adversarial(2000, gen.SEED_BASE + 83)


def test_decoded_topics_are_the_oracles(oracle):
    well, adv = _requests()
    reqs = well + adv
    allow_all = [api.PortRuleKafka()]
    qualified = np.zeros(len(reqs), bool)
    for c0 in range(0, len(reqs), CHUNK):
        chunk = reqs[c0:c0 + CHUNK]
        base = _classify(oracle, chunk, [[allow_all]] * len(chunk))
        plans, names_of = [], []
        for r, (v,) in zip(chunk, base):
            p = kafka_topics_py.parse(r)
            names = None
            if v in (ALLOW, DENY):
                # the oracle decoded the request: so must the helper
                assert p is not None, r[:64]
                assert v == ALLOW
                if p["typed"] == 1 and p["topics"]:
                    names = [r[o:o + n] for o, n in p["topics"]]
                    if not all(TOPIC_OK.match(t) for t in names):
                        names = None
            if names is None:
                plans.append([])
                names_of.append(None)
                continue
            distinct = sorted(set(names))
            rules = [api.PortRuleKafka(topic=t.decode()) for t in distinct]
            plans.append([rules] + [rules[:k] + rules[k + 1:] for k in range(len(rules))])
            names_of.append(distinct)
        got = _classify(oracle, chunk, plans)
        for j, (vs, distinct) in enumerate(zip(got, names_of)):
            if distinct is None:
                continue
            qualified[c0 + j] = True
            assert vs[0] == ALLOW, (c0 + j, distinct, vs)
            # (a single distinct topic dropped leaves no rule at all: still a DENY)
            assert all(v == DENY for v in vs[1:]), (c0 + j, distinct, vs)
    share = qualified[:len(well)].mean()
    print(f"qualifying: {share:.3f} of the well-formed generators' {len(well)} requests, "
          f"{qualified[len(well):].mean():.3f} of the adversarial {len(adv)}")
    assert share >= 0.60, share


def test_helper_refuses_what_the_oracle_refuses(oracle):
    """Where the helper decodes a request the oracle answers ALLOW / DENY or, for
    a compressed set that does not decode, PARSE_ERROR; where it does not, the
    oracle does neither."""
    well, adv = _requests()
    reqs = well + adv
    for c0 in range(0, len(reqs), 2000):
        chunk = reqs[c0:c0 + 2000]
        base = _classify(oracle, chunk, [[[api.PortRuleKafka()]]] * len(chunk))
        for r, (v,) in zip(chunk, base):
            if kafka_topics_py.parse(r) is None:
                assert v not in (ALLOW, DENY), r[:64]


@pytest.mark.parametrize("names", [[b"a"], [b"a", b"b"], [b"a", b"", b"a"], []])
def test_spans_of_hand_built_requests(names):
    r = gen.k_metadata(1, 7, "cl", [n.decode() for n in names])
    p = kafka_topics_py.parse(r)
    assert [r[o:o + n] for o, n in p["topics"]] == names
    assert all((o, n) == (0, 0) for (o, n), name in zip(p["topics"], names) if not name)
    assert (p["api_key"], p["api_version"], p["correlation_id"]) == (3, 1, 7)

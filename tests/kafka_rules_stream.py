"""The policy family, connection table and request stream of
tests/test_gpu_kafka_rules.py and tests/test_kafka_match_py.py (test helper).

The Kafka policy (policy 0 of the set) has an ingress entry on 9092 whose
groups are selected by remote_policies (some identities are admitted by two or
three of them), an ingress entry on port 0, an ingress entry on 9095 that holds
an L3-only group alone, and an egress entry on 9093.  Its rules name topics of
every length at which str_lookup (kafka_classify.hip) changes its path, pairs
of names that differ in one place, two names with one 32-bit hash, topics with
1, 2, 3 and 5 rules, and topicless rules before, between and after them.
Policy 1 is gen.mc_policy(), for the memcached requests of the large case.

The requests are built per rule set: for every rule one request that the
matcher model (kafka_match_py) says this rule allows, then that request with
one thing changed (version, client id, one topic byte, one more topic), then
drawn ones.
"""
import functools

import numpy as np

import kafka_match_py as M
from cilium_amd import api, gen
from cilium_amd._lib import PROTO_KAFKA

# ------------------------------------------------------------------ the hash, restated
MASK = 0xFFFFFFFF


def whash(s):
    """l7_whash of device_tables.h: the string's little-endian 32-bit words, the
    last zero-padded, then its length."""
    h = 0x811C9DC5
    for i in range(0, len(s), 4):
        w = int.from_bytes(s[i:i + 4].ljust(4, b"\0"), "little")
        h = ((h ^ w) * 0x9E3779B1) & MASK
        h ^= h >> 15
    h = ((h ^ len(s)) * 0x85EBCA6B) & MASK
    return h ^ (h >> 13)


COLLISION_PREFIX = b"hash.collision.-"  # 16 bytes: the part a slot keeps a copy of
_SUFFIX_ALPHABET = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789._", np.uint8)


def _suffixes(n):
    """Suffix i of 8 bytes: eight 6-bit digits of i * 0x9E3779B97F4A7C15 mod 2^64
    (digits of i itself would differ in a few low bits of each word, and a hash
    step is one-to-one in its word: such suffixes hardly collide)."""
    x = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    return np.stack([_SUFFIX_ALPHABET[((x >> np.uint64(16 + 6 * k)) & np.uint64(63)).astype(np.int64)] for k in range(8)],
                    axis=1)


def find_collision(n=400_000):
    """Two 24-byte names, COLLISION_PREFIX + 8 bytes, with one whash: a birthday
    search over the first n suffixes, the hash's two last steps vectorised."""
    assert len(COLLISION_PREFIX) == 16
    h0 = 0x811C9DC5
    for i in range(0, 16, 4):
        h0 = ((h0 ^ int.from_bytes(COLLISION_PREFIX[i:i + 4], "little")) * 0x9E3779B1) & MASK
        h0 ^= h0 >> 15
    suf = _suffixes(n)
    words = suf.reshape(n, 2, 4).astype(np.uint64)
    w = words[:, :, 0] | words[:, :, 1] << np.uint64(8) | words[:, :, 2] << np.uint64(16) | words[:, :, 3] << np.uint64(24)
    h = np.full(n, h0, np.uint64)
    for k in range(2):
        h = ((h ^ w[:, k]) * np.uint64(0x9E3779B1)) & np.uint64(MASK)
        h ^= h >> np.uint64(15)
    order = np.argsort(h, kind="stable")
    same = np.nonzero(h[order][1:] == h[order][:-1])[0]
    assert len(same), "no collision among the suffixes"
    a, b = sorted((int(order[same[0]]), int(order[same[0] + 1])))
    return COLLISION_PREFIX + suf[a].tobytes(), COLLISION_PREFIX + suf[b].tobytes()


# ------------------------------------------------------------------ names
_FILL = "abcdefghijklmnopqrstuvwxyz.ABCDEFGHIJKLMNOPQRSTUVWXYZ_0123456789-"
LENGTHS = [1, 3, 4, 5, 15, 16, 17, 19, 20, 31, 32, 33, 64, 249, 255]


def _named(tag, n):
    return (tag + _FILL * 5)[:n]


LEN_TOPICS = [_named("L%d." % n, n) if n > 3 else "qrs"[:n] for n in LENGTHS]
BASE16 = "pairs.0123456789"
PAIRS = [
    (BASE16 + "a", BASE16 + "b"),                            # equal in the first 16 bytes, different at byte 16
    (_named("last.", 32) + "x", _named("last.", 32) + "y"),  # 33 bytes, different in the last
    ("prefix.topic.name", "prefix.topic.name.longer"),       # one a strict prefix of the other
    ("qrs", "qrst"),                                         # (and a short one: lengths 3 and 4)
    ("Orders.Events-v2", "orders.events-v2"),                # letter case, 16 bytes
    ("dots.and_more-x\\y", "dots.and_more-x\\z"),            # . _ - \ in the name (17 bytes)
]
assert len(BASE16) == 16 and all(len(a) <= 255 for p in PAIRS for a in p)
C16A, C16B = "client.sixteen.a", "client.sixteen.b"          # 16 bytes, different in the last
C17A, C17B = C16A + "z", C16A + "y"                          # 17: C16A a strict prefix, different at byte 16
C40A, C40B = _named("client.forty.", 39) + "a", _named("client.forty.", 39) + "b"
assert (len(C16A), len(C17A), len(C40A)) == (16, 17, 40)
PLAIN_CLIENT = "plain"
T5, T3, T2, T1 = "five.rules", "three.rules.topic", "two", "one.rule.topic.of.31.bytes....."
P1, P2 = "behind.consume.1", "behind.consume.two"
E1, E2, W1 = "egress.only", "egress.other.group", "port.zero.only"


def K(**kw):
    return api.PortRuleKafka(**kw)


def policy(collision):
    """The policy set; collision: the two names of find_collision()."""
    ca, cb = (c.decode() for c in collision)
    # (a client-only rule matches every request of an untyped kind and every ConsumerMetadata request:
    # the rules for those stand ahead of it)
    g0 = [K(api_key="metadata", api_version="1"), K(api_key="heartbeat"), K(api_key="findcoordinator", client_id=C40B),
          K(client_id=C17A),
          K(topic=T5, api_key="produce", api_version="0"), K(topic=T5, api_key="produce", api_version="2", client_id=C16A),
          K(topic=T5, api_key="fetch", client_id=C40A), K(topic=T5, api_key="fetch", api_version="3"),
          K(topic=T5, role="consume", client_id=C16B),
          K(topic=T3, api_key="produce"), K(topic=T3, api_key="fetch", api_version="1"),
          K(topic=T3, api_key="offsetcommit", client_id=C17B),
          K(api_key="fetch", api_version="4"),
          K(topic=T2, role="produce", client_id=C16A), K(topic=T2, role="produce", api_version="1"),
          K(topic=T1, api_key="fetch"),
          K(api_version="5")]
    # one rule per name: the lengths, the pairs (their two names under different keys), the collision
    g2 = []
    for i, t in enumerate(LEN_TOPICS):
        g2.append([K(topic=t), K(topic=t, api_key="produce"), K(topic=t, api_key="fetch")][i % 3])
    for a, b in PAIRS[:3] + PAIRS[4:]:
        g2 += [K(topic=a, api_key="produce"), K(topic=b, api_key="fetch")]
    g2 += [K(topic="qrst", api_key="offsets")]
    g2 += [K(topic=ca, api_key="produce"), K(topic=cb, api_key="fetch"), K(api_key="offsetfetch", api_version="2")]
    g1 = [K(role="consume"), K(topic=P1, api_key="produce"), K(topic=P2, api_key="produce", api_version="1"),
          K(topic=P2, api_key="produce", client_id=C16A), K(role="produce", api_version="3")]
    g3 = [K(topic=T1, api_key="produce"), K()]
    gw = [K(api_version="2", client_id=C40A), K(topic=W1, api_key="offsets"),
          K(topic=W1, api_key="offsetfetch", api_version="1")]
    ge1 = [K(topic=E1, role="consume"), K(topic=E1, role="produce"), K(api_key="metadata")]
    ge2 = [K(topic=E2)]
    ingress = [
        (9092, [api.port_rule(remote_policies=[100, 101, 102], kafka=g0),
                api.port_rule(remote_policies=[101, 102], kafka=g2),
                api.port_rule(remote_policies=[101, 103], kafka=g1),
                api.port_rule(remote_policies=[104], kafka=g3),
                api.port_rule(remote_policies=[105])]),
        (0, [api.port_rule(remote_policies=[100, 107], kafka=gw)]),
        (9095, [api.port_rule(remote_policies=[105])]),
    ]
    egress = [(9093, [api.port_rule(remote_policies=[100, 108], kafka=ge1), api.port_rule(remote_policies=[108], kafka=ge2)])]
    kpol = api.network_policy("10.0.0.1", 3, ingress=ingress, egress=egress)
    return {"policies": [kpol, gen.mc_policy()["policies"][0]]}


# (identity, port, ingress, policy, flags)
PX = M.PROXYLIB
CONNS = [
    (100, 9092, 1, 0, 0), (101, 9092, 1, 0, 0), (102, 9092, 1, 0, 0), (103, 9092, 1, 0, 0), (104, 9092, 1, 0, 0),
    (105, 9092, 1, 0, 0),  # the L3-only group alone: rule -1
    (107, 9092, 1, 0, 0),  # the port-0 entry's group alone, beside an exact entry
    (999, 9092, 1, 0, 0),  # no group admits it
    (100, 9999, 1, 0, 0),  # the port-0 entry alone
    (100, 9093, 0, 0, 0), (108, 9093, 0, 0, 0),
    (100, 9094, 0, 0, 0),  # a port with no entry
    (100, 9092, 1, -1, 0),  # no policy
    (999, 9095, 1, 0, 0),  # an entry without L7 rules whose group does not admit it
    (101, 9092, 1, 0, PX), (102, 9092, 1, 0, PX), (105, 9092, 1, 0, PX), (999, 9092, 1, 0, PX), (100, 9094, 0, 0, PX),
    (104, 9092, 1, 0, PX), (999, 9095, 1, 0, PX),  # proxylib: an entry without L7 rules admits everyone
    (108, 9093, 0, 0, PX),
]


def conn_table():
    c = np.zeros(len(CONNS), gen.CONN_DTYPE)
    for i, (src, port, ingress, pol, flags) in enumerate(CONNS):
        c[i] = (pol, port, ingress, PROTO_KAFKA, flags, src, 7)
    return c


# ------------------------------------------------------------------ requests
TYPED_VERSIONS = {0: range(0, 4), 1: range(0, 7), 2: range(0, 3), 3: range(0, 6), 8: range(0, 4), 9: range(0, 4),
                  10: range(0, 2)}
UNTYPED = [12, 18, 11, 19, 4, 36, 63, 64, 1000, -1, -7]  # among them kinds outside 0..63 (bykey slot 64)


def build(kind, version, corr, client, topics):
    """One request of `kind` naming `topics` (bytes each; kinds without topics take none)."""
    tl = [(t, [0]) for t in topics]
    if kind == 0:
        return gen.k_produce(version, corr, client, [(t, [(0, [gen.k_message(b"v%d" % corr, version=version)])])
                                                     for t in topics])
    if kind == 1:
        return gen.k_fetch(version, corr, client, tl)
    if kind == 2:
        return gen.k_offset(version, corr, client, tl)
    if kind == 3:
        return gen.k_metadata(version, corr, client, topics)
    if kind == 8:
        return gen.k_offset_commit(version, corr, client, "grp", tl)
    if kind == 9:
        return gen.k_offset_fetch(version, corr, client, "grp", tl)
    if kind == 10:
        return gen.k_consumer_metadata(version, corr, client, "grp")
    return gen.k_request(kind, version, corr, client, b"\0" * (corr % 7))


def near_misses(t):
    """Names one byte off t at offset 0, 15, 16 or last, or one byte longer or shorter."""
    t = t if isinstance(t, bytes) else t.encode()
    out = []
    for o in (0, 15, 16, len(t) - 1):
        if 0 <= o < len(t):
            out.append(t[:o] + bytes([t[o] ^ 1 if t[o] ^ 1 != 0 else 0x41]) + t[o + 1:])
    out.append(t + b"a")
    if len(t) > 1:
        out.append(t[:-1])
    return [x for x in dict.fromkeys(out) if x != t]


class Stream:
    pass


@functools.lru_cache(maxsize=None)
def make(seed=gen.SEED_BASE + 91, nmc=600):
    """The stream: S.w (Workload: the Kafka requests, then nmc memcached ones),
    S.nk, S.collision, S.policies (the model's view), S.near (the near-miss
    names sent), S.rule_topics."""
    S = Stream()
    S.collision = find_collision()
    pol = policy(S.collision)
    S.policies = M.load_policy_set(pol)
    conns = conn_table()
    rule_topics = sorted({r["topic"].encode() for p in S.policies[:1] for d in p.values() for _, groups in d
                          for _, rules in groups if isinstance(rules, list) for r in rules if r["topic"]})
    S.rule_topics = rule_topics
    clients = [C16A, C16B, C17A, C17B, C40A, C40B]
    client_near = [C16A.upper(), C16A[:-1], C16A[:-1] + "c", "d" + C17A[1:], C17A[:15] + "Q" + C17A[16], C40A[:-1] + "c",
                   C40A + "a", "", None, PLAIN_CLIENT]
    S.near = set()
    rng = np.random.default_rng(seed)
    reqs, cids = [], []

    def add(ci, kind, version, client, topics):
        reqs.append(build(kind, version, len(reqs), client, topics))
        cids.append(ci)

    # the rule sets in use, by their rules' ids, and a connection of each (non-proxylib first)
    sets = {}
    for ci in range(len(conns)):
        rules, found = M.relevant_rules(S.policies, conns[ci])
        if found:
            sets.setdefault(tuple(r["gid"] for r in rules), (ci, rules))
    S.unreached = []
    for key, (ci, rules) in sets.items():
        own = sorted({r["topic"].encode() for r in rules if r["topic"]})
        other = [t for t in rule_topics if t not in own]
        for pos, rule in enumerate(rules):
            # a request this rule allows: try its keys (typed kinds first), the versions, its client or a plain one
            keys = sorted(rule["keys"]) if rule["keys"] is not None else [1, 0, 12, 64]
            hit = None
            for kind in keys:
                typed = 1 if kind in TYPED_VERSIONS and kind != 10 else 2 if kind == 10 else 0
                if rule["topic"] and typed != 1:
                    continue
                versions = [rule["version"]] if rule["version"] is not None else list(TYPED_VERSIONS.get(kind, range(3)))
                # (a request without topics is matched against the topic rules too: a topicless rule
                # behind them is reached by a request that names a topic no rule knows)
                names = [[rule["topic"].encode()]] if rule["topic"] else [[], [b"unknown.topic"]] if typed == 1 else [[]]
                for version in versions:
                    for topics in names:
                        client = rule["client"] or PLAIN_CLIENT
                        req = {"kind": kind, "version": version, "typed": typed,
                               "client": client.encode() if typed == 1 else None, "topics": topics}
                        if hit is None and M.matches_rule(req, rules) == pos:
                            hit = (kind, version, client, topics)
            if hit is None:
                S.unreached.append((key, pos))
                continue
            kind, version, client, topics = hit
            add(ci, kind, version, client, topics)
            for v in (version - 1, version + 1):
                add(ci, kind, v, client, topics)
            for c in client_near + ([rule["client"][:-1] + "~", rule["client"] + "x"] if rule["client"] else []):
                add(ci, kind, version, c, topics)
            if topics:
                t = topics[0]
                for nm in near_misses(t):
                    S.near.add(nm)
                    add(ci, kind, version, client, [nm])
                    if own:
                        add(ci, kind, version, client, [own[int(rng.integers(len(own)))], nm])
                extra = [own[int(rng.integers(len(own)))], t, b"", b"unknown.topic"]
                if other:
                    extra.append(other[int(rng.integers(len(other)))])
                for x in extra:
                    add(ci, kind, version, client, [t, x])
                    add(ci, kind, version, client, [x, t])
        # a topicless rule and a topic rule behind it that one request satisfies: the topicless rule
        # answers before the topics complete (alone, and with a second topic on either side of it)
        for p, tl in enumerate(rules):
            if tl["topic"]:
                continue
            for q in range(p + 1, len(rules)):
                tr = rules[q]
                if not tr["topic"]:
                    continue
                keys = set(TYPED_VERSIONS) - {10}
                for r in (tl, tr):
                    keys = keys & r["keys"] if r["keys"] is not None else keys
                vs = {r["version"] for r in (tl, tr) if r["version"] is not None}
                cs = {r["client"] for r in (tl, tr) if r["client"]}
                if not keys or len(vs) > 1 or len(cs) > 1:
                    continue
                kind = min(keys)
                version = vs.pop() if vs else TYPED_VERSIONS[kind][-1]
                client = cs.pop() if cs else PLAIN_CLIENT
                t = tr["topic"].encode()
                add(ci, kind, version, client, [t])
                for k in rng.integers(len(own), size=2):
                    add(ci, kind, version, client, [own[int(k)], t])
        # drawn requests on every connection of this rule set
        mine = [c for c in range(len(conns)) if M.relevant_rules(S.policies, conns[c])[1] and
                tuple(r["gid"] for r in M.relevant_rules(S.policies, conns[c])[0]) == key]
        pool_near = [nm for t in own for nm in near_misses(t)]
        for k in range(170 if len(rules) > 3 else 60):
            ci2 = mine[k % len(mine)]
            kind = int(rng.choice(list(TYPED_VERSIONS) + UNTYPED)) if k % 4 else int(rng.choice(UNTYPED))
            vs = TYPED_VERSIONS.get(kind, range(0, 7))
            version = int(rng.integers(vs[0], vs[-1] + 1))
            r = rng.random()
            client = clients[int(rng.integers(len(clients)))] if r < 0.6 else client_near[int(rng.integers(len(client_near)))]
            topics = []
            for _ in range(int(rng.integers(0, 6))):
                r = rng.random()
                if r < 0.6 and own:
                    topics.append(own[int(rng.integers(len(own)))])
                elif r < 0.72 and other:
                    topics.append(other[int(rng.integers(len(other)))])
                elif r < 0.8 and pool_near:
                    nm = pool_near[int(rng.integers(len(pool_near)))]
                    S.near.add(nm)
                    topics.append(nm)
                elif r < 0.86:
                    topics.append(b"unknown-%d" % int(rng.integers(50)))
                elif r < 0.9:
                    topics.append(b"")
                elif topics:
                    topics.append(topics[0])
            add(ci2, kind, version, client, topics)
    # connections that resolve to no rule set, or to the wildcard alone: a few requests of every kind
    for ci in range(len(conns)):
        rules, found = M.relevant_rules(S.policies, conns[ci])
        if found and len(rules) > 1:
            continue
        for k, kind in enumerate(list(TYPED_VERSIONS) + UNTYPED):
            add(ci, kind, k % 3, clients[k % len(clients)], [rule_topics[(7 * k + ci) % len(rule_topics)]] * (k % 3))
    S.nk = len(reqs)
    perm = np.random.default_rng(seed + 1).permutation(S.nk)
    arena, offs, lens = gen.pack([reqs[i] for i in perm])
    kc = np.array(cids, np.uint32)[perm]
    m = gen.memcache_workload(nmc, seed=seed + 2)
    mconns = m.conns.copy()
    mconns["policy"] = 1
    S.w = gen.Workload("kafka-rules", np.concatenate([arena, m.arena]),
                       np.concatenate([offs, m.offsets + np.uint64(len(arena))]), np.concatenate([lens, m.lengths]),
                       np.concatenate([kc, m.conn_ids + np.uint32(len(conns))]), np.concatenate([conns, mconns]), pol)
    return S


def request_bytes(w, i):
    return w.arena[int(w.offsets[i]):int(w.offsets[i]) + int(w.lengths[i])].tobytes()


def model_answers(S):
    """kafka_match_py.classify of every Kafka request of the stream (None where
    the request is not well-formed)."""
    w = S.w
    return [M.classify(S.policies, w.conns[w.conn_ids[i]], request_bytes(w, i)) for i in range(S.nk)]


def _without(rules, field, value):
    return [dict(r, **{field: value}) for r in rules]


def classes(S, answers):
    """Per request the classes of the coverage conditions it falls into (a set
    of names), from the model's facts."""
    near = S.near - set(S.rule_topics)
    out = []
    for a in answers:
        c = set()
        out.append(c)
        if a is None or a[3]["rules"] is None:
            continue
        allow, _, _, f = a
        req, rules, pos = f["req"], f["rules"], f["pos"]
        if not req["topics"] and not 0 <= req["kind"] <= 63:
            c.add("bykey_slot_64")
        if allow:
            if rules[pos]["gid"] == -1:
                c.add("rule_-1")
            if not f["topicless"] and f["first"][rules[pos]["topic"].encode()] >= 1:
                c.add("not_first_in_topic_list")
            if f["topicless"] and req["topics"] and f["completion"] is not None and pos < f["completion"]:
                c.add("topicless_before_completion")
            if not f["topicless"] and f["topicless_after"]:
                c.add("completion_before_topicless")
        else:
            open_ = [t for t, k in f["first"].items() if k is None]
            if len(open_) == 1 and open_[0] in near:
                c.add("one_near_miss_uncovered")
            if M.matches_rule(req, _without(rules, "version", None)) is not None:
                c.add("denied_by_version_only")
            if M.matches_rule(req, _without(rules, "client", "")) is not None:
                c.add("denied_by_client_only")
    return out


CLASSES = ["not_first_in_topic_list", "topicless_before_completion", "completion_before_topicless",
           "one_near_miss_uncovered", "denied_by_version_only", "denied_by_client_only", "rule_-1", "bykey_slot_64"]

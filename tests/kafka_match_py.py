"""The Kafka rule matcher in plain Python (test helper): which rules apply to a
connection and whether they allow a request, written from the reference's Go

  GetRelevantRules            pkg/policy/l4.go:118-141
  rules.Kafka == nil => deny  pkg/proxy/kafka.go:139-142
  ruleMatches / MatchesRule   pkg/kafka/policy.go:144-225

on top of the kafka_topics_py decoder.  It is the sequential loop of the Go
code: the ordered rule list, a set of the request's topics still to be
covered, the first rule that completes it.  No tables, no hashing, no
arithmetic on positions: the device's three precomputed views of the list
(kafka_compile.h) and the oracle's C restatement are what it is compared with
(tests/test_kafka_match_py.py, tests/test_gpu_kafka_rules.py).

A rule here is a dict: keys (a set of api keys, None = any), version (int or
None), topic and client (str, "" = not set), gid (the rule's global id: every
L7 rule of the policy set counts one, in the order policies, ingress entries,
egress entries, groups and rules are written; -1 for the L7 wildcard an
L3-only group contributes).
"""
import kafka_topics_py

# pkg/policy/api/kafka.go:153-197 (KafkaAPIKeyMap) and :274-293 (MapRoleToAPIKey)
API_KEYS = ["produce", "fetch", "offsets", "metadata", "leaderandisr", "stopreplica", "updatemetadata",
            "controlledshutdown", "offsetcommit", "offsetfetch", "findcoordinator", "joingroup", "heartbeat", "leavegroup",
            "syncgroup", "describegroups", "listgroups", "saslhandshake", "apiversions", "createtopics", "deletetopics",
            "deleterecords", "initproducerid", "offsetforleaderepoch", "addpartitionstotxn", "addoffsetstotxn", "endtxn",
            "writetxnmarkers", "txnoffsetcommit", "describeacls", "createacls", "deleteacls", "describeconfigs",
            "alterconfigs"]
ROLES = {"produce": {0, 3, 18}, "consume": {1, 2, 3, 8, 9, 10, 11, 12, 13, 14, 18}}
# isTopicAPIKey, pkg/kafka/policy.go:26-52
TOPIC_API_KEYS = {0, 1, 2, 3, 4, 5, 6, 8, 9, 19, 20, 21, 23, 24, 27, 28, 34, 35, 37}

WILDCARD = {"keys": None, "version": None, "topic": "", "client": "", "gid": -1}
PROXYLIB = 4  # L7G_CONN_PROXYLIB


def rule_from_json(j, gid):
    keys = None
    if j.get("apiKey"):
        keys = {API_KEYS.index(j["apiKey"].lower())}
    elif j.get("role"):
        keys = set(ROLES[j["role"].lower()])
    return {"keys": keys, "version": int(j["apiVersion"]) if j.get("apiVersion") else None,
            "topic": j.get("topic", ""), "client": j.get("clientID", ""), "gid": gid}


def load_policy_set(policy_set):
    """Per policy {True: ingress entries, False: egress entries}; an entry is
    (port, [group...]), a group (remotes or None, kafka rules or None when the
    group has no L7 rules)."""
    gid = 0
    out = []
    for p in policy_set["policies"]:
        dirs = {}
        for ingress, key in ((True, "ingress_per_port_policies"), (False, "egress_per_port_policies")):
            entries = []
            for e in p.get(key, []):
                groups = []
                for g in e.get("rules", []):
                    rules = None
                    for kind, inner in (("http_rules", "http_rules"), ("kafka_rules", "kafka_rules"), ("l7_rules", "l7_rules")):
                        if kind in g:
                            items = g[kind][inner]
                            if kind == "kafka_rules":
                                rules = [rule_from_json(k, gid + i) for i, k in enumerate(items)]
                            else:
                                rules = "other"
                            gid += len(items)
                    groups.append((g.get("remote_policies"), rules))
                entries.append((e["port"], groups))
            dirs[ingress] = entries
        out.append(dirs)
    return out


def relevant_rules(policies, conn):
    """GetRelevantRules for the connection's source identity over the exact-port
    entry, then the port-0 entry: (rules, found).  found False is rules.Kafka
    == nil: no group admits the identity.  With PROXYLIB in the connection's
    flags, the proxylib parser's view of the same entries: an
    entry without L7 rules, and a group whose L7 set is empty, let everything
    through."""
    rules, found = [], False
    pi = int(conn["policy"])
    if not 0 <= pi < len(policies):
        return rules, found
    entries = policies[pi][bool(conn["ingress"])]
    port = int(conn["port"])
    exact = [g for p, g in entries if p == port]
    wild = [g for p, g in entries if p == 0 and port != 0]
    px = bool(int(conn["flags"]) & PROXYLIB)
    for groups in exact[-1:] + wild[-1:]:
        if px and (not groups or all(not r for _, r in groups)):
            rules.append(WILDCARD)
            found = True
            continue
        for remotes, r in groups:
            if remotes and int(conn["src_id"]) not in remotes:
                continue
            if r is None or (px and r == []):
                rules.append(WILDCARD)
                found = True
            elif r != "other":
                rules.extend(r)
                found = True
    return rules, found


def rule_matches(req, rule):
    """ruleMatches, policy.go:144-195; req: kind, version, typed (0 nil request,
    1 typed, 2 ConsumerMetadata), client (bytes or None)."""
    if rule["keys"] is not None and req["kind"] not in rule["keys"]:  # CheckAPIKeyRole
        return False
    if rule["version"] is not None and rule["version"] != req["version"]:
        return False
    if rule["topic"] == "" and rule["client"] == "":
        return True
    if req["typed"] == 1:  # match*Req: the typed requests compare the client id
        return rule["client"] == "" or rule["client"].encode() == (req["client"] or b"")
    if req["typed"] == 2:
        return True
    # matchNonTopicRequests
    return not (rule["topic"] != "" and req["kind"] in TOPIC_API_KEYS)


def matches_rule(req, rules):
    """MatchesRule, policy.go:200-225: the position of the rule that allows the
    request, None if none does."""
    topics = req["topics"]
    pending = set(topics)  # reqTopicsMap
    for pos, rule in enumerate(rules):
        if rule["topic"] == "" or len(topics) == 0:
            if rule_matches(req, rule):
                return pos
        elif rule["topic"].encode() in pending:
            if rule_matches(req, rule):
                pending.discard(rule["topic"].encode())
                if not pending:
                    return pos
    return None


def walk_facts(req, rules, pos):
    """What the coverage checks ask about a walk that ended at pos (None:
    denied): topicless (the allowing rule names no topic), first (per distinct
    request topic, the index within the rules naming it of the first that
    matches, None if none does), completion (the position at which the topic
    rules alone cover every topic, None if they never do), topicless_after
    (a topicless rule behind `completion` matches too)."""
    topics = set(req["topics"])
    first, done_at = {}, {}
    for t in topics:
        own = [(p, r) for p, r in enumerate(rules) if r["topic"] != "" and r["topic"].encode() == t]
        hit = [(k, p) for k, (p, r) in enumerate(own) if rule_matches(req, r)]
        first[t] = hit[0][0] if hit else None
        done_at[t] = hit[0][1] if hit else None
    completion = None
    if topics and all(v is not None for v in done_at.values()):
        completion = max(done_at.values())
    after = completion is not None and any(r["topic"] == "" and rule_matches(req, r) for r in rules[completion + 1:])
    return {"topicless": pos is not None and (rules[pos]["topic"] == "" or not topics), "first": first,
            "completion": completion, "topicless_after": after}


def decode(buf):
    """The request as the matcher sees it, None if the reference answers
    neither ALLOW nor DENY (kafka_topics_py.parse)."""
    buf = bytes(buf)
    p = kafka_topics_py.parse(buf)
    if p is None:
        return None
    client = None
    if p["typed"] == 1:  # the typed decoders keep ClientID; a null or empty string reads as ""
        n = int.from_bytes(buf[12:14], "big", signed=True)
        client = buf[14:14 + n] if n > 0 else b""
    return {"kind": p["api_key"], "version": p["api_version"], "typed": p["typed"], "client": client,
            "topics": [buf[o:o + l] for o, l in p["topics"]], "rawlen": p["rawlen"]}


def classify(policies, conn, buf):
    """(allow, gid, consumed, facts) of a well-formed request, else None."""
    req = decode(buf)
    if req is None:
        return None
    rules, found = relevant_rules(policies, conn)
    if not found:
        return False, -1, req["rawlen"], {"pos": None, "rules": None, "req": req}
    pos = matches_rule(req, rules)
    f = dict(walk_facts(req, rules, pos), pos=pos, rules=rules, req=req)
    return pos is not None, (rules[pos]["gid"] if pos is not None else -1), req["rawlen"], f

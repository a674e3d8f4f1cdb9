"""Generated regular expressions as rule sets and request streams for the four
protocols whose verdicts hang on a regex (HTTP header matchers, the memcached
keyRegex, the r2d2 file and the cassandra query_table), so that the device's
DFA and NFA walks meet what tests/test_regex_diff.py only shows to the host
hooks.  CPU only and deterministic: the same seed gives the same bytes.

Patterns come from rand_pattern / ATOMS of tests/test_regex_diff.py; one the
oracle rejects, or that matches more than half of 300 random values of its
slot, is dropped.  Anchoring is each protocol's own (oracle/http_ref.c hmatch:
full match; oracle/memcache_ref.c, r2d2_ref.c, cassandra_ref.c: Go's
regexp.MatchString, unanchored).  One policy per protocol with one port per
rule set (1-4 rules of 1-3 matchers for HTTP, one regex per rule elsewhere);
besides the generated sets:

  nfa      P behind the blow-up prefix (a|b)*a(a|b){12}, which no DFA budget
           holds, so P is walked by the bit-parallel NFA at each call site
  twopass  two 256-state patterns with generated tails on one slot: two DFAs
           (HTTP: a second framing pass; memcached: a second pass over the keys)
  wide     130 rules (r2d2, cassandra): chunks 0, 1 and 2 of the rule masks
  pinned   hand-written patterns for what a device walk had never seen: an
           assertion deciding at the value's end, (?m) at a lone LF, folds,
           \\pL, classes above 0x7F, truncated UTF-8, the empty value

Every request targets one rule of its rule set: the values of that rule's
slots come from the pattern's hit pool (the random values of the slot's
alphabet the oracle's regex accepts), a single-byte edit of a hit, a random
value, the empty value or an absent header.  The alphabets are what the
oracle's framers let through (http_ref.c http_frame: target bytes above 0x20
but 0x7F, values with inner SP / HT; r2d2_ref.c: anything but SP and CR LF;
memcache_ref.c: text keys without a White_Space rune, binary keys any bytes;
cassandra_ref.c: a field of the query, lowered by the parser)."""
import random
import re
from dataclasses import dataclass, field

import numpy as np

import cass_query_cases as Q
import refpy
from cilium_amd import api, gen
from cilium_amd._lib import ALLOW, DENY, INCOMPLETE, PARSE_ERROR, PROTO_CASSANDRA, PROTO_HTTP, PROTO_MEMCACHE, PROTO_R2D2
from test_regex_diff import ATOMS, INPUT_CHARS, rand_pattern

SEED = 7
NFA_PREFIX = "(a|b)*a(a|b){12}"
POOL = 300            # random values per slot kind a pattern is tried on
MAX_RATE = 0.5        # a pattern matching more of them is dropped
# An unanchored pattern longer than this can leave the DFA budget on its own and take its whole policy to
# the NFA kernels; the DFA streams must stay on the DFA kernels (the host test asserts no NFA in them).
MAX_UNANCHORED = 40
ATOM_CLASSES = ("assertion", "unicode_class", "fold", "invalid_byte", "counted_repeat")


def atom_classes(pattern):
    """The generated atom classes a pattern holds."""
    p = pattern.replace("[^", "[")
    out = set()
    if re.search(r"\\b|\\B|\^|\$|\\A|\\z", p):
        out.add("assertion")
    if "\\p" in p:
        out.add("unicode_class")
    if "(?i" in p:
        out.add("fold")
    if "\\x{FFFD}" in p:
        out.add("invalid_byte")
    if re.search(r"\{\d", p.replace("\\x{FFFD}", "")):
        out.add("counted_repeat")
    return out


# ------------------------------------------------------------------ slot kinds
_BASE = [c for c in INPUT_CHARS if c not in (b" ", b"\n")] + [b"x", b"\xed\xa0\x80", b"B"]


@dataclass
class Kind:
    name: str
    alphabet: list
    anchored: bool
    min_atoms: int = 0
    edit: bytes = b"abc/.1A_x\xff\xc3\x82"   # bytes a single-byte edit may put in
    nfa: bool = False                          # values carry a string of the prefix language in front

    def view(self, value):
        """The bytes the protocol's regex sees for a value of this slot."""
        return value


class _CassKind(Kind):
    _parser = None
    _seen = {}

    def view(self, value):
        t = self._seen.get(value)
        if t is None:
            if _CassKind._parser is None:
                _CassKind._parser = refpy.Cassandra()
            rc, _, table = self._parser.parse_query(b"select * from " + value)
            t = self._seen[value] = table if rc == 0 else b""
        return t


KINDS = {
    "http_method": Kind("http_method", [b"a", b"b", b"c", b".", b"1", b"A", b"_", b"x", b"-", b"B"], True, 1, b"abc.1A_x-"),
    "http_path": Kind("http_path", _BASE, True, 1),
    "http_value": Kind("http_value", _BASE + [b" ", b"\t"], True, 0),
    "mc_key": Kind("mc_key", _BASE, False, 1),
    "r2_file": Kind("r2_file", _BASE + [b"\n", b"\n", b"\r"], False, 0, b"abc/.1A_x\xff\xc3\x82\n\r"),
    "cass_table": _CassKind("cass_table", [b"a", b"b", b"c", b".", b"1", b"A", b"B", "É".encode(), "é".encode(),
                                           "İ".encode(), "K".encode(), "ẞ".encode(), b"\xff", b"\xc3",
                                           b"\xe2\x82", b"\xef\xbf\xbd", b"_", b"x"], False, 1, b"abc.1AB_x\xff\xc3\x82"),
}
MC_BIN_EXTRA = [b" ", b"\n", b"\t", b"\r\n"]   # what only a binary key can hold


def _clean(kind, v):
    """A value as the slot can carry it."""
    if kind.name == "http_value":
        v = v.strip(b" \t")
    if kind.name == "r2_file":
        v = v.replace(b"\r\n", b"\r")
    if kind.name == "cass_table" and not v:
        v = b"a"
    if kind.min_atoms and not v:
        v = b"a"
    return v


def rand_value(rng, kind, lo=None):
    n = rng.randint(kind.min_atoms if lo is None else lo, 8)
    return _clean(kind, b"".join(rng.choice(kind.alphabet) for _ in range(n)))


def nfa_prefix_value(rng):
    """A string of (a|b)*a(a|b){12}'s language, or (one time in five) one without the a in place."""
    s = [rng.choice("ab") for _ in range(rng.randint(13, 20))]
    s[-13] = "a" if rng.random() < 0.8 else "b"
    return "".join(s).encode()


def edit_value(rng, kind, v):
    """A single-byte edit of v: a byte replaced, removed or put in."""
    b = bytes([rng.choice(kind.edit)])
    k = rng.randrange(3)
    at = rng.randrange(len(v) + 1)
    if k == 0 and v:
        at = min(at, len(v) - 1)
        v = v[:at] + b + v[at + 1:]
    elif k == 1 and v:
        at = min(at, len(v) - 1)
        v = v[:at] + v[at + 1:]
    else:
        v = v[:at] + b + v[at:]
    return _clean(kind, v)


_pools = {}


def value_pool(kind):
    """The POOL random values of a slot kind (the same for every pattern)."""
    p = _pools.get(kind.name)
    if p is None:
        rng = random.Random(f"{SEED}/pool/{kind.name}")
        p = _pools[kind.name] = [rand_value(rng, kind) for _ in range(POOL)]
    return p


# ------------------------------------------------------------------ patterns
class Pat:
    """A pattern on a slot kind: the oracle's regex, its hit pool and hit rate there."""

    def __init__(self, pattern, kind, rx, nfa_of=None):
        self.pattern, self.kind, self.rx, self.nfa_of = pattern, kind, rx, nfa_of
        if nfa_of is None:
            cand = value_pool(kind)
        else:  # a string of the prefix language, then a value for P
            rng = random.Random(f"{SEED}/nfa/{kind.name}/{pattern}")
            vals = value_pool(kind)
            cand = [nfa_prefix_value(rng) + (rng.choice(nfa_of.hits) if nfa_of.hits and rng.random() < 0.6 else
                                             rng.choice(vals)) for _ in range(POOL)]
            cand = [_clean(kind, c) for c in cand]
        self.hits = [v for v in cand if self.matches(v)]
        self.misses = [v for v in cand if not self.matches(v)][:40]
        self.rate = len(self.hits) / len(cand)
        self.classes = atom_classes(pattern if nfa_of is None else nfa_of.pattern)

    def matches(self, value):
        return self.rx.match(self.kind.view(value), self.kind.anchored)


_pats = {}


def get_pat(pattern, kind):
    key = (pattern, kind.name)
    if key not in _pats:
        try:
            _pats[key] = Pat(pattern, kind, refpy.Regex(pattern))
        except ValueError:
            _pats[key] = None
    return _pats[key]


def gen_patterns(rng, kind, n, max_rate=MAX_RATE, keep_hitless=0.15, need=None):
    """n distinct generated patterns the oracle accepts on a slot kind."""
    out, seen = [], set()
    while len(out) < n:
        p = rand_pattern(rng)
        if p in seen:
            continue
        seen.add(p)
        if not kind.anchored and len(p) > MAX_UNANCHORED:
            continue
        pat = get_pat(p, kind)
        if pat is None or pat.rate > max_rate or (need and not need(pat)):
            continue
        if not pat.hits and rng.random() >= keep_hitless:
            continue
        out.append(pat)
    return out


def nfa_pat(rng, kind):
    """(a|b)*a(a|b){12} + P, anchored as the protocol needs, on a slot kind."""
    full = Kind(kind.name + "/full", kind.alphabet, True, kind.min_atoms, kind.edit)
    full.view = kind.view
    _pools.setdefault(full.name, value_pool(kind))
    while True:
        p = rand_pattern(rng)
        inner = get_pat(p, full)
        if inner is None or inner.rate > MAX_RATE or not inner.hits:
            continue
        if kind.name == "cass_table":   # the table is "<keyspace>.<name>"
            wrapped = "^\\." + NFA_PREFIX + p + "$"
        else:
            wrapped = NFA_PREFIX + p if kind.anchored else "^" + NFA_PREFIX + p + "$"
        key = (wrapped, kind.name)
        if key in _pats:
            continue
        try:
            pat = _pats[key] = Pat(wrapped, kind, refpy.Regex(wrapped), nfa_of=inner)
        except ValueError:
            continue
        if pat.hits:
            return pat


# ------------------------------------------------------------------ rule sets
@dataclass
class Matcher:
    slot: str          # header name (HTTP) or the rule key (keyRegex, file, query_table)
    pat: Pat
    invert: bool = False


@dataclass
class Rule:
    matchers: list
    extra: dict = field(default_factory=dict)   # command / cmd / query_action


@dataclass
class RuleSet:
    proto: int
    port: int
    kind: str          # gen, nfa, twopass, wide, pinned
    rules: list
    first_id: int = 0  # global id of its first rule in the stream's policy

    def slots(self):
        out = []
        for r in self.rules:
            for m in r.matchers:
                if m.slot not in out:
                    out.append(m.slot)
        return out

    def describe(self):
        rules = "; ".join(
            f"[{self.first_id + i}] " + " ".join(f"{k}={v}" for k, v in r.extra.items()) + " " +
            " & ".join(f"{m.slot}{' !~ ' if m.invert else ' ~ '}{m.pat.pattern!r}" for m in r.matchers)
            for i, r in enumerate(self.rules[:12]))
        more = f" ... {len(self.rules)} rules" if len(self.rules) > 12 else ""
        return f"{self.kind} rule set on port {self.port}: {rules}{more}"


def _json_rules(rs):
    if rs.proto == PROTO_HTTP:
        out = []
        for r in rs.rules:
            hs = []
            for m in r.matchers:
                h = {"name": m.slot, "regex_match": m.pat.pattern}
                if m.invert:
                    h["invert_match"] = True
                hs.append(h)
            out.append({"headers": hs})
        return api.port_rule(http=out)
    proto = {PROTO_MEMCACHE: "memcache", PROTO_R2D2: "r2d2", PROTO_CASSANDRA: "cassandra"}[rs.proto]
    return api.port_rule(l7proto=proto, l7=[dict(r.extra, **{m.slot: m.pat.pattern for m in r.matchers}) for r in rs.rules])


@dataclass
class Stream:
    """One protocol's rule sets and requests.  values[i]: [(slot, bytes the
    regex of that slot sees, or None when the header is absent)] of request i."""
    name: str
    proto: int
    sets: list
    reqs: list
    req_set: np.ndarray
    values: list
    _w: object = None
    _ref: object = None

    def policy(self, name="ep", first_id=0):
        nid = first_id
        for rs in self.sets:
            rs.first_id = nid
            nid += len(rs.rules)
        return api.network_policy(name, 1, ingress=[(rs.port, [_json_rules(rs)]) for rs in self.sets])

    def conns(self, hot=None, policy=0):
        """One connection per rule set (connection id = its index), then three
        more on rule set `hot`, which then serves the most connections."""
        ports = [rs.port for rs in self.sets] + ([self.sets[hot].port] * 3 if hot is not None else [])
        return gen.make_conns(len(ports), policy, np.array(ports), True, self.proto, 1 + np.arange(len(ports)))

    @property
    def workload(self):
        if self._w is None:
            arena, offs, lens = gen.pack(self.reqs)
            self._w = gen.Workload(self.name, arena, offs, lens, self.req_set.astype(np.uint32), self.conns(),
                                   api.policy_set(self.policy()), {"sets": self.sets, "req_set": self.req_set})
        return self._w

    @property
    def ref(self):
        """The oracle's (verdict, rule, consumed), computed once."""
        if self._ref is None:
            self._ref = refpy.classify_workload(self.workload, 8)
        return self._ref


def describe(w, i):
    """Request i of a case workload for a mismatch message: rule set, patterns, bytes."""
    o, n = int(w.offsets[i]), int(w.lengths[i])
    req = bytes(w.arena[o:o + min(n, 400)])
    sets = w.meta.get("sets")
    rs = sets[int(w.meta["req_set"][i % len(w.meta["req_set"])])].describe() if sets else "?"
    return f"request {i} on connection {int(w.conn_ids[i])} ({n} bytes) {req!r}\n  {rs}"


def assert_same(got, ref, w):
    """Verdict, rule id and consumed bytes equal; the message names the rule
    set, its patterns and the request bytes of the first difference."""
    for name, a, b in zip(("verdict", "rule", "consumed"), got, ref):
        bad = np.nonzero(np.asarray(a) != np.asarray(b))[0]
        if len(bad):
            i = int(bad[0])
            raise AssertionError(f"{name} differs at {len(bad)} of {len(a)} requests; first: got ({got[0][i]}, {got[1][i]}, "
                                 f"{got[2][i]}) oracle ({ref[0][i]}, {ref[1][i]}, {ref[2][i]})\n  {describe(w, i)}")


# ------------------------------------------------------------------ value choice
def _pick(rng, m, targeted):
    """A value for matcher m's slot; targeted: the request aims at m's rule."""
    kind, pat = m.pat.kind, m.pat
    want_hit = targeted != m.invert
    k = rng.random()
    if targeted and k < (0.55 if pat.nfa_of is None else 0.42):
        pool = pat.hits if want_hit else pat.misses
        if pool:
            return rng.choice(pool)
    elif not targeted and k < 0.2 and pat.hits:
        return rng.choice(pat.hits)
    if k < 0.84 and pat.hits:
        return edit_value(rng, kind, rng.choice(pat.hits))
    if k < 0.94 or kind.min_atoms:
        v = rand_value(rng, kind)
        return _clean(kind, nfa_prefix_value(rng) + v) if pat.nfa_of is not None else v
    return b"" if k < 0.97 else None


def _values_for(rng, rs):
    """{slot: value or None} of a request on rule set rs aimed at one of its rules."""
    target = rng.randrange(len(rs.rules))
    vals = {}
    for m in rs.rules[target].matchers:
        vals.setdefault(m.slot, _pick(rng, m, True))
    others = [m for r in rs.rules for m in r.matchers if m.slot not in vals]
    rng.shuffle(others)
    for m in others:
        vals.setdefault(m.slot, _pick(rng, m, False))
    return target, vals


# ------------------------------------------------------------------ HTTP
HTTP_SLOTS = [(":method", "http_method"), (":path", "http_path"), (":path", "http_path"), (":authority", "http_value"),
              ("x-a", "http_value"), ("X-Token-B", "http_value")]
TWO_PASS = ("[a-z]*a[a-z]{7}", "[a-z]*b[a-z]{7}")
HTTP_PINNED = [
    (":path", "/p/.*\\bx"), (":path", "/q/[a-c]+$"), (":path", "(?i)/É.*k"), (":path", "/u/\\pL+"),
    (":path", "/t/.*\\x{FFFD}"), (":path", "/w/[^b]*\\bend"), (":authority", "x*"), (":authority", "[\\x{80}-\\x{10FFFF}]+"),
    ("x-a", ".*\\Bz"), ("x-a", "(a|\\x{FFFD})*\\b"),
]
HTTP_PINNED_VALUES = {
    ":path": [b"/p/a.x", b"/p/ax", b"/p/x", b"/p/\xc3\xa9x", b"/p/.xx", b"/q/abc", b"/q/abd", b"/q/", b"/\xc3\x89xk",
              b"/\xc3\xa9K", b"/\xc3\xa9\xe2\x84\xaa", b"/\xc3\xa9", b"/u/h\xc3\xa9llo", b"/u/h\xc3", b"/u/\xc3\xa9\xe2\x82",
              b"/t/a\xe2\x82", b"/t/\xc3", b"/t/\xff", b"/t/\xed\xa0\x80", b"/t/\xef\xbf\xbd", b"/t/a", b"/t/",
              b"/w/" + b"a" * 251 + b".end", b"/w/" + b"c" * 270 + b"end", b"/w/" + b"\xc3\xa9" * 130 + b".end",
              b"/w/" + b"a." * 128 + b"b.end", b"/w/" + b"." * 249 + b"end", b"/w/" + b"a" * 247 + b" end"],
    ":authority": [b"", b"x", b"xxxx", b"xy", b"\xc3\xa9", b"\xff", b"\xc3", b"\xe2\x82", b"\xc3\xa9a", b"\xed\xa0\x80",
                   b"x" * 280, b"\xe2\x82\xac" * 90, b"\xe2\x82\xac" * 90 + b"\xe2\x82"],
    "x-a": [b"zz", b"az", b"z", b".z", b"", b"a", b"a\xc3", b"\xc3", b"a\xff a", b"aa.", b"y" * 255 + b"z", b"y" * 256 + b" z"],
}


def _two_pass_pats(rng, kind, heads):
    """The two 256-state heads, each with a generated tail that has hits."""
    out = []
    for head in heads:
        while True:
            tail = rand_pattern(rng)
            if len(tail) > 6:   # (short: the two DFAs are to fit the LDS image together)
                continue
            t = get_pat(tail, Kind(kind.name + "/full", kind.alphabet, True, kind.min_atoms, kind.edit))
            if t is None or not t.hits or t.rate > MAX_RATE or atom_classes(tail) & {"assertion"}:
                continue
            try:
                rx = refpy.Regex(head + tail)
            except ValueError:
                continue
            pat = Pat(head + tail, kind, rx)
            rng2 = random.Random(f"{SEED}/two/{head}{tail}")
            letter = head[head.index("*") + 1].encode()
            for _ in range(200):
                s = bytearray(rng2.choice(b"abcxyz") for _ in range(rng2.randint(8, 14)))
                s[-8] = letter[0] if rng2.random() < 0.8 else ord("c")
                v = _clean(kind, bytes(s) + rng2.choice(t.hits if rng2.random() < 0.7 else value_pool(kind)))
                (pat.hits if pat.matches(v) else pat.misses).append(v)
            if pat.hits:
                out.append(pat)
                break
    return out


def http_sets(rng, n_gen=48, n_nfa=4):
    sets, port = [], 8000
    pools = {k: gen_patterns(rng, KINDS[k], 40) for k in ("http_method", "http_path", "http_value")}
    for _ in range(n_gen):
        rules = []
        for _ in range(rng.randint(1, 4)):
            picks, ms = rng.sample(HTTP_SLOTS, rng.randint(1, 3)), []
            for name, kind in picks:
                if name in [m.slot for m in ms]:
                    continue
                ms.append(Matcher(name, rng.choice(pools[kind]), rng.random() < 0.2))
            rules.append(Rule(ms))
        sets.append(RuleSet(PROTO_HTTP, port, "gen", rules))
        port += 1
    # the wrapped patterns on :path, :authority and a custom header, some inverted
    nfa_slots = [(":path", "http_path"), (":authority", "http_value"), ("x-a", "http_value")]
    for s in range(n_nfa):
        rules = []
        for r in range(3):
            name, kind = nfa_slots[(s + r) % 3]
            ms = [Matcher(name, nfa_pat(rng, KINDS[kind]), s == 1 and r == 2)]
            if r == 1:   # a DFA matcher beside the NFA one
                other = nfa_slots[(s + r + 1) % 3]
                ms.append(Matcher(other[0], rng.choice(pools[other[1]]), s % 2 == 1))
            rules.append(Rule(ms))
        sets.append(RuleSet(PROTO_HTTP, port, "nfa", rules))
        port += 1
    a, b = _two_pass_pats(rng, KINDS["http_value"], TWO_PASS)
    sets.append(RuleSet(PROTO_HTTP, port, "twopass", [Rule([Matcher(":authority", a)]),
                                                       Rule([Matcher(":authority", b)])]))
    port += 1
    pinned = []
    for name, p in HTTP_PINNED:
        pat = get_pat(p, KINDS["http_path" if name == ":path" else "http_value"])
        pat.hits = pat.hits + [v for v in HTTP_PINNED_VALUES[name] if pat.matches(v)]
        pat.misses = [v for v in HTTP_PINNED_VALUES[name] if not pat.matches(v)] + pat.misses
        pinned.append(Rule([Matcher(name, pat)]))
    sets.append(RuleSet(PROTO_HTTP, port, "pinned", pinned))
    return sets


_NAME_FORMS = {":authority": [b"Host", b"host", b"HOST"], "x-a": [b"X-A", b"x-a", b"X-a"],
               "X-Token-B": [b"X-Token-B", b"x-token-b", b"X-TOKEN-B"]}
_OWS_L = [b" ", b" ", b"", b"\t", b"  \t "]
_OWS_R = [b"", b"", b"", b" ", b"\t ", b"   "]


def http_request(rng, rs, vals, rule=None):
    """The request bytes and [(slot, value the regex sees)]."""
    method = vals.get(":method") or b"GET"
    path = vals.get(":path") or b"/"
    seen = [(":method", method), (":path", path)]
    first, again = [], []
    for name in [":authority"] + [s for s in rs.slots() if not s.startswith(":")]:
        v = vals.get(name, rng.choice([b"h", None]) if name == ":authority" else None)
        seen.append((name, None if v is None else v.strip(b" \t")))
        if v is None:
            continue
        nm = rng.choice(_NAME_FORMS[name])
        first.append(nm + b":" + rng.choice(_OWS_L) + v + rng.choice(_OWS_R) + b"\r\n")
        if rng.random() < 0.15:   # a second occurrence, which no matcher looks at
            again.append(nm + b": " + rand_value(rng, KINDS["http_value"]) + b"\r\n")
    if rng.random() < 0.3:
        first.append(b"X-Pad: " + b"p" * rng.randint(0, 30) + b"\r\n")
    rng.shuffle(first)
    req = method + b" " + path + b" HTTP/1.1\r\n" + b"".join(first + again) + b"\r\n"
    if rng.random() < 0.015:      # what the framer refuses, or has not all of
        k = rng.randrange(3)
        req = req.replace(b" HTTP", b"\x7f HTTP", 1) if k == 0 else req[:rng.randrange(len(req))] if k == 1 else \
            req.replace(b"\r\n", b"\n", 1)
        seen = []
    return req, seen


def _stream(name, proto, sets, per_set, build, seed):
    rng = random.Random(f"{SEED}/{name}/{seed}")
    reqs, req_set, values = [], [], []
    for si, rs in enumerate(sets):
        n = per_set(rs) if callable(per_set) else per_set
        for _ in range(n):
            target, vals = _values_for(rng, rs)
            req, seen = build(rng, rs, vals, rs.rules[target])
            reqs.append(req)
            req_set.append(si)
            values.append(seen)
    order = list(range(len(reqs)))
    rng.shuffle(order)
    return Stream(name, proto, sets, [reqs[i] for i in order], np.array([req_set[i] for i in order], np.int64),
                  [values[i] for i in order])


def http_stream(kinds=("gen", "twopass", "pinned"), name="http"):
    """kinds: which rule sets of http_sets() the policy holds (an NFA set in
    the policy sends every call through the NFA pre-pass)."""
    sets = [rs for rs in _cached("http_sets", lambda: http_sets(random.Random(f"{SEED}/http_sets"))) if rs.kind in kinds]
    if "gen" not in kinds:   # the NFA policy keeps a few DFA-only sets beside them
        sets = sets + [rs for rs in _cached("http_sets", None) if rs.kind == "gen"][:6]
    sets = [RuleSet(rs.proto, 8000 + i, rs.kind, rs.rules) for i, rs in enumerate(sets)]
    return _stream(name, PROTO_HTTP, sets, lambda rs: {"gen": 90, "pinned": 250}.get(rs.kind, 400), http_request, 1)


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ------------------------------------------------------------------ memcached
MC_COMMANDS = ["get", "set", "delete"]


def mc_sets(rng, nfa, n_gen=48):
    kind = KINDS["mc_key"]
    sets, port = [], 11000
    if not nfa:
        pool = gen_patterns(rng, kind, 80)
        for _ in range(n_gen):
            rules = [Rule([Matcher("keyRegex", rng.choice(pool))], {"command": rng.choice(MC_COMMANDS)})
                     for _ in range(rng.randint(1, 4))]
            sets.append(RuleSet(PROTO_MEMCACHE, port, "gen", rules))
            port += 1
        a, b = _two_pass_pats(rng, kind, tuple("^" + h for h in TWO_PASS))
        sets.append(RuleSet(PROTO_MEMCACHE, port, "twopass", [Rule([Matcher("keyRegex", a)], {"command": "get"}),
                                                               Rule([Matcher("keyRegex", b)], {"command": "get"})]))
    else:
        pool = gen_patterns(rng, kind, 12, keep_hitless=0.0)
        for s in range(4):
            rules = [Rule([Matcher("keyRegex", nfa_pat(rng, kind))], {"command": MC_COMMANDS[(s + r) % 3]}) for r in range(3)]
            rules.insert(1, Rule([Matcher("keyRegex", rng.choice(pool))], {"command": MC_COMMANDS[s % 3]}))
            sets.append(RuleSet(PROTO_MEMCACHE, port, "nfa", rules))
            port += 1
    return sets


def mc_request(rng, rs, vals, target):
    """A text or binary request, mostly of the command the targeted rule names."""
    cmd = target.extra["command"] if rng.random() < 0.9 else rng.choice(MC_COMMANDS)
    m = target.matchers[0]
    key = vals["keyRegex"] or b""
    binary = rng.random() < 0.3 or not key
    if binary and rng.random() < 0.3:   # bytes only a binary key holds
        at = rng.randrange(len(key) + 1)
        key = key[:at] + rng.choice(MC_BIN_EXTRA) + key[at:]
    if binary:
        op = {"get": [0, 9, 12, 13], "set": [1, 17], "delete": [4, 20]}[cmd]
        extras = bytes(8) if cmd == "set" else b""
        return gen.mc_bin(rng.choice(op), key, extras, b"vv" if cmd == "set" else b""), [("keyRegex", key)]
    if cmd == "get":
        keys = [key]
        for _ in range(rng.choice([0, 0, 1, 2, 3])):   # every key must match: mostly hits of the same rule
            keys.append(_pick(rng, m, True) or b"k")
        rng.shuffle(keys)
        return rng.choice([b"get ", b"gets "]) + b" ".join(keys) + b"\r\n", [("keyRegex", k) for k in keys]
    if cmd == "set":
        return b"set " + key + b" 0 0 2\r\nvv\r\n", [("keyRegex", key)]
    return b"delete " + key + b"\r\n", [("keyRegex", key)]


def mc_stream(nfa=False):
    sets = _cached(("mc_sets", nfa), lambda: mc_sets(random.Random(f"{SEED}/mc_sets/{nfa}"), nfa))
    return _stream("memcached_nfa" if nfa else "memcached", PROTO_MEMCACHE, sets,
                   lambda rs: 400 if rs.kind != "gen" else 100, mc_request, 2)


# ------------------------------------------------------------------ r2d2, cassandra
WIDE_RULES = 130
R2_PINNED = ["^\\x{FFFD}+$", "x\\b\\s", "(?m)^$", "^.$", "^(?s:.)$", "(?m:^)b", "a(?m:$)", "\\s", "[^a]$", "^\\S*$"]
R2_PINNED_VALUES = [b"a\nb", b"a\n", b"\nb", b"b", b"ab", b"\n", b"\r", b"a\rb", b"a\r", b"", b"x", b"x\n", b"x\r", b"xa",
                    b"\xc3", b"\xe2\x82", b"\xff\xff", b"\xef\xbf\xbd", b"\xc3\xa9", b"a\n\nb", b"\na", b"x\x0b"]


def _wide_rules(rng, kind, slot, literal, extra):
    """130 rules: literal fillers, each matching its own value only, with rare
    generated patterns among them in each of the three chunks."""
    fillers = [literal(i)[1] for i in range(WIDE_RULES)]
    rare = gen_patterns(rng, kind, 24, max_rate=0.04, keep_hitless=0.0,
                        need=lambda pat: not any(pat.matches(v) for v in fillers))
    at = set(rng.sample(range(WIDE_RULES), len(rare)))
    rules, k = [], 0
    for i in range(WIDE_RULES):
        if i in at:
            rules.append(Rule([Matcher(slot, rare[k])], dict(extra)))
            k += 1
            continue
        p, v = literal(i)
        pat = Pat(p, kind, refpy.Regex(p))
        pat.hits, pat.misses = [v], [v + b"0", v[:-1]]
        assert pat.matches(v), (p, v)
        rules.append(Rule([Matcher(slot, pat)], dict(extra)))
    return rules


def line_sets(rng, proto, nfa, n_gen=48):
    """r2d2 (slot file) or cassandra (slot query_table) rule sets."""
    r2 = proto == PROTO_R2D2
    kind, slot = (KINDS["r2_file"], "file") if r2 else (KINDS["cass_table"], "query_table")
    verbs = ["READ", "WRITE", None] if r2 else ["select", "insert", "update", "delete", None]
    vkey = "cmd" if r2 else "query_action"

    def extra():
        v = rng.choice(verbs)
        return {vkey: v} if v else {}
    sets, port = [], 4100 if r2 else 9100
    if nfa:
        pool = gen_patterns(rng, kind, 12, keep_hitless=0.0)
        for s in range(4):   # (verbs that differ, so that a rule is not always in the shadow of the one before)
            rules = [Rule([Matcher(slot, nfa_pat(rng, kind))], {vkey: verbs[(s + r) % 2]} if r < 2 else {}) for r in range(3)]
            rules.insert(1, Rule([Matcher(slot, rng.choice(pool))], {vkey: verbs[(s + 1) % 2]}))
            sets.append(RuleSet(proto, port + s, "nfa", rules))
        return sets
    pool = gen_patterns(rng, kind, 80)
    for _ in range(n_gen):
        rules = [Rule([Matcher(slot, rng.choice(pool))], extra()) for _ in range(rng.randint(1, 4))]
        sets.append(RuleSet(proto, port, "gen", rules))
        port += 1
    if r2:
        pinned = []
        for p in R2_PINNED:
            pat = get_pat(p, kind)
            pat.hits = pat.hits + [v for v in R2_PINNED_VALUES if pat.matches(v)]
            pat.misses = [v for v in R2_PINNED_VALUES if not pat.matches(v)] + pat.misses
            pinned.append(Rule([Matcher(slot, pat)], {"cmd": "READ"}))
        sets.append(RuleSet(proto, port, "pinned", pinned))
        port += 1
        wide = _wide_rules(rng, kind, slot, lambda i: ("^/f%03d$" % i, b"/f%03d" % i), {"cmd": "READ"})
    else:
        wide = _wide_rules(rng, kind, slot, lambda i: ("^\\.f%03d$" % i, b"F%03d" % i), {"query_action": "select"})
    sets.append(RuleSet(proto, port, "wide", wide))
    return sets


def r2_request(rng, rs, vals, rule):
    cmd = (rule.extra.get("cmd") or rng.choice(["READ", "WRITE"])) if rng.random() < 0.85 else rng.choice(["READ", "WRITE", "HALT"])
    f = vals["file"]
    k = rng.random()
    if f is None or k < 0.02:
        return cmd.encode() + b"\r\n", [("file", b"")]
    if k < 0.03:
        return cmd.encode() + b" " + f + b" x\r\n", [("file", b"")]       # three fields: no file
    if k < 0.04:
        return cmd.encode() + b" " + f, [("file", None)]                   # no line end yet
    return cmd.encode() + b" " + f + b"\r\n", [("file", f)]


_CASS_FORMS = {"select": b"select * from %s", "insert": b"insert into %s (a) values (1)", "update": b"update %s set a = 1",
               "delete": b"delete from %s where a = 1"}


def _spellings(word):
    """Q.variants without the long s, which does not lower into the word (the query is then no statement)."""
    return [v for v in Q.variants(word) if "\u017f" not in v]


def cass_request(rng, rs, vals, rule):
    """A QUERY (one in five a PREPARE) frame: the table plain, quoted or
    keyspace-qualified, the statement's words in any case."""
    verb = (rule.extra.get("query_action") or rng.choice(sorted(_CASS_FORMS))) if rng.random() < 0.85 else \
        rng.choice(sorted(_CASS_FORMS))
    name = vals["query_table"] or b"t"
    k = rng.random()
    if rs.kind != "wide" and rs.kind != "nfa":
        if k < 0.15:
            name = rng.choice([b"Ks", b"\xc3\x89t", b"\xe2\x84\xaas"]) + b"." + name   # keyspace-qualified
        elif k < 0.25:
            q = rng.choice([b"\"", b"'"])
            name = q + name + q
    words = (_CASS_FORMS[verb] % b"\x00").split(b" ")
    words = [rng.choice(_spellings(x.decode())).encode() if x.isalpha() and rng.random() < 0.3 else x for x in words]
    sep = rng.choice(Q.SPACES) if rng.random() < 0.15 else b" "
    query = sep.join(words).replace(b"\x00", name) + rng.choice([b"", b"", b";"])
    seen = KINDS["cass_table"].view(name) if b"/" not in name else None
    return gen.cass_query_frame(query, 0x09 if rng.random() < 0.2 else 0x07, rng.randrange(65536)), [("query_table", seen)]


def r2_stream(nfa=False):
    sets = _cached(("r2_sets", nfa), lambda: line_sets(random.Random(f"{SEED}/r2_sets/{nfa}"), PROTO_R2D2, nfa))
    return _stream("r2d2_nfa" if nfa else "r2d2", PROTO_R2D2, sets,
                   lambda rs: {"gen": 90, "wide": 700}.get(rs.kind, 300), r2_request, 3)


def cass_stream(nfa=False):
    sets = _cached(("cass_sets", nfa), lambda: line_sets(random.Random(f"{SEED}/cass_sets/{nfa}"), PROTO_CASSANDRA, nfa))
    return _stream("cassandra_nfa" if nfa else "cassandra", PROTO_CASSANDRA, sets,
                   lambda rs: {"gen": 90, "wide": 700}.get(rs.kind, 300), cass_request, 4)


# ------------------------------------------------------------------ all of them
STREAMS = {
    "http": lambda: http_stream(), "http_nfa": lambda: http_stream(("nfa",), "http_nfa"),
    "http_all": lambda: http_stream(("gen", "nfa", "twopass", "pinned"), "http_all"),
    "memcached": lambda: mc_stream(False), "memcached_nfa": lambda: mc_stream(True),
    "r2d2": lambda: r2_stream(False), "r2d2_nfa": lambda: r2_stream(True),
    "cassandra": lambda: cass_stream(False), "cassandra_nfa": lambda: cass_stream(True),
}


def stream(name):
    return _cached(("stream", name), STREAMS[name])


def mixed_workload(names=("http_all", "memcached_nfa", "r2d2_nfa", "cassandra_nfa", "memcached", "r2d2", "cassandra"),
                   per_stream=700):
    """One batch of all four protocols: one policy per stream, the requests interleaved."""
    rng = random.Random(f"{SEED}/mixed")
    policies, conns, reqs, cids, sets, req_set = [], [], [], [], [], []
    first_id = 0
    for pi, nm in enumerate(names):
        s = stream(nm)
        s = Stream(s.name, s.proto, [RuleSet(r.proto, r.port, r.kind, r.rules) for r in s.sets], s.reqs, s.req_set, s.values)
        policies.append(s.policy("ep%d" % pi, first_id))
        first_id += sum(len(r.rules) for r in s.sets)
        base, sbase = sum(len(c) for c in conns), len(sets)
        conns.append(s.conns(policy=pi))
        sets += s.sets
        for i in range(min(per_stream, len(s.reqs))):
            reqs.append(s.reqs[i])
            cids.append(base + int(s.req_set[i]))
            req_set.append(sbase + int(s.req_set[i]))
    order = list(range(len(reqs)))   # (the cassandra streams hold no USE frame: no request depends on another)
    rng.shuffle(order)
    arena, offs, lens = gen.pack([reqs[i] for i in order])
    rs = np.array([req_set[i] for i in order], np.int64)
    return gen.Workload("mixed", arena, offs, lens, np.array([cids[i] for i in order], np.uint32), np.concatenate(conns),
                        api.policy_set(*policies), {"sets": sets, "req_set": rs})


def reset():
    """Forget everything built so far (the determinism test builds twice)."""
    _cache.clear()
    _pats.clear()
    _pools.clear()


def conditions(s):
    """The oracle-only figures of a stream the host test holds against its thresholds."""
    v, r, _ = s.ref
    n = len(v)
    both, allowing, nrules = 0, set(r[v == ALLOW].tolist()), 0
    for si, rs in enumerate(s.sets):
        sel = s.req_set == si
        both += bool((v[sel] == ALLOW).any() and (v[sel] == DENY).any())
        nrules += len(rs.rules)
    return {"n": n, "allow": float((v == ALLOW).mean()), "deny": float((v == DENY).mean()),
            "sets": len(s.sets), "sets_both": both, "rules": nrules, "rules_allowing": len(allowing - {-1}),
            "other": float(((v == PARSE_ERROR) | (v == INCOMPLETE)).mean()),
            "patterns": len({m.pat.pattern for rs in s.sets for r in rs.rules for m in r.matchers})}

"""Cassandra queries for the parser tests (kernels/cass_parse.h against
oracle/cassandra_ref.c): a curated list with the answers read off
proxylib/cassandra/cassandraparser.go:368-469 and Go 1.10's strings.ToLower /
strings.Fields, and a seeded generator that composes queries from the grammar's
own parts.  Pure Python; no GPU, no oracle, no product code.

A case is (use, query, seps, invalid): the USE query that set the connection's
keyspace before it (bytes, or None), the query (bytes, never with a NUL: the
oracle's test hooks read C strings), the set of separators between its tokens
and the invalid-byte form put into it (or None)."""
import random
from collections import namedtuple

Case = namedtuple("Case", "use query seps invalid")

# Unicode White_Space (unicode.IsSpace), spelled out
WHITE_SPACE = [0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680,
               0x2000, 0x2001, 0x2002, 0x2003, 0x2004, 0x2005, 0x2006, 0x2007, 0x2008, 0x2009, 0x200A,
               0x2028, 0x2029, 0x202F, 0x205F, 0x3000]
SPACES = [chr(c).encode() for c in WHITE_SPACE]
# not spaces: ZERO WIDTH SPACE, the BOM, the ASCII separators FS GS RS US
LOOKALIKES = [chr(c).encode() for c in (0x200B, 0xFEFF, 0x1C, 0x1D, 0x1E, 0x1F)]

# invalid UTF-8: every byte of each form decodes as a RuneError of width 1
INVALID = {
    "continuation": b"\x80", "continuation_bf": b"\xbf", "cut2": b"\xc3", "cut3_1": b"\xe2", "cut3_2": b"\xe2\x80",
    "cut4_2": b"\xf0\x9f", "cut4_3": b"\xf0\x9f\x98", "surrogate": b"\xed\xa0\x80", "overlong": b"\xc0\xa0",
    "above_max": b"\xf4\x90\x80\x80", "raw_85": b"\x85", "raw_a0": b"\xa0",
}
FFFD = b"\xef\xbf\xbd"

STATEMENTS = ["select", "delete", "insert", "update", "use", "alter", "create", "drop", "truncate", "list"]
WORDS = STATEMENTS + ["from", "table", "keyspace", "if", "materialized", "custom", "index", "role", "user", "function",
                      "aggregate", "type", "trigger", "roles", "permissions", "users"]
KEYWORDS = WORDS + ["grant", "revoke"]
SECOND = ["table", "keyspace", "materialized", "custom", "index", "role", "user", "function", "aggregate", "type",
          "trigger", "roles", "permissions", "users"]
FILLERS = ["*", "a,", "(a)", "=", "1", "where", "into", "not", "exists", "view", "on", "set", "values", "with", "-", "/"]

# names by the decoder's ranges: (2-byte, below / from U+0400), (3-byte, below / from U+8000), 4-byte, plane 16;
# with and without a rune that ToLower changes
NAMES = {
    "ascii": ["t", "users", "Tmp1", "KS", "x9"],
    "b2_low": ["été", "ÉTÀ", "Ωm", "āĀ"],
    "b2_high": ["Дб", "дб", "Рф", "a\u0485b", "של", "با", "Աա"],
    "b3_low": ["あい", "中文", "Ḁḁ", "Ⰰx"],
    "b3_high": ["表験", "a뀀b", "한글", "Ａｂ", "Ꙁꙁ", "\ufffd"],
    "b4": ["\U0001f600", "\U0001d400x", "\U00010400\U00010428", "\U00016f00"],
    "plane16": ["\U00100000", "\U0010ffff", "q\U0010fffdZ"],
    "relength": ["Ⱥ", "ȾȺ", "ẞ", "Ɫ", "Ɽx", "\u212a", "\u0130", "\u212as\u0130", "ⱯⱭ"],
}
ALL_NAMES = [n for k in sorted(NAMES) for n in NAMES[k]]


def variants(word):
    """Spellings of a grammar word: lower, upper, mixed, Kelvin sign for k, dotted
    capital I for i (both lower into the word), long s for s (does not)."""
    out = [word, word.upper(), "".join(c.upper() if k % 2 else c for k, c in enumerate(word))]
    if "k" in word:
        out.append(word.replace("k", "\u212a", 1))
    if "i" in word:
        out.append(word.replace("i", "\u0130", 1).upper())
    if "s" in word:
        out.append(word.replace("s", "\u017f", 1))
    return out


# ------------------------------------------------------------------ curated
# (use, query, status or (status, parts[2], parts[3])): parts of
# "/<op>/<action>/<table>" split on "/" (CassandraRule.Matches).  Each list is
# one branch of parseQuery, ToLower or Fields that the fixed corpora of
# cilium_amd/gen.py do not reach.
def _b(s):
    return s if isinstance(s, bytes) else s.encode()


CURATED = {
    "observed": [  # the four queries that showed the oracle's decoder slip
        (None, "select * from Дб", (0, "select", ".дб")),
        (None, "select * from a뀀b", (0, "select", ".a뀀b")),
        (None, "select * from a\u0485b", (0, "select", ".a\u0485b")),
        (None, "SELECT * FROM t\ufeff", (0, "select", ".t\ufeff")),
    ],
    "create_table_if_short": [
        (None, "create table if", 1), (None, "create table if not", 1), (None, "CREATE TABLE IF NOT EXISTS", 1),
        (None, "create table if not exists T", (0, "create-table", ".t")),
        ("use k", "create table if not exists t (a int)", (0, "create-table", "k.t")),
    ],
    "drop_if_short": [
        (None, "drop table if", 1), (None, "drop table if exists", 1), (None, "drop keyspace if", 1),
        (None, "DROP KEYSPACE IF EXISTS", 1), (None, "drop table if exists t", (0, "drop-table", ".t")),
        (None, "drop keyspace if exists k.s", (0, "drop-keyspace", "k.s")),
    ],
    "drop_table_two": [
        (None, "drop table", 1), (None, "drop keyspace", 1), (None, "alter table", 1), (None, "truncate table;", 1),
        (None, "create keyspace", 1), (None, "drop index", (0, "drop-index", "")),
    ],
    "alter_if": [
        (None, "alter table if exists t", (0, "alter-table", ".if")),
        (None, "ALTER KEYSPACE IF x", (0, "alter-keyspace", ".if")),
        ("use k", "create keyspace if not exists z", (0, "create-keyspace", "k.if")),
        (None, "truncate table \u0130f exists t", (0, "truncate-table", ".if")),
        (None, "alter table if", (0, "alter-table", ".if")),
    ],
    "materialized": [(None, kw + " materialized view v", (0, kw + "-materialized-view", ""))
                     for kw in ("alter", "create", "drop", "truncate", "list")] +
                    [(None, "drop MATER\u0130AL\u0130ZED", (0, "drop-materialized-view", "")),
                     (None, "create materialized/ v", (0, "create-materialized", ""))],
    "custom": [(None, kw + " custom index i", (0, "create-index", ""))
               for kw in ("alter", "create", "drop", "truncate", "list")] +
              [(None, "LIST CUSTOM", (0, "create-index", "")), (None, "create custom/i x", (0, "create-custom", "i"))],
    "slash_in_field1": [
        (None, "create table/x y", (0, "create-table", "x")), (None, "drop /table t", (0, "drop-", "table")),
        (None, "create index/ x", (0, "create-index", "")), (None, "create role/a/b c", (0, "create-role", "a")),
        (None, "alter keyspace/K\u212a z", (0, "alter-keyspace", "kk")), (None, "list /", (0, "list-", "")),
        (None, "DROP TABLE/Д", (0, "drop-table", "д")), (None, "truncate x/table t", (0, "truncate-x", "table")),
    ],
    "trailing_from": [
        (None, "select a b c d e from", 2), (None, "select a from t b c d from", 2),
        (None, "delete a b c d e f g from;", 2), (None, "select a b c d e f FROM\u3000", 2),
        (None, "select a b c d e f from t", (0, "select", ".t")),
        (None, "select a from x b c d e from y z", (0, "select", ".y")),
    ],
    "comment_index": [
        (None, "-- select * from t", 1), (None, "/* x */ select * from t", 1), (None, "//select * from t", 1),
        (None, "select -- * from t", 1), (None, "select * from t where a = 1 --c", 1),
        (None, "select * from t where a = 1 and b = 2 //x", 1), (None, "select a b c d e f g h /*", 1),
        (None, "select * from t\u00a0--x", 1), (None, "use --", 1), (None, "create table t //", 1),
        (None, "select * from - x", (0, "select", ".-")), (None, "select * from -/- x", (0, "select", ".-")),
        (None, "select * from t /-", (0, "select", ".t")), (None, "select * from t -\u2003-", (0, "select", ".t")),
    ],
    "semicolons": [
        (None, "select * from t;;;", (0, "select", ".t")), (None, ";;;", 1), (None, ";", 1),
        (None, "select * from t; ;", (0, "select", ".t;")), (None, "select * from t ;", (0, "select", ".t")),
        (None, "select * from ;t", (0, "select", ".;t")), (None, "use ks;;", (0, "use", "ks")),
        (None, "select * from;", 2), (None, "select * from ;;", 2), (None, "use ;x;", (0, "use", ";x")),
        (None, "select;* from t", 1),
    ],
    "lookalikes": [(None, b"select * from a" + z + b"b", (0, b"select", b".a" + z + b"b")) for z in LOOKALIKES] +
                  [(None, b"select" + z + b"* from t", 1) for z in LOOKALIKES] +
                  [(None, b"SELECT * FROM" + LOOKALIKES[0] + b" T", 1), (None, b"use " + LOOKALIKES[1], (0, b"use", LOOKALIKES[1]))],
    "relength": [
        (None, "select * from Ⱥ", (0, "select", ".ⱥ")), (None, "select * from k.ẞx", (0, "select", "k.ßx")),
        (None, "select * from ⱢⱢ", (0, "select", ".ɫɫ")),
        (None, "select * from \u212a.\u0130", (0, "select", "k.i")),
        (None, "select * from \U00010400\U00010427", (0, "select", ".\U00010428\U0001044f")),
        ("use Ⱦ", "update Ɽ set", (0, "update", "ⱦ.ɽ")),
        (None, "use \u0130\u212a", (0, "use", "ik")), (None, "create \u212aȺ x", (0, "create-kⱥ", "")),
    ],
    "use_prefix": [
        ("use Дб", "select * from t", (0, "select", "дб.t")),
        ("USE \"Ks\"", "select * from T", (0, "select", "ks.t")), ("use 'a/b'", "select * from t", (0, "select", "a")),
        ("use ''", "select * from t", (0, "select", ".t")), ("use \\\"'", "insert into t", (0, "insert", ".t")),
        ("use 한", "update Ａ", (0, "update", "한.ａ")),
        ("use \U0010ffff", "delete from \U0001f600", (0, "delete", "\U0010ffff.\U0001f600")),
        (b"use k\xffs", "select * from t", (0, b"select", b"k\xffs.t")),
        (b"USE k\xffs", "select * from t", (0, b"select", b"k" + FFFD + b"s.t")),
        ("use", "select * from t", (0, "select", ".t")), ("use k --", "select * from t", (0, "select", ".t")),
        ("use k", "select * from a.b", (0, "select", "a.b")), ("use k", "use 'Z'", (0, "use", "z")),
    ],
}
# an invalid byte before the first rune that ToLower changes stays as it is; from there on it is U+FFFD
CURATED["invalid_before_fc"] = [(None, b"select * from t" + f + b"x", (0, b"select", b".t" + f + b"x"), k)
                                for k, f in INVALID.items()] + \
                               [(None, b"select * from " + f + b"X", (0, b"select", b"." + f + b"x"), k)
                                for k, f in INVALID.items()]
CURATED["invalid_after_fc"] = [(None, b"select * from T" + f, (0, b"select", b".t" + FFFD * len(f)), k)
                               for k, f in INVALID.items()] + \
                              [(None, b"Select * from t" + f + b"x", (0, b"select", b".t" + FFFD * len(f) + b"x"), k)
                               for k, f in INVALID.items()] + \
                              [(None, b"select * from \xc3\x89" + f, (0, b"select", b".\xc3\xa9" + FFFD * len(f)), k)
                               for k, f in INVALID.items()]
# each White_Space rune as the only separator, doubled in one place
CURATED["white_space"] = [(None, s.join([b"select", b"*", b"from" + s, b"w%d" % k, b"x"]), (0, b"select", b".w%d" % k))
                          for k, s in enumerate(SPACES)]


def curated():
    """[(branch, Case, want)]: want = status, or (status, parts[2], parts[3]) as bytes."""
    out = []
    for branch in sorted(CURATED):
        for use, q, want, *form in CURATED[branch]:
            if not isinstance(want, int):
                want = (want[0], _b(want[1]), _b(want[2]))
            out.append((branch, Case(None if use is None else _b(use), _b(q), frozenset(), form[0] if form else None), want))
    return out


# ------------------------------------------------------------------ generator
def _identifier(rng):
    name = rng.choice(ALL_NAMES)
    k = rng.random()
    if k < 0.25:
        name = rng.choice(ALL_NAMES) + "." + name
    elif k < 0.30:
        name = "." + name
    elif k < 0.33:
        name = name + "."
    k = rng.random()
    if k < 0.10:
        c = rng.choice("\"'\\")
        name = c + name + c
    elif k < 0.14:
        name = rng.choice("\"'\\") + name
    elif k < 0.24:
        at = rng.choice(["start", "mid", "end"])
        name = "/" + name if at == "start" else name + "/" if at == "end" else name + "/" + rng.choice(ALL_NAMES)
    elif k < 0.28:
        name = rng.choice(["--", "/*", "//"]) + name
    return name.encode()


def _word(rng, pool=WORDS):
    return rng.choice(variants(rng.choice(pool))).encode()


def _token(rng, glue=True):
    k = rng.random()
    t = _word(rng) if k < 0.30 else _identifier(rng) if k < 0.85 else rng.choice(FILLERS).encode()
    if glue and rng.random() < 0.04:  # a lookalike inside the token
        at = rng.randrange(len(t) + 1)
        while at < len(t) and t[at] & 0xC0 == 0x80:
            at += 1
        t = t[:at] + rng.choice(LOOKALIKES) + t[at:]
    return t


def _tokens(rng):
    n = rng.choice([0, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5, 6, 6, 6, 7, 7, 8, 9])
    if n == 0:
        return []
    kw = rng.choice(STATEMENTS) if rng.random() < 0.85 else rng.choice(KEYWORDS)
    toks = [rng.choice(variants(kw)).encode()] + [_token(rng) for _ in range(n - 1)]
    if kw in ("select", "delete") and n >= 2 and rng.random() < 0.7:
        toks[rng.randrange(1, n)] = _word(rng, ["from"])
    if kw in ("alter", "create", "drop", "truncate", "list") and n >= 2:
        k = rng.random()
        if k < 0.55:
            toks[1] = _word(rng, SECOND)
            if rng.random() < 0.06:
                toks[1] += b"/" + rng.choice(ALL_NAMES).encode()
            if n >= 3 and rng.random() < 0.3:
                toks[2] = _word(rng, ["if"])
        elif k < 0.75:  # "<kw>-<name>": an action outside queryActionMap
            toks[1] = rng.choice(ALL_NAMES + ["x%d" % rng.randrange(400)]).encode()
    return toks


def _keyspace_use(rng):
    """A USE query for the connection's keyspace: plain, upper case, quoted, with
    '/', empty, non-ASCII of each range, with an invalid byte."""
    k = rng.random()
    name = rng.choice(ALL_NAMES).encode()
    if k < 0.15:
        name = rng.choice(["ks1", "KS2", "System"]).encode()
    elif k < 0.30:
        c = rng.choice("\"'\\").encode()
        name = c + name + c
    elif k < 0.38:
        name = name + b"/" + rng.choice(ALL_NAMES).encode()
    elif k < 0.44:
        name = b"''"
    elif k < 0.52:
        name = name + rng.choice(sorted(INVALID.values())) + b"z"
    use = rng.choice(variants("use")).encode() + rng.choice(SPACES) + name
    return use + rng.choice([b"", b";", b" ;"])


def generate(n, seed=0x1C1D0C45):
    """n seeded cases."""
    rng = random.Random(seed)
    forms = sorted(INVALID)
    out = []
    for _ in range(n):
        toks = _tokens(rng)
        k = rng.random()
        if k < 0.45:
            seps = [b" "] * len(toks)
        elif k < 0.70:
            seps = [rng.choice(SPACES)] * len(toks)          # one rune is the only separator
        else:
            seps = [rng.choice(SPACES) * rng.choice([1, 1, 2]) + (rng.choice(SPACES) if rng.random() < 0.2 else b"")
                    for _ in toks]
        used = frozenset(s for s in SPACES for sep in seps[1:] if s in sep)
        q = b"".join((sep if i else b"") + t for i, (t, sep) in enumerate(zip(toks, seps)))
        if rng.random() < 0.10:
            q = rng.choice(SPACES) + q + rng.choice(SPACES)
        invalid = None
        if q and rng.random() < 0.18:
            invalid = forms[rng.randrange(len(forms))]
            at = rng.randrange(len(q) + 1)
            if rng.random() < 0.8:  # between runes (else anywhere, which may cut one)
                while at < len(q) and q[at] & 0xC0 == 0x80:
                    at += 1
            q = q[:at] + INVALID[invalid] + q[at:]
        q += rng.choice([b"", b"", b"", b";", b";;", b" ;", b"; "])
        use = _keyspace_use(rng) if rng.random() < 0.3 else None
        assert b"\x00" not in q and (use is None or b"\x00" not in use)
        out.append(Case(use, q, used, invalid))
    return out


def corpus(n=20000, seed=0x1C1D0C45):
    """The curated cases, then n generated ones."""
    return [c for _, c, _ in curated()] + generate(n, seed)


# queryActionMap (cassandraparser.go:319-366), in the order of the action ids of kernels/cass_parse.h
ACTIONS = ["select", "delete", "insert", "update", "create-table", "drop-table", "alter-table", "truncate-table", "use",
           "create-keyspace", "alter-keyspace", "drop-keyspace", "drop-index", "create-index", "create-materialized-view",
           "drop-materialized-view", "create-role", "alter-role", "drop-role", "grant-role", "revoke-role", "list-roles",
           "grant-permission", "revoke-permission", "list-permissions", "create-user", "alter-user", "drop-user",
           "list-users", "create-function", "drop-function", "create-aggregate", "drop-aggregate", "create-type",
           "alter-type", "drop-type", "create-trigger", "drop-trigger"]

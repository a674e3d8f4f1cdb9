"""The fields of the LogEntry_GenericL7 the proxylib parsers log per request,
restated in Python straight from the reference's Go (test infrastructure; the
device records of l7g_classify_logged_all are compared with it):

  memcached text    proxylib/memcached/text/parser.go:84-171
  memcached binary  proxylib/memcached/binary/parser.go:72-105, :174-191
  r2d2              proxylib/r2d2/r2d2parser.go:158-205
  cassandra         proxylib/cassandra/cassandraparser.go:230-244 (the split of
                    a path; the path itself is the oracle's, tests/refpy.py)

Each function takes the bytes OnData is handed and returns None where the
parser logs nothing for them (MORE, ERROR, a Go panic), else a dict with
"proto", "fields" (bytes values: Go strings are bytes) and the spans
(offset, length) of the pieces inside the request."""
import re

_SPACE_RUNES = {0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000} | \
    set(range(0x2000, 0x200B))  # unicode.IsSpace (White_Space)


def decode_rune(b, i):
    """utf8.DecodeRune(b[i:]): (rune, width); invalid UTF-8 is (0xFFFD, 1)."""
    c = b[i]
    if c < 0x80:
        return c, 1
    if c < 0xC2 or c > 0xF4:
        return 0xFFFD, 1
    need = 1 if c < 0xE0 else 2 if c < 0xF0 else 3
    if len(b) - i <= need:
        return 0xFFFD, 1
    lo, hi = 0x80, 0xBF
    if c == 0xE0:
        lo = 0xA0
    elif c == 0xED:
        hi = 0x9F
    elif c == 0xF0:
        lo = 0x90
    elif c == 0xF4:
        hi = 0x8F
    if not lo <= b[i + 1] <= hi:
        return 0xFFFD, 1
    r = (c & (0x7F >> (need + 1))) << 6 | (b[i + 1] & 0x3F)
    for k in range(2, need + 1):
        if not 0x80 <= b[i + k] <= 0xBF:
            return 0xFFFD, 1
        r = r << 6 | (b[i + k] & 0x3F)
    return r, need + 1


def go_fields(b):
    """bytes.Fields(b) as (start, end) spans: split around runs of
    unicode.IsSpace runes, decoding rune by rune."""
    out, start, i = [], -1, 0
    while i < len(b):
        r, w = decode_rune(b, i)
        if r in _SPACE_RUNES and not (w == 1 and r == 0xFFFD):
            if start >= 0:
                out.append((start, i))
                start = -1
        elif start < 0:
            start = i
        i += w
    if start >= 0:
        out.append((start, len(b)))
    return out


_STORAGE = (b"set", b"add", b"replace", b"append", b"prepend", b"cas")
_NOKEY = (b"slabs", b"lru", b"lru_crawler", b"stats", b"version", b"misbehave", b"flush_all", b"cache_memlimit", b"quit",
          b"watch")


def _atoi_ok(t):
    """strconv.Atoi succeeds (Go 1.10: sign, decimal digits, int64 range)."""
    return bool(re.fullmatch(rb"[+-]?[0-9]+", t)) and -(1 << 63) <= int(t) < (1 << 63)


def mc_text(data):
    linefeed = data.find(b"\r\n")
    if linefeed < 0:
        return None  # MORE
    toks = go_fields(data[:linefeed])
    if not toks:
        return None  # tokens[0] panics
    tok = [data[s:e] for s, e in toks]
    cmd = tok[0]
    if cmd.startswith(b"get"):
        keys = toks[1:]
    elif cmd.startswith(b"gat"):
        if len(toks) < 2:
            return None  # tokens[2:] panics
        keys = toks[2:]
    elif cmd in _STORAGE:
        if len(toks) < 5 or not _atoi_ok(tok[4]):
            return None  # tokens[4] panics / ERROR
        keys = toks[1:2]
    elif cmd in (b"delete", b"incr", b"decr", b"touch"):
        if len(toks) < 2:
            return None  # tokens[1:2] panics
        keys = toks[1:2]
    elif cmd in _NOKEY:
        keys = []
    else:
        return None  # ERROR
    return {"proto": "textmemcached",
            "fields": {"command": cmd, "keys": b", ".join(data[s:e] for s, e in keys)},
            "cmd": (toks[0][0], toks[0][1] - toks[0][0]), "keys": [(s, e - s) for s, e in keys]}


def mc_binary(data):
    if len(data) < 24:
        return None  # MORE
    key_len = int.from_bytes(data[2:4], "big")
    extras = data[4]
    if key_len > 0 and 24 + key_len + extras > len(data):
        return None  # MORE
    if data[0] & 0x80 != 0x80:
        return None  # ERROR_INVALID_FRAME_TYPE
    key = data[24 + extras:24 + extras + key_len] if key_len else b""
    return {"proto": "binarymemcached", "fields": {"opcode": str(data[1]).encode(), "key": key},
            "opcode": data[1], "key": (24 + extras if key_len else 0, key_len)}


def memcached(data, conn_flags=0):
    """The parser the classifier picks (the connection's L7G_CONN_MC_* flags,
    else the first byte >= 0x80), then its fields."""
    mode = conn_flags & 3
    if mode == 0:
        if not data:
            return None
        mode = 2 if data[0] >= 0x80 else 1
    return mc_binary(data) if mode == 2 else mc_text(data)


def r2d2(data):
    if b"\r\n" not in data:
        return None  # MORE
    msg = data.split(b"\r\n")[0]
    fields = msg.split(b" ")  # strings.Split: empty fields count
    f = fields[1] if len(fields) == 2 else b""
    return {"proto": "r2d2", "fields": {"cmd": fields[0], "file": f}, "cmd_len": len(fields[0]),
            "file": (len(fields[0]) + 1, len(f)) if len(fields) == 2 else (0, 0), "nfields": len(fields)}


def cassandra_path(path):
    """The entry logged for one path (cassandraparser.go:230-244): only a path
    of exactly four '/'-separated parts is logged."""
    if path is None:
        return None
    parts = path.split(b"/")
    if len(parts) != 4:
        return None
    return {"proto": "cassandra", "fields": {"query_action": parts[2], "query_table": parts[3]}}

"""Directed memcached requests for the classifier's position-dependent
machinery (csrc/kernels/memcache_classify.hip: text_fast's 16-byte chunks, the
binary header walk) and the arena layouts that put each of them at every chunk
position.  A helper module, not a test module; deterministic, no random numbers.

corpus(K) is the list of unique requests, by family:

  A  line ends: CR LF / lone CR / lone LF / LF CR / nothing after a key whose
     length is swept, and a second CR LF later in the buffer
  B  every White_Space rune of gen._MC_SPACES as a separator: between two keys,
     between the last key and the line end, after the command, before the
     command; a storage line separated by that rune only; runs of two and three
     different runes
  C  near misses in the same places: runes next to the White_Space ones,
     bare continuation bytes, controls (0x1C-0x1F are space to Python's
     str.split and not to Go), and lead bytes or rune prefixes that end the
     line or the request (a rune cut by the request's end cannot come before
     a line end inside the request, so the text parser answers MORE however
     the bytes are split: the verdict cannot tell `r + 2 < len` from
     `r + 2 <= len` in the kernel's rune test; a CR as the last byte with the
     neighbour's LF behind it, completions() below, is the case it can tell)
  D  every prefix of six representative requests
  E  the first token: every command name, shortened, lengthened, NUL-padded to
     16 and 17 bytes, upper case, 16 bytes that agree with it up to its length
  F  tokens[4] of a storage line: signs, junk, int64 and uint32 borders
  G  1 .. 300 keys, all allowed but one, denied first / middle / last / nowhere
  H  binary headers: extras 0-19 x key length 0-19, one byte short, body lengths
     around the uint32 wrap, magics, an opcode no group names
  I  the empty request, a binary request that holds a line end, text that reads
     as a binary header (the parser forced by the connection: conns() below
     gives every request connections with flags 0, 1 and 2)

K is the key material (Keys): per command class a key the installed policy
allows -- and keeps allowing when filler bytes are appended --, a key it denies,
and the filler byte; the same families are aimed at several policies with it.

full_layout() places every request at all 16 offsets mod 16, followed by bytes
that belong to no request: what would complete a rune, a line end or a key if a
kernel looked one byte past `len` (the oracle reads [off, off + len) only).
rotating_layout() places request i once, at offset i mod 16."""
from collections import namedtuple

import numpy as np

from cilium_amd import api, gen
from cilium_amd._lib import PROTO_MEMCACHE

Keys = namedtuple("Keys", "allow deny filler")   # allow: {"get","gat","storage","delete","touch"} -> key
Case = namedtuple("Case", "family req feat")     # feat: request offset of the byte the case is about (or None)
Placed = namedtuple("Placed", "arena offsets lengths conn_ids case align")

MC_POLICY_KEYS = Keys({"get": b"user:1", "gat": b"user:1", "storage": b"cache:1", "delete": b"tmp",
                       "touch": b"k\xc3\xa9y"}, b"obj7", ord("1"))   # for gen.mc_policy()

SPACES = gen._MC_SPACES
WIDE_SPACES = [s for s in SPACES if len(s) > 1]
NEAR = gen._MC_NOT_SPACES + [b"\xe2\x80\x7f", b"\xe2\x80\x8b", b"\xe2\x80\xa7", b"\xe2\x80\xb0", b"\xe2\x81\x9e",
                             b"\xe1\x9a\x81", b"\xc2\x86", b"\xe3\x80\x81", b"\x85", b"\xa0", b"\x80",
                             b"\x08", b"\x0e", b"\x1c", b"\x1f"]
LEADS = [b"\xc2", b"\xe1", b"\xe2", b"\xe3", b"\xe2\x80", b"\xe1\x9a", b"\xe3\x80", b"\xe2\x81"]
COMMANDS = [b"get", b"gets", b"gat", b"gats", b"set", b"add", b"replace", b"append", b"prepend", b"cas", b"delete",
            b"incr", b"decr", b"touch", b"slabs", b"lru", b"lru_crawler", b"stats", b"version", b"misbehave",
            b"flush_all", b"cache_memlimit", b"quit", b"watch"]
ATOI = [b"0", b"-1", b"-2", b"-3", b"+7", b"abc", b"-", b"+", b"007", b"-0", b"1e3", b"0x10",
        b"9223372036854775806", b"9223372036854775807", b"-9223372036854775808", b"-9223372036854775809",
        b"18446744073709551615", b"99999999999999999999", b"1" * 40,
        b"4294967270", b"4294967280", b"4294967290", b"4294967295", b"\xd9\xa1"]
KEY_COUNTS = [1, 2, 3, 17, 64, 255, 256, 257, 300]
BIN_OPCODES = {0: "get", 1: "storage", 4: "delete", 29: "gat"}
BODIES = [0, 1, 0xFFFFFFE7, 0xFFFFFFE8, 0xFFFFFFE9, 0x7FFFFFFF, 0xFFFFFFFF]
MAGICS = [0x80, 0x81, 0xFF, 0x00, 0x7F]
SWEEP = 17          # consecutive lengths of the token before a separator (one more than a chunk)
TRAILS = [b"", b"\n", b"\r\n", b"\x80", b"\x9a\x80", b"\xa0", b"\x80\x80", None]  # None: " <allowed key>\r\n"
NCONNS = 12         # conns(): flags c % 3, kind (0, 0, 1, 2)[c // 3]


def key(K, cls, n=None):
    """The class's allowed key, cut or filled to n bytes (filled: still allowed)."""
    k = K.allow[cls]
    return k if n is None else (k + bytes([K.filler]) * n)[:n]


def _class(cmd):
    return ("gat" if cmd.startswith(b"gat") else "delete" if cmd == b"delete" else "touch" if cmd == b"touch" else
            "storage" if cmd in (b"set", b"add", b"replace", b"append", b"prepend", b"cas", b"incr", b"decr") else "get")


def _placements(K, sep, n):
    """The four places of a separator (or a near miss): (request, offset of sep)."""
    kn, k2 = key(K, "get", n), key(K, "get")
    yield b"get " + kn + sep + k2 + b"\r\n", 4 + n                     # between two keys
    yield b"get " + kn + sep + b"\r\n", 4 + n                          # last key, then the line end
    cmd = b"get" + b"x" * (n - len(K.allow["get"]))                    # (the command token's length swept)
    yield cmd + sep + k2 + b"\r\n", len(cmd)                           # after the command
    yield sep + b"get " + kn + b"\r\n", 0                              # before the command


def corpus(K):
    out, seen = [], set()

    def add(fam, req, feat=None):
        if (fam, req) not in seen:
            seen.add((fam, req))
            out.append(Case(fam, bytes(req), feat))

    base = len(K.allow["get"])
    sweep = range(base, base + SWEEP)
    # ---- A
    for n in range(base, base + 33):
        line = b"get " + key(K, "get", n)
        for tail in (b"\r\n", b"\r", b"\n", b"\n\r", b"", b"\r\nget " + K.deny + b"\r\n", b"\r\r\n", b"\n\r\n"):
            add("A", line + tail, len(line))
    # ---- B
    for i, sp in enumerate(SPACES):
        for n in sweep:
            for req, f in _placements(K, sp, n):
                add("B", req, f)
            ks = key(K, "storage", n)
            add("B", sp.join([b"set", ks, b"0", b"0", b"3", b"noreply"]) + b"\r\n", 3 + len(sp) + n)
            for run in (sp + SPACES[(i + 1) % 16], sp + SPACES[(i + 5) % 16] + SPACES[(i + 11) % 16]):
                add("B", b"get " + key(K, "get", n) + run + key(K, "get") + b"\r\n", 4 + n)
    # ---- C
    for junk in NEAR:
        for n in sweep:
            for req, f in _placements(K, junk, n):
                add("C", req, f)
    for n in sweep:
        line = b"get " + key(K, "get", n)
        for lead in LEADS:
            add("C", line + lead + b"\r\n", len(line))                  # the line's last byte(s)
        for sp in WIDE_SPACES:
            for j in range(1, len(sp)):
                add("C", line + sp[:j], len(line))                      # the request ends inside the rune
    # ---- D
    kg, kt = key(K, "get"), key(K, "touch")
    for req in (b"get " + kg + b"\xe2\x80\x80" + key(K, "get", len(kg) + 9) + b" " + K.deny + b"\r\n",
                b"set " + key(K, "storage") + b" 0 0 5 noreply\r\nhello\r\n",
                b"gat 9\xc2\xa0" + key(K, "gat", 21) + b"\r\n",
                b"touch " + kt + b" 10\r\n",
                gen.mc_bin(0, key(K, "get", 19)),
                gen.mc_bin(1, key(K, "storage", 13), bytes(8), b"value")):
        for n in range(len(req) + 1):
            add("D", req[:n])
    # ---- E
    for c in COMMANDS:
        k = key(K, _class(c))
        firsts = [c, c[:-1], c + b"s", c + bytes(16 - len(c)), c + bytes(17 - len(c)), c.upper(),
                  c + b"x" * (16 - len(c))]
        for t in firsts:
            for rest in (b"", b" " + k, b" 5 " + k + b" " + k, b" " + k + b" 0 0 3", b" " + k + b" 0 0 3 noreply"):
                add("E", t + rest + b"\r\n", len(t))
    # ---- F
    bs = len(K.allow["storage"])
    for v in ATOI:
        for n in range(bs, bs + 16):
            line = b"set " + key(K, "storage", n) + b" 0 0 "
            add("F", line + v + b"\r\n", len(line))
    for c in (b"set", b"cas"):
        for toks in ([c], [c, key(K, "storage")], [c, key(K, "storage"), b"0"], [c, key(K, "storage"), b"0", b"0"]):
            add("F", b" ".join(toks) + b"\r\n")
    # ---- G
    for cmd, cls in ((b"get", "get"), (b"gats 9", "gat")):
        for nk in KEY_COUNTS:
            for bad in (0, nk // 2, nk - 1, None):
                ks = [key(K, cls, len(K.allow[cls]) + j % 5) for j in range(nk)]
                if bad is not None:
                    ks[bad] = K.deny
                add("G", cmd + b" " + b" ".join(ks) + b"\r\n")
    # ---- H
    for op, cls in BIN_OPCODES.items():
        for ex in range(20):
            for kl in range(20):
                req = gen.mc_bin(op, key(K, cls, kl), bytes(ex))
                add("H", req)
                add("H", req[:-1])
    kb = key(K, "get", 11)
    for body in BODIES:
        add("H", gen.mc_bin(0, kb, body=body))
        add("H", gen.mc_bin(1, key(K, "storage", 9), bytes(8), b"v", body=body))
    for magic in MAGICS:
        add("H", gen.mc_bin(0, kb, magic=magic))
        add("H", gen.mc_bin(0, kb, magic=magic)[:-1])
    add("H", gen.mc_bin(0x99, kb))
    add("H", gen.mc_bin(10))   # noop: no key
    # ---- I
    add("I", b"")
    add("I", b"version\r\n")
    # a binary request that holds a line end (the text parser frames its header as a line of one long token),
    # text behind a binary magic, a text line long enough to be read as a binary header
    add("I", gen.mc_bin(0, b"a\r\n" + kb))
    add("I", gen.mc_bin(0, kb, value=b"\r\nget " + kg + b"\r\n"))
    add("I", b"\x80get " + kg + b"\r\n")
    add("I", b"get " + key(K, "get", 40) + b"\r\n")
    add("I", b"ge\x00\x00\x00 " + key(K, "get", 40) + b"\r\n")   # (as a header: key length 0, extras 0, no request magic)
    return out


def completions(req):
    """Bytes after `req` that would change its answer if they were read as its
    own: the rest of a White_Space rune it ends inside, the LF of a last CR."""
    out = []
    for sp in WIDE_SPACES:
        for j in range(1, len(sp)):
            if req.endswith(sp[:j]) and sp[j:] not in out:
                out.append(sp[j:])
    if req.endswith(b"\r"):
        out.append(b"\n")
    return out


def _trail(K, n):
    t = TRAILS[n % len(TRAILS)]
    return b" " + key(K, "get") + b"\r\n" if t is None else t


def full_layout(cases, K):
    """(case index, alignment, trailing bytes): every case at all 16 offsets
    with the trailing bytes rotating through TRAILS, and again at all 16 with
    each of its completions()."""
    lay = []
    for i, c in enumerate(cases):
        lay.extend((i, a, _trail(K, i + a)) for a in range(16))
        for t in completions(c.req):
            lay.extend((i, a, t) for a in range(16))
    return lay


def rotating_layout(cases, K, idx=None):
    """Case i once, at offset i mod 16 (idx: only these cases); the last
    request gets no trailing bytes, so it ends at the arena's last byte."""
    idx = list(range(len(cases))) if idx is None else list(idx)
    lay = [(i, i % 16, _trail(K, i // 16)) for i in idx]
    lay[-1] = (lay[-1][0], lay[-1][1], b"")
    return lay


def place(cases, K, layout):
    """The arena of a layout: each request at its offset mod 16, its trailing
    bytes after it, filler up to the next request's offset."""
    buf, offs, lens, cids, cidx, al = bytearray(), [], [], [], [], []
    fill = bytes([K.filler])
    for i, a, trail in layout:
        pad = (a - len(buf)) % 16
        if pad == 0 and offs and offs[-1] + lens[-1] == len(buf):
            pad = 16   # (no trailing bytes and no padding: the neighbour is filler, not a request)
        buf += fill * pad
        offs.append(len(buf))
        buf += cases[i].req
        buf += trail
        lens.append(len(cases[i].req))
        cids.append((i + a) % NCONNS)
        cidx.append(i)
        al.append(a)
    return Placed(np.frombuffer(bytes(buf), np.uint8).copy(), np.array(offs, np.uint64), np.array(lens, np.uint32),
                  np.array(cids, np.uint32), np.array(cidx, np.int64), np.array(al, np.int64))


def conns(src_in=3000, src_out=9000, port=gen.MC_PORT, other_port=11212):
    """NCONNS connections: flags c % 3 (the parser left to the first byte,
    forced text, forced binary); kind (0, 0, 1, 2)[c // 3]: a remote inside the
    policy's remote group, the same, a remote outside it, another port (the
    port-0 entry)."""
    c = gen.make_conns(NCONNS, 0, port, True, PROTO_MEMCACHE, src_in)
    for i in range(NCONNS):
        kind = (0, 0, 1, 2)[i // 3]
        c["flags"][i] = i % 3
        c["src_id"][i] = (src_out if kind == 1 else src_in) + i
        c["port"][i] = other_port if kind == 2 else port
    return c


# ------------------------------------------------------------------ policies
# Each selects one build of the classifier (tests/test_gpu_mc_edges.py states
# the engine.stats() condition that proves it); Keys are the corpus keys it allows.
def _mc_port(*groups, wild=None):
    ports = [(gen.MC_PORT, list(groups))] + ([(0, [wild])] if wild else [])
    return api.policy_set(api.network_policy("10.0.0.5", 5, ingress=ports))


def many_rules_policy():
    """150 rules (three 64-rule chunks) of exact, prefix and regex keys; the
    rules that allow the corpus keys sit in the second and third chunk."""
    rules = []
    for k in range(150):
        rules.append([{"command": "get", "keyExact": f"zz:{k}"}, {"command": "storage", "keyPrefix": f"zc:{k}:"},
                      {"command": "get", "keyRegex": f"^zs:[0-9a-f]{{{k % 9 + 1}}}(x|y)*{k}$"},
                      {"command": "delete", "keyRegex": f"^zd{k}(a|b)*a(a|b){{{k % 3 + 1}}}$"},
                      {"command": "gat", "keyPrefix": f"zu:{k}"}][k % 5])
    rules[3] = {"command": "stats"}
    rules[70] = {"command": "get", "keyPrefix": "user:"}
    rules[75] = {"command": "gat", "keyRegex": "^user:[0-9]+$"}
    rules[130] = {"command": "storage", "keyPrefix": "cache:"}
    rules[135] = {"command": "delete", "keyExact": "tmp"}
    rules[140] = {"command": "touch", "keyRegex": "é|ü"}
    return _mc_port(api.port_rule(l7proto="memcache", l7=rules))


NFA_KEYS = Keys({"get": b"a" * 15, "gat": b"b" + b"a" * 15, "storage": b"cache:1", "delete": b"x" + b"a" * 12 + b"z",
                 "touch": b"k\xc3\xa9y"}, b"obj7", ord("a"))


def nfa_policy(base_rules):
    """base_rules (test_gpu_memcache.mc_nfa_policy's: keyRegex patterns over
    the DFA budget) with rules for the other command classes of NFA_KEYS."""
    rules = list(base_rules) + [{"command": "gat", "keyRegex": "(a|b)*a(a|b){14}"},
                                {"command": "storage", "keyPrefix": "cache:"}, {"command": "touch", "keyPrefix": "ké"}]
    return _mc_port(api.port_rule(l7proto="memcache", l7=rules))


BIG_KEYS = Keys({"get": b"a" * 10 + b"c0", "gat": b"a" * 10 + b"c1", "storage": b"ba" * 5 + b"c2", "delete": b"tmp",
                 "touch": b"k\xc3\xa9y"}, b"obj7", ord("1"))


def big_images_policy():
    """Key DFAs of about 1k states each ((a|b)*a(a|b){9}<tag>), five for the
    remotes inside the group and two for everyone: more than kMcLdsImages of
    mask words, and a line walked once per DFA."""
    def re(tag):
        return "(a|b)*a(a|b){9}" + tag
    inside = [{"command": "get", "keyRegex": re("c0")}, {"command": "gat", "keyRegex": re("c1")},
              {"command": "storage", "keyRegex": re("c2")}, {"command": "delete", "keyExact": "tmp"},
              {"command": "touch", "keyPrefix": "ké"}, {"command": "incr", "keyRegex": re("c3")},
              {"command": "decr", "keyRegex": re("c4")}]
    anyone = [{"command": "get", "keyRegex": re("d0")}, {"command": "storage", "keyRegex": re("d1")},
              {"command": "version"}]
    return _mc_port(api.port_rule(remote_policies=list(range(3000, 3000 + NCONNS)), l7proto="memcache", l7=inside),
                    api.port_rule(l7proto="memcache", l7=anyone),
                    wild=api.port_rule(l7proto="memcache", l7=[{"command": "noop"}, {"command": "flush_all"}]))


def workload(P, conn_arr, policy, name="mc-edges"):
    return gen.Workload(name, P.arena, P.offsets, P.lengths, P.conn_ids, conn_arr, policy)


def family_indices(cases):
    fam = {}
    for i, c in enumerate(cases):
        fam.setdefault(c.family, []).append(i)
    return fam


def core_layout(cases, K):
    """The one-wave subset, chosen by rule: every A-C request at the four
    offsets that put its feature byte at chunk position 13, 14, 15 and 0, and
    every D and H request at offset i mod 16."""
    lay = []
    for i, c in enumerate(cases):
        if c.family in "ABC" and c.feat is not None:
            for p in (13, 14, 15, 0):
                a = (p - c.feat) % 16
                lay.append((i, a, _trail(K, i + a)))
        elif c.family in "DH":
            lay.append((i, i % 16, _trail(K, i // 16)))
    return lay

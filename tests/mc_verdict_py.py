"""The verdict of one memcached request buffer, restated in plain Python from
the reference's Go (test infrastructure: an independent second opinion on the
oracle, tests/test_mc_edges_host.py).

Built on tests/generic_log_py.py (go_fields, mc_text, mc_binary: the command
and the key spans, or None), it adds what those do not return: the MORE
counts, the error codes, the frame length with Go's integer wrap-around, the
rule match and the evaluation over a port's rule groups.

  memcached dispatch  proxylib/memcached/parser.go:186-202
  text parser         proxylib/memcached/text/parser.go:84-198
  binary parser       proxylib/memcached/binary/parser.go:72-139, :174-191
  Rule.Matches        proxylib/memcached/parser.go:47-110
  rule parsing        proxylib/memcached/parser.go:114-148
  groups and ports    proxylib/proxylib/policymap.go:91-236

Batch conventions: PASS / DROP are ALLOW / DENY with consumed =
the frame length; MORE n is INCOMPLETE with consumed n (NOP: 0); a Go panic or
ERROR 0 is PARSE_ERROR with consumed 0; ERROR_INVALID_FRAME_TYPE is PARSE_ERROR
with consumed 2; a frame length outside 1..2^32-1 is PARSE_ERROR.

Only rules of `command`, `keyExact` and `keyPrefix` are modelled: a rule set
with a keyRegex is the oracle's business (no regex engine here)."""
import generic_log_py as G

DENY, ALLOW, PARSE_ERROR, INCOMPLETE = 0, 1, 2, 3  # cilium_amd._lib's values (asserted by the host test)

# MemcacheOpCodeMap (parser.go:214-474): group -> (text commands, binary opcodes)
_STORE8 = "add set replace append prepend cas incr decr"
GROUPS = {
    "add": ("add", (2, 18)), "set": ("set", (1, 17)), "replace": ("replace", (3, 19)),
    "append": ("append", (14, 25)), "prepend": ("prepend", (15, 26)), "cas": ("cas", ()),
    "incr": ("incr", (5, 21)), "decr": ("decr", (6, 22)),
    "storage": (_STORE8, (1, 2, 3, 5, 6, 17, 18, 19, 21, 22, 25, 26)),
    "get": ("get gets", (0, 9, 12, 13)), "delete": ("delete", (4, 20)), "touch": ("touch", (28,)),
    "gat": ("gat gats", (29, 30)),
    "writeGroup": (_STORE8 + " delete touch", (1, 2, 3, 4, 5, 6, 17, 18, 19, 20, 21, 22, 25, 26, 28)),
    "slabs": ("slabs", ()), "lru": ("lru", ()), "lru_crawler": ("lru_crawler", ()), "watch": ("watch", ()),
    "stats": ("stats", (16,)), "flush_all": ("flush_all", (8, 24)), "cache_memlimit": ("cache_memlimit", ()),
    "version": ("version", (11,)), "misbehave": ("misbehave", ()), "quit": ("quit", (7, 23)),
    "noop": ("", (10,)), "verbosity": ("", (27,)),
}
_I64 = 1 << 64


class Rule:
    """One memcache.Rule (parser.go:114-148): a command that names no group
    leaves the rule `empty` when it has no key predicate either (:137-143)."""

    def __init__(self, d):
        assert set(d) <= {"command", "keyExact", "keyPrefix"}, d  # keyRegex: not modelled
        g = GROUPS.get(d.get("command"))
        self.exact = d.get("keyExact", "").encode()
        self.prefix = d.get("keyPrefix", "").encode()
        self.empty = g is None
        assert not (self.empty and (self.exact or self.prefix)), d  # ParseError in the Go
        self.text = set(g[0].encode().split()) if g else set()
        self.binary = set(g[1]) if g else set()

    def matches(self, cmd, opcode, keys):
        """Rule.Matches (parser.go:47-100); cmd None: a binary request
        (MemcacheMeta.IsBinary, meta.go:29-31: no text command)."""
        if self.empty:                                    # :57-59
            return True
        if cmd is None:                                   # :61-64
            if opcode not in self.binary:
                return False
        elif cmd not in self.text:                        # :65-69
            return False
        if self.exact:                                    # :71-78  every key, vacuously true with none
            return all(k == self.exact for k in keys)
        if self.prefix:                                   # :80-87
            return all(k.startswith(self.prefix) for k in keys)
        return True                                       # :98-99


class Port:
    """PortNetworkPolicyRules (policymap.go:113-148) of memcache groups."""

    def __init__(self, groups):
        self.groups = []
        for g in groups:
            assert g.get("l7_proto") == "memcache", g
            l7 = [Rule(x["rule"]) for x in g.get("l7_rules", {}).get("l7_rules", [])]
            self.groups.append((set(g.get("remote_policies", ())), l7))
        self.have_l7 = any(l7 for _, l7 in self.groups)   # :135-137

    def match(self, remote, cmd, opcode, keys):
        """PortNetworkPolicyRules.Matches (:150-171) over
        PortNetworkPolicyRule.Matches (:91-111): (matched, (group, rule) or None)."""
        if not self.have_l7 or not self.groups:           # :151-163
            return True, None
        for gi, (remotes, l7) in enumerate(self.groups):
            if remotes and remote not in remotes:         # :93-98
                continue
            if not l7:                                    # :108-110
                return True, None
            for ri, r in enumerate(l7):                   # :99-106
                if r.matches(cmd, opcode, keys):
                    return True, (gi, ri)
        return False, None


class Policy:
    """The ingress ports of the first network policy of an api.policy_set."""

    def __init__(self, policy_set):
        np_ = policy_set["policies"][0]
        self.ports = {p["port"]: Port(p["rules"]) for p in np_["ingress_per_port_policies"]}

    def match(self, port, remote, cmd, opcode, keys):
        """PortNetworkPolicies.Matches (policymap.go:208-236): the exact port,
        then port 0; the rule position is (0 exact / 1 wildcard, group, rule)."""
        for k, p in enumerate((self.ports.get(port), self.ports.get(0))):
            if p is None or (k == 1 and port == 0):
                continue
            ok, pos = p.match(remote, cmd, opcode, keys)
            if ok:
                return True, None if pos is None else (k,) + pos
        return False, None


def _go_int(x):
    """A Go int (64-bit two's complement) holding x."""
    x &= _I64 - 1
    return x - _I64 if x >> 63 else x


def frame(data, flags=0):
    """The parser's answer before policy: ("more", n), ("error", n), or
    ("frame", length, cmd, opcode, keys) with the length as the Go computes it."""
    mode = flags & 3
    if mode == 0:                                         # parser.go:187-200
        if not data:
            return ("more", 0)                            # NOP, 0
        mode = 2 if data[0] >= 128 else 1
    if mode == 2:
        if len(data) < 24:                                # binary/parser.go:72-76
            return ("more", 24 - len(data))
        key_len, extras = int.from_bytes(data[2:4], "big"), data[4]
        if key_len > 0 and 24 + key_len + extras > len(data):  # :83-90
            return ("more", 24 + key_len + extras - len(data))
        if data[0] & 0x80 != 0x80:                        # :175-178  ERROR_INVALID_FRAME_TYPE = 2
            return ("error", 2)
        m = G.mc_binary(data)
        ks, kl = m["key"]
        body = int.from_bytes(data[8:12], "big")
        return ("frame", (body + 24) & 0xFFFFFFFF, None, m["opcode"], [data[ks:ks + kl]])  # :112 uint32 sum, then int()
    lf = data.find(b"\r\n")                               # text/parser.go:87-94
    if lf < 0:
        return ("more", 1 if data[-1:] == b"\r" else 2)
    m = G.mc_text(data)
    if m is None:                                         # a panic, or ERROR 0 (:119-123, :159-161)
        return ("error", 0)
    length = lf + 2                                       # :106
    cmd = m["fields"]["command"]
    if cmd in (b"set", b"add", b"replace", b"append", b"prepend", b"cas"):
        s, e = G.go_fields(data[:lf])[4]
        length = _go_int(length + _go_int(int(data[s:e]) + 2))  # :119-125  int arithmetic wraps
    return ("frame", length, cmd, 0, [data[s:s + n] for s, n in m["keys"]])


def verdict(policy, conn, data):
    """(verdict, rule position or None, consumed) of `data` on connection
    conn = (port, remote, flags)."""
    port, remote, flags = conn
    f = frame(data, flags)
    if f[0] == "more":
        return INCOMPLETE, None, f[1]
    if f[0] == "error":
        return PARSE_ERROR, None, f[1]
    _, length, cmd, opcode, keys = f
    if not 1 <= length <= 0xFFFFFFFF:
        return PARSE_ERROR, None, 0
    ok, pos = policy.match(port, remote, cmd, opcode, keys)
    return (ALLOW if ok else DENY), pos, length

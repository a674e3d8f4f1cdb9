"""The HTTP framer's DFA walks (one branch-free step: the null DFA for slots
without one, state 0 a looping row, unguarded look-ahead reads) against the
oracle, bit-exact on verdict, rule id and consumed bytes, at the smallest
shapes where they can go wrong: tokens ending around the 256-byte window
boundary at several alignments, walks that die or turn absorbing on their
first, middle and last byte, slots without a DFA, a rule set framed in two
passes, duplicate / padded / empty constrained values, 0..10 constrained
tokens in one head, and 64-request tiles that mix well-formed heads with
heads the framer handles byte by byte.  The same streams also run with their
rule set cold (image read from global memory) and through the grouped kernel.

Every batch is larger than 64 requests: smaller calls take the latency kernel."""
import numpy as np
import pytest

from cilium_amd import api, gen
from cilium_amd._lib import ALLOW, DENY, INCOMPLETE, PARSE_ERROR, PROTO_HTTP
from http_image import H_MAX_SLOT_DFAS, H_NDFA, LDS_IMAGE_BYTES, http_images

pytestmark = pytest.mark.gpu

# ports = rule sets of the one policy
P_FULL, P_PATH, P_NONE, P_TWO = 80, 81, 82, 83
TOK = b"12345678"
CUSTOM = [b"X-C%d" % i for i in range(1, 7)]


def _rx(name, rx):
    return {"name": name, "regex_match": rx}


def _policy():
    full = api.http_rules_from_api([
        api.PortRuleHTTP(method="GET", path="/a/.*", host="h[0-9]+\\.x"),
        api.PortRuleHTTP(path="/exact", host="abc"),
        api.PortRuleHTTP(method="PUT", path="/pq.*"),
        api.PortRuleHTTP(method="[A-Z]+", path="/m"),
    ]) + [
        {"headers": api.sort_header_matchers([_rx(":path", "/t/.*"), _rx("X-Tok", "[0-9]+")])},
        {"headers": api.sort_header_matchers([_rx(":path", "/nine"), _rx(":method", "GET"), _rx(":authority", "abc")] +
                                             [_rx(c.decode(), "v[0-9]+") for c in CUSTOM])},
    ]
    path_only = api.http_rules_from_api([api.PortRuleHTTP(path="/p/.*")])
    none = [{}]  # one rule without matchers: no DFA on any slot
    # [a-z]*a[a-z]{7} and [a-z]*b[a-z]{7} have 256 states each and 3^8 together:
    # over the compiler's state budget, so the host slot gets two DFAs, two
    # framing passes (and both still fit the LDS image)
    two = api.http_rules_from_api([api.PortRuleHTTP(path="/w/.*", host="[a-z]*a[a-z]{7}"),
                                   api.PortRuleHTTP(path="/w/.*", host="[a-z]*b[a-z]{7}")])
    return api.policy_set(api.network_policy("ep", 1, ingress=[
        (P_FULL, [api.port_rule(http=api.sort_http_rules(full))]), (P_PATH, [api.port_rule(http=path_only)]),
        (P_NONE, [api.port_rule(http=none)]), (P_TWO, [api.port_rule(http=two)])]))


PORTS = [P_FULL, P_PATH, P_NONE, P_TWO]


def _conns(hot):
    """One connection per port (conn id = index in PORTS), then extra ones on
    `hot` so that its rule set serves the most connections (staged in LDS)."""
    ports = PORTS + [hot] * 3
    return gen.make_conns(len(ports), 0, np.array(ports), True, PROTO_HTTP, 1 + np.arange(len(ports)))


def _place(reqs, aligns):
    """Arena with request i starting at an offset = aligns[i] mod 16."""
    parts, offs, p = [], [], 0
    for r, a in zip(reqs, aligns):
        gap = (a - p) % 16
        parts.append(b"#" * gap)
        p += gap
        offs.append(p)
        parts.append(r)
        p += len(r)
    arena = np.frombuffer(b"".join(parts) + b"#" * 16, np.uint8).copy()
    return arena, np.array(offs, np.uint64), np.array([len(r) for r in reqs], np.uint32)


def _head(method=b"GET", path=b"/a/x", lines=(), end=b"\r\n"):
    return method + b" " + path + b" HTTP/1.1\r\n" + b"".join(lines) + end


def _cases():
    """[(request, port, alignment)]"""
    out = []
    add = lambda r, port=P_FULL, a=0: out.append((r, port, a))  # noqa: E731
    # ---- window boundaries: the token's end at window byte 252..260 (the window
    # starts at the request's start rounded down to 16, so request position =
    # window byte - alignment), on the rule set with DFAs and on the one without
    for a0 in (0, 5, 15):
        for e in range(252, 261):
            k = e - a0
            for port in (P_FULL, P_NONE):
                add(_head(b"M" * k, b"/m", [b"Host: abc\r\n"]), port, a0)                         # method
                add(_head(b"GET", b"/a/" + b"x" * (k - 4 - 3), [b"Host: h1.x\r\n"]), port, a0)   # target
                pre = b"GET /a/x HTTP/1.1\r\nHost: h"
                add(pre + b"7" * (k - len(pre) - 2) + b".x\r\nX-Tok: 1\r\n\r\n", port, a0)        # constrained value
                pre = b"GET /t/x HTTP/1.1\r\nX-Pad: " + b"p" * 150 + b"\r\nX-Tok: "
                add(pre + b"7" * (k - len(pre)) + b"\r\n\r\n", port, a0)                          # custom header
    for a0 in (0, 9):
        pre = b"GET /a/x HTTP/1.1\r\nHost: h"
        add(pre + b"7" * 300 + b".x\r\n\r\n", P_FULL, a0)            # value straddling the window boundary
        add(pre + b"7" * 300 + b".y\r\n\r\n", P_FULL, a0)
        add(b"GET /t/" + b"y" * 600 + b" HTTP/1.1\r\nX-Tok: 5\r\n\r\n", P_FULL, a0)  # absorbing target over windows
        for total in (255, 256, 257, 256 - a0, 272 - a0):                 # heads of exactly one window
            pre = b"GET /t/x HTTP/1.1\r\nX-Tok: "
            add(pre + b"7" * (total - len(pre) - 4) + b"\r\n\r\n", P_FULL, a0)
            pre = b"GET /a/x HTTP/1.1\r\nHost: h1.x\r\nX-Pad: "
            add(pre + b"p" * (total - len(pre) - 4) + b"\r\n\r\n", P_FULL, a0)
    # ---- states: dead / absorbing on the first, middle and last byte of a walk
    for path in (b"x/a/", b"/a", b"/a/", b"/a/z", b"/a/" + b"z" * 50, b"/exact", b"/exacX", b"/exaXt", b"Xexact",
                 b"/exactly", b"/pq", b"/pqr", b"/p", b"/", b"/m", b"/mm", b"/nine", b"/t/", b"/t"):
        for host in (b"abc", b"xbc", b"aXc", b"abX", b"abcd", b"a", b"h1.x", b"h.x", b"h12.", b"h12.xx", b"X", b""):
            for method in (b"GET", b"PUT", b"G", b"get", b"GETT"):
                add(_head(method, path, [b"Host: " + host + b"\r\n", b"X-Tok: " + TOK + b"\r\n"]))
    for path in (b"/p/", b"/p/x", b"/p", b"/q/x", b"x", b"/p/" + b"z" * 250):  # slots without a DFA
        for port in (P_PATH, P_NONE):
            add(_head(b"POST", path, [b"Host: abc\r\n", b"X-Tok: 1\r\n", b"X-C1: v1\r\n"]), port)
    for host in (b"acdefghi", b"bcdefghi", b"acdefgh", b"xacdefghi", b"abcdefgh", b"bacdefghib", b"c" * 40,
                 b"a" * 8, b"b" * 9, b"", b"acdefghi ", b" \tbcdefghi\t ", b"acdef1hi", b"zzzzbzzzzzzz"):  # two framing passes
        for path in (b"/w/", b"/w/x", b"/v/"):
            add(_head(b"GET", path, [b"X-Pad: zz\r\n", b"Host: " + host + b"\r\n"]), P_TWO)
            add(_head(b"GET", path, [b"Host: " + host + b"\r\n", b"Host: acdefghi\r\n"]), P_TWO)
    # ---- lines and spacing
    for v in (b"abc", b" abc", b"\tabc", b"   abc", b"abc ", b"abc\t", b"abc \t ", b" abc ", b"ab c", b"abc x", b"",
              b" ", b" \t ", b"abc" + b" " * 20, b" " * 20 + b"abc", b"abc\x01", b"a\x7fc"):
        add(_head(b"GET", b"/exact", [b"Host:" + v + b"\r\n"]))
        add(_head(b"GET", b"/exact", [b"Host:" + v + b"\r\n", b"Host: abc\r\n"]))      # first occurrence wins
        add(_head(b"GET", b"/exact", [b"Host: zzz\r\n", b"Host:" + v + b"\r\n"]))
        add(_head(b"GET", b"/t/x", [b"X-Tok:" + v.replace(b"abc", b"123") + b"\r\n", b"X-Tok: 9\r\n"]))
    # ---- line counts: 0, 1, 4, 5, 9, 10 constrained tokens in one head
    nine = [b"Host: abc\r\n"] + [c + b": v%d\r\n" % i for i, c in enumerate(CUSTOM)]
    for lines in (nine, nine[:-1], nine[:2], nine[:1], nine[::-1], [nine[0]] + [b"X-Pad: q\r\n"] + nine[1:],
                  nine[:3] + [b"X-C3: w\r\n"] + nine[4:], nine + nine):
        for port in (P_FULL, P_PATH, P_NONE):
            add(_head(b"GET", b"/nine", lines), port)
            add(_head(b"GET", b"/nine", lines + [b"X-Tok: " + TOK + b"\r\n"]), port)
    return out


def _mixed_tile(i):
    """64 requests: well-formed heads beside heads the framer takes byte by
    byte or refuses."""
    good = [_head(b"GET", b"/a/%d" % k, [b"Host: h%d.x\r\n" % k, b"X-Tok: " + TOK + b"\r\n"]) for k in range(24)]
    body = [
        _head(b"POST", b"/exact", [b"Host: abc\r\n", b"Content-Length: 3\r\n"]) + b"abc",
        _head(b"POST", b"/exact", [b"Content-Length: 5\r\n", b"Host: abc\r\n"]) + b"abc",
        _head(b"POST", b"/exact", [b"Host: abc\r\n", b"Content-Length: 1\r\n", b"Content-Length: 1\r\n"]) + b"a",
        _head(b"POST", b"/t/x", [b"X-Tok: 1\r\n", b"Transfer-Encoding: chunked\r\n"]) + b"3\r\nabc\r\n0\r\n\r\n",
        _head(b"POST", b"/t/x", [b"Transfer-Encoding: chunked\r\n", b"X-Tok: 1\r\n"]) + b"3\r\nab",
        _head(b"GET", b"/exact", [b"Host: abc\r\n", b" folded: x\r\n"]),             # obs-fold
        _head(b"GET", b"/exact", [b"Host: ab\r\n", b"\tc\r\n"]),
        _head(b"GET", b"/exact", [b"Host: a\x01bc\r\n"]),                              # CTL inside a value
        _head(b"GET", b"/t/x", [b"X-Pad: a\x00b\r\n", b"X-Tok: 1\r\n"]),
        _head(b"GET", b"/exact", [b"Host: abc\n"]),                                    # bare LF
        b"GET /exact HTTP/1.1\nHost: abc\r\n\r\n",
        _head(b"GET", b"/exact", [b"Host: abc\r\n"])[:-1],                             # truncated
        b"GET /exact HTTP/1.1\r\nHost: ab",
        b"GET /a/xyz",
        b"GE",
        _head(b"GET", b"/a/x", [b"X-Pad: " + b"p" * 3500 + b"\r\n", b"Host: h1.x\r\n"]),   # longer than the 3 KiB map
        _head(b"GET", b"/a/x", [b"Host: h" + b"1" * 3300 + b".x\r\n"]),
        _head(b"GET", b"/a/" + b"x" * 700, [b"Host: h1.x\r\n"]),
    ]
    reqs = good + body + good[:64 - len(good) - len(body)]
    assert len(reqs) == 64
    rng = np.random.default_rng(100 + i)
    return [reqs[j] for j in rng.permutation(64)]


@pytest.fixture(scope="module")
def streams():
    """The case list as arrays, and the oracle's answers (computed once)."""
    import refpy
    refpy.build()
    cases = _cases()
    reqs = [c[0] for c in cases]
    ports = [c[1] for c in cases]
    aligns = [c[2] for c in cases]
    for i in range(3):  # whole tiles of the mix, each at a tile boundary
        pad = (-len(reqs)) % 64
        reqs += [_head()] * pad
        ports += [P_FULL] * pad
        aligns += [0] * pad
        t = _mixed_tile(i)
        reqs += t
        ports += [P_FULL] * 64
        aligns += [int(a) for a in np.random.default_rng(i).integers(0, 16, 64)]
    arena, offs, lens = _place(reqs, aligns)
    cid = np.array([PORTS.index(p) for p in ports], np.uint32)
    pol = _policy()
    w = gen.Workload("dfa-steps", arena, offs, lens, cid, _conns(P_FULL), pol)
    ref = refpy.classify_workload(w, 8)
    hist = np.bincount(ref[0], minlength=5)
    assert hist[ALLOW] > 100 and hist[DENY] > 100 and hist[PARSE_ERROR] > 10 and hist[INCOMPLETE] > 5, hist
    return w, ref


def _assert_same(got, ref, w):
    for name, a, b in zip(("verdict", "rule", "consumed"), got, ref):
        bad = np.nonzero(a != b)[0]
        if len(bad):
            i = int(bad[0])
            o, n = int(w.offsets[i]), int(w.lengths[i])
            raise AssertionError(f"{name} differs at {len(bad)} of {len(a)} requests; first {i} (conn {w.conn_ids[i]}, "
                                 f"offset {o} mod 16 = {o % 16}, len {n}): got ({got[0][i]},{got[1][i]},{got[2][i]}) "
                                 f"ref ({ref[0][i]},{ref[1][i]},{ref[2][i]}) {bytes(w.arena[o:o + min(n, 320)])!r}")


def _run(engine, w, conns):
    engine.update_policy(w.policy)
    engine.set_connections(conns)
    return engine.classify(w.arena, w.offsets, w.lengths, w.conn_ids)


def test_rule_sets_are_what_the_cases_need(engine, streams):
    """The full rule set fits LDS; the no-matcher one has no DFA; the host slot
    of the two-pass one has two DFAs (ImgHeader::max_slot_dfas)."""
    w, _ = streams
    engine.update_policy(w.policy)
    engine.set_connections(_conns(P_FULL))
    imgs = http_images(engine.export_tables())
    ndfa = sorted(img[H_NDFA] for img in imgs)
    passes = sorted(img[H_MAX_SLOT_DFAS] for img in imgs)
    assert len(imgs) == 4 and ndfa[0] == 0 and ndfa[1] == 1 and passes[-1] == 2 and passes[-2] == 1
    assert all(len(img) <= LDS_IMAGE_BYTES for img in imgs)


@pytest.mark.parametrize("hot", PORTS)
def test_streams_hot_and_cold(engine, streams, hot):
    """Each rule set in turn staged in LDS (hot); the others' requests take the
    global-image instantiation of the same framer."""
    w, ref = streams
    _assert_same(_run(engine, w, _conns(hot)), ref, w)


def test_streams_grouped(engine, streams):
    """The same requests through http_grouped_kernel: several rule sets in use
    and the smallest batch that takes that path (65536 requests)."""
    w, ref = streams
    reps = -(-65536 // w.n)
    offs, lens, cid = np.tile(w.offsets, reps), np.tile(w.lengths, reps), np.tile(w.conn_ids, reps)
    engine.update_policy(w.policy)
    engine.set_connections(_conns(P_FULL))
    # what sends a batch to the grouped kernel (classify.cc): at least kGroupMin
    # = 65536 requests, several HTTP rule sets, some request off the hot one
    assert len(offs) >= 65536 and engine.stats()["http_rulesets"] >= 2 and len(set(cid.tolist())) >= 2
    got = engine.classify(w.arena, offs, lens, cid)
    big = gen.Workload("dfa-steps-grouped", w.arena, offs, lens, cid, w.conns, w.policy)
    _assert_same(got, tuple(np.tile(r, reps) for r in ref), big)

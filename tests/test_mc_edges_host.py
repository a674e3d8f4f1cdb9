"""The directed memcached corpus (tests/mc_edge_cases.py) on the CPU: the oracle
against an independent Python model of the Go (tests/mc_verdict_py.py) on every
placed request, and checks -- computed from the arena's bytes, never from a
kernel -- that the layout still puts every edge at every chunk position, so a
later edit cannot thin the sweep unnoticed.  No GPU."""
import numpy as np
import pytest

import generic_log_py as G
import mc_edge_cases as E
import mc_verdict_py as M
from cilium_amd import api, gen
from cilium_amd._lib import ALLOW, DENY, INCOMPLETE, PARSE_ERROR

K = E.MC_POLICY_KEYS
STORAGE = (b"set", b"add", b"replace", b"append", b"prepend", b"cas")


def model_policy():
    """Exact and prefix rules only: a group for the remotes of E.conns()'s
    kinds 0 and 2, a catch-all group, a port-0 entry."""
    inside = [{"command": "get", "keyPrefix": "user:"}, {"command": "gat", "keyPrefix": "user:"},
              {"command": "storage", "keyPrefix": "cache:"}, {"command": "delete", "keyExact": "tmp"},
              {"command": "touch", "keyPrefix": "ké"}, {"command": "stats"},
              {"command": "writeGroup", "keyExact": "counter"}]
    anyone = [{"command": "version"}, {"command": "get", "keyExact": "user:1"}]
    wild = [{"command": "flush_all"}, {"command": "noop"}, {"command": "delete", "keyPrefix": "t"}]
    P = api.port_rule
    return api.policy_set(api.network_policy("10.0.0.5", 5, ingress=[
        (gen.MC_PORT, [P(remote_policies=list(range(3000, 3000 + E.NCONNS)), l7proto="memcache", l7=inside),
                       P(l7proto="memcache", l7=anyone)]),
        (0, [P(remote_policies=list(range(3000, 3000 + E.NCONNS)), l7proto="memcache", l7=wild)])]))


class _Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(oracle):
    c = _Ctx()
    c.cases = E.corpus(K)
    c.P = E.place(c.cases, K, E.full_layout(c.cases, K))
    c.conns = E.conns()
    c.policy = model_policy()
    c.w = E.workload(c.P, c.conns, c.policy)
    c.ref = oracle.classify_workload(c.w, 8)
    order = np.argsort(c.P.case, kind="stable")
    cuts = np.searchsorted(c.P.case[order], np.arange(len(c.cases) + 1))
    c.of_case = [order[cuts[i]:cuts[i + 1]] for i in range(len(c.cases))]   # placements of each case
    return c


def test_verdict_constants():
    assert (M.ALLOW, M.DENY, M.INCOMPLETE, M.PARSE_ERROR) == (ALLOW, DENY, INCOMPLETE, PARSE_ERROR)


def test_corpus_shape(ctx):
    fam = E.family_indices(ctx.cases)
    assert sorted(fam) == list("ABCDEFGHI")
    assert len(ctx.cases) >= 8000 and len(ctx.P.offsets) >= 16 * len(ctx.cases)
    P = ctx.P
    for i, idx in enumerate(ctx.of_case):   # every request at every offset mod 16, its bytes in place
        assert set((P.offsets[idx] % 16).tolist()) == set(range(16)), i
    for j in range(0, len(P.offsets), 37):
        o, n = int(P.offsets[j]), int(P.lengths[j])
        assert bytes(P.arena[o:o + n]) == ctx.cases[P.case[j]].req
    # the rotating layout of each family ends at the arena's last byte
    for f, idx in fam.items():
        R = E.place(ctx.cases, K, E.rotating_layout(ctx.cases, K, idx))
        assert int(R.offsets[-1]) + int(R.lengths[-1]) == len(R.arena), f
        assert (R.offsets % 16 == R.case % 16).all()
    # every request is classified on connections of all three flags
    flags = ctx.conns["flags"][P.conn_ids]
    for f in (0, 1, 2):
        assert len(np.unique(P.case[flags == f])) == len(ctx.cases)


def test_model_equals_oracle(ctx):
    P, cases = ctx.P, ctx.cases
    pol = M.Policy(ctx.policy)
    v, r, c = ctx.ref
    frames, to_id, to_pos, bad = {}, {}, {}, []
    for j in range(len(P.offsets)):
        cn = ctx.conns[P.conn_ids[j]]
        fk = (int(P.case[j]), int(cn["flags"]))
        f = frames.get(fk)
        if f is None:
            f = frames[fk] = M.frame(cases[fk[0]].req, fk[1])
        if f[0] == "more":
            want = (INCOMPLETE, None, f[1])
        elif f[0] == "error" or not 1 <= f[1] <= 0xFFFFFFFF:
            want = (PARSE_ERROR, None, f[1] if f[0] == "error" else 0)
        else:
            ok, pos = pol.match(int(cn["port"]), int(cn["src_id"]), f[2], f[3], f[4])
            want = (ALLOW if ok else DENY, pos, f[1])
        if (int(v[j]), int(c[j])) != (want[0], want[2]) or (want[1] is None) != (r[j] < 0):
            bad.append((j, want, (int(v[j]), int(r[j]), int(c[j])), cases[fk[0]].req[:80], fk[1]))
        elif want[1] is not None:   # rule ids: a one-to-one image of the model's positions
            assert to_id.setdefault(want[1], int(r[j])) == int(r[j]), (j, want, int(r[j]))
            assert to_pos.setdefault(int(r[j]), want[1]) == want[1], (j, want, int(r[j]))
    assert not bad, (len(bad), bad[:5])
    assert len(to_id) >= 6


def test_oracle_verdict_coverage(ctx):
    v, r, _ = ctx.ref
    flags = ctx.conns["flags"][ctx.P.conn_ids]
    for f in (0, 1, 2):
        assert set(v[flags == f].tolist()) == {ALLOW, DENY, INCOMPLETE, PARSE_ERROR}, f
    assert len(set(r[v == ALLOW].tolist())) >= 6
    fam = np.array([c.family for c in ctx.cases])[ctx.P.case]
    for f in "ABCDEFGH":
        assert {ALLOW, DENY} <= set(v[fam == f].tolist()), f


def test_policies_select_their_builds():
    """The table conditions tests/test_gpu_mc_edges.py relies on, from the
    compiler alone (a host-only engine)."""
    import cilium_amd
    from test_gpu_memcache import mc_nfa_policy
    host = cilium_amd.Engine(-1)
    base = mc_nfa_policy()["policies"][0]["ingress_per_port_policies"][0]["rules"][0]["l7_rules"]["l7_rules"]
    want = {"cfg5": lambda st: st["mc_rules"] <= 64 and st["mc_nfas"] == 0 and st["mc_dfas"] == 1,
            "many_rules": lambda st: st["mc_rules"] > 64 and st["mc_nfas"] == 0,
            "nfa": lambda st: st["mc_nfas"] >= 2,
            "big_images": lambda st: st["mc_dfa_states"] * 8 > 32768 and st["mc_dfas"] >= 3 and st["mc_nfas"] == 0}
    pols = {"cfg5": gen.mc_policy(), "many_rules": E.many_rules_policy(),
            "nfa": E.nfa_policy([x["rule"] for x in base]), "big_images": E.big_images_policy()}
    for name, pol in pols.items():
        host.update_policy(pol)
        host.set_connections(E.conns())
        st = host.stats()
        assert want[name](st), (name, st)
        if name == "big_images":
            assert (st["mc_dfas"], st["mc_dfa_states"]) == (10, 9252)   # (the figure the GPU module's docstring quotes)


def _text_line(req):
    """End of the command line of a request the text parser would take by its
    first byte, else -1."""
    return req.find(b"\r\n") if req and req[0] < 0x80 else -1


def test_line_end_at_every_chunk_position(ctx):
    P = ctx.P
    lf = np.array([_text_line(c.req) for c in ctx.cases])[P.case]
    sel = lf >= 0
    at = (P.offsets[sel] + lf[sel].astype(np.uint64)).astype(np.int64)
    assert (P.arena[at] == 13).all() and (P.arena[at + 1] == 10).all()
    seen = set(zip((P.offsets[sel] % 16).tolist(), (at % 16).tolist()))
    assert seen == {(a, p) for a in range(16) for p in range(16)}
    # a request whose last byte is a CR, the neighbour's LF behind it: the CR at every chunk position
    last_cr = np.array([lf < 0 and c.req[-1:] == b"\r" and c.req[0] < 0x80
                        for lf, c in zip((_text_line(c.req) for c in ctx.cases), ctx.cases)])[P.case]
    end = (P.offsets + P.lengths).astype(np.int64)
    lent = last_cr & (end < len(P.arena)) & (P.arena[np.minimum(end, len(P.arena) - 1)] == 10)
    assert set(((end[lent] - 1) % 16).tolist()) == set(range(16))


def test_wide_runes_at_chunk_edges(ctx):
    P = ctx.P
    for sp in E.WIDE_SPACES:
        inside, cut, lent = set(), set(), set()
        for i, c in enumerate(ctx.cases):
            req, lf = c.req, _text_line(c.req)
            offs = P.offsets[ctx.of_case[i]].astype(np.int64)
            j = req.find(sp, 0, lf) if lf >= 0 else -1
            while j >= 0:   # complete inside the line
                inside |= set(((offs + j) % 16).tolist())
                j = req.find(sp, j + 1, lf)
            for k in range(1, len(sp)):
                if lf < 0 and req.endswith(sp[:k]) and req[0] < 0x80:
                    j = len(req) - k
                    cut |= set(((offs + j) % 16).tolist())
                    for o in offs.tolist():   # the neighbour's bytes complete it
                        if bytes(P.arena[o + len(req):o + len(req) + len(sp) - k]) == sp[k:]:
                            lent.add((o + j) % 16)
        for got in (inside, cut, lent):
            assert {13, 14, 15} <= got, (sp, inside, cut, lent)


def test_tokens_end_at_chunk_end(ctx):
    P = ctx.P
    seen = set()
    for i, c in enumerate(ctx.cases):
        lf = _text_line(c.req)
        if lf < 0:
            continue
        toks = G.go_fields(c.req[:lf])
        if not toks:
            continue
        m = G.mc_text(c.req)
        ends = [("command", toks[0][1])]
        if m is not None:
            ends += [("key", s + n) for s, n in m["keys"][:2]]
            if m["fields"]["command"] in STORAGE:
                ends.append(("tokens[4]", toks[4][1]))
        a15 = (P.offsets[ctx.of_case[i]].astype(np.int64) % 16).tolist()
        for kind, e in ends:
            if any((a + e - 1) % 16 == 15 for a in a15):
                seen.add((kind, "line end" if e == lf else "separator"))
    assert seen >= {("command", "separator"), ("key", "separator"), ("tokens[4]", "separator"), ("key", "line end"),
                    ("tokens[4]", "line end")}


def test_binary_keys_at_every_chunk_position(ctx):
    P = ctx.P
    full_s, full_e, short_s, short_e = set(), set(), set(), set()
    for i, c in enumerate(ctx.cases):
        req = c.req
        if c.family != "H" or len(req) < 24 or req[0] != 0x80:
            continue
        ks = 24 + req[4]
        ke = ks + int.from_bytes(req[2:4], "big")
        if ke == ks:
            continue
        res = (P.offsets[ctx.of_case[i]].astype(np.int64) % 16).tolist()
        if len(req) == ke:
            full_s |= {(a + ks) % 16 for a in res}
            full_e |= {(a + ke) % 16 for a in res}
        elif len(req) == ke - 1:
            short_s |= {(a + ks) % 16 for a in res}
            short_e |= {(a + ke) % 16 for a in res}
    for got in (full_s, full_e, short_s, short_e):
        assert got == set(range(16))
    # independent of the alignment sweep: the key's offset inside the request alone covers every residue
    starts = {(24 + c.req[4]) % 16 for c in ctx.cases if c.family == "H" and len(c.req) >= 24}
    assert starts == set(range(16))


def test_core_subset_is_chosen_by_rule(ctx):
    lay = E.core_layout(ctx.cases, K)
    assert len(lay) >= 1024
    fams = {ctx.cases[i].family for i, _, _ in lay}
    assert fams == set("ABCDH")
    for i, a, _ in lay:
        c = ctx.cases[i]
        if c.family in "ABC":
            assert (a + c.feat) % 16 in (13, 14, 15, 0)

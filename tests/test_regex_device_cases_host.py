"""The generated-regex device cases (tests/regex_device_cases.py) on the CPU:
what the streams must be for the GPU parity tests to mean something, and the
compiled tables themselves.

  1. the builder is deterministic, and each stream meets its conditions with
     the oracle alone (shares of ALLOW and DENY, rule sets with both verdicts,
     rules that allow, little framing noise, every atom class hit and missed);
  2. the case policies compile on a host-only engine: nothing refused, the NFA
     counts the wrapped patterns imply, HTTP images on both sides of the LDS
     limit, a slot with two DFAs, three 64-rule chunks in the wide sets;
  3. the serialized tables, walked in Python: every constrained value of every
     request through its slot's DFAs; a rule's bit in the end state's mask row
     is the oracle regex's answer (XOR invert_match for HTTP, where a rule
     another DFA or an NFA evaluates keeps its bit), and the states numbered
     absorb and above are exactly the ones that loop on every token byte.

With 3 the product DFA, the group split at the state budget, SortAbsorbing and
the serialization are pinned here, so a mismatch in tests/test_gpu_regex_parity.py
points at a device walker or a call site, not at the tables."""
import json

import pytest

import cilium_amd
import regex_device_cases as C
from cilium_amd._lib import ALLOW
from http_image import (H_MAX_SLOT_DFAS, H_NNFA, LDS_IMAGE_BYTES, export_images, generic_image_tables, http_image_tables)

PROTOCOLS = {"http": ["http", "http_nfa"], "memcached": ["memcached", "memcached_nfa"], "r2d2": ["r2d2", "r2d2_nfa"],
             "cassandra": ["cassandra", "cassandra_nfa"]}
IMAGE_KEY = {"memcached": "memcache", "r2d2": "r2d2", "cassandra": "cassandra"}


@pytest.fixture(scope="module", autouse=True)
def _oracle_built(oracle):
    return oracle


def _fingerprint(names):
    return [(C.stream(n).reqs, json.dumps(C.stream(n).workload.policy, sort_keys=True)) for n in names]


def test_same_seed_same_bytes():
    names = ["http_nfa", "memcached", "r2d2_nfa", "cassandra_nfa"]
    first = _fingerprint(names)
    C.reset()
    assert _fingerprint(names) == first
    assert all(len(r) < 300 for n in names for r in C.stream(n).reqs)


# ------------------------------------------------------------------ 1. conditions
@pytest.mark.parametrize("name", list(C.STREAMS))
def test_stream_conditions(name):
    """Conditions, not measurements: if the inputs miss them, the inputs change."""
    s = C.stream(name)
    c = C.conditions(s)
    print(name, c)
    assert c["allow"] >= 0.20 and c["deny"] >= 0.20, c
    assert c["sets_both"] >= 0.80 * c["sets"], c
    assert c["rules_allowing"] >= 0.70 * c["rules"], c
    assert c["other"] <= 0.05, c
    if "_nfa" not in name and name != "http_all":
        assert 4000 <= c["n"] <= 6000 and c["sets"] >= 48, c
    long = [r for r in s.reqs if len(r) >= 300]
    assert len(long) <= (60 if s.proto == C.PROTO_HTTP else 0)   # (HTTP: the values crossing the 256-byte window)


def _outcomes(s):
    """{Pat: {answers of the oracle's regex over the values the stream shows it}}."""
    out = {}
    for seen, si in zip(s.values, s.req_set):
        for slot, v in seen:
            if v is None:
                continue
            for r in s.sets[si].rules:
                for m in r.matchers:
                    if m.slot == slot:
                        out.setdefault(m.pat, set()).add(m.pat.rx.match(v, m.pat.kind.anchored))
    return out


@pytest.mark.parametrize("proto", list(PROTOCOLS))
def test_every_atom_class_hits_and_misses(proto):
    hit, miss = set(), set()
    for name in PROTOCOLS[proto]:
        for pat, answers in _outcomes(C.stream(name)).items():
            if True in answers:
                hit |= pat.classes
            if False in answers:
                miss |= pat.classes
    assert hit >= set(C.ATOM_CLASSES) and miss >= set(C.ATOM_CLASSES), (sorted(hit), sorted(miss))


@pytest.mark.parametrize("name", ["r2d2", "cassandra"])
def test_wide_set_allows_from_three_chunks(name):
    s = C.stream(name)
    (wide,) = [rs for rs in s.sets if rs.kind == "wide"]
    assert len(wide.rules) == C.WIDE_RULES
    v, r, _ = s.ref
    at = {(int(x) - wide.first_id) // 64 for x in r[v == ALLOW] if wide.first_id <= x < wide.first_id + C.WIDE_RULES}
    assert at == {0, 1, 2}


# ------------------------------------------------------------------ 2. compile stats
@pytest.fixture(scope="module")
def compiled():
    """{stream: (stats, images by compiler)} on a host-only engine."""
    out = {}
    for name in C.STREAMS:
        w = C.stream(name).workload
        e = cilium_amd.Engine(-1)
        e.update_policy(w.policy)     # (raises PolicyError if anything is refused)
        e.set_connections(w.conns)
        out[name] = (e.stats(), export_images(e.export_tables()))
        e.close()
    return out


def _wrapped(s):
    return {m.pat.pattern for rs in s.sets for r in rs.rules for m in r.matchers if m.pat.nfa_of is not None}


def test_compile_stats(compiled):
    for name, (st, imgs) in compiled.items():
        s = C.stream(name)
        proto = name.split("_")[0]
        key = "http" if proto == "http" else IMAGE_KEY[proto]
        assert len(imgs[key]) == len(s.sets), name
        nfas = len(_wrapped(s))
        assert nfas == (0 if name in ("http", "memcached", "r2d2", "cassandra") else nfas)
        if proto == "http":
            assert st["http_nfas"] == nfas and st["http_rulesets"] == len(s.sets), (name, st)
            assert sum(img[H_NNFA] for img in imgs["http"]) == \
                sum(m.pat.nfa_of is not None for rs in s.sets for r in rs.rules for m in r.matchers)
            assert max(img[H_NNFA] for img in imgs["http"]) <= 64
        elif proto == "memcached":
            assert st["mc_nfas"] == nfas, (name, st)
        else:
            got = sum(img[3] for img in imgs[key])
            assert got == sum(m.pat.nfa_of is not None for rs in s.sets for r in rs.rules for m in r.matchers), name
    assert len(_wrapped(C.stream("http_nfa"))) >= 11 and len(_wrapped(C.stream("memcached_nfa"))) >= 11
    sizes = [len(img) for img in compiled["http"][1]["http"]]
    print("http image bytes", sorted(sizes))
    assert min(sizes) <= LDS_IMAGE_BYTES < max(sizes)
    assert max(img[H_MAX_SLOT_DFAS] for img in compiled["http"][1]["http"]) == 2
    two = [i for i, rs in enumerate(C.stream("memcached").sets) if rs.kind == "twopass"]
    assert compiled["memcached"][1]["memcache"][two[0]][2] >= 2      # McImgHeader::ndfa: a second pass over the keys
    for name in ("r2d2", "cassandra"):
        assert max(img[0] for img in compiled[name][1][name]) >= 3   # nchunks of the wide set


# ------------------------------------------------------------------ 3. the tables, walked
def _where(s, i, extra):
    return f"{extra}\n  {C.describe(s.workload, i)}"


@pytest.mark.parametrize("name", ["http", "http_nfa"])
def test_http_image_masks_and_absorbing_states(compiled, name):
    s = C.stream(name)
    tabs = [http_image_tables(img) for img in compiled[name][1]["http"]]
    for rs, t in zip(s.sets, tabs):
        assert t["ids"] == list(range(rs.first_id, rs.first_id + len(rs.rules))), rs.describe()
        # (b) [absorb, nstates) are the states that loop on every token byte; below, only the dead state 0 does
        for slot, dfas in t["slots"].items():
            for d in dfas:
                assert 1 <= d.absorb <= d.nstates and d.loops(0)
                for st in range(1, d.nstates):
                    assert d.loops(st) == (st >= d.absorb), (rs.describe(), slot, st, d.absorb)
        assert sum(d.nstates for dfas in t["slots"].values() for d in dfas) == t["total_states"]
    walked = n_two = n_nfa = 0
    for i, (seen, si) in enumerate(zip(s.values, s.req_set)):
        rs, t = s.sets[si], tabs[si]
        for slot, v in seen:
            if v is None or slot not in rs.slots():
                continue
            dfas = t["slots"][slot.lower()]
            rows = [d.masks[d.walk(v)] for d in dfas]
            for r, rule in enumerate(rs.rules):
                ms = [m for m in rule.matchers if m.slot == slot]
                bits = [(row >> r) & 1 for row in rows]
                if not ms:   # not constrained on this slot: the bit stays
                    assert all(bits), _where(s, i, f"rule {r} has no matcher on {slot}")
                    continue
                (m,) = ms
                want = int(m.pat.rx.match(v, True) != m.invert)
                nfa = [(k, lo, hi) for k, (nslot, lo, hi) in enumerate(t["nfa"]) if nslot == slot.lower() and
                       ((lo >> r) & 1) != ((hi >> r) & 1)]
                if nfa:      # evaluated by an NFA: every DFA keeps the bit, the NFA's two rows decide
                    assert m.pat.nfa_of is not None and all(bits), _where(s, i, f"rule {r} on {slot}: NFA")
                    (_, lo, hi) = nfa[0]
                    assert ((hi if m.pat.rx.match(v, True) else lo) >> r) & 1 == want, _where(s, i, f"rule {r}: NFA rows")
                    n_nfa += 1
                    continue
                assert m.pat.nfa_of is None, _where(s, i, f"rule {r} on {slot}: a wrapped pattern in a DFA")
                # (a) the DFA that evaluates it answers as the oracle; another DFA of the slot keeps the bit
                assert min(bits) == want and all(b == 1 or b == want for b in bits), \
                    _where(s, i, f"rule {r} on {slot} value {v!r}: mask bits {bits}, oracle {want}")
                n_two += len(bits) > 1
                walked += 1
    print(name, "values walked", walked, "on two-DFA slots", n_two, "NFA rows", n_nfa)
    assert walked > 2000 and (n_two > 100 if name == "http" else n_nfa > 500)


@pytest.mark.parametrize("name", ["memcached", "memcached_nfa", "r2d2", "r2d2_nfa", "cassandra", "cassandra_nfa"])
def test_generic_image_masks(compiled, name):
    """memcached, r2d2, cassandra: the OR of the DFAs' end-state mask rows holds
    exactly the rules whose regex the oracle accepts (the rules an NFA evaluates
    are in its own mask and in no DFA's)."""
    s = C.stream(name)
    key = IMAGE_KEY[name.split("_")[0]]
    tabs = [generic_image_tables(img, key) for img in compiled[name][1][key]]
    walked = 0
    for rs, t in zip(s.sets, tabs):
        assert t["ids"] == list(range(rs.first_id, rs.first_id + len(rs.rules))), rs.describe()
        by_nfa = 0
        for m in t["nfa"]:
            assert bin(m).count("1") == 1 and not by_nfa & m
            by_nfa |= m
        want_nfa = sum(1 << r for r, rule in enumerate(rs.rules) if rule.matchers[0].pat.nfa_of is not None)
        assert by_nfa == want_nfa, rs.describe()
        for d in t["dfas"]:
            assert d.absorb == d.nstates and not any(row & by_nfa for row in d.masks)
    for i, (seen, si) in enumerate(zip(s.values, s.req_set)):
        rs, t = s.sets[si], tabs[si]
        for _, v in seen:
            if v is None:
                continue
            got = 0
            for d in t["dfas"]:
                got |= d.masks[d.walk(v)]
            for r, rule in enumerate(rs.rules):
                pat = rule.matchers[0].pat
                if pat.nfa_of is None:
                    assert (got >> r) & 1 == int(pat.rx.match(v, False)), \
                        _where(s, i, f"rule {r} {pat.pattern!r} on {v!r}: mask bit {(got >> r) & 1}")
                    walked += 1
    print(name, "values walked", walked)
    assert walked > 1000

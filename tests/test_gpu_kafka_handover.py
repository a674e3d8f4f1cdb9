"""Produce requests aimed at the hand-over in kafka_classify_kernel's message
walk: the block a message's CRC leaves in the lane's slot is where the walk
reads the next message's window, or the partition / topic header behind the
set, when they lie in it (kafka_sched.h, GRd::span).  Verdict, rule id,
consumed length and counters against the oracle, bit for bit.

One stream, classified once by the oracle; each family at every arena alignment
0 .. 15:
  a  follow-on messages: 2 .. 6 messages per set, the first one's length swept
     so that its end takes every residue mod 64, both message formats, no key,
     a short key, and a key so long that the value length lies outside the slot
  b  chains of tiny messages (14 .. 40 bytes), several to a block
  c  set boundaries: a second partition of the same topic; a next topic whose
     name is 1, 10, 40 or 255 bytes long (its header inside the kept block,
     across its end, past it); the last set ending at the request's last byte,
     and 1 .. 15 bytes before it (bytes of the frame, and bytes of the entry
     behind the frame); the last request of the arena
  d  a slot that no longer holds what a careless walk would think: a bad CRC in
     the first, middle and last message of a set with a further topic behind
     it (and the same request with good CRCs); a set whose size cuts its last
     message, a further set behind it; trailing bytes behind the last message;
     a set that runs past the request; codecs 1 .. 3
  e  family a through l7g_classify_logged with four topic spans per request
Every family runs through kafka_classify_kernel<5, false> (a call without
memcached connections); one call of just over kBesideMin requests, memcached
ones among them, runs the whole stream through <6, false> and its helper grid."""
import struct

import numpy as np
import pytest
import torch

from cilium_amd import api, gen
from cilium_amd._lib import ALLOW, DENY, PARSE_ERROR, PROTO_KAFKA

gpu = pytest.mark.gpu
BESIDE_MIN = 1 << 20  # engine_state.h kBesideMin
ODD_TOPICS = ["a", "q" * 40, "z" * 255]  # with the 10-byte names of gen.kafka_topics(): 1, 10, 40, 255
GOOD = gen.kafka_topics()[:500]   # a produce rule each (gen.cfg3_rules)
OTHER = gen.kafka_topics()[500:]  # no produce rule: DENY


def _val(k, n):
    return bytes((k * 7 + i) & 0xFF for i in range(n))


def _req(v, corr, topics, frame_tail=0):
    """A produce request; topics: [(name, [(partition, set bytes, set size or
    None)])].  Returns the bytes and the topic names' (offset, length) spans."""
    head = struct.pack(">hhi", 0, v, corr) + gen.k_str("client-01")
    body = (gen.k_str(None) if v >= 3 else b"") + struct.pack(">hi", -1, 1000) + struct.pack(">i", len(topics))
    spans = []
    for name, parts in topics:
        spans.append((4 + len(head) + len(body) + 2, len(name)))
        body += gen.k_str(name) + struct.pack(">i", len(parts))
        for pid, ms, size in parts:
            body += struct.pack(">ii", pid, len(ms) if size is None else size) + ms
    payload = head + body + bytes(range(1, frame_tail + 1))
    return struct.pack(">i", len(payload)) + payload, spans


def _msgs(v, lens, key=None, bad=()):
    return [gen.k_message(_val(k, n), key=key, version=v, bad_crc=k in bad) for k, n in enumerate(lens)]


def _family_a():
    out = []
    for v in (0, 1):
        for first in range(64):  # the first message's end takes every residue mod 64
            for key in (None, b"k" * 5, b"K" * 70):
                n = 2 + (first + v) % 5
                lens = [first + 40] + [(first * 13 + 29 * j) % 300 for j in range(1, n)]
                ms = b"".join(_msgs(v, lens, key))
                name = GOOD[first] if first % 4 else OTHER[first]
                out.append(_req(v, first, [(name, [(0, ms, None)]), (GOOD[first + 64], [(1, ms[:0], None)])]))
    return out


def _family_b():
    out = []
    for v in (0, 1):
        top = 26 if v == 0 else 18  # value bytes: message sizes 14 .. 40 (v0), 22 .. 40 (v1)
        for k in range(96):
            lens = [(k + 5 * j) % (top + 1) for j in range(4 + k % 7)]
            ms = b"".join(_msgs(v, lens))
            out.append(_req(v, k, [(GOOD[k] if k % 3 else OTHER[k], [(0, ms, None), (1, ms, None)])]))
    return out


def _family_c():
    out = []
    names = [ODD_TOPICS[0], GOOD[7], ODD_TOPICS[1], ODD_TOPICS[2], OTHER[7]]
    for v in (0, 1):
        for end in range(0, 64, 3):  # where the first set ends in its block
            ms = b"".join(_msgs(v, [100, end + 30]))
            ms2 = b"".join(_msgs(v, [17, 80]))
            out.append(_req(v, end, [(GOOD[end], [(0, ms, None), (1, ms2, None)])]))  # a second partition
            for name in names:  # a next topic behind the set
                out.append(_req(v, end, [(GOOD[end], [(0, ms, None)]), (name, [(0, ms2, None)])]))
        for tail in range(15, -1, -1):  # the last set ends `tail` bytes before the request's last byte
            ms = b"".join(_msgs(v, [70 + tail, 90]))
            out.append(_req(v, tail, [(GOOD[tail], [(0, ms, None)])], frame_tail=tail))
            r, s = _req(v, tail, [(GOOD[tail + 16], [(0, ms, None)])])
            out.append((r + bytes(tail), s))  # bytes of the entry behind the frame
    return out


def _family_d():
    out, pairs = [], []
    for v in (0, 1):
        for k in range(20):
            lens = [60 + 9 * k, 45 + k, 130 - k]
            nxt = (GOOD[k + 100], [(0, b"".join(_msgs(v, [33 + k])), None)])
            for where in (0, 1, 2):  # a bad CRC in the first, middle, last message; and the good twin
                good = len(out)
                out.append(_req(v, k, [(GOOD[k], [(0, b"".join(_msgs(v, lens)), None)]), nxt]))
                out.append(_req(v, k, [(GOOD[k], [(0, b"".join(_msgs(v, lens, bad=(where,))), None)]), nxt]))
                pairs.append((good, good + 1, where))
            ms = b"".join(_msgs(v, lens))
            cut = len(ms) - 20 - k  # the set's size cuts its last message; a further set behind it
            out.append(_req(v, k, [(GOOD[k], [(0, ms[:cut], None)]), nxt]))
            out.append(_req(v, k, [(GOOD[k], [(0, ms, cut)]), nxt]))
            out.append(_req(v, k, [(GOOD[k], [(0, ms + _val(k, 1 + k % 11), None)]), nxt]))  # trailing bytes
            out.append(_req(v, k, [(GOOD[k], [(0, ms, len(ms) + 1 + 200 * k)])]))  # the set runs past the request
            inner = b"".join(_msgs(v, [20, 30]))
            for codec in (1, 2):
                z = gen.k_compressed(inner, codec, version=v)
                out.append(_req(v, k, [(GOOD[k], [(0, b"".join(_msgs(v, lens[:1])) + z, None)]), nxt]))
            z3 = gen.k_message(_val(k, 40), version=v, attributes=3)
            out.append(_req(v, k, [(GOOD[k], [(0, b"".join(_msgs(v, lens[:2])) + z3 + ms, None)]), nxt]))
    return out, pairs


class _Stream:
    pass


@pytest.fixture(scope="module")
def stream(oracle):
    S = _Stream()
    fam_d, S.pairs = _family_d()
    fams = {"a": _family_a(), "b": _family_b(), "d": fam_d, "c": _family_c()}
    rules = gen.cfg3_rules() + [api.PortRuleKafka(role="produce", topic=t) for t in ODD_TOPICS]
    kpol = api.policy_set(api.network_policy("10.0.0.1", 3, ingress=[(9092, [api.port_rule(kafka=rules)])]))
    m = gen.memcache_workload(600, seed=gen.SEED_BASE + 77)
    mconns = m.conns.copy()
    mconns["policy"] = 1
    kconns = gen.make_conns(1, 0, 9092, True, PROTO_KAFKA, [2000])
    # memcached first, then the families, each request at every alignment; family c last: its last
    # request (the set ends at the request's last byte) ends the arena
    chunks, offs, lens, S.fam, S.spans, S.base = [m.arena.tobytes()], list(m.offsets), list(m.lengths), {}, {}, {}
    at = len(m.arena)
    for name, reqs in fams.items():
        first = len(offs)
        for pad in range(16):
            for r, _ in reqs:
                chunks.append(bytes(pad) + r)
                offs.append(at + pad)
                lens.append(len(r))
                at += pad + len(r)
        S.fam[name] = np.arange(first, len(offs))
        S.spans[name] = [s for _ in range(16) for _, s in reqs]
        S.base[name] = first
    n = len(offs)
    conn_ids = np.concatenate([m.conn_ids + np.uint32(1), np.zeros(n - m.n, np.uint32)])
    S.w = gen.Workload("kafka-handover", np.frombuffer(b"".join(chunks), np.uint8).copy(), np.array(offs, np.uint64),
                       np.array(lens, np.uint32), conn_ids, np.concatenate([kconns, mconns]),
                       {"policies": [kpol["policies"][0], gen.mc_policy()["policies"][0]]})
    assert int(S.w.offsets[-1]) + int(S.w.lengths[-1]) == len(S.w.arena)
    S.nmc = m.n
    S.ref = oracle.classify_workload(S.w, 8)
    return S


def test_stream_is_not_vacuous(stream):
    """On the oracle's answers alone: every family allows and refuses; family
    d's good twins are allowed, a bad CRC in a set's first or middle message
    leaves the walk inside the set (DENY or PARSE_ERROR), one in its last
    message leaves it at the set's end (ALLOW, as the twin)."""
    v = stream.ref[0]
    for name, idx in stream.fam.items():
        assert 1000 <= len(idx) <= 9000, (name, len(idx))
        assert (v[idx] == ALLOW).sum() >= 100 and (v[idx] != ALLOW).sum() >= 100, name
    per = len(stream.fam["d"]) // 16
    for pad in range(16):
        for good, bad, where in stream.pairs:
            g, b = (stream.base["d"] + pad * per + k for k in (good, bad))
            assert v[g] == ALLOW
            assert (v[b] == ALLOW) if where == 2 else (v[b] in (DENY, PARSE_ERROR)), (where, v[b])


class _Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(engine, stream):
    c = _Ctx()
    engine.update_policy(stream.w.policy)
    engine.set_connections(stream.w.conns)
    c.dev = torch.device("cuda", 0)
    c.arena = torch.from_numpy(stream.w.arena).to(c.dev)
    return c


def _classify(c, eng, w, idx, logged=False):
    ins = [torch.from_numpy(np.ascontiguousarray(a)).to(c.dev)
           for a in (w.offsets[idx].view(np.int64), w.lengths[idx].view(np.int32), w.conn_ids[idx].view(np.int32))]
    n = len(idx)
    o = [torch.full((n,), 7, dtype=t, device=c.dev) for t in (torch.uint8, torch.int32, torch.int32)]
    cnt = torch.zeros(eng.nrules + 8, dtype=torch.int64, device=c.dev)
    args = [c.arena.data_ptr(), c.arena.numel(), *[t.data_ptr() for t in ins], n, *[t.data_ptr() for t in o]]
    top = None
    torch.cuda.synchronize()
    if logged:
        rec = torch.zeros(n * 32, dtype=torch.uint8, device=c.dev)
        top = torch.zeros(n * 4 * 2, dtype=torch.int32, device=c.dev)
        eng.classify_logged_device(*args, rec.data_ptr(), top.data_ptr(), 4, counters_ptr=cnt.data_ptr())
    else:
        eng.classify_device(*args, counters_ptr=cnt.data_ptr())
    torch.cuda.synchronize()
    got = (o[0].cpu().numpy(), o[1].cpu().numpy(), o[2].cpu().numpy().view(np.uint32))
    return got, cnt.cpu().numpy(), None if top is None else top.cpu().numpy().view(np.uint32).reshape(n, 4, 2)


def _same(S, idx, got, cnt, nrules):
    ref = tuple(r[idx] for r in S.ref)
    bad = np.nonzero((got[0] != ref[0]) | (got[1] != ref[1]) | (got[2] != ref[2]))[0]
    if len(bad):
        i = int(idx[bad[0]])
        o, L = int(S.w.offsets[i]), int(S.w.lengths[i])
        raise AssertionError(f"{len(bad)} of {len(idx)} differ; request {i} at arena offset {o} (mod 16: {o % 16}): got "
                             f"{[int(g[bad[0]]) for g in got]}, oracle {[int(r[bad[0]]) for r in ref]}; "
                             f"{S.w.arena[o:o + min(L, 96)].tobytes()!r}")
    want = np.zeros(nrules + 8, np.int64)
    allowed = ref[1][(ref[0] == ALLOW) & (ref[1] >= 0)]
    want[:nrules] = np.bincount(allowed, minlength=nrules)[:nrules]
    want[nrules:nrules + 5] = np.bincount(ref[0], minlength=5)[:5]
    assert (cnt[:nrules + 5] == want[:nrules + 5]).all(), np.nonzero(cnt[:nrules + 5] != want[:nrules + 5])[0][:8]


@gpu
@pytest.mark.parametrize("family", ["a", "b", "c", "d"])
def test_family_matches_oracle(engine, stream, ctx, family):
    """A call of Kafka requests alone: kafka_classify_kernel<5, false>."""
    idx = stream.fam[family]
    got, cnt, _ = _classify(ctx, engine, stream.w, idx)
    _same(stream, idx, got, cnt, engine.nrules)


@gpu
def test_logged_call(engine, stream, ctx):
    """Family a through l7g_classify_logged (kafka_classify_kernel<4, true>): the
    same answers, and the topic spans where the names lie in the request."""
    idx = stream.fam["a"]
    got, cnt, top = _classify(ctx, engine, stream.w, idx, logged=True)
    _same(stream, idx, got, cnt, engine.nrules)
    want = np.array([[list(s) for s in spans] for spans in stream.spans["a"]], np.uint32)
    assert want.shape == (len(idx), 2, 2)
    assert np.isin(stream.ref[0][idx], (ALLOW, DENY)).all()
    assert (top[:, :2, :] == want).all(), np.nonzero((top[:, :2, :] != want).any(axis=(1, 2)))[0][:8]


@gpu
def test_beside_memcached(engine, stream, ctx):
    """Just past kBesideMin, memcached requests among them: the whole stream's
    indices repeated over the same arena in a shuffled order, through
    kafka_classify_kernel<6, false> and its helper grid."""
    n = BESIDE_MIN + 4321
    idx = np.tile(np.arange(stream.w.n), -(-n // stream.w.n))[:n]
    np.random.default_rng(5).shuffle(idx)
    assert (idx < stream.nmc).sum() > 1000
    got, cnt, _ = _classify(ctx, engine, stream.w, idx)
    _same(stream, idx, got, cnt, engine.nrules)

"""The memcached classifier over the directed edge corpus
(tests/mc_edge_cases.py), bit-exact against the oracle on verdict, rule and
consumed, in every build of csrc/kernels/memcache_classify.hip and through
every way a request reaches it (LaunchMemcacheClassify, classify.cc).

Builds -- the whole placed corpus (every request at all 16 offsets mod 16:
more than kPartitionMin memcached-only requests, so the partition's packed lists
feed the kernel) in one host call per policy; what selects the build, from
engine.stats():

  gen.mc_policy()          mc_rules <= 64 (one mask chunk per rule set),
                           mc_nfas == 0, mc_dfas == 1: memcache_classify_kernel<1>,
                           images staged in LDS
  many_rules_policy()      mc_rules > 64, mc_nfas == 0:
                           memcache_classify_kernel<kMcMaxChunks>; rules 70-140
                           allow, so ids[c * 64 + ...] is read with c = 1 and 2
  nfa_policy()             mc_nfas >= 2: memcache_classify_nfa_kernel (family G's
                           300-key lines run the NFAs at every key's end)
  big_images_policy()      mc_dfa_states * 8 > kMcLdsImages (every state holds at
                           least one 8-byte mask word), mc_dfas >= 3,
                           mc_nfas == 0: images read from global memory, the
                           line walked once per key DFA.  It compiles to 10 DFAs
                           of 9252 states in all (7 of them walked by the
                           in-group rule set).

Call paths (gen.mc_policy() unless noted):

  by-index chunk loop      the rotating corpus (request i at offset i mod 16),
                           a family per host call (65 .. kPartitionMin - 1
                           requests, each arena ending with its last request);
                           device-resident inputs in calls of 1500; the host
                           calls again under big_images_policy()
  one wave                 the core subset (mc_edge_cases.core_layout) in calls
                           of 64 -- and of 1 and 63 --: host calls with the
                           service off (memcache_classify_sync_kernel; service
                           counters unchanged), the same under nfa_policy()
                           (its <true, ...> build), device calls (the launched
                           kernel's m <= 64 branch), host calls with the service
                           on (memcache_service_kernel; mc_calls grows by the
                           number of calls)
  mixed batch              the rotating corpus interleaved with HTTP and Kafka
                           requests, 2 * kPartitionMin and more, one device call
"""
import numpy as np
import pytest
import torch

import mc_edge_cases as E
from cilium_amd import gen
from cilium_amd._lib import ALLOW, DENY
from test_gpu_http import assert_same
from test_gpu_memcache import mc_nfa_policy

pytestmark = pytest.mark.gpu

K_PARTITION_MIN = 4096       # engine_state.h
K_MC_LDS_IMAGES = 32 * 1024  # memcache_classify.hip


def _nfa_policy():
    base = mc_nfa_policy()["policies"][0]["ingress_per_port_policies"][0]["rules"][0]["l7_rules"]["l7_rules"]
    return E.nfa_policy([x["rule"] for x in base])


POLICIES = {
    "cfg5": (gen.mc_policy, E.MC_POLICY_KEYS),
    "many_rules": (E.many_rules_policy, E.MC_POLICY_KEYS),
    "nfa": (_nfa_policy, E.NFA_KEYS),
    "big_images": (E.big_images_policy, E.BIG_KEYS),
}


class _Set:
    """One policy's corpus: its layouts and the oracle's answers, computed once."""

    def __init__(self, oracle, name):
        mk, self.K = POLICIES[name]
        self.policy = mk()
        self.conns = E.conns()
        self.cases = E.corpus(self.K)
        self.oracle = oracle
        self._w = {}

    def workload(self, layout_name, idx=None):
        """(workload, oracle's answers) of a layout: "full", "rotating"
        (idx: a family's cases), "core"."""
        k = (layout_name, None if idx is None else tuple(idx))
        if k not in self._w:
            lay = {"full": lambda: E.full_layout(self.cases, self.K),
                   "rotating": lambda: E.rotating_layout(self.cases, self.K, idx),
                   "core": lambda: E.core_layout(self.cases, self.K)}[layout_name]()
            w = E.workload(E.place(self.cases, self.K, lay), self.conns, self.policy)
            self._w[k] = (w, self.oracle.classify_workload(w, 8))
        return self._w[k]


@pytest.fixture(scope="module")
def sets(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Set(oracle, name)
        return cache[name]
    return get


def _install(engine, s):
    engine.update_policy(s.policy)
    engine.set_connections(s.conns)
    return engine.stats()


def _device_arrays(w):
    dev = torch.device("cuda", 0)
    return (torch.from_numpy(w.arena).to(dev), torch.from_numpy(w.offsets.view(np.int64)).to(dev),
            torch.from_numpy(w.lengths.view(np.int32)).to(dev), torch.from_numpy(w.conn_ids.view(np.int32)).to(dev))


def _device_call(engine, d, lo, hi):
    """Requests [lo, hi) of device-resident inputs d through l7g_classify."""
    arena, off, ln, cid = d
    n = hi - lo
    out = [torch.full((n,), 7, dtype=t, device=arena.device) for t in (torch.uint8, torch.int32, torch.int32)]
    ins = [t[lo:hi].clone() for t in (off, ln, cid)]   # (arrays of their own, aligned as an allocation is)
    torch.cuda.synchronize()
    engine.classify_device(arena.data_ptr(), arena.numel(), *[t.data_ptr() for t in ins], n,
                           *[t.data_ptr() for t in out])
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy().view(np.uint32)


def _host_call(engine, w, lo, hi):
    """Requests [lo, hi) as a small host call of their own: the arena cut at
    16-byte boundaries around them (the offsets mod 16 stay), up to the next
    request, so the bytes behind the last one are its neighbour's as before."""
    a0 = int(w.offsets[lo]) & ~15
    a1 = int(w.offsets[hi]) if hi < w.n else len(w.arena)
    return engine.classify(w.arena[a0:a1], w.offsets[lo:hi] - np.uint64(a0), w.lengths[lo:hi], w.conn_ids[lo:hi])


def _spans(n):
    """Calls of 1 and 63 first, then of exactly 64 (the rest in a last one)."""
    cuts = [0, 1, 64, 65, 128]
    cuts += list(range(192, n, 64))
    return list(zip(cuts, cuts[1:] + [n]))


def _same(got, ref, w, lo=0, hi=None):
    sub = gen.Workload(w.name, w.arena, w.offsets[lo:hi], w.lengths[lo:hi], w.conn_ids[lo:hi], w.conns, w.policy)
    assert_same(got, tuple(r[lo:hi] for r in ref), sub)


# ------------------------------------------------------------------ builds
@pytest.mark.parametrize("name", list(POLICIES))
def test_whole_corpus_per_build(engine, sets, name):
    s = sets(name)
    w, ref = s.workload("full")
    assert w.n >= 16 * len(s.cases) > K_PARTITION_MIN
    st = _install(engine, s)
    if name == "cfg5":
        assert st["mc_rules"] <= 64 and st["mc_nfas"] == 0 and st["mc_dfas"] == 1
    elif name == "many_rules":
        assert st["mc_rules"] > 64 and st["mc_nfas"] == 0
    elif name == "nfa":
        assert st["mc_nfas"] >= 2
    else:
        assert st["mc_dfa_states"] * 8 > K_MC_LDS_IMAGES and st["mc_dfas"] >= 3 and st["mc_nfas"] == 0
    v = ref[0]
    framed = int(((v == ALLOW) | (v == DENY)).sum())
    assert (v == ALLOW).sum() >= 0.05 * framed and (v == DENY).sum() >= 0.05 * framed
    if name == "many_rules":
        allowed = set(ref[1][v == ALLOW].tolist())
        assert any(64 <= r < 128 for r in allowed) and any(128 <= r < 192 for r in allowed)
    _same(engine.classify(w.arena, w.offsets, w.lengths, w.conn_ids), ref, w)


# ------------------------------------------------------------------ by-index chunk loop
def _family_calls(s):
    fam = E.family_indices(s.cases)
    fam["G"] = fam["G"] + fam.pop("I")   # (two requests: with the family before them)
    return fam


@pytest.mark.parametrize("name", ["cfg5", "big_images"])
def test_chunk_loop_host_calls(engine, sets, name):
    s = sets(name)
    _install(engine, s)
    for f, idx in _family_calls(s).items():
        assert 64 < len(idx) < K_PARTITION_MIN, f
        w, ref = s.workload("rotating", idx)
        assert int(w.offsets[-1]) + int(w.lengths[-1]) == len(w.arena)
        _same(engine.classify(w.arena, w.offsets, w.lengths, w.conn_ids), ref, w)


def test_chunk_loop_device_calls(engine, sets):
    s = sets("cfg5")
    _install(engine, s)
    w, ref = s.workload("rotating")
    d = _device_arrays(w)
    for lo in range(0, w.n, 1500):
        hi = min(lo + 1500, w.n)
        assert 64 < hi - lo < K_PARTITION_MIN
        _same(_device_call(engine, d, lo, hi), ref, w, lo, hi)


# ------------------------------------------------------------------ one wave
@pytest.mark.parametrize("name", ["cfg5", "nfa"])
def test_one_wave_sync_kernel(engine, sets, name):
    s = sets(name)
    _install(engine, s)
    w, ref = s.workload("core")
    assert w.n >= 1024
    prev, before = engine.service(False)
    try:
        for lo, hi in _spans(w.n):
            _same(_host_call(engine, w, lo, hi), ref, w, lo, hi)
        assert engine.service()[1] == before   # no call went to the service
    finally:
        engine.service(prev)


def test_one_wave_launched_kernel(engine, sets):
    s = sets("cfg5")
    _install(engine, s)
    w, ref = s.workload("core")
    d = _device_arrays(w)
    for lo, hi in _spans(w.n):
        _same(_device_call(engine, d, lo, hi), ref, w, lo, hi)


def test_one_wave_service_kernel(engine, sets):
    s = sets("cfg5")
    _install(engine, s)
    w, ref = s.workload("core")
    prev, _ = engine.service(True)
    try:
        before = engine.service()[1]
        spans = _spans(w.n)
        for lo, hi in spans:
            _same(_host_call(engine, w, lo, hi), ref, w, lo, hi)
        after = engine.service()[1]
        assert after["mc_calls"] - before["mc_calls"] == len(spans)   # the service answered every call
    finally:
        engine.service(False)   # off, then as it was
        engine.service(prev)


# ------------------------------------------------------------------ mixed batch
def test_mixed_batch_lists(engine, oracle, sets):
    s = sets("cfg5")
    m, _ = s.workload("rotating")
    h = gen.http_workload(2, 3000)
    k = gen.kafka_workload(2000)
    pol = {"policies": [m.policy["policies"][0], h.policy["policies"][0], dict(k.policy["policies"][0], name="10.0.0.2")]}
    conns = np.concatenate([m.conns, h.conns, k.conns])
    nm, nh = len(m.conns), len(h.conns)
    conns["policy"][nm:nm + nh] = 1
    conns["policy"][nm + nh:] = 2
    pad = np.full(-len(m.arena) % 16, 0x20, np.uint8)   # (the memcached arena first: its offsets mod 16 stay)
    arena = np.concatenate([m.arena, pad, h.arena, k.arena])
    a1 = len(m.arena) + len(pad)
    offs = np.concatenate([m.offsets, h.offsets + np.uint64(a1), k.offsets + np.uint64(a1 + len(h.arena))])
    lens = np.concatenate([m.lengths, h.lengths, k.lengths])
    cids = np.concatenate([m.conn_ids, h.conn_ids + np.uint32(nm), k.conn_ids + np.uint32(nm + nh)])
    # interleaved, deterministically: the three streams merged by their relative position
    pos = np.concatenate([np.arange(x.n) / x.n for x in (m, h, k)])
    perm = np.argsort(pos, kind="stable")
    w = gen.Workload("mixed-edges", arena, offs[perm], lens[perm], cids[perm], conns, pol)
    assert w.n >= 2 * K_PARTITION_MIN
    engine.update_policy(pol)
    engine.set_connections(conns)
    ref = oracle.classify_workload(w, 8)
    _same(_device_call(engine, _device_arrays(w), 0, w.n), ref, w)

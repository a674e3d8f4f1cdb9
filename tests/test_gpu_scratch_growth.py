"""A per-stream scratch buffer regrown while the previous call on the same
stream may still be running (StreamScratch::Grow, the launch plan in
classify.cc).  l7g_classify calls of growing size are issued back to back on
one caller stream, with no host synchronisation between them, on a fresh
engine (its scratch starts empty, so the larger call must regrow what the
smaller one still uses); after one final synchronisation every call's
verdicts, rule ids and consumed lengths equal the oracle's.  One case per
grow-only buffer: the partition lists, the NFA pre-pass bits, the large NFAs'
state sets with cassandra's USE scratch, and the grouped HTTP lists."""
import random

import numpy as np
import pytest
import torch

import nfa_cases
import test_gpu_large_nfa as big
from cilium_amd import Engine, api, gen
from cilium_amd._lib import ALLOW, DENY, PROTO_HTTP
from test_gpu_http import assert_same, wl_from_reqs

pytestmark = pytest.mark.gpu


def _back_to_back(w, ref, sizes):
    """Calls over w's first n requests, n in sizes, in a row on one stream."""
    eng = Engine(0)
    try:
        eng.update_policy(w.policy)
        eng.set_connections(w.conns)
        dev = torch.device("cuda", 0)
        d_arena = torch.from_numpy(w.arena).to(dev)
        d_off = torch.from_numpy(w.offsets.view(np.int64)).to(dev)
        d_len = torch.from_numpy(w.lengths.view(np.int32)).to(dev)
        d_cid = torch.from_numpy(w.conn_ids.view(np.int32)).to(dev)
        outs = [[torch.full((n,), 7, dtype=t, device=dev) for t in (torch.uint8, torch.int32, torch.int32)]
                for n in sizes]
        s = torch.cuda.Stream()
        torch.cuda.synchronize()  # inputs and output fills are done before the stream's first call
        for n, o in zip(sizes, outs):
            eng.classify_device(d_arena.data_ptr(), d_arena.numel(), d_off.data_ptr(), d_len.data_ptr(),
                                d_cid.data_ptr(), n, *[t.data_ptr() for t in o], stream=s.cuda_stream)
        torch.cuda.synchronize()
        for n, o in zip(sizes, outs):
            got = (o[0].cpu().numpy(), o[1].cpu().numpy(), o[2].cpu().numpy().view(np.uint32))
            assert_same(got, tuple(r[:n] for r in ref), w)
    finally:
        eng.close()


def test_partition_lists_regrown(oracle):
    """d_sel: HTTP, Kafka and memcached in one engine, 4096 -> 8192 -> 4096."""
    w = gen.mixed_workload(8192)
    _back_to_back(w, oracle.classify_workload(w, 8), [4096, 8192, 4096])


def test_nfa_bits_regrown(oracle):
    """d_nfa: an HTTP rule set with NFA-fallback matchers, 64 -> 512."""
    pol = nfa_cases.policy()
    w = wl_from_reqs(nfa_cases.requests(512, seed=5), pol, nfa_cases.conns())
    ref = oracle.classify_workload(w, 8)
    assert (ref[0][:64] == ALLOW).any() and (ref[0][:64] == DENY).any()
    _back_to_back(w, ref, [64, 512])


def test_large_nfa_and_cassandra_scratch_regrown(oracle):
    """d_bignfa and d_use: large NFAs on HTTP, memcached, cassandra and r2d2,
    256 -> 1024.  Both buffers are sized by the request count, so most values
    are short (they cannot match: DENY); a quarter are full length."""
    rng = random.Random(23)
    reqs, ids = [], []
    for i in range(1024):
        kind = i % 4
        if i % 16 < 4:
            v = big._path_value(rng, 1) if kind < 2 else big._value(rng, 1)
        else:
            v = "".join(rng.choice("abcyx") for _ in range(rng.randint(1, 120)))
        reqs.append(big._request(kind, v))
        ids.append(kind)
    pol = big._policy(big.PATS[1])  # (the pattern that compiles in a fraction of a second)
    w = wl_from_reqs(reqs, pol, big.CONNS, np.array(ids, np.uint32))
    ref = oracle.classify_workload(w, 8)
    assert (ref[0][:256] == ALLOW).sum() > 4 and (ref[0] == ALLOW).sum() > 16 and (ref[0] == DENY).sum() > 768
    _back_to_back(w, ref, [256, 1024])


def test_grouped_lists_regrown(oracle):
    """d_grp: two HTTP rule sets in use, 65536 (the grouped path's floor) ->
    131072 short requests (2048 distinct ones, repeated)."""
    groups = [api.port_rule(remote_policies=[256 + g], http=api.http_rules_from_api(gen.cfg2_rules(8 * g, 8)))
              for g in range(2)]
    pol = api.policy_set(api.network_policy("10.0.0.1", 3, ingress=[(80, groups)]))
    reqs = [b"%s /api/v%d/svc%d/x HTTP/1.1\r\nHost: svc-%d.x\r\n\r\n" % ([b"GET", b"POST", b"PUT"][k % 3], k % 3 + 1,
                                                                     k % 16, k % 16) for k in range(2048)]
    conns = gen.make_conns(3, 0, 80, True, PROTO_HTTP, np.array([256, 257, 257]))
    base = wl_from_reqs(reqs, pol, conns, np.arange(2048, dtype=np.uint32) % 3)
    ref_base = oracle.classify_workload(base, 8)
    assert (ref_base[0] == ALLOW).any() and (ref_base[0] == DENY).any()
    idx = np.tile(np.arange(2048), 64)
    w = gen.Workload("grouped", base.arena, base.offsets[idx], base.lengths[idx], base.conn_ids[idx], conns, pol)
    _back_to_back(w, tuple(r[idx] for r in ref_base), [65536, 131072])

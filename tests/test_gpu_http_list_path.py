"""The HTTP kernels that stage a rule-set image in LDS, reading the partition's
entry lists: http_classify_kernel<true, N> (the hot rule set) and
http_grouped_kernel (the other rule sets, from kGroupMin = 65,536 requests).

One mixed HTTP / Kafka stream of 2 * kPartitionMin = 8192 requests (so every
call is partitioned and the HTTP kernels walk lists of entries) is classified
by the oracle once.  Its HTTP requests are on four rule sets -- remote 256 on
half the connections (the hot one), 257-259 on the rest, as cfg4 spreads its
rules over remote identities -- and their lengths are

  * 703-705, 1151-1153, 1599-1601: each length-class edge of the partition
    (704, 1152, 1600) at edge - 1, edge and edge + 1;
  * 320-335: every length modulo 16, and with the packed arena every start
    alignment;
  * 3500 and 5000: past the 3 KiB a tile maps, so the span mode runs;
  * ordinary lengths in between.

The stream runs once as it is (the hot kernel and the general one) and once
tiled eight times over the same arena, 65,536 requests (the hot kernel and the
grouped one)."""
import numpy as np
import pytest
import torch

from cilium_amd import api, gen
from cilium_amd._lib import ALLOW, DENY, PROTO_HTTP
from test_gpu_http import assert_same

pytestmark = pytest.mark.gpu

K_PARTITION_MIN = 4096
K_GROUP_MIN = 1 << 16
N = 2 * K_PARTITION_MIN
NH = 6000
EDGES = [703, 704, 705, 1151, 1152, 1153, 1599, 1600, 1601]
LENS = EDGES + list(range(320, 336)) + [120, 200, 900, 1300, 2040, 2900]
LONG = {17: 3500, 4001: 5000, 5555: 3073}


def _http_request(k):
    total = LONG.get(k, LENS[k % len(LENS)])
    head = b"%s /api/v%d/svc%d/x HTTP/1.1\r\nHost: svc-%d.x\r\n" % ([b"GET", b"POST", b"PUT"][k % 3], k % 3 + 1, k % 16,
                                                                 k % 16)
    r = head + b"X-Pad: " + b"p" * (total - len(head) - 11) + b"\r\n\r\n"
    assert len(r) == total
    return r


class _Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(engine, oracle):
    groups = [api.port_rule(remote_policies=[256 + g], http=api.http_rules_from_api(gen.cfg2_rules(8 * g, 8)))
              for g in range(4)]
    hpol = api.policy_set(api.network_policy("10.0.0.1", 3, ingress=[(80, groups)]))
    hconns = gen.make_conns(8, 0, 80, True, PROTO_HTTP, np.array([256, 256, 256, 256, 257, 258, 259, 257]))
    hreqs = [_http_request(k) for k in range(NH)]
    k = gen.kafka_workload(N - NH, seed=gen.SEED_BASE + 95)
    conns = np.concatenate([hconns, k.conns])
    conns["policy"][len(hconns):] = 1
    pol = {"policies": [hpol["policies"][0], dict(k.policy["policies"][0], name="10.0.0.2")]}
    kbuf = k.arena.tobytes()
    reqs = hreqs + [kbuf[int(o):int(o) + int(l)] for o, l in zip(k.offsets, k.lengths)]
    # (method, version and service repeat every 48 requests: each such run on one connection)
    cids = np.concatenate([np.arange(NH) // 48 % 8, k.conn_ids + len(hconns)]).astype(np.uint32)
    perm = np.random.default_rng(gen.SEED_BASE + 97).permutation(N)
    arena, offs, lens = gen.pack([reqs[i] for i in perm])
    c = _Ctx()
    c.w = w = gen.Workload("http-lists", arena, offs, lens, cids[perm], conns, pol)
    c.ref = oracle.classify_workload(w, 8)
    engine.update_policy(w.policy)
    engine.set_connections(w.conns)
    c.engine = engine
    c.dev = torch.device("cuda", 0)
    c.d_arena = torch.from_numpy(w.arena).to(c.dev)
    return c


def _run(c, idx):
    w = c.w
    n = len(idx)
    d_off = torch.from_numpy(np.ascontiguousarray(w.offsets[idx]).view(np.int64)).to(c.dev)
    d_len = torch.from_numpy(np.ascontiguousarray(w.lengths[idx]).view(np.int32)).to(c.dev)
    d_cid = torch.from_numpy(np.ascontiguousarray(w.conn_ids[idx]).view(np.int32)).to(c.dev)
    out = [torch.full((n,), 7, dtype=t, device=c.dev) for t in (torch.uint8, torch.int32, torch.int32)]
    torch.cuda.synchronize()
    c.engine.classify_device(c.d_arena.data_ptr(), c.d_arena.numel(), d_off.data_ptr(), d_len.data_ptr(),
                             d_cid.data_ptr(), n, *[t.data_ptr() for t in out])
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy().view(np.uint32)


def test_stream_covers_the_cases(ctx):
    """The stream is what the docstring says (host-side checks of the fixture)."""
    w, ref = ctx.w, ctx.ref
    http = w.conns["proto"][w.conn_ids] == PROTO_HTTP
    assert int(http.sum()) == NH and w.n == N
    hl = w.lengths[http]
    for L in EDGES + list(LONG.values()):
        assert (hl == L).any(), L
    assert {int(x) % 16 for x in hl} == set(range(16))
    assert {int(x) % 16 for x in w.offsets[http]} == set(range(16))
    hot = http & (w.conn_ids < 4)
    for sel in (hot, http & ~hot):
        assert (ref[0][sel] == ALLOW).any() and (ref[0][sel] == DENY).any()
    for L in LONG.values():  # the long requests are read to their end, not refused
        assert ref[0][http & (w.lengths == L)][0] in (ALLOW, DENY)


def test_lists_hot_and_general(ctx):
    idx = np.arange(N)
    assert_same(_run(ctx, idx), ctx.ref, ctx.w)


def test_lists_hot_and_grouped(ctx):
    w = ctx.w
    idx = np.arange(K_GROUP_MIN) % N
    got = _run(ctx, idx)
    assert_same(got, tuple(r[idx] for r in ctx.ref), gen.Workload("t", w.arena, w.offsets[idx], w.lengths[idx],
                                                                  w.conn_ids[idx], w.conns, w.policy))

"""Which memcached kernel serves which call (LaunchMemcacheClassify).

A host call of at most 64 requests on a memcached-only engine (fuse_mc,
classify.cc) runs the one-workgroup build memcache_classify_sync_kernel, which
copies the call's inputs in and stores its done word; every other call runs
memcache_classify_kernel, whose one-wave path serves up to 64 entries and whose
chunk loop serves more.  The sizes below sit on both sides of that boundary
(64 / 65) and just under kPartitionMin = 4096 (engine_state.h), above which a
memcached-only batch is partitioned first.

One memcached-only stream (text retrievals, other text commands and binary
requests; connections whose flags force the text parser, force the binary one
or leave it to the first byte) is classified by the oracle once; each case
classifies a prefix of it:

  * through l7g_classify_host (Engine.classify): host buffers, so up to 64
    requests are copied in by the kernel and the done word is stored by it;
  * through l7g_classify (Engine.classify_device) with device-resident inputs:
    nothing to copy, no done word;
  * the same with `counters` set (the host entry point takes none): the
    counters kernel ends the call, not the classifier;
  * one mixed HTTP / Kafka / memcached batch of 2 * kPartitionMin requests:
    the partition's lists, read by memcache_classify_kernel.
"""
import numpy as np
import pytest
import torch

from cilium_amd import gen
from cilium_amd._lib import ALLOW, DENY
from test_gpu_http import assert_same

pytestmark = pytest.mark.gpu

K_PARTITION_MIN = 4096
SIZES = [1, 63, 64, 65, K_PARTITION_MIN - 1]


class _Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(engine, oracle):
    c = _Ctx()
    w = gen.memcache_workload(K_PARTITION_MIN - 1, seed=gen.SEED_BASE + 91)
    conns = w.conns.copy()
    conns["flags"] = np.arange(len(conns)) % 3  # by first byte / text / binary
    c.w = w = gen.Workload(w.name, w.arena, w.offsets, w.lengths, w.conn_ids, conns, w.policy)
    c.ref = oracle.classify_workload(w, 8)
    engine.update_policy(w.policy)
    engine.set_connections(w.conns)
    c.engine = engine
    c.dev = torch.device("cuda", 0)
    c.d_arena = torch.from_numpy(w.arena).to(c.dev)
    return c


def _device(c, w, n, counters=None):
    d_off = torch.from_numpy(np.ascontiguousarray(w.offsets[:n]).view(np.int64)).to(c.dev)
    d_len = torch.from_numpy(np.ascontiguousarray(w.lengths[:n]).view(np.int32)).to(c.dev)
    d_cid = torch.from_numpy(np.ascontiguousarray(w.conn_ids[:n]).view(np.int32)).to(c.dev)
    out = [torch.full((n,), 7, dtype=t, device=c.dev) for t in (torch.uint8, torch.int32, torch.int32)]
    torch.cuda.synchronize()
    c.engine.classify_device(c.d_arena.data_ptr(), c.d_arena.numel(), d_off.data_ptr(), d_len.data_ptr(),
                             d_cid.data_ptr(), n, *[t.data_ptr() for t in out],
                             counters_ptr=counters.data_ptr() if counters is not None else 0)
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy().view(np.uint32)


def test_stream_mixes_text_and_binary(ctx):
    """Host-side check of the fixture: every prefix of 63 or more requests holds text
    retrievals, other text commands and binary requests, allowed and denied."""
    w, ref = ctx.w, ctx.ref
    first = np.where(w.lengths > 0, w.arena[np.minimum(w.offsets, len(w.arena) - 1).astype(np.int64)], 0)
    for n in SIZES[1:]:
        f = first[:n]
        assert (f == ord("g")).any() and (f >= 0x80).any() and ((f < 0x80) & (f != ord("g"))).any(), n
        assert (ref[0][:n] == ALLOW).any() and (ref[0][:n] == DENY).any(), n
        assert len(set(w.conns["flags"][w.conn_ids[:n]].tolist())) == 3, n


@pytest.mark.parametrize("n", SIZES)
def test_host_call_matches_oracle(ctx, n):
    w = ctx.w
    got = ctx.engine.classify(w.arena, w.offsets[:n], w.lengths[:n], w.conn_ids[:n])
    assert_same(got, tuple(r[:n] for r in ctx.ref), w)


@pytest.mark.parametrize("n", SIZES)
def test_device_call_matches_oracle(ctx, n):
    assert_same(_device(ctx, ctx.w, n), tuple(r[:n] for r in ctx.ref), ctx.w)


@pytest.mark.parametrize("n", [64, 65])
def test_device_call_with_counters(ctx, n):
    nr = ctx.engine.nrules
    cnt = torch.zeros(nr + 8, dtype=torch.int64, device=ctx.dev)
    ref = tuple(r[:n] for r in ctx.ref)
    assert_same(_device(ctx, ctx.w, n, counters=cnt), ref, ctx.w)
    want = np.zeros(nr + 8, np.int64)
    np.add.at(want, ref[1][ref[0] == ALLOW], 1)
    want[nr:nr + 5] = np.bincount(ref[0], minlength=5)[:5]
    np.testing.assert_array_equal(cnt.cpu().numpy(), want)


def test_partitioned_mixed_batch(engine, oracle):
    """Runs last in this module: it installs its own policy and connections."""
    w = gen.mixed_workload(2 * K_PARTITION_MIN, seed=gen.SEED_BASE + 93)
    nmc = int((w.conns["proto"][w.conn_ids] == gen.PROTO_MEMCACHE).sum())
    assert nmc > 1024  # more than one chunk per wave of a workgroup
    engine.update_policy(w.policy)
    engine.set_connections(w.conns)
    c = _Ctx()
    c.engine, c.dev = engine, torch.device("cuda", 0)
    c.d_arena = torch.from_numpy(w.arena).to(c.dev)
    assert_same(_device(c, w, w.n), oracle.classify_workload(w, 8), w)

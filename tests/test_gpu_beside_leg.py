"""The Kafka / memcached leg of a large mixed batch (classify.cc: from
engine_state.h kBesideMin = 2^20 requests the memcached kernel runs on the side
stream beside the Kafka kernel's persistent grid, as a persistent grid of its
own at a raised wave priority, and a second small Kafka grid follows it on that
stream and draws from the main grid's work counter) against the oracle: every
verdict, rule id and consumed length, and the counters.

One unique stream of under 20k requests (HTTP, Kafka with compressed and
corrupt-CRC produce requests, memcached) is generated and given to the oracle
once.  Each case reaches its size by repeating request indices of that stream
over the same arena, so its expected answers are the oracle's, indexed."""
import numpy as np
import pytest
import torch

from cilium_amd import gen

pytestmark = pytest.mark.gpu

BESIDE_MIN = 1 << 20  # engine_state.h kBesideMin


class _Stream:
    pass


@pytest.fixture(scope="module")
def stream(oracle):
    """The unique stream (one arena; HTTP, Kafka and memcached connections and
    policies as gen.mixed_workload lays them out), its index ranges per kind,
    and the oracle's answers."""
    h = gen.http_workload(2, 6000, seed=gen.SEED_BASE + 71)
    kreqs = (gen.kafka_requests(2500, gen.SEED_BASE + 72) + gen.kafka_compressed_requests(600, gen.SEED_BASE + 73) +
             gen.kafka_adversarial(900, gen.SEED_BASE + 74))
    k0 = gen.kafka_workload(16, seed=gen.SEED_BASE + 75)  # (its connections and policy)
    ka, ko, kl = gen.pack(kreqs)
    kc = np.random.default_rng(76).integers(0, len(k0.conns), size=len(kreqs)).astype(np.uint32)
    m = gen.memcache_workload(5000, seed=gen.SEED_BASE + 77)
    pol = {"policies": [h.policy["policies"][0], dict(k0.policy["policies"][0], name="10.0.0.2"),
                        m.policy["policies"][0]]}
    conns = np.concatenate([h.conns, k0.conns, m.conns])
    ch, ck = len(h.conns), len(k0.conns)
    conns["policy"][ch:ch + ck] = 1
    conns["policy"][ch + ck:] = 2
    S = _Stream()
    S.w = gen.Workload(
        "beside-unique", np.concatenate([h.arena, ka, m.arena]),
        np.concatenate([h.offsets, ko + np.uint64(len(h.arena)), m.offsets + np.uint64(len(h.arena) + len(ka))]),
        np.concatenate([h.lengths, kl, m.lengths]),
        np.concatenate([h.conn_ids, kc + np.uint32(ch), m.conn_ids + np.uint32(ch + ck)]), conns, pol)
    nh, nk = h.n, len(kreqs)
    S.http = np.arange(0, nh)
    S.kafka = np.arange(nh, nh + nk)
    S.kafka_z = np.arange(nh + 2500, nh + nk)  # the compressed and the adversarial (corrupt CRC) requests
    S.mc = np.arange(nh + nk, S.w.n)
    assert S.w.n <= 20000
    S.ref = oracle.classify_workload(S.w, 8)
    # the produce requests with compressed sets and corrupt CRCs give every verdict but UNSUPPORTED
    assert len(np.unique(S.ref[0][S.kafka_z])) >= 4
    return S


@pytest.fixture(scope="module")
def device(engine, stream):
    engine.update_policy(stream.w.policy)
    engine.set_connections(stream.w.conns)
    dev = torch.device("cuda", 0)
    return dev, torch.from_numpy(stream.w.arena).to(dev)


def _repeat(idx, n, seed):
    """n request indices: idx repeated, in a shuffled (arrival) order."""
    out = np.tile(idx, -(-n // len(idx)))[:n]
    np.random.default_rng(seed).shuffle(out)
    return out


def _upload(stream, device, idx):
    dev, _ = device
    w = stream.w
    return [torch.from_numpy(a).to(dev) for a in (w.offsets[idx].view(np.int64), w.lengths[idx].view(np.int32),
                                                  w.conn_ids[idx].view(np.int32))]


def _launch(engine, device, inputs, s):
    dev, d_arena = device
    n = inputs[0].numel()
    with torch.cuda.stream(s):  # (the outputs' fills are ordered before the call on its stream)
        o = [torch.full((n,), 7, dtype=t, device=dev) for t in (torch.uint8, torch.int32, torch.int32)]
        cnt = torch.zeros(engine.nrules + 8, dtype=torch.int64, device=dev)
        engine.classify_device(d_arena.data_ptr(), d_arena.numel(), *[t.data_ptr() for t in inputs], n,
                               *[t.data_ptr() for t in o], counters_ptr=cnt.data_ptr(), stream=s.cuda_stream)
    return o, cnt


def _check(engine, stream, idx, o, cnt):
    ref = tuple(r[idx] for r in stream.ref)
    v, r, c = o[0].cpu().numpy(), o[1].cpu().numpy(), o[2].cpu().numpy().view(np.uint32)
    bad = np.nonzero((v != ref[0]) | (r != ref[1]) | (c != ref[2]))[0]
    assert len(bad) == 0, (len(bad), bad[:8], idx[bad[:8]])
    nr = engine.nrules
    want = np.zeros(nr + 8, np.int64)
    want[:nr] = np.bincount(ref[1][ref[0] == 1], minlength=nr)[:nr]
    want[nr:nr + 5] = np.bincount(ref[0], minlength=5)[:5]
    got = cnt.cpu().numpy()
    assert (got[:nr + 5] == want[:nr + 5]).all(), np.nonzero(got[:nr + 5] != want[:nr + 5])[0][:8]


def _run(engine, stream, device, idx):
    o, cnt = _launch(engine, device, _upload(stream, device, idx), torch.cuda.current_stream())
    torch.cuda.synchronize()
    _check(engine, stream, idx, o, cnt)
    return o


@pytest.mark.parametrize("n", [BESIDE_MIN, BESIDE_MIN + 4321, BESIDE_MIN - 1],
                         ids=["2^20", "2^20+4321", "2^20-1_one_after_the_other"])
def test_sizes_around_the_threshold(engine, stream, device, n):
    _run(engine, stream, device, _repeat(np.arange(stream.w.n), n, 1))


def test_no_memcached_requests(engine, stream, device):
    """The engine serves memcached, the batch has none: the memcached kernel finds
    an empty list, and the second Kafka grid works beside the main one from the start."""
    _run(engine, stream, device, _repeat(np.concatenate([stream.http, stream.kafka]), BESIDE_MIN + 77, 2))


def test_kafka_list_shorter_than_one_sweep(engine, stream, device):
    """Fewer Kafka requests than the persistent grid's first sweep takes (its
    workgroups x 256): the second Kafka grid finds the work counter past the list's end."""
    rest = _repeat(np.concatenate([stream.http, stream.mc]), BESIDE_MIN, 3)
    idx = np.concatenate([rest, _repeat(stream.kafka, 1500, 4)])
    np.random.default_rng(5).shuffle(idx)
    _run(engine, stream, device, idx)


def test_no_kafka_requests(engine, stream, device):
    _run(engine, stream, device, _repeat(np.concatenate([stream.http, stream.mc]), BESIDE_MIN + 5, 6))


def _mixed(parts, seed):
    """(indices, count) parts, each repeated to its count, in one shuffled order."""
    idx = np.concatenate([_repeat(i, n, seed + k) for k, (i, n) in enumerate(parts)])
    np.random.default_rng(seed).shuffle(idx)
    return idx


def test_compressed_and_corrupt_produce_requests(engine, stream, device):
    """150k produce requests with gzip / snappy sets or adversarial ones (corrupt
    CRCs among them) in a Kafka list of 600k, longer than the main grid's first
    sweep: both Kafka grids append to the compressed-request list, and the
    inflate kernel, after the join, decides all of it."""
    plain = np.setdiff1d(stream.kafka, stream.kafka_z)
    idx = _mixed([(stream.kafka_z, 150_000), (plain, 450_000), (stream.mc, 200_000),
                  (stream.http, BESIDE_MIN + 999 - 800_000)], 7)
    o = _run(engine, stream, device, idx)
    z = np.isin(idx, stream.kafka_z)
    assert z.sum() == 150_000
    assert (o[0].cpu().numpy()[z] == stream.ref[0][idx[z]]).all()


def test_calls_back_to_back_on_one_and_two_streams(engine, stream, device):
    """The work counters, the lists and the side stream reused: two calls in a
    row on one stream (different batches), then the same two on two streams."""
    a = _repeat(np.arange(stream.w.n), BESIDE_MIN + 4321, 8)
    plain = np.setdiff1d(stream.kafka, stream.kafka_z)
    b = _mixed([(plain, 500_000), (stream.kafka_z, 40_000), (stream.mc, BESIDE_MIN + 1 - 540_000)], 9)
    s0, s1 = torch.cuda.current_stream(), torch.cuda.Stream()
    da, db = _upload(stream, device, a), _upload(stream, device, b)
    torch.cuda.synchronize()  # the inputs are on the device before either stream reads them
    runs = [(a, _launch(engine, device, da, s0)), (b, _launch(engine, device, db, s0)),
            (a, _launch(engine, device, da, s1)), (b, _launch(engine, device, db, s0))]
    torch.cuda.synchronize()
    for idx, (o, cnt) in runs:
        _check(engine, stream, idx, o, cnt)

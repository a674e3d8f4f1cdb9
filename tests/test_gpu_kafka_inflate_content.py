"""kafka_inflate_kernel's decoded bytes, seen through the verdict.

A produce request's verdict does not depend on what its compressed messages
hold, only on whether they decode, and a decoded message with a wrong CRC ends
its set silently: a device that decodes a byte wrong still answers ALLOW.  The
streams of tests/kafka_codec_cases.py therefore end every decoded set with a
tripwire message T (valid CRC, gzip attribute, a value that is no gzip
stream).  The walk reaches T only when every CRC before it held over the
decoded bytes, and reaching it fails the request:

    the device decoded every byte right   PARSE_ERROR
    any CRC-covered byte wrong            ALLOW (DENY on the other topic)

Each content stream comes with a twin that differs in one value byte and must
be ALLOW; tests/test_kafka_codec_streams_host.py checks all of them against
the oracle, zlib and a Python model first.  Every case here is compared bit-exact
(verdict, rule, consumed) with the oracle and with the answer written down in
kafka_codec_cases.expected.

All cases go to the device as one batch: 64 workgroups decode them, request k
on workgroup k % 64, so each workgroup decodes a large stream and then small
ones over the same region slice and history ring.
"""
import numpy as np
import pytest

from cilium_amd import gen
from cilium_amd._lib import ALLOW, PROTO_KAFKA, UNSUPPORTED

import kafka_codec_cases as kc
from test_gpu_http import assert_same, both
from test_kafka_compressed_host import policy

pytestmark = pytest.mark.gpu

BLOCKS = 64  # workgroups of kafka_inflate_kernel


def conns():
    return gen.make_conns(1, 0, 9092, True, PROTO_KAFKA, [7], 9)


def workload(reqs):
    """The requests in one arena, 0..15 bytes of junk before each."""
    parts, offs, at = [], [], 0
    for k, r in enumerate(reqs):
        gap = (5 * k + 3) % 16
        parts += [b"\xa5" * gap, r]
        offs.append(at + gap)
        at += gap + len(r)
    arena = np.frombuffer(b"".join(parts), np.uint8).copy()
    lens = np.fromiter((len(r) for r in reqs), np.uint32, len(reqs))
    return gen.Workload("t", arena, np.array(offs, np.uint64), lens, np.zeros(len(reqs), np.uint32), conns(), policy())


def ordered():
    """Positions 0..63: a large stream (>= 100 KiB) on every even one; 64..127:
    the tail-length cases, so every workgroup decodes one of them over what its
    first request left in the slice; then the rest, large and small in turn."""
    cs = kc.cases()
    tails = [c for c in cs if c.group == "tail_lengths"]
    large = [c for c in cs if c.large]
    rest = [c for c in cs if not c.large and c.group != "tail_lengths"]
    assert len(tails) == BLOCKS and len(large) >= BLOCKS // 2 and len(rest) >= BLOCKS // 2
    out = []
    for k in range(BLOCKS // 2):
        out += [large[k], rest[k]]
    out += tails
    large, rest = large[BLOCKS // 2:], rest[BLOCKS // 2:]
    while large or rest:
        if large:
            out.append(large.pop(0))
        if rest:
            out.append(rest.pop(0))
    assert len(out) == len(cs)
    return out


@pytest.fixture(scope="module")
def batch(engine, oracle):
    cs = ordered()
    w = workload([c.request for c in cs])
    got, ref = both(engine, oracle, w, 8)
    return cs, w, got, ref


def answers(res, i):
    return tuple(int(a[i]) for a in res)


def test_batch_layout():
    cs = ordered()
    w = workload([c.request for c in cs])
    assert len(cs) >= 130
    assert {c.version for c in cs} == {0, 1, 3}
    gaps = [int(w.offsets[0])] + [int(w.offsets[k] - w.offsets[k - 1] - w.lengths[k - 1]) for k in range(1, len(cs))]
    assert set(gaps) == set(range(16))
    for k, c in enumerate(cs):
        assert bytes(w.arena[int(w.offsets[k]):int(w.offsets[k]) + int(w.lengths[k])]) == c.request
    for b in range(BLOCKS):  # every workgroup decodes at least twice, half of them large first
        mine = cs[b::BLOCKS]
        assert len(mine) >= 2 and mine[1].group == "tail_lengths"
        assert b % 2 or (mine[0].large and len(mine[0].decoded or mine[0].value) >= 100 * 1024)


def test_batch_equals_oracle(batch):
    cs, w, got, ref = batch
    assert_same(got, ref, w)


@pytest.mark.parametrize("group", kc.GROUPS)
def test_content(batch, group):
    cs, w, got, ref = batch
    n = 0
    for i, c in enumerate(cs):
        if c.group != group:
            continue
        n += 1
        assert answers(got, i) == kc.expected(c), f"{c.name}: device {answers(got, i)}, oracle {answers(ref, i)}"
        assert answers(ref, i) == kc.expected(c), c.name
    assert n


def some_ordinary():
    cs = kc.cases()
    return [c for c in cs if c.group in ("deflate_hand_codes", "nested_7")] + [c for c in cs if c.group == "tail_lengths"][:8]


def test_beyond_nesting_depth(engine, oracle):
    """A compressed message inside the seventh decoded set (the request's own
    set and seven decoded ones are on the stack) is UNSUPPORTED on the device,
    decodable or not; Go has no such bound, so the oracle differs there, and
    only there."""
    deep = kc.beyond_depth()
    usual = some_ordinary()
    reqs = [c.request for c in usual]
    at = [3, 11, len(reqs) + 2]
    for i, (r, _) in zip(at, deep):
        reqs.insert(i, r)
    w = workload(reqs)
    got, ref = both(engine, oracle, w, 1)
    it = iter(usual)
    for i in range(len(reqs)):
        if i in at:
            assert answers(got, i) == (UNSUPPORTED, -1, 0), i
            assert int(ref[0][i]) == deep[at.index(i)][1]
        else:
            c = next(it)
            assert answers(got, i) == answers(ref, i) == kc.expected(c), c.name


def test_region_bound(engine, oracle):
    """Three compressions inside each other, the first two decoding to nearly
    6,553,500 bytes each.  The levels of one nesting path share the workgroup's
    16 MiB region slice: the path decodes when they total 16 MiB - 4 KiB, and
    is UNSUPPORTED (no fault) when they total more than 16 MiB, for a gzip and
    for a snappy innermost level (snappy is refused from its length header,
    gzip when the output reaches the end of the slice).

    This is the slowest test of the file by far (about 12 s on an MI355X,
    where test_size_limit takes about 5 s): one lane decodes a nesting path,
    at about 1.4 MB/s, and no three levels of at most 6,553,500 bytes each
    total more than 16 MiB with less than 16.8 MB to decode.  The levels are
    padded with zeros, not with a message, so nothing but the decode is paid."""
    fits, over = kc.REGION_BYTES - 4096, kc.REGION_BYTES + 1
    usual = some_ordinary()[:4]
    reqs = [kc.region_request(fits, False), kc.region_request(over, False), kc.region_request(fits, True),
            kc.region_request(over, True)] + [c.request for c in usual]
    w = workload(reqs)
    got, ref = both(engine, oracle, w, 8)
    assert [int(v) for v in ref[0][:4]] == [ALLOW] * 4
    for i in (0, 2):
        assert answers(got, i) == answers(ref, i) == (ALLOW, 0, len(reqs[i]))
    for i in (1, 3):
        assert answers(got, i) == (UNSUPPORTED, -1, 0)
    for i, c in enumerate(usual, 4):
        assert answers(got, i) == answers(ref, i) == kc.expected(c), c.name

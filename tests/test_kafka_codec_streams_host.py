"""The shaped streams of tests/kafka_codec_cases.py against the oracle and
zlib (no GPU): what tests/test_gpu_kafka_inflate_content.py sends to the
device is checked here first.

For every stream: the Python model's bytes equal refpy.gunzip / refpy.unsnappy
(and zlib's raw inflate for every DEFLATE body), a corrupt stream is None, and
the oracle's verdict is PARSE_ERROR for the intact stream (the tripwire
message was reached: every CRC before it held), ALLOW / DENY for its twin with
one value byte changed, PARSE_ERROR for each error case.  Nothing is skipped
or filtered: a stream that does not behave as stated fails here.
"""
import zlib

import numpy as np
import pytest

from cilium_amd import gen
from cilium_amd._lib import ALLOW, DENY, PARSE_ERROR, PROTO_KAFKA

import kafka_codec_cases as kc
import kafka_codec_streams as ks
import refpy
from test_kafka_compressed_host import policy

GROUPS = kc.GROUPS


def oracle_verdicts(reqs):
    conns = gen.make_conns(1, 0, 9092, True, PROTO_KAFKA, [7], 9)
    arena, offs, lens = gen.pack(reqs)
    return [tuple(int(x) for x in t) for t in
            zip(*refpy.Policy(policy()).classify(conns, arena, offs, lens, np.zeros(len(reqs), np.uint32)))]


def test_groups_are_all_named():
    assert sorted({c.group for c in kc.cases()}) == sorted(GROUPS)
    names = [c.name for c in kc.cases()]
    assert len(set(names)) == len(names)


def test_emitters_against_zlib_and_known_bytes():
    """The bit writer and the code tables on their own: zlib inflates what they
    write, and the snappy emitter writes the tags of the format description."""
    body, dec = ks.deflate_emit([("fixed", [b"abc", (3, 3), (258, 1, 284)])])
    assert dec == b"abcabc" + b"c" * 258 and zlib.decompress(body, -15) == dec
    body, dec = ks.deflate_emit([("dyn", ks.FLAT_LIT_LENS, ks.FLAT_DIST_LENS, [bytes(range(256)), (10, 256)])])
    assert zlib.decompress(body, -15) == dec == bytes(range(256)) + bytes(range(10))
    assert ks.deflate_emit([("stored", [b"hi"])])[0] == b"\x01\x02\x00\xfd\xffhi"
    blk, dec = ks.snappy_emit([b"abcd", ("C", 1, 4, 4), ("C", 2, 2, 1), ("C", 4, 1, 8), ("L", b"z", 4)])
    assert blk == b"\x0c" + b"\x0cabcd" + b"\x01\x04" + b"\x06\x01\x00" + b"\x03\x08\x00\x00\x00" + b"\xfc\0\0\0\0z"
    assert dec == b"abcdabcdddcz"
    assert ks.snappy_emit([b"ab", ("C", 2, 1, 3)])[1] is None


@pytest.mark.parametrize("group", GROUPS)
def test_model_equals_oracle_decoders_and_zlib(group):
    for c in (c for c in kc.cases() if c.group == group):
        got = refpy.gunzip(c.value) if c.codec == 1 else refpy.unsnappy(c.value)
        assert got == c.decoded, c.name
        for body, dec in c.bodies:
            z = zlib.decompressobj(-15)
            try:
                out = z.decompress(body)
                zok = z.eof and not z.unused_data
            except zlib.error:
                zok = False
            if dec is not None:
                assert zok and out == dec, c.name   # zlib accepts every well-formed body here
            else:
                assert not zok, c.name


@pytest.mark.parametrize("group", GROUPS)
def test_oracle_verdicts(group):
    cs = [c for c in kc.cases() if c.group == group]
    got = oracle_verdicts([c.request for c in cs])
    for c, g in zip(cs, got):
        assert g == kc.expected(c), c.name
        if c.decoded is None:
            assert c.expect == PARSE_ERROR, c.name
    # every content stream comes with the twin that shows its tripwire is what fails it
    for c in cs:
        if c.name.endswith("/twin"):
            assert c.expect in (ALLOW, DENY)
            assert any(o.name == c.name[:-5] and o.expect == PARSE_ERROR for o in cs), c.name


def test_coverage_of_the_shapes():
    """The ring positions the snappy streams claim to reach, recomputed from
    their ops; the batch's mix of sizes and versions."""
    cs = {c.name: c for c in kc.cases()}
    assert sum(c.large for c in cs.values()) >= 32 and len(cs) >= 130
    assert {c.version for c in cs.values()} == {0, 1, 3}
    W = kc.WIN
    for n in kc.SNAPPY_LENGTHS:
        c = cs[f"snappy_stations_len{n}"]
        cnt, seen = 0, set()
        for op in c.spec[1]:
            if not isinstance(op, tuple):
                cnt += kc.hlen(c.version) if op is ks.HDR else len(ks.tripwire(c.version)) if op is ks.TRIP else len(op)
                continue
            _, kind, length, offset = op
            off = cnt if offset == "base" else offset
            dst, src = (cnt // W != (cnt + length - 1) // W), ((cnt - off) // W != (cnt - off + length - 1) // W)
            if n == 1:  # one byte cannot cross: the ring's last slot instead
                dst, src = cnt % W == W - 1, (cnt - off) % W == W - 1
            seen |= {(offset, k) for k, on in (("dst", dst), ("src", src), ("neither", not (dst or src))) if on}
            if offset == "base":
                assert cnt > 2 * W and length <= 11
            else:
                assert (kind == 4) == (off >= W) and cnt > 2 * W
            cnt += length
        assert cnt == len(c.decoded)
        for offset in kc.SNAPPY_OFFSETS:
            assert (offset, "dst") in seen and (offset, "neither") in seen, (n, offset)
            assert offset == "base" or (offset, "src") in seen, (n, offset)
    tails = sorted(len(c.decoded) for c in cs.values() if c.group == "tail_lengths" and c.expect == PARSE_ERROR)
    assert tails == sorted(list(range(5008, 5024)) * 2)


def test_beyond_the_device_bounds_in_the_oracle():
    """What the oracle answers where the device says UNSUPPORTED (no bound in Go)."""
    reqs = kc.beyond_depth()
    assert [v for v, _, _ in oracle_verdicts([r for r, _ in reqs])] == [e for _, e in reqs]

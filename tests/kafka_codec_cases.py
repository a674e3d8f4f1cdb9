"""The streams of tests/test_kafka_codec_streams_host.py (oracle, zlib) and
tests/test_gpu_kafka_inflate_content.py (device), built once per process from
tests/kafka_codec_streams.py.  TEST INFRASTRUCTURE ONLY.

A case is one produce request with one compressed message and the verdict
it must get:
  content cases  decode to [message, T]: PARSE_ERROR; their twins (one value
                 byte changed): ALLOW, or DENY on the topic the policy lacks
  error cases    a corrupt stream: PARSE_ERROR (decoded is None)
Positions below are offsets into one decode output (the device's `cnt`); its
history ring holds the last 65536 bytes, so `cnt & 65535` is the ring slot.
"""
import functools
import struct
import zlib
from dataclasses import dataclass, field

import numpy as np

from cilium_amd import gen
from cilium_amd._lib import ALLOW, DENY, PARSE_ERROR

import kafka_codec_streams as ks
from kafka_codec_streams import HDR, TRIP, Mut

TOPIC, OTHER = "orders", "other"
WIN = 65536
LARGE = 100 * 1024
VERSIONS = (0, 1, 3)
SNAPPY_OFFSETS = (1, 2, 3, 4, 8, 2047, 2048, 65535, 65536, 65537, 65540, 131072, "base")
SNAPPY_LENGTHS = (1, 4, 11, 64)


@dataclass
class Case:
    name: str
    group: str
    version: int
    topic: str
    codec: int
    value: bytes            # the compressed message value
    decoded: object         # the model's bytes of the outermost stream, None: corrupt
    expect: int             # verdict
    bodies: list = field(default_factory=list)   # (DEFLATE body, model bytes or None) per gzip member
    spec: object = None     # what the stream was emitted from (content and error cases)

    @property
    def large(self):
        return max(len(self.value), len(self.decoded or b"")) >= LARGE

    @functools.cached_property
    def request(self):
        return ks.request(self.value, self.codec, self.version, self.topic)


GROUPS = ["snappy_copies", "snappy_literals", "xerial", "snappy_late_errors", "deflate_codes", "deflate_bad_symbols",
          "deflate_stored", "deflate_zlib", "deflate_hand_codes", "gzip_members", "tail_lengths", "siblings", "nested_7"]


def expected(case):
    """(verdict, rule, consumed): a request that fails is answered (PARSE_ERROR, -1, 0);
    an allowed one names the policy's one rule and consumes the whole request."""
    n = len(case.request)
    return {PARSE_ERROR: (PARSE_ERROR, -1, 0), ALLOW: (ALLOW, 0, n), DENY: (DENY, -1, n)}[case.expect]


def rnd(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def hlen(version):
    return len(gen.k_message(b"", version=version))


# ------------------------------------------------------------------ snappy
def snappy_stations(rng, h, length):
    """For every offset: a copy whose destination crosses a multiple of 65536,
    one where neither end does, and one whose source crosses the next multiple.
    Offset "base" reads the block's first bytes: the message's offset and size
    fields, which no CRC covers until the copy puts them into the value (at
    most 11 bytes, the CRC field comes next)."""
    ops, cnt, first = [HDR], h, True

    def fill_to(target):
        nonlocal cnt, first
        assert target > cnt, (target, cnt)
        d = rnd(rng, target - cnt)
        ops.append(Mut(d) if first else d)
        first, cnt = False, target

    def copy(n, offset):
        nonlocal cnt
        off = cnt if offset == "base" else offset
        ops.append(("C", 1 if 4 <= n <= 11 and off < 2048 else 2 if off < 65536 else 4, n, offset))
        cnt += n

    for offset in SNAPPY_OFFSETS:
        n = min(length, 11) if offset == "base" else length
        half = (n + 1) // 2
        B = max(3, (cnt + 1000) // WIN + 1) * WIN
        fill_to(B - half)
        copy(n, offset)                       # destination over the wrap
        fill_to(B + 30000)
        copy(n, offset)                       # neither
        if offset != "base":
            B = max(1, (cnt + 10 + half - offset) // WIN + 1) * WIN
            fill_to(B - half + offset)
            copy(n, offset)                   # source over the wrap
    fill_to(cnt + 40)
    ops.append(TRIP)
    return ("snappy", ops)


def snappy_literal_forms(rng, h):
    ops = [HDR, ("L", rnd(rng, 1), 0), ("L", rnd(rng, 60), 0), ("L", rnd(rng, 61), 1), ("L", rnd(rng, 256), 1),
           ("L", rnd(rng, 5), 1), ("L", rnd(rng, 257), 2), ("L", rnd(rng, 65536), 2), ("L", rnd(rng, 7), 2),
           ("L", Mut(rnd(rng, 70000)), 3), ("L", rnd(rng, 10), 3), ("L", rnd(rng, 1), 4), ("L", rnd(rng, 300), 4),
           ("C", 4, 64, 1), ("C", 4, 11, 5), ("C", 4, 4, 2047), ("C", 4, 1, 2), ("C", 2, 64, 3), ("C", 2, 1, 1),
           TRIP]
    return ("snappy", ops)


def xerial_chunks(rng, h, reach=0, zero_chunk=False):
    """More than 64 KiB over several chunks.  `reach` = 1 makes one copy reach
    one byte before its chunk, into bytes that are still in the ring."""
    chunks = [[HDR, Mut(rnd(rng, 30000))],
              [rnd(rng, 20000), ("C", 2, 64, "base"), rnd(rng, 100), ("C", 2, 64, 1)],
              b"\x00",
              [rnd(rng, 1)],
              [rnd(rng, 40000), ("C", 2, 64, 40000 + reach), rnd(rng, 30000), ("C", 4, 64, "base"), ("C", 1, 11, 3)],
              [rnd(rng, 50), TRIP]]
    if zero_chunk:
        chunks.insert(4, b"")
    return ("xerial", chunks)


def snappy_late_error(rng, h, kind):
    """Errors raised only after more than 64 KiB of good output (d = bytes so far)."""
    ops = [HDR, rnd(rng, 70000)]
    if kind == "offset_d_plus_1":
        return ("snappy", ops + [("C", 4, 4, h + 70001)])
    if kind == "copy_length_past_dlen":
        return ("snappy", ops + [("C", 2, 10, 5)], -1)
    if kind == "dlen_one_short":
        return ("snappy", ops + [rnd(rng, 10)], -1)
    assert kind == "dlen_one_over"
    return ("snappy", ops, 1)


# ----------------------------------------------------------------- DEFLATE
def deflate_codes(rng, h, prefix, dyn, first=None, tail=False):
    """After `prefix` bytes of output (header + random literals): every length
    code at its least and greatest extra bits, every distance code likewise
    (code 29's greatest is 32768), then matches of 258 / 3 at 32768 and 258 at
    1.  `first`: a match right after the prefix (distance = output so far)."""
    ops, cnt = [HDR, Mut(rnd(rng, prefix - h))], prefix
    if first:
        ops.append(first)
        cnt += first[0]
    for i in range(29):
        for e in sorted({0, (1 << ks.LEXT[i]) - 1}):
            ops += [(ks.LBASE[i] + e, int(rng.integers(1, min(cnt, 32768) + 1)), 257 + i), rnd(rng, 3)]
            cnt += ks.LBASE[i] + e + 3
    ops += [(258, int(rng.integers(1, 32769)), 284), rnd(rng, 2)]  # 258 as code 284, extra 31
    cnt += 260
    for i in range(30):
        for e in sorted({0, (1 << ks.DEXT[i]) - 1}):
            n = int(rng.integers(3, 40))
            ops += [(n, ks.DBASE[i] + e), rnd(rng, 2)]
            cnt += n + 2
    ops += [(258, 32768), (3, 32768), (258, 1), rnd(rng, 5)]
    cnt += 258 + 3 + 258 + 5
    if tail:  # a match whose source lies across the 64 KiB wrap
        target = WIN + 32768 - 100
        assert target > cnt
        ops += [rnd(rng, target - cnt), (258, 32768), (258, 32768 - 258), rnd(rng, 5000)]
    ops.append(TRIP)
    blk = ("dyn", ks.FLAT_LIT_LENS, ks.FLAT_DIST_LENS, ops) if dyn else ("fixed", ops)
    return ("gzip", [[blk]])


def deflate_bad_symbol(rng, h, op):
    return ("gzip", [[("fixed", [HDR, rnd(rng, 1000), op, rnd(rng, 20), TRIP])]])


def deflate_stored(rng, h):
    blocks = [("stored", [HDR]),
              ("fixed", [b"abcde"], "midbyte"),       # 3 + 40 + 7 bits: the next block starts mid-byte
              ("stored", []),
              ("stored", [rnd(rng, 1)]),
              ("stored", [Mut(rnd(rng, 65535))]),     # lies across the wrap
              ("fixed", [(258, 32768), (100, 20000), rnd(rng, 3), (3, 1), (258, 300), (64, 400), (11, 32767)]),
              ("stored", [rnd(rng, 40000)]),
              ("stored", [rnd(rng, 10), TRIP])]
    return ("gzip", [blocks])


def text(rng, n):
    words = [rnd(rng, int(k)) for k in rng.integers(2, 12, 400)]
    out = bytearray()
    while len(out) < n:
        if len(out) > 40000 and rng.integers(0, 50) == 0:
            at = int(rng.integers(0, len(out) - 300))
            out += out[at:at + int(rng.integers(3, 300))]
        out += words[int(rng.integers(0, len(words)))]
        if rng.integers(0, 8) == 0:
            out += bytes([int(rng.integers(0, 256))] * int(rng.integers(1, 40)))
    return bytes(out[:n])


def deflate_zlib(rng, h, level, strategy):
    return ("gzip", [("zlib", level, strategy, [HDR, Mut(text(rng, 150000)), TRIP])])


ALPHA = bytes(range(0x60, 0x6C))  # 12 literals, closed under xor 1


def hand_lit_lens():
    """Every code length 1..15 in one literal/length code: 1, 2, ..., 14, 15, 15."""
    lens = [0] * 286
    for k, s in enumerate(ALPHA):
        lens[s] = k + 1
    lens[257], lens[270], lens[285], lens[256] = 13, 14, 15, 15
    return lens


SINGLE_DIST = [0] * 10 + [1]  # one distance symbol (10: 33..48) with the 1-bit code 0


def deflate_hand(rng, h, missing=False):
    a = np.frombuffer(ALPHA, np.uint8)

    def alpha(n):
        return bytes(rng.choice(a, n, p=[2.0 ** -(k + 1) for k in range(11)] + [2.0 ** -11]))

    use = ("dbits", 3, 1, 1) if missing else (3, 33)   # the code 1 does not exist
    ops = [Mut(alpha(300)), use, (258, 40), alpha(20), (24, 48), (26, 33), alpha(5), (23, 47), ALPHA]
    blocks = [("stored", [HDR]),
              ("dyn", hand_lit_lens(), SINGLE_DIST, ops),
              ("dyn", ks.LITERAL_ONLY_LENS, [0], [rnd(rng, 300)]),   # no distance code at all
              ("fixed", [TRIP])]
    return ("gzip", [blocks])


def deflate_two_members(rng, h, reach=0):
    """The second member starts after more than 64 KiB of output; its first
    match reaches its own first byte (reach = 1: one byte of the member before)."""
    return ("gzip", [[("fixed", [HDR, Mut(rnd(rng, 66000))])],
                     [("fixed", [rnd(rng, 5), (258, 5 + reach), rnd(rng, 10), (30, 273), TRIP])]])


# ----------------------------------------------------------------- nesting
def comp(inner, codec, version=0):
    """`inner` (a message set) as one compressed message."""
    if codec == 1:
        m = ("zlib", 1, 0, [inner]) if len(inner) > 20000 else [("fixed", [inner])]
        value = ks.gzip_emit([m])[0]
    else:
        value = gen.snappy_block(inner)
    return gen.k_message(value, version=version, attributes=codec)


def flip(msg, back=3):
    """A message with one value byte changed after its CRC was computed."""
    b = bytearray(msg)
    b[-back] ^= 1
    return bytes(b)


def nested(rng, version, levels, trip_at, damaged=False, trip=None):
    """`levels` compressions inside each other, codecs alternating.  Level 0 is
    the request's own set; the set of level l (1 <= l < levels) holds the next
    compression and a plain message after it; the innermost set (level
    `levels`) one plain message.  The tripwire ends level `trip_at` (None:
    nowhere); `damaged` spoils the message before it.  Returns (the codec of
    the outermost compression, the set of level 1)."""
    T = ks.tripwire(version) if trip is None else trip
    plain = gen.k_message(rnd(rng, 50), version=version)
    s = (flip(plain) if damaged and trip_at == levels else plain) + (T if trip_at == levels else b"")
    for l in range(levels - 1, 0, -1):
        plain = gen.k_message(rnd(rng, 30), version=version)
        s = comp(s, 1 + (l & 1), version) + (flip(plain) if damaged and trip_at == l else plain) \
            + (T if trip_at == l else b"")
    return 1, s


@functools.lru_cache(None)
def cases():
    out = []
    count = [0]

    def version():
        count[0] += 1
        return VERSIONS[count[0] % 3]

    def content(group, name, build, with_twin=True):
        v = version()
        rng = np.random.default_rng(abs(hash_name(name)))
        spec = build(rng, hlen(v))
        codec, value, dec, bodies = ks.emit_set(spec, v)
        assert dec is not None, name
        out.append(Case(name, group, v, TOPIC, codec, value, dec, PARSE_ERROR, bodies, spec))
        if with_twin:
            codec, value, dec2, bodies = ks.emit(ks.twin(spec), _env(v, dec))
            assert dec2 is not None and len(dec2) == len(dec)
            assert dec2 != dec  # the changed byte, and whatever copies it
            topic = OTHER if count[0] % 4 == 0 else TOPIC
            out.append(Case(name + "/twin", group, v, topic, codec, value, dec2, DENY if topic == OTHER else ALLOW,
                            bodies))

    def error(group, name, build):
        v = version()
        rng = np.random.default_rng(abs(hash_name(name)))
        codec, value, dec, bodies = ks.emit_set(build(rng, hlen(v)), v)
        assert dec is None, name
        out.append(Case(name, group, v, TOPIC, codec, value, None, PARSE_ERROR, bodies))

    def raw_set(group, name, v, codec_set, expect):
        codec, s = codec_set
        out.append(Case(name, group, v, TOPIC, codec, m_value(comp(s, codec, v), v), s, expect))

    # --- snappy
    for n in SNAPPY_LENGTHS:
        content("snappy_copies", f"snappy_stations_len{n}", lambda r, h, n=n: snappy_stations(r, h, n))
    content("snappy_literals", "snappy_literal_forms", snappy_literal_forms)
    content("xerial", "xerial_chunks", xerial_chunks)
    error("xerial", "xerial_copy_into_previous_chunk", lambda r, h: xerial_chunks(r, h, reach=1))
    error("xerial", "xerial_zero_length_chunk", lambda r, h: xerial_chunks(r, h, zero_chunk=True))
    for kind in ("offset_d_plus_1", "copy_length_past_dlen", "dlen_one_short", "dlen_one_over"):
        error("snappy_late_errors", f"snappy_{kind}", lambda r, h, k=kind: snappy_late_error(r, h, k))

    # --- DEFLATE / gzip
    for dyn in (False, True):
        kind = "dynamic" if dyn else "fixed"
        # prefix 32768: the first match's distance is all the output so far
        content("deflate_codes", f"deflate_codes_{kind}_after_32k",
                lambda r, h, d=dyn: deflate_codes(r, h, 32768, d, first=(3, 32768)))
        content("deflate_codes", f"deflate_codes_{kind}_over_64k_mark",
                lambda r, h, d=dyn: deflate_codes(r, h, WIN - 300, d))
        content("deflate_codes", f"deflate_codes_{kind}_after_72k",
                lambda r, h, d=dyn: deflate_codes(r, h, 72000, d, tail=True))
        error("deflate_codes", f"deflate_{kind}_distance_one_past_output",
              lambda r, h, d=dyn: deflate_codes(r, h, 32767, d, first=(3, 32768)))
    for nm, op in (("litlen_286", ("sym", 286)), ("litlen_287", ("sym", 287)),
                   ("dist_30", ("dsym", 5, 30)), ("dist_31", ("dsym", 5, 31))):
        error("deflate_bad_symbols", f"deflate_{nm}", lambda r, h, op=op: deflate_bad_symbol(r, h, op))
    content("deflate_stored", "deflate_stored_blocks", deflate_stored)
    for nm, level, strategy in (("level1", 1, 0), ("level6", 6, 0), ("level9", 9, 0), ("fixed", 6, zlib.Z_FIXED),
                                ("rle", 6, zlib.Z_RLE)):
        content("deflate_zlib", f"deflate_zlib_{nm}", lambda r, h, l=level, s=strategy: deflate_zlib(r, h, l, s))
    content("deflate_hand_codes", "deflate_hand_codes", deflate_hand)
    error("deflate_hand_codes", "deflate_missing_distance_code", lambda r, h: deflate_hand(r, h, missing=True))
    error("deflate_hand_codes", "deflate_nlit_287", lambda r, h: ("gzip", [[("stored", [HDR]), ("dynhdr", 287, 30)]]))
    error("deflate_hand_codes", "deflate_ndist_31", lambda r, h: ("gzip", [[("stored", [HDR]), ("dynhdr", 286, 31)]]))
    content("gzip_members", "gzip_second_member_own_first_byte", deflate_two_members)
    error("gzip_members", "gzip_second_member_into_previous", lambda r, h: deflate_two_members(r, h, reach=1))

    # --- nesting and the region stack
    # decoded lengths L .. L+15 with T last: T's end lies in the partly filled
    # dword and in the last 16-byte chunk, above what an earlier, larger
    # request of the same workgroup left in the slice
    L = 5008
    for codec in (1, 2):
        for i in range(16):
            v = version()
            rng = np.random.default_rng(7000 + 16 * codec + i)
            T = ks.tripwire(v)
            msg = gen.k_message(rnd(rng, L + i - hlen(v) - len(T)), version=v)
            assert len(msg + T) == L + i
            name = f"tail_len_{L + i}_codec{codec}"
            raw_set("tail_lengths", name, v, (codec, msg + T), PARSE_ERROR)
            raw_set("tail_lengths", name + "/twin", v, (codec, flip(msg, 100) + T), ALLOW)
    # two compressed siblings in one parent: the second decodes over the first one's bytes
    for k, (c0, c1, c2) in enumerate(((1, 2, 1), (2, 1, 2))):
        v = version()
        rng = np.random.default_rng(7100 + k)
        T = ks.tripwire(v)
        big = b"".join(gen.k_message(rnd(rng, 25 * 1024), version=v) for _ in range(4))
        small = gen.k_message(rnd(rng, 200), version=v)
        after = gen.k_message(b"between", version=v)
        raw_set("siblings", f"siblings_trip_in_parent_{k}", v, (c0, comp(big, c1, v) + comp(small, c2, v) + after + T),
                PARSE_ERROR)
        raw_set("siblings", f"siblings_trip_in_parent_{k}/twin", v,
                (c0, comp(big, c1, v) + comp(small, c2, v) + flip(after) + T), ALLOW)
        raw_set("siblings", f"siblings_trip_in_second_{k}", v,
                (c0, comp(big, c1, v) + comp(small + T, c2, v) + after), PARSE_ERROR)
        raw_set("siblings", f"siblings_trip_in_second_{k}/twin", v,
                (c0, comp(big, c1, v) + comp(flip(small) + T, c2, v) + after), ALLOW)
    # seven compressions inside each other: the device's stack takes the request's own set
    # and seven decoded ones.  T at each level in turn, after the nested message, so the
    # parent's walk has to resume after the pop.  T is itself a compressed message, so in the
    # innermost set it would be an eighth compression: there the plain tripwire stands in.
    for at in range(1, 8):
        for damaged in (False, True):
            v = version()
            rng = np.random.default_rng(7200 + at)
            trip = ks.tripwire_plain(v) if at == 7 else None
            raw_set("nested_7", f"nested_7_trip_at_{at}" + ("/twin" if damaged else ""), v,
                    nested(rng, v, 7, at, damaged, trip), ALLOW if damaged else PARSE_ERROR)
    return out


def beyond_depth(version=0):
    """Requests with a compressed message in the seventh decoded set, one more
    level than the device's stack takes: eight compressions well-formed, eight
    with T innermost, and seven whose innermost set ends with T (T is a gzip
    message, so an eighth compression that Go would fail to decode).
    [(request, the oracle's verdict)]"""
    res = []
    for k, (levels, at) in enumerate(((8, None), (8, 8), (7, 7))):
        codec, s = nested(np.random.default_rng(7300 + k), version, levels, at)
        req = ks.request(m_value(comp(s, codec, version), version), codec, version, TOPIC)
        res.append((req, ALLOW if at is None else PARSE_ERROR))
    return res


def m_value(msg, version):
    """The value bytes of a message built by gen.k_message with no key."""
    h = hlen(version)
    n = struct.unpack(">i", msg[h - 4:h])[0]
    assert h + n == len(msg)
    return msg[h:]


def hash_name(name):
    return zlib.crc32(name.encode())


def _env(version, dec):
    return {HDR: dec[:hlen(version)], TRIP: ks.tripwire(version)}


# ------------------------------------------------------------ region bound
REGION_BYTES = 16 << 20
LEVEL_BYTES = 6_553_488  # a multiple of 16 just under the 6,553,500 readMessageSet accepts


def region_request(total, snappy_last, version=0):
    """Three compressions inside each other, constant bytes: the first two
    decode to LEVEL_BYTES each, the three to `total` together."""
    def padded(child, n):  # a set of exactly n bytes: the child, then zeros (size 0: the set ends there)
        return child + bytes(n - len(child))

    def gz(s):
        return gen.k_message(ks.gzip_emit([("zlib", 1, 0, [s])])[0], version=version, attributes=1)

    n3 = total - 2 * LEVEL_BYTES
    s3 = padded(gen.k_message(b"innermost", version=version), n3)
    m3 = gen.k_message(ks.snappy_emit([("L", s3, 4)])[0], version=version, attributes=2) if snappy_last else gz(s3)
    m2 = gz(padded(m3, LEVEL_BYTES))
    m1 = gz(padded(m2, LEVEL_BYTES))
    return gen.k_produce(version, 1, "c", [(TOPIC, [(0, [m1])])])

"""Snappy and DEFLATE / gzip streams of chosen shape for the Kafka decode tests.

TEST INFRASTRUCTURE ONLY.  The encoders here write exactly the tags, blocks and
codes an op list names (forced literal forms, forced length codes, hand-made
Huffman codes), and the decoded bytes come from a few lines of Python that
apply the same ops (`_copy` below), never from the oracle or the device.

The verdict of a produce request does not depend on what its compressed
messages hold, only on whether they decode; a decoded message whose CRC is
wrong ends the set silently (messages.go readMessageSet).  So every decoded
set built here ends with a *tripwire* message T: valid CRC, attributes = 1
(gzip), and a value that is no gzip stream.  The walk reaches T only if every
message before it verified its CRC over the decoded bytes, and reaching it
fails the request:

    every decoded byte right  -> PARSE_ERROR
    any CRC-covered byte wrong -> ALLOW (DENY on a topic the policy lacks)

A message's 8-byte offset field is covered by no CRC; streams that want those
bytes checked copy them into the value with a back-reference.

Each stream has a *twin*: the same ops with one byte of the literal marked
`Mut` changed.  A gzip trailer is computed over the model's (changed) bytes,
so only the message CRC can notice.  The twin's verdict (ALLOW) shows the
stream's PARSE_ERROR really comes from T.
"""
import struct
import zlib

import numpy as np

from cilium_amd import gen


class _Mark:
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return self.name


HDR = _Mark("HDR")    # the big message's header bytes (offset .. value length)
TRIP = _Mark("TRIP")  # the tripwire message


class Mut(bytes):
    """A literal of the value; the twin changes its middle byte (xor 1)."""


def _res(x, env):
    return env[x] if isinstance(x, _Mark) else bytes(x)


def _copy(out, base, length, dist):
    """The decoders' back-reference, byte by byte: False if it reaches before
    `base` (the block's / member's first byte)."""
    if dist == 0 or dist > len(out) - base:
        return False
    for _ in range(length):
        out.append(out[-dist])
    return True


# ------------------------------------------------------------------ snappy
def uvarint(v):
    b = bytearray()
    while True:
        b.append((v & 0x7F) | (0x80 if v >> 7 else 0))
        v >>= 7
        if not v:
            return bytes(b)


def snappy_emit(ops, env=None, dlen_delta=0):
    """ops: a literal (bytes / HDR / TRIP / Mut) in its shortest form,
    ("L", literal, form) with form 0 (inline, 1..60 bytes) or 1..4 (that many
    length bytes, non-minimal allowed), or ("C", kind, length, offset) with
    kind 1 (length 4..11, offset < 2048), 2 or 4 (length 1..64); offset "base"
    is the distance back to the block's first byte.  The block's length header
    is the model's length plus dlen_delta.  Returns (block, decoded or None)."""
    enc, out, ok = bytearray(), bytearray(), True
    for op in ops:
        if not isinstance(op, tuple):
            op = ("L", op, None)
        if op[0] == "L":
            data, form = _res(op[1], env), op[2]
            n = len(data) - 1
            assert n >= 0
            if form is None:
                form = 0 if n < 60 else 1 if n < 1 << 8 else 2 if n < 1 << 16 else 3 if n < 1 << 24 else 4
            if form == 0:
                assert n < 60
                enc.append(n << 2)
            else:
                enc.append((59 + form) << 2)
                enc += n.to_bytes(form, "little")
            enc += data
            out += data
            continue
        _, kind, length, offset = op
        if offset == "base":
            offset = len(out)
        if kind == 1:
            assert 4 <= length <= 11 and offset < 2048
            enc += bytes([1 | (length - 4) << 2 | (offset >> 8) << 5, offset & 255])
        elif kind == 2:
            assert 1 <= length <= 64 and offset < 65536
            enc += bytes([2 | (length - 1) << 2]) + struct.pack("<H", offset)
        else:
            assert kind == 4 and 1 <= length <= 64
            enc += bytes([3 | (length - 1) << 2]) + struct.pack("<I", offset)
        ok = ok and _copy(out, 0, length, offset)
    block = uvarint(len(out) + dlen_delta) + bytes(enc)
    return block, bytes(out) if ok and dlen_delta == 0 else None


XERIAL_MAGIC = b"\x82SNAPPY\x00" + struct.pack(">ii", 1, 1)


def xerial_emit(chunks, env=None):
    """snappy-java framing around chunks: each an op list (a block of its own,
    so a copy cannot reach before the chunk's first byte) or raw chunk bytes."""
    enc, out, ok = bytearray(XERIAL_MAGIC), bytearray(), True
    for ch in chunks:
        if isinstance(ch, (bytes, bytearray)):
            blk, dec = bytes(ch), (b"" if bytes(ch) == b"\x00" else None)
        else:
            blk, dec = snappy_emit(ch, env)
        enc += struct.pack(">i", len(blk)) + blk
        if dec is None:
            ok = False
        else:
            out += dec
    return bytes(enc), bytes(out) if ok else None


# ----------------------------------------------------------------- DEFLATE
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class Bits:
    """LSB-first bit writer (RFC 1951 3.1.1): (value, width) pairs, packed once."""

    def __init__(self):
        self.v, self.n, self.total = [], [], 0

    def put(self, val, nbits):
        assert 0 <= val < (1 << nbits) or nbits == 0
        if nbits:
            self.v.append(val)
            self.n.append(nbits)
            self.total += nbits

    def many(self, vals, widths):
        self.v.extend(vals.tolist())
        self.n.extend(widths.tolist())
        self.total += int(widths.sum())

    def align(self):
        self.put(0, -self.total % 8)

    def data(self, b):
        assert self.total % 8 == 0
        self.v.extend(b)
        self.n.extend([8] * len(b))
        self.total += 8 * len(b)

    def done(self):
        self.align()
        if not self.v:
            return b""
        v, n = np.array(self.v, np.uint32), np.array(self.n, np.int64)
        idx = np.repeat(np.arange(len(n)), n)
        k = np.arange(int(n.sum())) - (np.cumsum(n) - n)[idx]
        return np.packbits(((v[idx] >> k.astype(np.uint32)) & 1).astype(np.uint8), bitorder="little").tobytes()


def canon(lengths):
    """Canonical Huffman codes (RFC 1951 3.2.2) as (bit-reversed code, width)
    arrays, ready for the LSB-first writer; width 0 = no code."""
    lengths = np.asarray(lengths, np.int64)
    code, nxt = 0, [0] * 17
    for l in range(1, 16):
        code = (code + int((lengths == l - 1).sum() if l > 1 else 0)) << 1
        nxt[l] = code
    vals = np.zeros(len(lengths), np.uint32)
    for i, l in enumerate(lengths.tolist()):
        if l:
            vals[i] = int(format(nxt[l], "0%db" % l)[::-1], 2)
            nxt[l] += 1
    return vals, lengths


FIXED_LIT = canon([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canon([5] * 32)
# complete codes over every symbol: 286 literal/length symbols, 30 distances
FLAT_LIT_LENS = [9] * 256 + [5] * 2 + [6] * 28
FLAT_DIST_LENS = [4] * 2 + [5] * 28
# literals only: no length codes, a distance "code" with no symbol
LITERAL_ONLY_LENS = [9] * 256 + [1]


def _len_code(length, lcode=None):
    if lcode is None:
        lcode = 257 + max(i for i in range(29) if LBASE[i] <= length)
    i = lcode - 257
    e = length - LBASE[i]
    assert 0 <= e < (1 << LEXT[i]) or (e == 0 and LEXT[i] == 0), (length, lcode)
    return lcode, e, LEXT[i]


def _dist_code(dist):
    i = max(i for i in range(30) if DBASE[i] <= dist)
    return i, dist - DBASE[i], DEXT[i]


def _huff_ops(bw, ops, lit, dist, out, env):
    """ops: literal bytes; (length, dist[, length code]); ("sym", s) a raw
    literal/length symbol (286, 287: corrupt); ("dsym", length, code) a raw
    distance symbol (30, 31: corrupt); ("dbits", length, value, width) raw
    bits where the distance code goes.  Ends with the end-of-block symbol."""
    ok = True

    def sym(table, s):
        assert table[1][s], ("no code for symbol", s)
        bw.put(int(table[0][s]), int(table[1][s]))

    for op in ops:
        if not isinstance(op, tuple):
            a = np.frombuffer(_res(op, env), np.uint8)
            assert (lit[1][a] > 0).all()
            bw.many(lit[0][a], lit[1][a])
            out += a.tobytes()
        elif op[0] == "sym":
            sym(lit, op[1])
            ok = False
        elif op[0] in ("dsym", "dbits"):
            lc, e, eb = _len_code(op[1])
            sym(lit, lc)
            bw.put(e, eb)
            if op[0] == "dsym":
                sym(dist, op[2])
            else:
                bw.put(op[2], op[3])
            ok = False
        else:
            lc, e, eb = _len_code(op[0], op[2] if len(op) > 2 else None)
            sym(lit, lc)
            bw.put(e, eb)
            dc, e, eb = _dist_code(op[1])
            sym(dist, dc)
            bw.put(e, eb)
            ok = ok and _copy(out, 0, op[0], op[1])
    sym(lit, 256)
    return ok


def deflate_emit(blocks, env=None):
    """blocks, the last one final:
      ("stored", [literal, ...])
      ("fixed", ops[, "midbyte"])         "midbyte": must not end on a byte boundary
      ("dyn", lit lengths, dist lengths, ops)   header: 19 code-length codes, symbols
                                          0..15 as 4-bit codes, 16..18 unused
      ("dynhdr", nlit, ndist)             only the counts (286 < nlit or 30 < ndist: corrupt)
    Returns (body, decoded or None)."""
    bw, out, ok = Bits(), bytearray(), True
    for bi, blk in enumerate(blocks):
        bw.put(1 if bi == len(blocks) - 1 else 0, 1)
        if blk[0] == "stored":
            data = b"".join(_res(p, env) for p in blk[1])
            assert len(data) <= 65535
            bw.put(0, 2)
            bw.align()
            bw.data(struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data)
            out += data
        elif blk[0] == "fixed":
            bw.put(1, 2)
            ok = _huff_ops(bw, blk[1], FIXED_LIT, FIXED_DIST, out, env) and ok
            if len(blk) > 2:
                assert blk[2] == "midbyte" and bw.total % 8 != 0
        elif blk[0] == "dyn":
            ll, dl = list(blk[1]), list(blk[2])
            bw.put(2, 2)
            bw.put(len(ll) - 257, 5)
            bw.put(len(dl) - 1, 5)
            bw.put(15, 4)
            for s in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
                bw.put(4 if s < 16 else 0, 3)
            for l in ll + dl:
                bw.put(int(format(l, "04b")[::-1], 2), 4)
            ok = _huff_ops(bw, blk[3], canon(ll), canon(dl), out, env) and ok
        else:
            assert blk[0] == "dynhdr"
            bw.put(2, 2)
            bw.put(blk[1] - 257, 5)
            bw.put(blk[2] - 1, 5)
            bw.put(15, 4)
            ok = False
    return bw.done(), bytes(out) if ok else None


GZ_HEADER = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF])


def gzip_emit(members, env=None):
    """members: block lists, or ("zlib", level, strategy, [literal, ...]) for a
    body made by zlib.  Each trailer holds the CRC and length of the model's
    bytes for that member.  Returns (stream, decoded or None, bodies)."""
    enc, out, ok, bodies = bytearray(), bytearray(), True, []
    for m in members:
        if isinstance(m, tuple) and m[0] == "zlib":
            dec = b"".join(_res(p, env) for p in m[3])
            c = zlib.compressobj(m[1], zlib.DEFLATED, -15, 9, m[2])
            body = c.compress(dec) + c.flush()
        else:
            body, dec = deflate_emit(m, env)
        bodies.append((body, dec))
        if dec is None:
            ok, dec = False, b""
        enc += GZ_HEADER + body + struct.pack("<II", zlib.crc32(dec) & 0xFFFFFFFF, len(dec))
        out += dec
    return bytes(enc), bytes(out) if ok else None, bodies


# ---------------------------------------------------------------- wrapping
def tripwire(version=0):
    return gen.k_message(b"\x1f\x8b\x08\0garbage", version=version, attributes=1)


def tripwire_plain(version=0):
    """A plain message, valid CRC, whose key length runs past its end: an error
    in readMessageSet wherever the walk reaches it.  For the innermost set of
    the deepest nesting, where T would be one compression too many."""
    body = struct.pack(">bb", 1 if version >= 1 else 0, 0) + (bytes(8) if version >= 1 else b"") + struct.pack(">i", 100)
    msg = struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF) + body
    return struct.pack(">qi", 0, len(msg)) + msg


def emit(spec, env=None):
    """spec: ("snappy", ops[, dlen_delta]) | ("xerial", chunks) | ("gzip", members).
    Returns (codec, value, decoded or None, DEFLATE bodies)."""
    if spec[0] == "snappy":
        return (2,) + snappy_emit(spec[1], env, *spec[2:]) + ([],)
    if spec[0] == "xerial":
        return (2,) + xerial_emit(spec[1], env) + ([],)
    assert spec[0] == "gzip"
    return (1,) + gzip_emit(spec[1], env)


def emit_set(spec, version=0):
    """The spec's HDR and TRIP filled in so that it decodes to one message
    (header HDR, value = everything between) followed by T.  The value comes
    from a first pass with a blank header, and its CRC from those model bytes;
    a value that copies CRC-covered header bytes cannot be built (asserted)."""
    T = tripwire(version)
    h = len(gen.k_message(b"", version=version))
    env = {HDR: bytes(h), TRIP: T}
    out = emit(spec, env)
    for _ in range(3):  # a value may copy the header's offset / size bytes: settle
        dec = out[2]
        if dec is None:
            return out
        assert dec[:h] == env[HDR] and dec.endswith(T) and len(dec) >= h + len(T)
        msg = gen.k_message(dec[h:len(dec) - len(T)], version=version)
        if dec == msg + T:
            return out
        env[HDR] = msg[:h]
        out = emit(spec, env)
    raise AssertionError("the value depends on CRC-covered header bytes")


def twin(spec):
    """The same spec with the middle byte of its first Mut literal changed."""
    done = []

    def walk(x):
        if isinstance(x, Mut) and not done:
            b = bytearray(x)
            b[len(b) // 2] ^= 1
            done.append(1)
            return bytes(b)
        if isinstance(x, (list, tuple)) and not isinstance(x, _Mark):
            return type(x)(walk(y) for y in x)
        return x

    t = walk(spec)
    assert done, "no Mut literal in the spec"
    return t


def request(value, codec, version=0, topic="orders"):
    """A produce request whose one message carries `value` with that codec."""
    return gen.k_produce(version, 1, "c", [(topic, [(0, [gen.k_message(value, version=version, attributes=codec)])])])

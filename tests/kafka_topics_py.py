"""Where a Kafka request's topic names lie (test helper): a position-only
Python restatement of oracle/kafka_ref.c's read_body and read_message_set, the
decode path the access-log records are checked against.

It follows the oracle's reads step by step (io.ReadFull / LimitReader
semantics, message sets that stop without draining after a bad CRC, a message
of four bytes or fewer, or codec 3), so the byte at which each later topic
starts is the one the reference's decoder reaches.  It needs zlib.crc32 but no
inflate: a compressed set that fails to decode makes the whole request a
PARSE_ERROR, which the verdict reports anyway.  tests/test_kafka_topics_py.py
pins it to the oracle.

parse(buf) returns None where the reference answers neither ALLOW nor DENY for
a reason this helper can see (framing, decode error), else a dict: api_key,
api_version, correlation_id, typed (0 nil request, 1 typed, 2
ConsumerMetadata), topics_nil and topics, the (offset, length) spans of
GetTopics() in wire order, offsets from the request's first byte, an empty name
as (0, 0).
"""
import zlib

MAX_PARSE_BUF = 6553500


class _Buf:
    def __init__(self, b, pos, end):
        self.b, self.pos, self.end = b, pos, end


class _Dec:
    """oracle kdec: a decoder over a shared buffer position, with a LimitReader."""

    def __init__(self, buf, limit=-1):
        self.r, self.limit, self.err = buf, limit, 0

    def read(self, n):
        r = self.r
        at = r.pos
        if n == 0:
            return at
        avail = r.end - r.pos
        if 0 <= self.limit < avail:
            avail = self.limit
        if avail == 0:
            self.err = 1
            return at
        take = min(avail, n)
        r.pos += take
        if self.limit >= 0:
            self.limit -= take
        if take < n:
            self.err = 2
        return at

    def int(self, n):
        if self.err:
            return 0
        at = self.read(n)
        if self.err:
            return 0
        return int.from_bytes(self.r.b[at:at + n], "big", signed=True)

    def string(self):
        if self.err:
            return 0, 0
        sl = self.int(2)
        if self.err or sl < 1:
            return 0, 0
        at = self.read(sl)
        if self.err:
            return 0, 0
        return at, sl

    def arraylen(self, nullable):
        """(length or -1 for a null array, bad)"""
        n = self.int(4)
        if n < 0:
            return (-1, False) if nullable else (0, True)
        if n > MAX_PARSE_BUF:
            return 0, True
        return n, False

    def bytes(self):
        if self.err:
            return
        sl = self.int(4)
        if self.err or sl < 1:
            return
        if sl > MAX_PARSE_BUF:
            self.err = 3
            return
        self.read(sl)


def _message_set(buf, size, version):
    """readMessageSet on the shared position; 0 ok, -1 error."""
    if size < 0:
        return 0
    if size > MAX_PARSE_BUF:
        return -1
    dec = _Dec(buf, size)
    while True:
        dec.int(8)
        if dec.err:
            return 0
        msize = dec.int(4)
        if dec.err or msize <= 0:
            return 0
        if msize > MAX_PARSE_BUF:
            return -1
        at = dec.read(msize)
        if dec.err:
            return 0
        md = _Dec(_Buf(buf.b, at, at + msize))
        crc = md.int(4) & 0xFFFFFFFF
        if msize <= 4:
            return 0
        if crc != zlib.crc32(buf.b[at + 4:at + msize]):
            return 0  # stop, no drain
        md.int(1)
        attr = md.int(1)
        if version >= 1:
            md.int(8)
        if attr & 3 == 3:
            return 0
        md.bytes()
        md.bytes()
        if md.err:
            return -1
        # (codec 1 / 2: the inner set is decoded by the oracle; its failure is a PARSE_ERROR)


def _read_body(kind, raw, rawlen, topics):
    """The typed decoders; 0 ok, -1 error, and whether the topic array was null."""
    buf = _Buf(raw, 0, rawlen)
    d = _Dec(buf)
    nil = False
    d.int(4)
    d.int(2)
    ver = d.int(2)
    d.int(4)
    d.string()
    if kind == 0:
        if ver >= 3:
            d.string()
        d.int(2)
        d.int(4)
        nt, bad = d.arraylen(False)
        if bad:
            return -1, nil
        for _ in range(nt):
            t = d.string()
            if d.err:
                break
            topics.append(t)
            np_, bad = d.arraylen(False)
            if bad:
                return -1, nil
            for _ in range(np_):
                d.int(4)
                if d.err:
                    return -1, nil
                ss = d.int(4)
                if d.err:
                    return -1, nil
                if _message_set(buf, ss, ver):
                    return -1, nil
    elif kind in (1, 2, 8, 9):
        if kind == 1:
            d.int(4), d.int(4), d.int(4)
            if ver >= 3:
                d.int(4)
            if ver >= 4:
                d.int(1)
        elif kind == 2:
            d.int(4)
            if ver >= 2:
                d.int(1)
        elif kind == 8:
            d.string()
            if ver >= 1:
                d.int(4)
                d.string()
            if ver >= 2:
                d.int(8)
        else:
            d.string()
        nt, bad = d.arraylen(kind == 9)
        if bad:
            return -1, nil
        nil = nt < 0
        for _ in range(max(nt, 0)):
            topics.append(d.string())
            np_, bad = d.arraylen(False)
            if bad:
                return -1, nil
            for _ in range(np_):
                if kind == 1:
                    d.int(4), d.int(8)
                    if ver >= 5:
                        d.int(8)
                    d.int(4)
                elif kind == 2:
                    d.int(4), d.int(8)
                    if ver == 0:
                        d.int(4)
                elif kind == 8:
                    d.int(4), d.int(8)
                    if ver == 1:
                        d.int(8)
                    d.string()
                else:
                    d.int(4)
                if d.err:
                    break
            if d.err:
                break
    elif kind == 3:
        nt, bad = d.arraylen(True)
        if bad:
            return -1, nil
        nil = nt < 0
        for _ in range(max(nt, 0)):
            topics.append(d.string())
            if d.err:
                break
        if ver >= 4:
            d.int(1)
    elif kind == 10:
        d.string()
        if ver >= 1:
            d.int(1)
    return (-1 if d.err else 0), nil


def parse(buf):
    buf = bytes(buf)
    n = len(buf)
    if n < 4:
        return None
    size = int.from_bytes(buf[0:4], "big", signed=True)
    if size <= 0 or n < 6 or size + 4 > MAX_PARSE_BUF:
        return None
    rawlen = size + 4
    if rawlen > n or rawlen < 12:
        return None
    kind = int.from_bytes(buf[4:6], "big", signed=True)
    typed = 1 if kind in (0, 1, 2, 3, 8, 9) else 2 if kind == 10 else 0
    topics, nil = [], False
    if typed:
        e, nil = _read_body(kind, buf, rawlen, topics)
        if e:
            return None
    if typed != 1:
        topics = []  # GetTopics(): nil for ConsumerMetadata and a nil request
    return {"api_key": kind, "api_version": int.from_bytes(buf[6:8], "big", signed=True),
            "correlation_id": int.from_bytes(buf[8:12], "big", signed=True), "typed": typed, "topics_nil": nil,
            "topics": topics, "rawlen": rawlen}

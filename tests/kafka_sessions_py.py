"""A Python restatement of the reference's Kafka correlation cache
(pkg/kafka/correlation_cache.go:116-178, the collector of :180-213 with an
explicit clock): one dict per connection plus its next sequence number.  The
yardstick of the device sessions (l7g_kafka_forward / l7g_kafka_responses);
tests/test_kafka_sessions_host.py pins it to the host cache
(_lib.KafkaCorrelationCache), connection by connection."""
import numpy as np

ALLOW = 1
PROTO_KAFKA = 2


def be(b):
    return int.from_bytes(b, "big")


class Cache:
    """One connection's CorrelationCache."""

    def __init__(self):
        self.next = 1   # nextSequenceNumber (:100)
        self.cache = {}  # new id -> (orig id, api key, api version, tag, created)

    def handle_request(self, frame, tag=0, now_ms=0, dropped=False):
        """HandleRequest (:120-147) on a mutable frame (bytearray); returns the
        new id.  dropped: the device table had no slot -- the number is spent,
        the bytes stay, nothing is cached."""
        orig = be(frame[8:12]) if len(frame) >= 12 else 0   # request.go:57-63
        new = self.next
        self.next = (self.next + 1) & 0xFFFFFFFF
        if dropped:
            return new
        if len(frame) >= 12:                                  # request.go:66-70
            frame[8:12] = new.to_bytes(4, "big")
        key = be(frame[4:6]) if len(frame) >= 6 else 0
        ver = be(frame[6:8]) if len(frame) >= 8 else 0
        self.cache[new] = (orig, key - (key >> 15 << 16), ver - (ver >> 15 << 16), int(tag), int(now_ms))
        return new

    def correlate_response(self, frame):
        """CorrelateResponse (:161-178) on a mutable frame; the entry or None."""
        cid = be(frame[4:8]) if len(frame) >= 8 else 0       # response.go:33-39
        ent = self.cache.pop(cid, None)
        if ent is not None and len(frame) >= 8:               # response.go:42-46
            frame[4:8] = ent[0].to_bytes(4, "big")
        return ent

    def gc(self, now_ms, lifetime_ms):
        """The collector's pass (:190-205) at now_ms: entries created at or
        before now - lifetime go (the <= cutoff of l7g_kafka_corr_gc)."""
        old = [k for k, v in self.cache.items() if now_ms - v[4] >= lifetime_ms]
        for k in old:
            del self.cache[k]
        return len(old)


class Sessions:
    """The caches of a connection table, driven by batches as the device calls are."""

    STATS = ("live", "dropped", "forwarded", "found", "missed", "expired")

    def __init__(self, conns):
        self.set_connections(conns)
        self.counts = dict.fromkeys(self.STATS[1:], 0)

    def set_connections(self, conns):
        self.kafka = [int(p) == PROTO_KAFKA for p in conns["proto"]]
        self.caches = [Cache() for _ in self.kafka]

    def reset(self, c):
        self.caches[c] = Cache()

    def forwarded(self, verdict, c):
        return int(verdict) == ALLOW and c < len(self.kafka) and self.kafka[c]

    def forward(self, frames, conn, verdict, tags=None, now_ms=0, dropped=()):
        """-> (fwd, new_id, frames after); dropped: batch indices the device
        reported fwd == 2 for (the model cannot know the table's occupancy
        pattern; it is told, and checks stay exact for everything else)."""
        dropped = set(int(i) for i in dropped)
        n = len(frames)
        fwd, new_id, out = np.zeros(n, np.uint8), np.zeros(n, np.uint32), []
        for i, (f, c) in enumerate(zip(frames, np.asarray(conn).tolist())):
            f = bytearray(f)
            if self.forwarded(verdict[i], c):
                nid = self.caches[c].handle_request(f, 0 if tags is None else tags[i], now_ms, i in dropped)
                fwd[i] = 2 if i in dropped else 1
                new_id[i] = 0 if i in dropped else nid
                self.counts["dropped" if i in dropped else "forwarded"] += 1
            out.append(bytes(f))
        return fwd, new_id, out

    def responses(self, frames, conn):
        """-> (found, orig_id, api_key, api_version, tag, frames after)"""
        n = len(frames)
        found, orig = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        key, ver, tag = np.zeros(n, np.int16), np.zeros(n, np.int16), np.zeros(n, np.uint64)
        out = []
        for i, (f, c) in enumerate(zip(frames, np.asarray(conn).tolist())):
            f = bytearray(f)
            ent = self.caches[c].correlate_response(f) if c < len(self.kafka) and self.kafka[c] else None
            if ent is not None:
                found[i], orig[i], key[i], ver[i], tag[i] = 1, ent[0], ent[1], ent[2], ent[3]
            self.counts["found" if ent is not None else "missed"] += 1
            out.append(bytes(f))
        return found, orig, key, ver, tag, out

    def gc(self, now_ms, lifetime_ms):
        n = sum(c.gc(now_ms, lifetime_ms) for c in self.caches)
        self.counts["expired"] += n
        return n

    def stats(self):
        return dict(self.counts, live=sum(len(c.cache) for c in self.caches))

"""Host-side engine: the Python face of the C-ABI (include/l7gpu.h).

Mirrors the reference's per-request verdict interface for this path:
policies in (NPDS cilium.NetworkPolicy shape), connections opened with their
(policy, port, direction, identities) as in proxylib OnNewConnection
(proxylib/proxylib.go:57-74), then batches of requests classified into
(verdict, matched rule, consumed bytes).
"""
import ctypes as C
import json

import numpy as np

from . import _lib
from ._lib import Conn


class PolicyError(ValueError):
    """The policy set was rejected (the reference would NACK it)."""


class Engine:
    def __init__(self, device=0, lib_path=None):
        self._lib = _lib.load(lib_path)
        err = C.create_string_buffer(512)
        h = self._lib.l7g_engine_create(device, err, 512)
        if not h:
            raise RuntimeError("l7g_engine_create: " + err.value.decode(errors="replace"))
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.l7g_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- policy
    def update_policy(self, policy):
        js = policy if isinstance(policy, (str, bytes)) else json.dumps(policy)
        b = js.encode() if isinstance(js, str) else js
        err = C.create_string_buffer(1024)
        if self._lib.l7g_policy_update(self._h, b, len(b), err, 1024) != 0:
            raise PolicyError(err.value.decode(errors="replace"))

    def update_policy_proto(self, buf):
        """A serialized NPDS DiscoveryResponse (cilium.NetworkPolicy resources)."""
        b = bytes(buf)
        err = C.create_string_buffer(1024)
        if self._lib.l7g_policy_update_proto(self._h, b, len(b), err, 1024) != 0:
            raise PolicyError(err.value.decode(errors="replace"))

    def export_tables(self):
        """The current policy version's compiled tables (l7g_tables_export):
        what rank 0 broadcasts so that the other ranks install them without
        compiling (cilium_amd/dist.py)."""
        n = C.c_size_t(0)
        self._lib.l7g_tables_export(self._h, None, 0, C.byref(n))
        buf = (C.c_uint8 * max(n.value, 1))()
        if self._lib.l7g_tables_export(self._h, buf, n.value, C.byref(n)) != 0:
            raise RuntimeError("l7g_tables_export failed")
        return bytes(buf)[:n.value]

    def import_tables(self, image):
        b = bytes(image)
        err = C.create_string_buffer(1024)
        if self._lib.l7g_tables_import(self._h, b, len(b), err, 1024) != 0:
            raise PolicyError(err.value.decode(errors="replace"))

    @property
    def tables_compiled(self):
        """Rule sets this engine compiled itself since its policy version was installed."""
        return int(self._lib.l7g_tables_compiled(self._h))

    @property
    def tables_digest(self):
        """FNV-1a 64 of the device table blob (equal <=> byte-identical tables)."""
        return int(self._lib.l7g_tables_digest(self._h))

    def policy_index(self, name):
        b = name.encode()
        return self._lib.l7g_policy_index(self._h, b, len(b))

    @property
    def nrules(self):
        return self._lib.l7g_policy_nrules(self._h)

    # ----------------------------------------------------------- connections
    def set_connections(self, conns):
        """conns: sequence of dicts/tuples (policy, port, ingress, proto, src_id, dst_id)
        or a numpy structured array with those fields."""
        arr = conns_array(conns)
        err = C.create_string_buffer(1024)
        if self._lib.l7g_conns_set(self._h, arr.ctypes.data, len(arr), err, 1024) != 0:
            raise PolicyError(err.value.decode(errors="replace"))
        self._conns = arr

    # --------------------------------------------------------- classification
    def classify_device(self, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, n, verdict_ptr, rule_ptr,
                        consumed_ptr, counters_ptr=0, stream=0):
        """All pointers are device addresses (e.g. torch tensor .data_ptr());
        every request lies inside [arena_ptr, arena_ptr + arena_len)."""
        rc = self._lib.l7g_classify(self._h, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, n, verdict_ptr,
                                    rule_ptr, consumed_ptr, counters_ptr or None, stream or None)
        if rc != 0:
            raise RuntimeError(f"l7g_classify failed: HIP error {rc}")

    def classify_streams_device(self, arena_ptr, arena_len, s_off_ptr, s_len_ptr, s_conn_ptr, n, max_frames,
                                frame_off_ptr, frame_len_ptr, frame_conn_ptr, nframes_ptr, verdict_ptr=0, rule_ptr=0,
                                consumed_ptr=0, counters_ptr=0, stream=0):
        """l7g_frame_streams (no verdict pointers) or l7g_classify_streams: device
        framing of n connection streams into n * max_frames frame slots."""
        if verdict_ptr:
            rc = self._lib.l7g_classify_streams(self._h, arena_ptr, arena_len, s_off_ptr, s_len_ptr, s_conn_ptr, n,
                                                max_frames, frame_off_ptr, frame_len_ptr, frame_conn_ptr, nframes_ptr,
                                                verdict_ptr, rule_ptr, consumed_ptr, counters_ptr or None,
                                                stream or None)
        else:
            rc = self._lib.l7g_frame_streams(self._h, arena_ptr, arena_len, s_off_ptr, s_len_ptr, s_conn_ptr, n,
                                             max_frames, frame_off_ptr, frame_len_ptr, frame_conn_ptr, nframes_ptr,
                                             stream or None)
        if rc != 0:
            raise RuntimeError(f"l7g_frame_streams / l7g_classify_streams failed: HIP error {rc}")

    def classify(self, arena, offsets, lengths, conn_ids):
        """Host-buffer convenience: copies to the device, classifies, copies back."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        cid = np.ascontiguousarray(conn_ids, dtype=np.uint32)
        n = len(off)
        v = np.zeros(n, np.uint8)
        r = np.zeros(n, np.int32)
        c = np.zeros(n, np.uint32)
        rc = self._lib.l7g_classify_host(self._h, arena.ctypes.data, arena.nbytes, off.ctypes.data,
                                         ln.ctypes.data, cid.ctypes.data, n, v.ctypes.data,
                                         r.ctypes.data, c.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"l7g_classify_host failed: HIP error {rc}")
        return v, r, c

    # ------------------------------------------------------------ access log
    def classify_logged_device(self, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, n, verdict_ptr, rule_ptr,
                               consumed_ptr, records_ptr, topics_ptr=0, topic_stride=0, counters_ptr=0, stream=0):
        """l7g_classify_logged: classify_device, and one 32-byte record per
        request at records_ptr (16-byte aligned) plus n rows of topic_stride
        8-byte spans at topics_ptr; all pointers are device addresses."""
        lo = _lib.LogOut(records_ptr, topics_ptr or None, topic_stride)
        rc = self._lib.l7g_classify_logged(self._h, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, n, verdict_ptr,
                                           rule_ptr, consumed_ptr, counters_ptr or None, C.byref(lo), stream or None)
        if rc != 0:
            raise RuntimeError(f"l7g_classify_logged failed: HIP error {rc}")

    def classify_logged(self, arena, offsets, lengths, conn_ids, topic_stride=4, topics=None):
        """classify(), with the access-log outputs: returns (verdict, rule,
        consumed, records, topics).  records is a LOGREC_DTYPE array (read its
        http_* fields where kind == 1, its kafka_* fields where kind == 2, and
        only where the verdict is ALLOW or DENY); topics is an (n,
        topic_stride) SPAN_DTYPE array whose row i holds the first
        min(ntopics, topic_stride) topic-name spans of Kafka request i.  Rows
        of other requests are not written: they keep what `topics` held (zeros
        when not given)."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        cid = np.ascontiguousarray(conn_ids, dtype=np.uint32)
        n = len(off)
        v = np.zeros(n, np.uint8)
        r = np.zeros(n, np.int32)
        c = np.zeros(n, np.uint32)
        rec = np.zeros(n, LOGREC_DTYPE)
        if topics is None:
            topics = np.zeros((n, topic_stride), SPAN_DTYPE)
        topics = np.ascontiguousarray(topics, dtype=SPAN_DTYPE)
        if topics.shape != (n, topic_stride):
            raise ValueError("topics must have shape (n, topic_stride)")
        lo = _lib.LogOut(rec.ctypes.data, topics.ctypes.data if topic_stride else None, topic_stride)
        rc = self._lib.l7g_classify_logged_host(self._h, arena.ctypes.data, arena.nbytes, off.ctypes.data,
                                                ln.ctypes.data, cid.ctypes.data, n, v.ctypes.data, r.ctypes.data,
                                                c.ctypes.data, C.byref(lo))
        if rc != 0:
            raise RuntimeError(f"l7g_classify_logged_host failed: HIP error {rc}")
        return v, r, c, rec, topics

    def classify_logged_all_device(self, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, n, verdict_ptr, rule_ptr,
                                   consumed_ptr, records_ptr, spans_ptr=0, span_stride=0, text_ptr=0, text_stride=0,
                                   counters_ptr=0, stream=0):
        """l7g_classify_logged_all: classify_logged_device, with the records of
        memcached, r2d2 and cassandra requests as well; spans_ptr: n rows of
        span_stride 8-byte spans (Kafka topics, memcached text keys), text_ptr:
        n rows of text_stride bytes (cassandra query_table).  All pointers are
        device addresses."""
        lo = _lib.LogAllOut(records_ptr, spans_ptr or None, span_stride, text_ptr or None, text_stride)
        rc = self._lib.l7g_classify_logged_all(self._h, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, n,
                                               verdict_ptr, rule_ptr, consumed_ptr, counters_ptr or None, C.byref(lo),
                                               stream or None)
        if rc != 0:
            raise RuntimeError(f"l7g_classify_logged_all failed: HIP error {rc}")

    def classify_logged_all(self, arena, offsets, lengths, conn_ids, span_stride=4, text_stride=64, spans=None,
                            text=None):
        """classify_logged(), for every parser: returns (verdict, rule,
        consumed, records, spans, text).  records is a LOGREC_DTYPE array: read
        the mc_* fields where kind == 3, mcb_* where 4, r2_* where 5, cass_*
        where 6 (and http_* / kafka_* as before), only where the verdict is
        ALLOW or DENY.  spans is an (n, span_stride) SPAN_DTYPE array (Kafka
        topics, memcached text keys), text an (n, text_stride) uint8 array
        (cassandra query_table); what no kernel writes keeps what `spans` /
        `text` held (zeros when not given).  log_entries() turns the outputs
        into the reference's log entries."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        cid = np.ascontiguousarray(conn_ids, dtype=np.uint32)
        n = len(off)
        v = np.zeros(n, np.uint8)
        r = np.zeros(n, np.int32)
        c = np.zeros(n, np.uint32)
        rec = np.zeros(n, LOGREC_DTYPE)
        if spans is None:
            spans = np.zeros((n, span_stride), SPAN_DTYPE)
        spans = np.ascontiguousarray(spans, dtype=SPAN_DTYPE)
        if text is None:
            text = np.zeros((n, text_stride), np.uint8)
        text = np.ascontiguousarray(text, dtype=np.uint8)
        if spans.shape != (n, span_stride) or text.shape != (n, text_stride):
            raise ValueError("spans must have shape (n, span_stride) and text (n, text_stride)")
        lo = _lib.LogAllOut(rec.ctypes.data, spans.ctypes.data if span_stride else None, span_stride,
                            text.ctypes.data if text_stride else None, text_stride)
        rc = self._lib.l7g_classify_logged_all_host(self._h, arena.ctypes.data, arena.nbytes, off.ctypes.data,
                                                    ln.ctypes.data, cid.ctypes.data, n, v.ctypes.data, r.ctypes.data,
                                                    c.ctypes.data, C.byref(lo))
        if rc != 0:
            raise RuntimeError(f"l7g_classify_logged_all_host failed: HIP error {rc}")
        return v, r, c, rec, spans, text

    # ---------------------------------------------------------- deny replies
    def deny_replies_device(self, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, n, verdict_ptr, buf_ptr, cap,
                            reply_off_ptr, reply_len_ptr, total_ptr, stream=0):
        """l7g_deny_replies: the replies of the requests whose verdict is DENY,
        packed in request order into buf_ptr[0, cap) (0 with cap 0: sizes
        only); reply_off_ptr (n uint64), reply_len_ptr (n uint32) and total_ptr
        (2 uint64) are always written.  All pointers are device addresses."""
        ro = _lib.ReplyOut(buf_ptr or None, cap, reply_off_ptr, reply_len_ptr, total_ptr)
        rc = self._lib.l7g_deny_replies(self._h, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, n, verdict_ptr,
                                        C.byref(ro), stream or None)
        if rc != 0:
            raise RuntimeError(f"l7g_deny_replies failed: HIP error {rc}")

    def deny_replies_arrays(self, arena, offsets, lengths, conn_ids, verdict, cap=0, buf=None):
        """l7g_deny_replies_host on host buffers: returns (buf, off, len,
        total); buf is a uint8 array of cap bytes (the caller's, when given:
        only the replies that fit are written into it)."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        cid = np.ascontiguousarray(conn_ids, dtype=np.uint32)
        v = np.ascontiguousarray(verdict, dtype=np.uint8)
        n = len(off)
        if buf is None:
            buf = np.zeros(cap, np.uint8)
        ro_off = np.zeros(n, np.uint64)
        ro_len = np.zeros(n, np.uint32)
        total = np.zeros(2, np.uint64)
        ro = _lib.ReplyOut(buf.ctypes.data if cap else None, cap, ro_off.ctypes.data, ro_len.ctypes.data,
                           total.ctypes.data)
        rc = self._lib.l7g_deny_replies_host(self._h, arena.ctypes.data, arena.nbytes, off.ctypes.data, ln.ctypes.data,
                                             cid.ctypes.data, n, v.ctypes.data, C.byref(ro))
        if rc != 0:
            raise RuntimeError(f"l7g_deny_replies_host failed: HIP error {rc}")
        return buf, ro_off, ro_len, total

    def deny_replies(self, arena, offsets, lengths, conn_ids, verdict, cap=None):
        """What to send back for each denied request (host buffers): a list of
        bytes per request, b"" where there is nothing to send (the verdict is
        not DENY, a memcached connection, a Kafka request without a response).
        cap=None sizes first, then writes; with a cap, a reply that does not
        fit under it comes back as None."""
        if cap is None:
            _, _, _, total = self.deny_replies_arrays(arena, offsets, lengths, conn_ids, verdict)
            cap = int(total[0])
        buf, ro_off, ro_len, _ = self.deny_replies_arrays(arena, offsets, lengths, conn_ids, verdict, cap)
        raw = buf.tobytes()
        return [b"" if l == 0 else (raw[o:o + l] if o + l <= cap else None)
                for o, l in zip(ro_off.tolist(), ro_len.tolist())]

    # ---------------------------------------------------- cassandra sessions
    def cass_sessions(self, max_statements):
        """Device-resident cassandra sessions (l7g_cass_sessions_enable): with
        max_statements > 0 the engine keeps each connection's keyspace and
        prepared statements across classify calls; 0 turns them off."""
        err = C.create_string_buffer(512)
        rc = self._lib.l7g_cass_sessions_enable(self._h, int(max_statements), err, 512)
        if rc != 0:
            raise RuntimeError(f"l7g_cass_sessions_enable: HIP error {rc}: " + err.value.decode(errors="replace"))

    def cass_replies(self, arena, offsets, lengths, conn_ids):
        """The reply direction of cassandra connections (host buffers): frames
        each reply and binds RESULT/prepared ids; returns (verdict, consumed)."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        cid = np.ascontiguousarray(conn_ids, dtype=np.uint32)
        n = len(off)
        v = np.zeros(n, np.uint8)
        c = np.zeros(n, np.uint32)
        rc = self._lib.l7g_cass_replies_host(self._h, arena.ctypes.data, arena.nbytes, off.ctypes.data,
                                             ln.ctypes.data, cid.ctypes.data, n, v.ctypes.data, c.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"l7g_cass_replies_host failed: HIP error {rc}")
        return v, c

    def cass_replies_device(self, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, n, verdict_ptr, consumed_ptr,
                            stream=0):
        """l7g_cass_replies: all pointers are device addresses."""
        rc = self._lib.l7g_cass_replies(self._h, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, n, verdict_ptr,
                                        consumed_ptr, stream or None)
        if rc != 0:
            raise RuntimeError(f"l7g_cass_replies failed: HIP error {rc}")

    def cass_session_reset(self, conn_ids):
        cid = np.ascontiguousarray(conn_ids, dtype=np.uint32)
        rc = self._lib.l7g_cass_session_reset(self._h, cid.ctypes.data, len(cid))
        if rc != 0:
            raise RuntimeError(f"l7g_cass_session_reset failed: HIP error {rc}")

    SESSION_STATS = ("stream_entries", "id_entries", "dropped", "overflows", "resolved", "unprepared")

    def cass_session_stats(self):
        out = (C.c_uint64 * 6)()
        self._lib.l7g_cass_session_stats(self._h, out)
        return dict(zip(self.SESSION_STATS, [int(x) for x in out]))

    # -------------------------------------------------------- kafka sessions
    def kafka_sessions(self, max_inflight):
        """Device-resident Kafka correlation caches (l7g_kafka_sessions_enable):
        with max_inflight > 0 the engine renumbers forwarded requests and
        correlates responses per connection; 0 turns that off."""
        err = C.create_string_buffer(512)
        rc = self._lib.l7g_kafka_sessions_enable(self._h, int(max_inflight), err, 512)
        if rc != 0:
            raise RuntimeError(f"l7g_kafka_sessions_enable: HIP error {rc}: " + err.value.decode(errors="replace"))

    def kafka_forward(self, arena, offsets, lengths, conn_ids, verdict, now_ms, tags=None):
        """HandleRequest over a batch (host buffers): the ids of the forwarded
        requests are rewritten in `arena` (a writable contiguous uint8 array);
        returns (fwd, new_id)."""
        if not (isinstance(arena, np.ndarray) and arena.dtype == np.uint8 and arena.flags.c_contiguous
                and arena.flags.writeable):
            raise TypeError("arena: a writable contiguous uint8 array (it is rewritten in place)")
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        cid = np.ascontiguousarray(conn_ids, dtype=np.uint32)
        v = np.ascontiguousarray(verdict, dtype=np.uint8)
        tg = None if tags is None else np.ascontiguousarray(tags, dtype=np.uint64)
        n = len(off)
        fwd = np.zeros(n, np.uint8)
        new_id = np.zeros(n, np.uint32)
        rc = self._lib.l7g_kafka_forward_host(self._h, arena.ctypes.data, arena.nbytes, off.ctypes.data, ln.ctypes.data,
                                              cid.ctypes.data, v.ctypes.data, None if tg is None else tg.ctypes.data, n,
                                              int(now_ms), fwd.ctypes.data, new_id.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"l7g_kafka_forward_host failed: HIP error {rc}")
        return fwd, new_id

    def kafka_forward_device(self, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, verdict_ptr, tag_ptr, n, now_ms,
                             fwd_ptr, new_id_ptr, stream=0):
        """l7g_kafka_forward: all pointers are device addresses (tag_ptr may be 0)."""
        rc = self._lib.l7g_kafka_forward(self._h, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, verdict_ptr,
                                         tag_ptr or None, n, int(now_ms), fwd_ptr, new_id_ptr, stream or None)
        if rc != 0:
            raise RuntimeError(f"l7g_kafka_forward failed: HIP error {rc}")

    def kafka_responses(self, arena, offsets, lengths, conn_ids):
        """CorrelateResponse over a batch (host buffers): the original ids are
        restored in `arena`; returns (found, orig_id, api_key, api_version, tag)."""
        if not (isinstance(arena, np.ndarray) and arena.dtype == np.uint8 and arena.flags.c_contiguous
                and arena.flags.writeable):
            raise TypeError("arena: a writable contiguous uint8 array (it is rewritten in place)")
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        cid = np.ascontiguousarray(conn_ids, dtype=np.uint32)
        n = len(off)
        found = np.zeros(n, np.uint8)
        orig = np.zeros(n, np.uint32)
        key = np.zeros(n, np.int16)
        ver = np.zeros(n, np.int16)
        tag = np.zeros(n, np.uint64)
        rc = self._lib.l7g_kafka_responses_host(self._h, arena.ctypes.data, arena.nbytes, off.ctypes.data,
                                                ln.ctypes.data, cid.ctypes.data, n, found.ctypes.data, orig.ctypes.data,
                                                key.ctypes.data, ver.ctypes.data, tag.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"l7g_kafka_responses_host failed: HIP error {rc}")
        return found, orig, key, ver, tag

    def kafka_responses_device(self, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, n, found_ptr, orig_id_ptr,
                               api_key_ptr, api_version_ptr, tag_ptr, stream=0):
        """l7g_kafka_responses: all pointers are device addresses."""
        rc = self._lib.l7g_kafka_responses(self._h, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, n, found_ptr,
                                           orig_id_ptr, api_key_ptr, api_version_ptr, tag_ptr, stream or None)
        if rc != 0:
            raise RuntimeError(f"l7g_kafka_responses failed: HIP error {rc}")

    def kafka_session_gc(self, now_ms, lifetime_ms):
        """Drops the entries older than lifetime_ms at now_ms and compacts the table; returns how many."""
        gone = C.c_uint64(0)
        rc = self._lib.l7g_kafka_session_gc(self._h, int(now_ms), int(lifetime_ms), C.byref(gone))
        if rc != 0:
            raise RuntimeError(f"l7g_kafka_session_gc failed: HIP error {rc}")
        return int(gone.value)

    def kafka_session_reset(self, conn_ids):
        cid = np.ascontiguousarray(conn_ids, dtype=np.uint32)
        rc = self._lib.l7g_kafka_session_reset(self._h, cid.ctypes.data, len(cid))
        if rc != 0:
            raise RuntimeError(f"l7g_kafka_session_reset failed: HIP error {rc}")

    KAFKA_SESSION_STATS = ("live", "used_slots", "dropped", "forwarded", "found", "missed", "expired")

    def kafka_session_stats(self):
        out = (C.c_uint64 * 7)()
        self._lib.l7g_kafka_session_stats(self._h, out)
        return dict(zip(self.KAFKA_SESSION_STATS, [int(x) for x in out]))

    # ----------------------------------------------------- memcached sessions
    def mc_sessions(self, max_pending):
        """Device-resident memcached reply queues (l7g_mc_sessions_enable): with
        max_pending > 0 the engine keeps each connection's text reply queue (a
        ring of that capacity, rounded up to a power of two) and binary
        counters; 0 turns that off."""
        err = C.create_string_buffer(512)
        rc = self._lib.l7g_mc_sessions_enable(self._h, int(max_pending), err, 512)
        if rc != 0:
            raise RuntimeError(f"l7g_mc_sessions_enable: HIP error {rc}: " + err.value.decode(errors="replace"))

    def mc_forward(self, arena, offsets, lengths, conn_ids, verdict, tags=None):
        """The request direction over a batch (host buffers), after classify
        with its verdicts; returns act (l7gpu.h has the codes)."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        cid = np.ascontiguousarray(conn_ids, dtype=np.uint32)
        v = np.ascontiguousarray(verdict, dtype=np.uint8)
        tg = None if tags is None else np.ascontiguousarray(tags, dtype=np.uint64)
        n = len(off)
        act = np.zeros(n, np.uint8)
        rc = self._lib.l7g_mc_forward_host(self._h, arena.ctypes.data, arena.nbytes, off.ctypes.data, ln.ctypes.data,
                                           cid.ctypes.data, v.ctypes.data, None if tg is None else tg.ctypes.data, n,
                                           act.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"l7g_mc_forward_host failed: HIP error {rc}")
        return act

    def mc_forward_device(self, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, verdict_ptr, tag_ptr, n, act_ptr,
                          stream=0):
        """l7g_mc_forward: all pointers are device addresses (tag_ptr may be 0)."""
        rc = self._lib.l7g_mc_forward(self._h, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, verdict_ptr,
                                      tag_ptr or None, n, act_ptr, stream or None)
        if rc != 0:
            raise RuntimeError(f"l7g_mc_forward failed: HIP error {rc}")

    def mc_replies(self, arena, offsets, lengths, conn_ids, max_ops=16):
        """The reply direction over a batch of streams (host buffers): returns
        (op_kind[n, max_ops], op_n, op_aux, nops[n], result[n], taken[n])."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        cid = np.ascontiguousarray(conn_ids, dtype=np.uint32)
        n = len(off)
        kind = np.zeros((n, max_ops), np.uint8)
        opn = np.zeros((n, max_ops), np.uint32)
        aux = np.zeros((n, max_ops), np.uint64)
        nops = np.zeros(n, np.uint32)
        res = np.zeros(n, np.uint8)
        taken = np.zeros(n, np.uint64)
        rc = self._lib.l7g_mc_replies_host(self._h, arena.ctypes.data, arena.nbytes, off.ctypes.data, ln.ctypes.data,
                                           cid.ctypes.data, n, int(max_ops), kind.ctypes.data, opn.ctypes.data,
                                           aux.ctypes.data, nops.ctypes.data, res.ctypes.data, taken.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"l7g_mc_replies_host failed: HIP error {rc}")
        return kind, opn, aux, nops, res, taken

    def mc_replies_device(self, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, n, max_ops, op_kind_ptr, op_n_ptr,
                          op_aux_ptr, nops_ptr, result_ptr, taken_ptr, stream=0):
        """l7g_mc_replies: all pointers are device addresses (op_aux_ptr may be 0)."""
        rc = self._lib.l7g_mc_replies(self._h, arena_ptr, arena_len, off_ptr, len_ptr, conn_ptr, n, int(max_ops),
                                      op_kind_ptr, op_n_ptr, op_aux_ptr or None, nops_ptr, result_ptr, taken_ptr,
                                      stream or None)
        if rc != 0:
            raise RuntimeError(f"l7g_mc_replies failed: HIP error {rc}")

    def mc_session_reset(self, conn_ids):
        cid = np.ascontiguousarray(conn_ids, dtype=np.uint32)
        rc = self._lib.l7g_mc_session_reset(self._h, cid.ctypes.data, len(cid))
        if rc != 0:
            raise RuntimeError(f"l7g_mc_session_reset failed: HIP error {rc}")

    MC_SESSION_STATS = ("queued", "sessions", "full", "mismatch", "inject_now", "inject_queued", "passed", "errors")

    def mc_session_stats(self):
        out = (C.c_uint64 * 8)()
        self._lib.l7g_mc_session_stats(self._h, out)
        return dict(zip(self.MC_SESSION_STATS, [int(x) for x in out]))

    def conn_update(self, index, conn):
        """One connection set (or added) alone: l7g_conn_update, the new-connection event."""
        arr = conns_array([conn])
        err = C.create_string_buffer(1024)
        if self._lib.l7g_conn_update(self._h, int(index), arr.ctypes.data, err, 1024) != 0:
            raise PolicyError(err.value.decode(errors="replace"))

    STAGES = ("partition", "http", "kafka", "memcache")

    def profile(self, on=True):
        """Record HIP events around each kernel of every l7g_classify call."""
        rc = self._lib.l7g_profile_enable(self._h, 1 if on else 0)
        if rc != 0:
            raise RuntimeError(f"l7g_profile_enable failed: HIP error {rc}")

    def profile_last(self):
        """Device ms per stage of the last classify call (profiling on)."""
        out = np.zeros(4, np.float32)
        rc = self._lib.l7g_profile_last(self._h, out.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"l7g_profile_last failed: HIP error {rc}")
        return dict(zip(self.STAGES, out.tolist()))

    def kafka_phase_times(self, reset=True):
        """Per-phase cycle totals of the Kafka kernel (-DL7G_KX_TIMING build only), or None."""
        out = np.zeros(8, np.uint64)
        if self._lib.l7g_debug_kafka_phase_times(self._h, out.ctypes.data, 1 if reset else 0) != 0:
            return None
        return out

    def frame_phase_times(self, reset=True):
        """Per-phase cycle totals of the text-stream framer (-DL7G_FRAME_PHASES build only), or None."""
        out = np.zeros(8, np.uint64)
        if self._lib.l7g_debug_frame_phase_times(self._h, out.ctypes.data, 1 if reset else 0) != 0:
            return None
        return out

    def phase_times(self, reset=True):
        """Per-phase cycle totals of the HTTP kernels (timing build only; 16 slots,
        include/l7gpu.h), or None."""
        out = np.zeros(16, np.uint64)
        if self._lib.l7g_debug_phase_times(self._h, out.ctypes.data, 1 if reset else 0) != 0:
            return None
        return out

    def flow_stats_enable(self, on=True):
        rc = self._lib.l7g_flow_stats_enable(self._h, 1 if on else 0)
        if rc != 0:
            raise RuntimeError(f"l7g_flow_stats_enable: {rc}")

    def flow_stats(self, reset=False):
        """{(policy, proto, port, ingress): (received, forwarded, denied, error)}
        accumulated since the last reset (pkg/endpoint UpdateProxyStatistics)."""
        n = C.c_uint32(0)
        rc = self._lib.l7g_flow_stats(self._h, None, 0, C.byref(n), 0)
        if rc != 0:
            raise RuntimeError(f"l7g_flow_stats: {rc}")
        arr = (_lib.FlowStat * max(1, n.value))()
        rc = self._lib.l7g_flow_stats(self._h, arr, n.value, C.byref(n), 1 if reset else 0)
        if rc != 0:
            raise RuntimeError(f"l7g_flow_stats: {rc}")
        return {(x.policy, x.proto, x.port, x.ingress): (x.received, x.forwarded, x.denied, x.error)
                for x in arr[:n.value]}

    def service(self, on=None):
        """Resident services (l7g_service_enable): with on given, enable (True)
        or stop and disable (False); returns the previous setting and the
        counts {http_calls, http_launches, mc_calls, mc_launches}."""
        prev = None
        if on is not None:
            prev = bool(self._lib.l7g_service_enable(self._h, 1 if on else 0))
        out = (C.c_uint64 * 4)()
        self._lib.l7g_service_stats(self._h, out)
        return prev, dict(zip(("http_calls", "http_launches", "mc_calls", "mc_launches"), list(out)))

    def stats(self):
        s = _lib.Stats()
        self._lib.l7g_stats(self._h, C.byref(s))
        return {k: getattr(s, k) for k, _ in s._fields_}


CONN_DTYPE = np.dtype([("policy", "<i4"), ("port", "<u4"), ("ingress", "u1"), ("proto", "u1"),
                       ("flags", "<u2"), ("src_id", "<u4"), ("dst_id", "<u4")])
assert CONN_DTYPE.itemsize == C.sizeof(Conn)


# l7g_logrec_t as a numpy record: the union's two views over the same bytes
# (mc_*: u.mc_text, mcb_*: u.mc_binary, r2_*: u.r2d2, cass_*: u.cassandra -- l7g_classify_logged_all's)
_LOGREC_GENERIC = [("mc_cmd_off", 4), ("mc_cmd_len", 8), ("mc_nkeys", 12), ("mcb_key_off", 4), ("mcb_key_len", 8),
                   ("r2_cmd_len", 4), ("r2_file_off", 8), ("r2_file_len", 12), ("r2_nfields", 16),
                   ("cass_table_len", 4), ("cass_keyword", 8), ("cass_word_off", 12), ("cass_word_len", 16)]
LOGREC_DTYPE = np.dtype({
    "names": ["kind", "flags", "api_key", "method_len", "path_len", "host_off", "host_len", "head_len", "nheaders",
              "api_version", "correlation_id", "ntopics"] + [k for k, _ in _LOGREC_GENERIC],
    "formats": ["u1", "u1", "<i2", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<i2", "<i4", "<u4"] +
               ["<u4"] * len(_LOGREC_GENERIC),
    "offsets": [0, 1, 2, 4, 8, 12, 16, 20, 24, 4, 8, 12] + [o for _, o in _LOGREC_GENERIC],
    "itemsize": 32})
SPAN_DTYPE = np.dtype([("off", "<u4"), ("len", "<u4")])
assert LOGREC_DTYPE.itemsize == C.sizeof(_lib.LogRec) and SPAN_DTYPE.itemsize == C.sizeof(_lib.Span)


CASS_KEYWORDS = ("alter", "create", "drop", "truncate", "list")  # l7g_logrec_t u.cassandra.keyword


def log_entries(verdict, records, spans, text, arena, offsets, lengths):
    """The LogEntry_GenericL7 entries of a classify_logged_all() batch as the
    proxylib parsers log them: a list with, per request, None (no entry: a
    verdict other than ALLOW / DENY, an HTTP or Kafka request, a cassandra
    request whose path has no four parts) or (entry_type, proto, fields) with
    entry_type "Request" (ALLOW) or "Denied" (DENY), proto the parser's name
    and fields a dict of bytes values (Go strings are bytes).  A request whose
    span or text row was too short for it (flags bit0), or a cassandra EXECUTE
    whose stored action has no name (flags bit2), raises ValueError."""
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    out = []
    for i in range(len(records)):
        r = records[i]
        kind, v = int(r["kind"]), int(verdict[i])
        if v not in (_lib.ALLOW, _lib.DENY) or kind < _lib.LOG_MC_TEXT:
            out.append(None)
            continue
        et = "Request" if v == _lib.ALLOW else "Denied"
        req = arena[int(offsets[i]):int(offsets[i]) + int(lengths[i])].tobytes()
        flags = int(r["flags"])

        def cut(o, n):
            return req[int(o):int(o) + int(n)]
        if kind == _lib.LOG_MC_TEXT:
            if flags & 1:
                raise ValueError(f"request {i}: {int(r['mc_nkeys'])} keys, more than the span stride")
            keys = [cut(s["off"], s["len"]) for s in spans[i][:int(r["mc_nkeys"])]]
            out.append((et, "textmemcached", {"command": cut(r["mc_cmd_off"], r["mc_cmd_len"]),
                                              "keys": b", ".join(keys)}))
        elif kind == _lib.LOG_MC_BINARY:
            out.append((et, "binarymemcached", {"opcode": str(int(r["api_key"])).encode(),
                                                "key": cut(r["mcb_key_off"], r["mcb_key_len"])}))
        elif kind == _lib.LOG_R2D2:
            out.append((et, "r2d2", {"cmd": cut(0, r["r2_cmd_len"]), "file": cut(r["r2_file_off"], r["r2_file_len"])}))
        elif kind == _lib.LOG_CASSANDRA:
            if not flags & 2:
                out.append(None)
                continue
            if flags & 1:
                raise ValueError(f"request {i}: a table of {int(r['cass_table_len'])} bytes, more than the text stride")
            if flags & 4:
                raise ValueError(f"request {i}: the stored statement's action has no name")
            a = int(r["api_key"])
            if a >= 0:
                action = _lib.cass_action_name(a).encode()
            else:
                # (Go lowers the whole query first; ASCII-only lowering here is exact for ASCII words)
                word = cut(r["cass_word_off"], r["cass_word_len"]).decode("utf-8", "surrogateescape").lower() \
                    .encode("utf-8", "surrogateescape")
                action = CASS_KEYWORDS[int(r["cass_keyword"])].encode() + b"-" + word
                if word == b"materialized":
                    action += b"-view"
            out.append((et, "cassandra", {"query_action": action,
                                          "query_table": text[i][:int(r["cass_table_len"])].tobytes()}))
        else:
            out.append(None)
    return out


def conns_array(conns):
    if isinstance(conns, np.ndarray) and conns.dtype == CONN_DTYPE:
        return np.ascontiguousarray(conns)
    arr = np.zeros(len(conns), CONN_DTYPE)
    for i, c in enumerate(conns):
        if isinstance(c, dict):
            for k in ("policy", "port", "ingress", "proto", "flags", "src_id", "dst_id"):
                arr[i][k] = c.get(k, 0)
        else:
            arr[i] = (c[0], c[1], c[2], c[3], 0, c[4], c[5])
    return arr

"""ctypes binding of include/l7gpu.h (the product's C-ABI).

The shared library is built in-tree by cilium_amd/build.py.  There is no
fallback: if libl7gpu.so is missing or fails to load, importing the engine
raises, so nothing can silently classify on the CPU.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# L7G_LIB may name the profiling build (libl7gpu_timing.so) for experiments
LIB_PATH = os.environ.get("L7G_LIB") or os.path.join(HERE, "libl7gpu.so")

DENY, ALLOW, PARSE_ERROR, INCOMPLETE, UNSUPPORTED = 0, 1, 2, 3, 4
PROTO_HTTP, PROTO_KAFKA, PROTO_MEMCACHE, PROTO_R2D2, PROTO_CASSANDRA = 1, 2, 3, 4, 5
VERDICT_NAMES = {DENY: "DENY", ALLOW: "ALLOW", PARSE_ERROR: "PARSE_ERROR",
                 INCOMPLETE: "INCOMPLETE", UNSUPPORTED: "UNSUPPORTED"}


class Conn(C.Structure):
    """l7g_conn_t (20 bytes; same layout as the oracle's ref_conn_t)."""
    _fields_ = [("policy", C.c_int32), ("port", C.c_uint32), ("ingress", C.c_uint8),
                ("proto", C.c_uint8), ("flags", C.c_uint16), ("src_id", C.c_uint32),
                ("dst_id", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "policies", "rules", "http_rulesets", "http_chunks", "http_dfas", "http_dfa_states",
        "kafka_rulesets", "kafka_rules", "kafka_topics")] + [
        ("table_bytes", C.c_uint64), ("http_image_bytes", C.c_uint64), ("hot_ruleset", C.c_int32),
        ("hot_image_bytes", C.c_uint32)] + [
        (n, C.c_uint32) for n in ("mc_rulesets", "mc_rules", "mc_dfas", "mc_dfa_states", "http_nfas", "mc_nfas")] + [
        ("nfa_pool_bytes", C.c_uint64), ("r2d2_rulesets", C.c_uint32), ("r2d2_rules", C.c_uint32)]


EXPORTS = (
    "l7g_engine_create", "l7g_engine_destroy", "l7g_policy_update", "l7g_policy_index",
    "l7g_policy_nrules", "l7g_conns_set", "l7g_conn_update", "l7g_classify", "l7g_classify_host", "l7g_stats",
    "l7g_debug_regex", "l7g_debug_phase_times", "l7g_profile_enable", "l7g_profile_last",
    "l7g_debug_kafka_phase_times", "l7g_debug_frame_phase_times", "l7g_kafka_deny_response", "l7g_debug_regex_nfa", "l7g_policy_update_proto", "l7g_kafka_corr_create", "l7g_kafka_corr_destroy",
    "l7g_kafka_corr_requests", "l7g_kafka_corr_responses", "l7g_kafka_corr_gc", "l7g_kafka_corr_size",
    "l7g_flow_stats_enable", "l7g_flow_stats",
    "l7g_tables_export", "l7g_tables_import", "l7g_tables_compiled", "l7g_tables_digest",
    "l7g_frame_streams", "l7g_classify_streams", "l7g_service_enable", "l7g_service_stats",
    "l7g_cass_sessions_enable", "l7g_cass_replies", "l7g_cass_replies_host", "l7g_cass_session_reset",
    "l7g_cass_session_stats",
    "l7g_classify_logged", "l7g_classify_logged_host", "l7g_kafka_api_key_name",
    "l7g_deny_replies", "l7g_deny_replies_host", "l7g_deny_reply_template",
    "l7g_classify_logged_all", "l7g_classify_logged_all_host", "l7g_cass_action_name",
    "l7g_kafka_sessions_enable", "l7g_kafka_forward", "l7g_kafka_responses", "l7g_kafka_forward_host",
    "l7g_kafka_responses_host", "l7g_kafka_session_gc", "l7g_kafka_session_reset", "l7g_kafka_session_stats",
    "l7g_mc_sessions_enable", "l7g_mc_forward", "l7g_mc_replies", "l7g_mc_forward_host", "l7g_mc_replies_host",
    "l7g_mc_session_reset", "l7g_mc_session_stats", "l7g_mc_denied_message",
)


class FlowStat(C.Structure):
    _fields_ = [("policy", C.c_int32), ("proto", C.c_uint8), ("ingress", C.c_uint8), ("port", C.c_uint16),
                ("received", C.c_uint64), ("forwarded", C.c_uint64), ("denied", C.c_uint64), ("error", C.c_uint64)]


class Span(C.Structure):
    """l7g_span_t: bytes from the request's first byte."""
    _fields_ = [("off", C.c_uint32), ("len", C.c_uint32)]


class _LogHttp(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("method_len", "path_len", "host_off", "host_len", "head_len", "nheaders")]


class _LogKafka(C.Structure):
    _fields_ = [("api_version", C.c_int16), ("pad", C.c_int16), ("correlation_id", C.c_int32),
                ("ntopics", C.c_uint32)]


class _LogMcText(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("cmd_off", "cmd_len", "nkeys")]


class _LogMcBinary(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("key_off", "key_len")]


class _LogR2d2(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("cmd_len", "file_off", "file_len", "nfields")]


class _LogCassandra(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("table_len", "keyword", "word_off", "word_len")]


class _LogUnion(C.Union):
    _fields_ = [("http", _LogHttp), ("kafka", _LogKafka), ("mc_text", _LogMcText), ("mc_binary", _LogMcBinary),
                ("r2d2", _LogR2d2), ("cassandra", _LogCassandra)]


class LogRec(C.Structure):
    """l7g_logrec_t (32 bytes): one access-log record per request."""
    _fields_ = [("kind", C.c_uint8), ("flags", C.c_uint8), ("api_key", C.c_int16), ("u", _LogUnion),
                ("reserved", C.c_uint32)]


class LogOut(C.Structure):
    """l7g_log_out_t."""
    _fields_ = [("rec", C.c_void_p), ("topics", C.c_void_p), ("topic_stride", C.c_uint32)]


class LogAllOut(C.Structure):
    """l7g_log_all_out_t."""
    _fields_ = [("rec", C.c_void_p), ("spans", C.c_void_p), ("span_stride", C.c_uint32),
                ("text", C.c_void_p), ("text_stride", C.c_uint32)]


LOG_NONE, LOG_HTTP, LOG_KAFKA = 0, 1, 2
LOG_MC_TEXT, LOG_MC_BINARY, LOG_R2D2, LOG_CASSANDRA = 3, 4, 5, 6


class ReplyOut(C.Structure):
    """l7g_reply_out_t."""
    _fields_ = [("buf", C.c_void_p), ("cap", C.c_uint64), ("off", C.c_void_p), ("len", C.c_void_p),
                ("total", C.c_void_p)]


_libs = {}


def load(path=None):
    """The product library (or, for kernel experiments, a variant build of it
    named by path: tools/exp_*.py)."""
    path = path or LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run python -m cilium_amd.build (no CPU fallback exists)")
    # One HIP runtime per process: torch ships its own libamdhip64 under the same
    # soname, and whichever loads first serves both.  Loading torch's first keeps
    # torch.cuda working in processes that use both (batches in torch tensors).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    vp, sz, cp = C.c_void_p, C.c_size_t, C.c_char_p
    lib.l7g_engine_create.restype = vp
    lib.l7g_engine_create.argtypes = [C.c_int, cp, sz]
    lib.l7g_engine_destroy.argtypes = [vp]
    lib.l7g_policy_update.argtypes = [vp, cp, sz, cp, sz]
    lib.l7g_policy_update_proto.argtypes = [vp, cp, sz, cp, sz]
    lib.l7g_policy_index.restype = C.c_int32
    lib.l7g_policy_index.argtypes = [vp, cp, sz]
    lib.l7g_policy_nrules.restype = C.c_int32
    lib.l7g_policy_nrules.argtypes = [vp]
    lib.l7g_conns_set.argtypes = [vp, vp, C.c_uint32, cp, sz]
    lib.l7g_tables_export.argtypes = [vp, vp, sz, C.POINTER(sz)]
    lib.l7g_tables_import.argtypes = [vp, cp, sz, cp, sz]
    lib.l7g_tables_compiled.restype = C.c_uint64
    lib.l7g_tables_compiled.argtypes = [vp]
    lib.l7g_tables_digest.restype = C.c_uint64
    lib.l7g_tables_digest.argtypes = [vp]
    lib.l7g_conn_update.argtypes = [vp, C.c_uint32, vp, cp, sz]
    lib.l7g_classify.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint32, vp, vp, vp, vp, vp]
    lib.l7g_frame_streams.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]
    lib.l7g_classify_streams.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp,
                                         vp, vp, vp]
    lib.l7g_classify_host.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint32, vp, vp, vp]
    lib.l7g_cass_sessions_enable.argtypes = [vp, C.c_uint32, cp, sz]
    lib.l7g_cass_replies.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint32, vp, vp, vp]
    lib.l7g_cass_replies_host.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint32, vp, vp]
    lib.l7g_cass_session_reset.argtypes = [vp, vp, C.c_uint32]
    lib.l7g_cass_session_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.l7g_cass_session_stats.restype = None
    lib.l7g_service_enable.argtypes = [vp, C.c_int]
    lib.l7g_service_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.l7g_service_stats.restype = None
    lib.l7g_stats.argtypes = [vp, C.POINTER(Stats)]
    lib.l7g_debug_regex.argtypes = [cp, sz, C.c_int, cp, sz, cp, sz]
    lib.l7g_debug_regex_nfa.argtypes = [cp, sz, C.c_int, cp, sz, cp, sz]
    lib.l7g_debug_phase_times.argtypes = [vp, vp, C.c_int]
    lib.l7g_debug_kafka_phase_times.argtypes = [vp, vp, C.c_int]
    lib.l7g_debug_frame_phase_times.argtypes = [vp, vp, C.c_int]
    lib.l7g_kafka_corr_create.restype = vp
    lib.l7g_kafka_corr_destroy.argtypes = [vp]
    lib.l7g_kafka_corr_requests.argtypes = [vp, vp, vp, vp, C.c_uint32, vp]
    lib.l7g_kafka_corr_responses.argtypes = [vp, vp, vp, vp, C.c_uint32, vp]
    lib.l7g_kafka_corr_gc.restype = C.c_uint64
    lib.l7g_kafka_corr_gc.argtypes = [vp, C.c_uint64]
    lib.l7g_kafka_corr_size.restype = C.c_uint64
    lib.l7g_kafka_corr_size.argtypes = [vp]
    lib.l7g_kafka_deny_response.argtypes = [cp, sz, vp, sz, C.POINTER(C.c_size_t)]
    lib.l7g_profile_enable.argtypes = [vp, C.c_int]
    lib.l7g_flow_stats_enable.argtypes = [vp, C.c_int]
    lib.l7g_flow_stats.argtypes = [vp, vp, C.c_uint32, C.POINTER(C.c_uint32), C.c_int]
    lib.l7g_profile_last.argtypes = [vp, vp]
    # (a library named by L7G_LIB or by path may be an earlier build without the logged calls, as in an
    # A/B against the parent commit's: it loads, and calling them raises AttributeError.  libl7gpu.so
    # has them: tests/test_access_log_abi.py)
    if hasattr(lib, "l7g_classify_logged"):
        lib.l7g_classify_logged.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint32, vp, vp, vp, vp,
                                            C.POINTER(LogOut), vp]
        lib.l7g_classify_logged_host.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint32, vp, vp, vp,
                                                 C.POINTER(LogOut)]
        lib.l7g_kafka_api_key_name.restype = cp
        lib.l7g_kafka_api_key_name.argtypes = [C.c_int16]
    # (the same for every parser's records: tests/test_generic_log_abi.py)
    if hasattr(lib, "l7g_classify_logged_all"):
        lib.l7g_classify_logged_all.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint32, vp, vp, vp, vp,
                                                C.POINTER(LogAllOut), vp]
        lib.l7g_classify_logged_all_host.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint32, vp, vp, vp,
                                                     C.POINTER(LogAllOut)]
        lib.l7g_cass_action_name.restype = cp
        lib.l7g_cass_action_name.argtypes = [C.c_int16]
    # (the same for the deny replies: tests/test_deny_replies_host.py)
    if hasattr(lib, "l7g_deny_replies"):
        lib.l7g_deny_replies.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint32, vp, C.POINTER(ReplyOut), vp]
        lib.l7g_deny_replies_host.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint32, vp, C.POINTER(ReplyOut)]
        lib.l7g_deny_reply_template.restype = vp
        lib.l7g_deny_reply_template.argtypes = [C.c_int, C.POINTER(C.c_size_t)]
    # (the same for the Kafka sessions: tests/test_kafka_sessions_host.py)
    if hasattr(lib, "l7g_kafka_sessions_enable"):
        u64, u32 = C.c_uint64, C.c_uint32
        lib.l7g_kafka_sessions_enable.argtypes = [vp, u32, cp, sz]
        lib.l7g_kafka_forward.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, u32, u64, vp, vp, vp]
        lib.l7g_kafka_responses.argtypes = [vp, vp, u64, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp]
        lib.l7g_kafka_forward_host.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, u32, u64, vp, vp]
        lib.l7g_kafka_responses_host.argtypes = [vp, vp, u64, vp, vp, vp, u32, vp, vp, vp, vp, vp]
        lib.l7g_kafka_session_gc.argtypes = [vp, u64, u64, C.POINTER(u64)]
        lib.l7g_kafka_session_reset.argtypes = [vp, vp, u32]
        lib.l7g_kafka_session_stats.argtypes = [vp, C.POINTER(u64)]
        lib.l7g_kafka_session_stats.restype = None
    # (the same for the memcached sessions: tests/test_mc_sessions_host.py)
    if hasattr(lib, "l7g_mc_sessions_enable"):
        u64, u32 = C.c_uint64, C.c_uint32
        lib.l7g_mc_sessions_enable.argtypes = [vp, u32, cp, sz]
        lib.l7g_mc_forward.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, u32, vp, vp]
        lib.l7g_mc_replies.argtypes = [vp, vp, u64, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp]
        lib.l7g_mc_forward_host.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, u32, vp]
        lib.l7g_mc_replies_host.argtypes = [vp, vp, u64, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp]
        lib.l7g_mc_session_reset.argtypes = [vp, vp, u32]
        lib.l7g_mc_session_stats.argtypes = [vp, C.POINTER(u64)]
        lib.l7g_mc_session_stats.restype = None
        lib.l7g_mc_denied_message.restype = vp
        lib.l7g_mc_denied_message.argtypes = [C.c_int, C.POINTER(C.c_size_t)]
    _libs[path] = lib
    return lib


def debug_regex(pattern, data, anchored=True, nfa=False):
    """Compile `pattern` with the product's Go-regexp DFA compiler (nfa=True:
    the bit-parallel NFA fallback) and run the compiled tables on `data` (host
    walk of the device tables; test hook).  Returns True/False, or raises
    ValueError with Go's compile error text."""
    lib = load()
    p = pattern.encode() if isinstance(pattern, str) else pattern
    d = data.encode() if isinstance(data, str) else data
    err = C.create_string_buffer(512)
    fn = lib.l7g_debug_regex_nfa if nfa else lib.l7g_debug_regex
    r = fn(p, len(p), 1 if anchored else 0, d, len(d), err, 512)
    if r < 0:
        raise ValueError(err.value.decode(errors="replace"))
    return bool(r)


def kafka_api_key_name(key):
    """The policy language's name of a Kafka API key (apiKeyToString), or None
    for a key it does not name (print that one in decimal)."""
    r = load().l7g_kafka_api_key_name(int(key))
    return r.decode() if r is not None else None


def cass_action_name(action):
    """The cassandra parser's name of action id 0..37 (its queryActionMap, in
    kernels/cass_parse.h order), or None outside."""
    r = load().l7g_cass_action_name(int(action))
    return r.decode() if r is not None else None


def deny_reply_template(proto):
    """The fixed reply a denied request on a PROTO_HTTP, PROTO_CASSANDRA or
    PROTO_R2D2 connection is answered with (csrc/deny_templates.h; cassandra's
    before its three request bytes are set); b"" for any other protocol."""
    n = C.c_size_t(0)
    p = load().l7g_deny_reply_template(int(proto), C.byref(n))
    return C.string_at(p, n.value) if p else b""


# bytes a wave of the memcached sessions' reply kernel looks at per step (csrc/kernels/mc_session.h kMcSessStep)
MC_SESS_WINDOW = 64


def mc_denied_message(binary=False):
    """The memcached parsers' denied message (csrc/deny_templates.h): the text
    parser's 28 bytes, or the binary parser's 37 (the sender sets byte 0 =
    0x81 | the request's byte 0)."""
    n = C.c_size_t(0)
    p = load().l7g_mc_denied_message(1 if binary else 0, C.byref(n))
    return C.string_at(p, n.value)


def kafka_deny_response(req):
    """The bytes the Kafka proxy answers a denied request with
    (CreateResponse(ErrTopicAuthorizationFailed)), or None (untyped kind /
    undecodable request: no response)."""
    lib = load()
    cap = 4 * len(req) + 256
    out = C.create_string_buffer(cap)
    n = C.c_size_t(0)
    rc = lib.l7g_kafka_deny_response(req, len(req), out, cap, C.byref(n))
    if rc == -1:
        return None
    if rc != 0:
        raise RuntimeError(f"l7g_kafka_deny_response: {rc}")
    return out.raw[:n.value]


class KafkaCorrelationCache:
    """One client connection's correlation cache (l7g_kafka_corr_*): batches
    of frames given as (arena: writable uint8 numpy array, offsets, lengths)."""

    def __init__(self):
        self._lib = load()
        self._h = self._lib.l7g_kafka_corr_create()

    def __del__(self):
        try:
            self._lib.l7g_kafka_corr_destroy(self._h)
        except Exception:
            pass

    def requests(self, arena, offs, lens):
        import numpy as np
        o = np.ascontiguousarray(offs, np.uint64)
        n = np.ascontiguousarray(lens, np.uint32)
        ids = np.zeros(len(o), np.uint32)
        self._lib.l7g_kafka_corr_requests(self._h, arena.ctypes.data, o.ctypes.data, n.ctypes.data, len(o), ids.ctypes.data)
        return ids

    def responses(self, arena, offs, lens):
        import numpy as np
        o = np.ascontiguousarray(offs, np.uint64)
        n = np.ascontiguousarray(lens, np.uint32)
        found = np.zeros(len(o), np.uint8)
        self._lib.l7g_kafka_corr_responses(self._h, arena.ctypes.data, o.ctypes.data, n.ctypes.data, len(o),
                                           found.ctypes.data)
        return found.astype(bool)

    def gc(self, lifetime_ms):
        return int(self._lib.l7g_kafka_corr_gc(self._h, lifetime_ms))

    def __len__(self):
        return int(self._lib.l7g_kafka_corr_size(self._h))

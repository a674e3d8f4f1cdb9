"""The access-log part of the C-ABI (include/l7gpu.h: l7g_logrec_t, l7g_span_t,
l7g_classify_logged, l7g_classify_logged_host, l7g_kafka_api_key_name) as the
Python binding sees it; no device needed."""
import ctypes as C

import numpy as np

from cilium_amd import _lib, api, engine


def test_structure_sizes():
    assert C.sizeof(_lib.LogRec) == 32
    assert C.sizeof(_lib.Span) == 8
    assert engine.LOGREC_DTYPE.itemsize == 32 and engine.SPAN_DTYPE.itemsize == 8


def test_numpy_record_matches_the_ctypes_one():
    rec = _lib.LogRec()
    rec.kind, rec.flags, rec.api_key = 2, 1, -3
    rec.u.kafka.api_version, rec.u.kafka.correlation_id, rec.u.kafka.ntopics = 7, -5, 300
    a = np.frombuffer(bytes(rec), engine.LOGREC_DTYPE)[0]
    assert (a["kind"], a["flags"], a["api_key"], a["api_version"], a["correlation_id"], a["ntopics"]) == \
        (2, 1, -3, 7, -5, 300)
    rec = _lib.LogRec()
    rec.kind = 1
    for k, name in enumerate(("method_len", "path_len", "host_off", "host_len", "head_len", "nheaders")):
        setattr(rec.u.http, name, 100 + k)
    a = np.frombuffer(bytes(rec), engine.LOGREC_DTYPE)[0]
    assert [int(a[n]) for n in ("method_len", "path_len", "host_off", "host_len", "head_len", "nheaders")] == \
        list(range(100, 106))


def test_symbols_are_exported():
    lib = _lib.load()
    for name in ("l7g_classify_logged", "l7g_classify_logged_host", "l7g_kafka_api_key_name"):
        assert getattr(lib, name) is not None
        assert name in _lib.EXPORTS


def test_api_key_names_are_the_policy_languages():
    lib = _lib.load()
    by_key = {v: k for k, v in api.KAFKA_API_KEYS.items()}
    assert len(by_key) == len(api.KAFKA_API_KEYS)
    for key in range(0, 41):
        got = lib.l7g_kafka_api_key_name(key)
        if key in by_key:
            assert got is not None and got.decode() == by_key[key], key
        else:
            assert got is None, key
    for key in (-1, -32768, 41, 64, 32767):
        assert lib.l7g_kafka_api_key_name(key) is None
    assert _lib.kafka_api_key_name(0) == "produce" and _lib.kafka_api_key_name(99) is None


def test_host_only_engine_refuses_the_logged_calls():
    e = engine.Engine(device=-1)
    rec = np.zeros(1, engine.LOGREC_DTYPE)
    lo = _lib.LogOut(rec.ctypes.data, None, 0)
    z = np.zeros(4, np.uint64)
    assert lib_rc(e, z, lo) != 0
    e.close()


def lib_rc(e, z, lo):
    return e._lib.l7g_classify_logged_host(e._h, z.ctypes.data, 0, z.ctypes.data, z.ctypes.data, z.ctypes.data, 1,
                                           z.ctypes.data, z.ctypes.data, z.ctypes.data, C.byref(lo))

"""The part of the C-ABI l7g_classify_logged_all adds (include/l7gpu.h: the
mc_text / mc_binary / r2d2 / cassandra members of l7g_logrec_t,
l7g_log_all_out_t, l7g_classify_logged_all, l7g_classify_logged_all_host,
l7g_cass_action_name) as the Python binding sees it; no device needed."""
import ctypes as C

import numpy as np

from cilium_amd import _lib, api, engine

HIP_INVALID_VALUE, HIP_NO_DEVICE = 1, 100

MEMBERS = {  # union member -> (numpy prefix, fields in order: consecutive uint32 from byte 4)
    "mc_text": ("mc_", ("cmd_off", "cmd_len", "nkeys")),
    "mc_binary": ("mcb_", ("key_off", "key_len")),
    "r2d2": ("r2_", ("cmd_len", "file_off", "file_len", "nfields")),
    "cassandra": ("cass_", ("table_len", "keyword", "word_off", "word_len")),
}


def test_sizes_stay():
    assert C.sizeof(_lib.LogRec) == 32 and engine.LOGREC_DTYPE.itemsize == 32
    assert _lib.LogRec.u.offset == 4 and _lib.LogRec.reserved.offset == 28
    assert C.sizeof(_lib.LogAllOut) == 40
    assert [(_lib.LogAllOut.rec.offset, _lib.LogAllOut.spans.offset, _lib.LogAllOut.span_stride.offset,
             _lib.LogAllOut.text.offset, _lib.LogAllOut.text_stride.offset)] == [(0, 8, 16, 24, 32)]
    assert (_lib.LOG_MC_TEXT, _lib.LOG_MC_BINARY, _lib.LOG_R2D2, _lib.LOG_CASSANDRA) == (3, 4, 5, 6)


def test_new_members_against_numpy():
    for member, (prefix, names) in MEMBERS.items():
        rec = _lib.LogRec()
        rec.kind, rec.flags, rec.api_key = 6, 5, -1
        for k, name in enumerate(names):
            setattr(getattr(rec.u, member), name, 1000 + k)
            assert getattr(type(getattr(rec.u, member)), name).offset == 4 * k, (member, name)
            assert engine.LOGREC_DTYPE.fields[prefix + name][1] == 4 + 4 * k, (member, name)
        a = np.frombuffer(bytes(rec), engine.LOGREC_DTYPE)[0]
        assert (a["kind"], a["flags"], a["api_key"]) == (6, 5, -1)
        assert [int(a[prefix + n]) for n in names] == list(range(1000, 1000 + len(names))), member
    # the members of the HTTP and Kafka views are where they were
    f = engine.LOGREC_DTYPE.fields
    assert [f[n][1] for n in ("method_len", "nheaders", "api_version", "correlation_id", "ntopics")] == [4, 24, 4, 8, 12]


def test_symbols_are_exported():
    lib = _lib.load()
    for name in ("l7g_classify_logged_all", "l7g_classify_logged_all_host", "l7g_cass_action_name"):
        assert getattr(lib, name) is not None
        assert name in _lib.EXPORTS


# queryActionMap's keys (cassandraparser.go:319-366) in the order of the action ids (kernels/cass_parse.h)
CASS_ACTIONS = (
    "select", "delete", "insert", "update", "create-table", "drop-table", "alter-table", "truncate-table", "use",
    "create-keyspace", "alter-keyspace", "drop-keyspace", "drop-index", "create-index", "create-materialized-view",
    "drop-materialized-view", "create-role", "alter-role", "drop-role", "grant-role", "revoke-role", "list-roles",
    "grant-permission", "revoke-permission", "list-permissions", "create-user", "alter-user", "drop-user", "list-users",
    "create-function", "drop-function", "create-aggregate", "drop-aggregate", "create-type", "alter-type", "drop-type",
    "create-trigger", "drop-trigger")


def test_cass_action_names_are_the_policy_parsers():
    lib = _lib.load()
    assert len(CASS_ACTIONS) == 38 and len(set(CASS_ACTIONS)) == 38
    for a in range(-1, 41):
        got = lib.l7g_cass_action_name(a)
        if 0 <= a < 38:
            assert got is not None and got.decode() == CASS_ACTIONS[a], a
        else:
            assert got is None, a
    assert _lib.cass_action_name(0) == "select" and _lib.cass_action_name(38) is None
    assert _lib.cass_action_name(-1) is None
    # the policy parser takes exactly these names as a rule's query_action
    e = engine.Engine(device=-1)

    def pol(action):
        return api.policy_set(api.network_policy("cs", 11, ingress=[(9042, [api.port_rule(
            l7proto="cassandra", l7=[{"query_action": action}])])]))
    for name in CASS_ACTIONS:
        e.update_policy(pol(name))
    for name in ("truncate-foo", "alter-materialized-view", "selectx"):
        try:
            e.update_policy(pol(name))
        except Exception as ex:  # PolicyError
            assert "query_action" in str(ex)
        else:
            raise AssertionError(name)
    e.close()


def _call(e, lo, host=True):
    z = np.zeros(8, np.uint64)
    p = z.ctypes.data
    if host:
        return e._lib.l7g_classify_logged_all_host(e._h, p, 0, p, p, p, 1, p, p, p, C.byref(lo))
    return e._lib.l7g_classify_logged_all(e._h, p, 0, p, p, p, 1, p, p, p, None, C.byref(lo), None)


def test_host_only_engine_refuses_both_calls():
    e = engine.Engine(device=-1)
    rec = np.zeros(2, engine.LOGREC_DTYPE)
    lo = _lib.LogAllOut(rec.ctypes.data, None, 0, None, 0)
    assert _call(e, lo, host=True) == HIP_NO_DEVICE
    assert _call(e, lo, host=False) == HIP_NO_DEVICE
    e.close()


def test_argument_errors():
    e = engine.Engine(device=-1)
    rec = np.zeros(2, engine.LOGREC_DTYPE)
    row = np.zeros(64, np.uint8)
    for lo in (_lib.LogAllOut(None, None, 0, None, 0),                        # no records
               _lib.LogAllOut(rec.ctypes.data, None, 4, None, 0),             # a span stride without rows
               _lib.LogAllOut(rec.ctypes.data, None, 0, None, 16),            # a text stride without rows
               _lib.LogAllOut(rec.ctypes.data, row.ctypes.data, 4, None, 16)):
        assert _call(e, lo, host=True) == HIP_INVALID_VALUE
    z = np.zeros(8, np.uint64)
    p = z.ctypes.data
    assert e._lib.l7g_classify_logged_all_host(e._h, p, 0, p, p, p, 1, p, p, p, None) == HIP_INVALID_VALUE
    assert e._lib.l7g_classify_logged_all(e._h, p, 0, p, p, p, 1, p, p, p, None, None, None) == HIP_INVALID_VALUE
    # NULL rows with stride 0 are valid: the call gets as far as the missing device
    assert _call(e, _lib.LogAllOut(rec.ctypes.data, None, 0, None, 0)) == HIP_NO_DEVICE
    e.close()

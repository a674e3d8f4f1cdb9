"""Return codes of the host-buffer calls and of the device-pointer entries
behind them, on a host-only engine.  Each entry checks its arguments and the
device in an order of its own (l7g_classify_logged_host rejects a null log
before it looks at the device; l7g_deny_replies_host reports no-device first),
and callers see that order in the code they get.  The table below was recorded
from the library before its entries came to share their prologue (the memcached
rows before the three protocols' session entries came to share theirs); run this
file as a script to print the table of the library as built.  Nothing here
reaches a GPU call."""
import ctypes as C

import numpy as np

from cilium_amd import _lib
from cilium_amd.engine import Engine

OK, INVALID, NOT_READY, NO_DEVICE = 0, 1, 600, 100  # hipSuccess, hipErrorInvalidValue, NotReady, NoDevice

EXPECTED = {
    "l7g_classify": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100},
    "l7g_classify_host": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100},
    "l7g_classify_logged": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100, "null_log": 1,
                            "null_rec": 100, "stride_no_rows": 100},
    "l7g_classify_logged_host": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100, "null_log": 1,
                                 "null_rec": 1, "stride_no_rows": 1},
    "l7g_classify_logged_all": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100, "null_log": 1,
                                "null_rec": 100, "stride_no_rows": 100, "text_stride_no_rows": 100},
    "l7g_classify_logged_all_host": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100, "null_log": 1,
                                     "null_rec": 1, "stride_no_rows": 1, "text_stride_no_rows": 1},
    "l7g_deny_replies": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100, "null_out": 100,
                         "null_out_off": 100, "cap_no_buf": 100},
    "l7g_deny_replies_host": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100, "null_out": 100,
                              "null_out_off": 100, "cap_no_buf": 100},
    "l7g_cass_replies": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100},
    "l7g_cass_replies_host": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100},
    "l7g_kafka_forward": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100},
    "l7g_kafka_forward_host": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100},
    "l7g_kafka_responses": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100},
    "l7g_kafka_responses_host": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100},
    "l7g_cass_sessions_enable": {"on": 100, "off": 100},
    "l7g_kafka_sessions_enable": {"on": 100, "off": 100},
    "l7g_cass_session_reset": {"sessions_off": 100},
    "l7g_kafka_session_reset": {"sessions_off": 100},
    "l7g_kafka_session_gc": {"sessions_off": 100},
    "l7g_mc_forward": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100},
    "l7g_mc_forward_host": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100},
    "l7g_mc_replies": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100},
    "l7g_mc_replies_host": {"ok": 100, "n0": 100, "null_arrays": 100, "null_outputs": 100},
    "l7g_mc_sessions_enable": {"on": 100, "off": 100},
    "l7g_mc_session_reset": {"sessions_off": 100},
}


class _Bufs:
    """One request of 16 bytes on connection 0, and every output a call could ask for."""

    def __init__(self):
        self.arena = np.zeros(64, np.uint8)
        self.off = np.zeros(1, np.uint64)
        self.len = np.full(1, 16, np.uint32)
        self.conn = np.zeros(1, np.uint32)
        self.verdict = np.zeros(1, np.uint8)
        self.rule = np.zeros(1, np.int32)
        self.consumed = np.zeros(1, np.uint32)
        self.rec = np.zeros(32, np.uint8)
        self.spans = np.zeros(2 * 8, np.uint8)
        self.text = np.zeros(16, np.uint8)
        self.r_off = np.zeros(1, np.uint64)
        self.r_len = np.zeros(1, np.uint32)
        self.total = np.zeros(2, np.uint64)
        self.buf = np.zeros(64, np.uint8)
        self.fwd = np.zeros(1, np.uint8)
        self.ids = np.zeros(1, np.uint32)
        self.key = np.zeros(1, np.int16)
        self.ver = np.zeros(1, np.int16)
        self.tag = np.zeros(1, np.uint64)


def _p(a):
    return a.ctypes.data


def table():
    """{entry: {case: return code}} of the library as built, on a host-only engine."""
    e = Engine(device=-1)
    L, h, b = e._lib, e._h, _Bufs()
    got = {}

    def inputs(case):
        n = 0 if case == "n0" else 1
        if case == "null_arrays":
            return (_p(b.arena), b.arena.nbytes, None, None, None, n)
        return (_p(b.arena), b.arena.nbytes, _p(b.off), _p(b.len), _p(b.conn), n)

    def vrc(case):
        return (None, None, None) if case == "null_outputs" else (_p(b.verdict), _p(b.rule), _p(b.consumed))

    common = ("ok", "n0", "null_arrays", "null_outputs")
    try:
        got["l7g_classify"] = {c: L.l7g_classify(h, *inputs(c), *vrc(c), None, None) for c in common}
        got["l7g_classify_host"] = {c: L.l7g_classify_host(h, *inputs(c), *vrc(c)) for c in common}

        def log(case):
            if case == "null_log":
                return None
            lo = _lib.LogOut(_p(b.rec), _p(b.spans), 2)
            if case == "null_rec":
                lo.rec = None
            if case == "stride_no_rows":
                lo.topics = None
            return C.byref(lo)

        def log_all(case):
            if case == "null_log":
                return None
            lo = _lib.LogAllOut(_p(b.rec), _p(b.spans), 2, _p(b.text), 16)
            if case == "null_rec":
                lo.rec = None
            if case == "stride_no_rows":
                lo.spans = None
            if case == "text_stride_no_rows":
                lo.text = None
            return C.byref(lo)

        logged = common + ("null_log", "null_rec", "stride_no_rows")
        got["l7g_classify_logged"] = {c: L.l7g_classify_logged(h, *inputs(c), *vrc(c), None, log(c), None)
                                      for c in logged}
        got["l7g_classify_logged_host"] = {c: L.l7g_classify_logged_host(h, *inputs(c), *vrc(c), log(c))
                                           for c in logged}
        logged_all = logged + ("text_stride_no_rows",)
        got["l7g_classify_logged_all"] = {c: L.l7g_classify_logged_all(h, *inputs(c), *vrc(c), None, log_all(c), None)
                                          for c in logged_all}
        got["l7g_classify_logged_all_host"] = {c: L.l7g_classify_logged_all_host(h, *inputs(c), *vrc(c), log_all(c))
                                               for c in logged_all}

        def reply(case):
            if case == "null_out":
                return None
            ro = _lib.ReplyOut(_p(b.buf), b.buf.nbytes, _p(b.r_off), _p(b.r_len), _p(b.total))
            if case == "null_out_off":
                ro.off = None
            if case == "cap_no_buf":
                ro.buf = None
            return C.byref(ro)

        def v_in(case):
            return None if case == "null_outputs" else _p(b.verdict)

        deny = common + ("null_out", "null_out_off", "cap_no_buf")
        got["l7g_deny_replies"] = {c: L.l7g_deny_replies(h, *inputs(c), v_in(c), reply(c), None) for c in deny}
        got["l7g_deny_replies_host"] = {c: L.l7g_deny_replies_host(h, *inputs(c), v_in(c), reply(c)) for c in deny}

        # sessions are not enabled (a host-only engine cannot enable them)
        got["l7g_cass_replies"] = {c: L.l7g_cass_replies(h, *inputs(c), *vrc(c)[::2], None) for c in common}
        got["l7g_cass_replies_host"] = {c: L.l7g_cass_replies_host(h, *inputs(c), *vrc(c)[::2]) for c in common}

        def fwd_args(c):
            out = (None, None) if c == "null_outputs" else (_p(b.fwd), _p(b.ids))
            return (*inputs(c)[:5], v_in(c), None, inputs(c)[5], 1000, *out)

        def resp_args(c):
            out = (None,) * 5 if c == "null_outputs" else (_p(b.fwd), _p(b.ids), _p(b.key), _p(b.ver), _p(b.tag))
            return (*inputs(c), *out)

        got["l7g_kafka_forward"] = {c: L.l7g_kafka_forward(h, *fwd_args(c), None) for c in common}
        got["l7g_kafka_forward_host"] = {c: L.l7g_kafka_forward_host(h, *fwd_args(c)) for c in common}
        got["l7g_kafka_responses"] = {c: L.l7g_kafka_responses(h, *resp_args(c), None) for c in common}
        got["l7g_kafka_responses_host"] = {c: L.l7g_kafka_responses_host(h, *resp_args(c)) for c in common}

        def mc_fwd_args(c):
            out = (None,) if c == "null_outputs" else (_p(b.fwd),)
            return (*inputs(c)[:5], v_in(c), None, inputs(c)[5], *out)

        def mc_rep_args(c):
            out = (None,) * 6 if c == "null_outputs" else (_p(b.fwd), _p(b.ids), _p(b.tag), _p(b.r_len), _p(b.verdict),
                                                           _p(b.total))
            return (*inputs(c), 1, *out)

        got["l7g_mc_forward"] = {c: L.l7g_mc_forward(h, *mc_fwd_args(c), None) for c in common}
        got["l7g_mc_forward_host"] = {c: L.l7g_mc_forward_host(h, *mc_fwd_args(c)) for c in common}
        got["l7g_mc_replies"] = {c: L.l7g_mc_replies(h, *mc_rep_args(c), None) for c in common}
        got["l7g_mc_replies_host"] = {c: L.l7g_mc_replies_host(h, *mc_rep_args(c)) for c in common}

        err = C.create_string_buffer(256)
        got["l7g_cass_sessions_enable"] = {"on": L.l7g_cass_sessions_enable(h, 64, err, 256),
                                           "off": L.l7g_cass_sessions_enable(h, 0, err, 256)}
        got["l7g_kafka_sessions_enable"] = {"on": L.l7g_kafka_sessions_enable(h, 64, err, 256),
                                            "off": L.l7g_kafka_sessions_enable(h, 0, err, 256)}
        got["l7g_mc_sessions_enable"] = {"on": L.l7g_mc_sessions_enable(h, 64, err, 256),
                                         "off": L.l7g_mc_sessions_enable(h, 0, err, 256)}
        got["l7g_mc_session_reset"] = {"sessions_off": L.l7g_mc_session_reset(h, _p(b.conn), 1)}
        got["l7g_cass_session_reset"] = {"sessions_off": L.l7g_cass_session_reset(h, _p(b.conn), 1)}
        got["l7g_kafka_session_reset"] = {"sessions_off": L.l7g_kafka_session_reset(h, _p(b.conn), 1)}
        gone = C.c_uint64(7)
        got["l7g_kafka_session_gc"] = {"sessions_off": L.l7g_kafka_session_gc(h, 1000, 10, C.byref(gone))}
        assert gone.value == 0
    finally:
        e.close()
    return got


def test_return_codes_match_the_recorded_table():
    got = table()
    assert set(got) == set(EXPECTED)
    diff = {(k, c): (got[k].get(c), EXPECTED[k].get(c)) for k in EXPECTED for c in set(got[k]) | set(EXPECTED[k])
            if got[k].get(c) != EXPECTED[k].get(c)}
    assert not diff, diff  # {(entry, case): (got, recorded)}


def test_the_table_sees_both_orders():
    # the two orders the table exists to pin: arguments first, and the device first
    assert EXPECTED["l7g_classify_logged_host"]["null_rec"] == INVALID
    assert EXPECTED["l7g_classify_logged"]["null_rec"] == NO_DEVICE
    assert EXPECTED["l7g_deny_replies_host"]["null_out"] == NO_DEVICE
    assert all(c in (INVALID, NO_DEVICE) for row in EXPECTED.values() for c in row.values())


if __name__ == "__main__":
    import pprint

    pprint.pprint(table(), width=120)

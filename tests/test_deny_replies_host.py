"""The deny-reply calls (include/l7gpu.h: l7g_deny_replies,
l7g_deny_replies_host) as far as a machine without a GPU can see them: the
symbols, their behaviour on a host-only engine, and the shared reply templates
(csrc/deny_templates.h), restated here from the reference lines they cite."""
import ctypes as C

import numpy as np
import pytest

from cilium_amd import _lib
from cilium_amd._lib import PROTO_CASSANDRA, PROTO_HTTP, PROTO_KAFKA, PROTO_MEMCACHE, PROTO_R2D2
from cilium_amd.engine import Engine

HIP_ERROR_INVALID_VALUE = 1
HIP_ERROR_NO_DEVICE = 100

# envoy/cilium_l7policy.cc:90-96,171-177: sendLocalReply(Forbidden, "Access denied\r\n")
DENIED_403 = (b"HTTP/1.1 403 Forbidden\r\ncontent-length: 15\r\ncontent-type: text/plain\r\n\r\n"
              b"Access denied\r\n")
# proxylib/cassandra/cassandraparser.go:269-278 unauthMsgBase
CASS_UNAUTH = bytes([0, 0, 0, 0, 0, 0, 0, 0, 0x1a, 0, 0, 0x21, 0, 0, 0x14]) + b"Request Unauthorized"
R2D2_ERROR = b"ERROR\r\n"


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for name in ("l7g_deny_replies", "l7g_deny_replies_host", "l7g_deny_reply_template"):
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes is not None
    assert C.sizeof(_lib.ReplyOut) == 40  # l7g_reply_out_t: five 8-byte members
    assert callable(Engine.deny_replies) and callable(Engine.deny_replies_device)


def _host_args(n=1):
    arena = np.zeros(64, np.uint8)
    off = np.zeros(n, np.uint64)
    ln = np.full(n, 16, np.uint32)
    cid = np.zeros(n, np.uint32)
    v = np.zeros(n, np.uint8)
    ro = np.zeros(n, np.uint64)
    rl = np.zeros(n, np.uint32)
    tot = np.zeros(2, np.uint64)
    keep = (arena, off, ln, cid, v, ro, rl, tot)
    out = _lib.ReplyOut(None, 0, ro.ctypes.data, rl.ctypes.data, tot.ctypes.data)
    return keep, (arena.ctypes.data, arena.nbytes, off.ctypes.data, ln.ctypes.data, cid.ctypes.data, n,
                  v.ctypes.data), out


def test_host_only_engine_has_no_device():
    e = Engine(device=-1)
    try:
        keep, args, out = _host_args()
        assert e._lib.l7g_deny_replies(e._h, *args, C.byref(out), None) == HIP_ERROR_NO_DEVICE
        assert e._lib.l7g_deny_replies_host(e._h, *args, C.byref(out)) == HIP_ERROR_NO_DEVICE
        with pytest.raises(RuntimeError):
            e.deny_replies(keep[0], keep[1], keep[2], keep[3], keep[4])
    finally:
        e.close()


def test_templates_are_the_cited_literals():
    assert (len(DENIED_403), len(CASS_UNAUTH), len(R2D2_ERROR)) == (87, 35, 7)
    assert _lib.deny_reply_template(PROTO_HTTP) == DENIED_403
    assert _lib.deny_reply_template(PROTO_CASSANDRA) == CASS_UNAUTH
    assert _lib.deny_reply_template(PROTO_R2D2) == R2D2_ERROR
    assert _lib.deny_reply_template(PROTO_KAFKA) == b"" and _lib.deny_reply_template(PROTO_MEMCACHE) == b""

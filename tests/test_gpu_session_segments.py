"""The sorted-key segments the session kernels share (kernels/sess_common.h:
segment_head, segment_end, the key past every connection), at the smallest
shapes where they can go wrong, through l7g_kafka_forward and l7g_mc_forward:
one request; 257 requests of one connection (the segment crosses a workgroup
and ends at n); two connections whose boundary lies at sorted positions
255 | 256 and 256 | 257; no request, every request and only the last request
taking no part (the sentinel segment absent, everything, a single key at the
end); and connection nconns - 1 of a power-of-two nconns (the sort's last
connection bit).  Every batch is sent twice: a segment's end shows in what the
slot has advanced by, which the second call's outputs depend on.

Held to the models the session tests use (tests/kafka_sessions_py.py,
tests/mc_sessions_py.py) through those tests' own Dev classes, which compare
every output array, the rewritten arena and the session statistics in full
after every call."""
import numpy as np
import pytest

from cilium_amd import gen
from test_gpu_kafka_sessions import Dev as KafkaDev, kafka_conns, req
from test_gpu_mc_sessions import Dev as McDev, mc_conns

pytestmark = pytest.mark.gpu

DENY, ALLOW, OTHER = 0, 1, 4  # (OTHER: a verdict with which a memcached request takes no part)


def _shapes():
    """name -> (nconns, connection per request, takes part per request)"""
    rng = np.random.default_rng(5)
    s = {"n1": (1, [0], [True]),
         "one_connection_257": (3, [1] * 257, [True] * 257)}
    for a in (256, 257):    # connection 0 holds sorted positions 0 .. a - 1, connection 2 the rest, in a shuffled batch
        s[f"boundary_{a - 1}_{a}"] = (3, rng.permutation([0] * a + [2] * (300 - a)).tolist(), [True] * 300)
    mixed = rng.integers(0, 4, size=257).tolist()
    s["sentinel_absent"] = (4, mixed, [True] * 257)
    s["sentinel_is_everything"] = (4, mixed, [False] * 257)
    s["sentinel_is_the_last_key"] = (4, mixed, [True] * 256 + [False])
    s["sentinel_n1"] = (1, [0], [False])
    # nconns = 64: connection 63 sets every connection bit, and the key of a request that takes no part one more
    s["last_connection_of_64"] = (64, [63, 0, 63, 17, 63, 62, 63, 0], [True, True, True, False, True, True, True, True])
    return s


SHAPES = _shapes()


@pytest.fixture(scope="module")
def sengine():
    from cilium_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_kafka_forward_segments(sengine, shape):
    nconns, conn, part = SHAPES[shape]
    sengine.update_policy(gen.cfg3_policy())
    d = KafkaDev(sengine, kafka_conns(nconns), 1024)
    frames = [req(1000 + i, key=i % 7, extra=b"x" * (i % 3)) for i in range(len(conn))]
    verdict = [ALLOW if p else DENY for p in part]
    want = {}
    for call in range(2):
        fwd, nid, _ = d.forward(frames, conn, verdict, now=call)
        # (the model's ids, spelled out: a connection numbers its forwarded requests 1, 2, ... in batch order)
        for i, (c, p) in enumerate(zip(conn, part)):
            want[c] = want.get(c, 0) + int(p)
            assert (int(fwd[i]), int(nid[i])) == ((1, want[c]) if p else (0, 0))
    st = d.check_stats()
    assert (st["forwarded"], st["dropped"], st["live"]) == (2 * sum(part), 0, 2 * sum(part))


@pytest.mark.parametrize("binary", [False, True], ids=["text", "binary"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_mc_forward_segments(sengine, shape, binary):
    nconns, conn, part = SHAPES[shape]
    sengine.update_policy(gen.mc_policy())
    d = McDev(sengine, mc_conns(nconns, flags=2 if binary else 1), 1024, device=True)
    n = len(conn)
    if binary:
        frames = [gen.mc_bin(0, key=b"k%d" % i) for i in range(n)]
    else:
        frames = [(b"get k%d\r\n", b"delete k%d\r\n", b"set k%d 0 0 1 noreply\r\nx\r\n")[i % 3] % i for i in range(n)]
    verdict = [(DENY if i % 4 == 2 else ALLOW) if p else OTHER for i, p in enumerate(part)]
    for _ in range(2):
        act, _ = d.forward(frames, conn, verdict)
        assert [a != 0 for a in act.tolist()] == part
    st = d.check_stats()
    assert st["sessions"] == len({c for c, p in zip(conn, part) if p}) and st["full"] == 0

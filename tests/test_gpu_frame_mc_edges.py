"""The stream framer (kernels/frame.hip: frame_text_kernel's separator masks
and byte-wise tokenizer, which write out the White_Space rule of
kernels/text_bytes.h; frame_streams_kernel's binary headers) on the directed edge corpus of
tests/mc_edge_cases.py.

Streams are built from the corpus requests that the oracle frames completely
inside their buffer (ALLOW or DENY with consumed <= len) in families A, B, C,
E, F and H: one wire format per stream (text streams on a connection whose
flags hold the text parser, binary ones on a binary connection), the Unicode
separators and near misses left in place.  Stream k starts at arena offset
k mod 16, so stream starts cover every residue, and the requests' lengths put
the frame boundaries inside the streams at every offset mod 16 (asserted).
Every fifth stream is cut: inside a White_Space rune, or between the CR and the
LF of a line end.  A storage line whose tokens[4] is negative has a size the
framer cannot read ahead of parsing (include/l7gpu.h: the walk stops there and
the classifier's consumed length says where the next frame starts), so such a
line is only ever a stream's last request, and the ones the Go frames shorter
than their line ("-3": the next frame would start inside it) stay out of the
streams; the classifier tests hold them.  test_gpu_frame._run checks the
frames against the oracle's sequential walk and the verdicts of every frame
against the oracle."""
import numpy as np
import pytest

import mc_edge_cases as E
from cilium_amd import gen
from cilium_amd._lib import ALLOW, DENY
from test_gpu_frame import _run

pytestmark = pytest.mark.gpu

PER_STREAM = 24
TEXT_CONN, BINARY_CONN = 1, 2   # E.conns(): flags 1 and 2, a remote inside gen.mc_policy()'s group


def _negative_size(req):
    t = req.split(b"\r\n")[0].split()
    return len(t) >= 5 and t[0] in (b"set", b"add", b"replace", b"append", b"prepend", b"cas") and \
        t[4][:1] == b"-" and t[4].strip(b"-0") != b""


def edge_streams(oracle):
    """(workload of the connections and policy, (connections, streams, request
    boundaries), arena residues of the frame boundaries inside streams)."""
    K = E.MC_POLICY_KEYS
    cases = [c for c in E.corpus(K) if c.family in "ABCEFH" and c.req]
    conns = E.conns()
    assert conns["flags"][TEXT_CONN] == 1 and conns["flags"][BINARY_CONN] == 2
    arena, offs, lens = gen.pack([c.req for c in cases])
    binary = np.array([c.family == "H" for c in cases])
    cid = np.where(binary, BINARY_CONN, TEXT_CONN).astype(np.uint32)
    base = gen.Workload("mc-edge-streams", arena, offs, lens, cid, conns, gen.mc_policy())
    v, _, c = oracle.classify_workload(base, 8)
    keep = ((v == ALLOW) | (v == DENY)) & (c <= lens)
    s_conns, streams, bounds, residues = [], [], [], set()
    for fmt, conn in ((False, TEXT_CONN), (True, BINARY_CONN)):
        idx = np.nonzero(keep & (binary == fmt))[0]
        reqs = [cases[i].req for i in idx if not _negative_size(cases[i].req)]
        lasts = [cases[i].req for i in idx if _negative_size(cases[i].req) and c[i] == lens[i]]
        for lo in range(0, len(reqs), PER_STREAM):
            k = len(streams)
            qs = reqs[lo:lo + PER_STREAM]
            if lasts and k % 5 != 3:
                qs.append(lasts.pop())
            s = b"".join(qs)
            b = list(np.cumsum([0] + [len(q) for q in qs[:-1]]))
            residues |= {(k + int(x)) % 16 for x in b[1:]}
            if k % 10 == 3 and not fmt:      # cut inside a White_Space rune
                at = [s.find(sp, len(s) // 2) for sp in E.WIDE_SPACES]
                at = [x for x in at if x >= 0]
                if at:
                    s = s[:min(at) + 1]
            elif k % 10 == 8 and not fmt:    # cut between a line end's CR and LF
                s = s[:s.rfind(b"\r\n") + 1]
            elif k % 5 == 3:                 # (binary: inside the last request's key)
                s = s[:-1]
            s_conns.append(conn)
            streams.append(s)
            bounds.append(b)
    return base, (s_conns, streams, bounds), residues


def test_edge_streams(engine, oracle):
    base, streams, residues = edge_streams(oracle)
    n = len(streams[1])
    assert n >= 64 and residues == set(range(16))
    assert {c for c in streams[0]} == {TEXT_CONN, BINARY_CONN}
    cut_rune = sum(1 for s in streams[1] if any(s.endswith(sp[:1]) for sp in E.WIDE_SPACES))
    cut_crlf = sum(1 for s in streams[1] if s.endswith(b"\r"))
    assert cut_rune >= 3 and cut_crlf >= 3
    ns, whole, frames = _run(engine, oracle, base, max_frames=64, streams=streams, align=16,
                             gaps=[k % 16 for k in range(n)])
    assert ns == n and frames > n * PER_STREAM * 3 // 4

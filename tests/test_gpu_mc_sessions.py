"""Memcached sessions on the GPU (l7g_mc_sessions_enable): l7g_mc_forward and
l7g_mc_replies against the literal Python model of the reference's two parsers
and op loop (tests/mc_sessions_py.py, pinned to the reference's recorded op
sequences by tests/test_mc_sessions_host.py).  Every comparison is exact:
act, ops, op_aux, nops, result, taken and the statistics, call by call; device
results are never compared with device results.

The engine of this file is its own: the session-scoped engine of conftest.py
never has sessions on."""
import numpy as np
import pytest

from cilium_amd import _lib, gen
from cilium_amd import proxylib as P
import mc_sessions_py as model
from mc_sessions_py import MORE, PASS, DROP, INJECT, OK, PARSER_ERROR
from test_mc_sessions_host import replay_golden
from test_oracle_kats import memcache_policy

pytestmark = pytest.mark.gpu

DENY, ALLOW = 0, 1
HIP_ERROR_NOT_READY = 600
W = _lib.MC_SESS_WINDOW
WAYS = pytest.mark.parametrize("device", [False, True], ids=["host", "device"])


@pytest.fixture(scope="module")
def sengine():
    from cilium_amd import Engine
    e = Engine(0)
    e.update_policy(gen.mc_policy())
    yield e
    e.close()


def mc_conns(n, flags=0, other=()):
    conns = gen.make_conns(n, 0, gen.MC_PORT, True, gen.PROTO_MEMCACHE, [3000 + k % 128 for k in range(n)])
    conns["flags"] = flags
    for c in other:
        conns["proto"][c] = gen.PROTO_KAFKA
    return conns


def pack(frames):
    """gen.pack with 16 spare bytes behind the arena: -> (arena, true length, offs, lens)"""
    arena, offs, lens = gen.pack(list(frames)) if len(frames) else (np.zeros(0, np.uint8), np.zeros(0, np.uint64),
                                                                    np.zeros(0, np.uint32))
    return np.concatenate([arena, np.zeros(16, np.uint8)]), len(arena), offs, lens


class Dev:
    """The engine and the model, kept in step; every call is compared in full."""

    def __init__(self, engine, conns, max_pending, device=False):
        self.e, self.device = engine, device
        self.e.mc_sessions(max_pending)
        self.e.set_connections(conns)
        self.m = model.Sessions(conns, max_pending)

    def _tensors(self, arrays):
        import torch
        dev = torch.device("cuda", 0)
        return [torch.from_numpy(a).to(dev) for a in arrays]

    def forward(self, frames, conn, verdict, tags=None, offs=None):
        n = len(frames)
        conn, verdict = np.asarray(conn, np.uint32), np.asarray(verdict, np.uint8)
        tags = np.arange(1, n + 1, dtype=np.uint64) * 1000003 if tags is None else np.asarray(tags, np.uint64)
        arena, alen, o, lens = pack(frames)
        inside = None
        if offs is not None:    # (a test of requests outside the arena)
            o = np.asarray(offs, np.uint64)
            inside = [int(a) + int(b) <= alen for a, b in zip(o, lens)]
        if not self.device:
            act = self.e.mc_forward(arena[:alen], o, lens, conn, verdict, tags)
        else:
            import torch
            d = self._tensors((arena, o.view(np.int64), lens.view(np.int32), conn.view(np.int32), verdict,
                               tags.view(np.int64)))
            out = torch.full((n,), 9, dtype=torch.uint8, device=d[0].device)
            self.e.mc_forward_device(d[0].data_ptr(), alen, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                     d[4].data_ptr(), d[5].data_ptr(), n, out.data_ptr(),
                                     stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            act = out.cpu().numpy()
        want, inj = self.m.forward(frames, conn, verdict, tags, inside)
        assert act.tolist() == want.tolist()
        self.check_stats()
        return act, inj

    def replies(self, streams, conn, max_ops=8, offs=None):
        n = len(streams)
        conn = np.asarray(conn, np.uint32)
        arena, alen, o, lens = pack(streams)
        inside = None
        if offs is not None:
            o = np.asarray(offs, np.uint64)
            inside = [int(a) + int(b) <= alen for a, b in zip(o, lens)]
        if not self.device:
            kind, opn, aux, nops, res, taken = self.e.mc_replies(arena[:alen], o, lens, conn, max_ops)
        else:
            import torch
            d = self._tensors((arena, o.view(np.int64), lens.view(np.int32), conn.view(np.int32)))
            dev = d[0].device
            t = [torch.full(shape, 9, dtype=ty, device=dev) for shape, ty in
                 (((n, max_ops), torch.uint8), ((n, max_ops), torch.int32), ((n, max_ops), torch.int64),
                  ((n,), torch.int32), ((n,), torch.uint8), ((n,), torch.int64))]
            self.e.mc_replies_device(d[0].data_ptr(), alen, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n,
                                     max_ops, *[x.data_ptr() for x in t], stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            g = [x.cpu().numpy() for x in t]
            kind, opn, aux, nops, res, taken = g[0], g[1].view(np.uint32), g[2].view(np.uint64), g[3].view(np.uint32), \
                g[4], g[5].view(np.uint64)
        want = self.m.replies(streams, conn, max_ops, inside)
        for s, (ops, result, tk, _) in enumerate(want):
            k = int(nops[s])
            got = list(zip(kind[s, :k].tolist(), opn[s, :k].tolist(), aux[s, :k].tolist()))
            assert (got, int(res[s]), int(taken[s])) == (ops, result, tk), (s, streams[s][:80])
        self.check_stats()
        return want

    def check_stats(self):
        st = self.e.mc_session_stats()
        assert st == self.m.stats()
        return st


def injected(ops):
    """The bytes a caller sends for the INJECT ops of a reply call."""
    out = b""
    for kind, n, aux in ops:
        if kind == INJECT and n == 37:
            out += bytes([aux]) + _lib.mc_denied_message(True)[1:]
        elif kind == INJECT:
            assert n % 28 == 0
            out += _lib.mc_denied_message(False) * (n // 28)
    return out


# ------------------------------------------------------------------ 1. the reference's own sequences
@WAYS
def test_reference_sequences_on_the_device(sengine, kats, device):
    """classify + mc_forward for a request call, mc_replies for a reply call."""
    M = kats["memcache"]
    c = M["conn"]
    rules = {k["name"]: k["l7_rules"] for k in M["cases"]}
    state = {}

    def forward(name):
        sengine.update_policy(memcache_policy(M, rules[name]))
        conns = gen.make_conns(1, 0, c["port"], c["ingress"], gen.PROTO_MEMCACHE, [c["src_id"]], c["dst_id"])
        state[name] = Dev(sengine, conns, 16, device)

        def f(frames, verdicts):
            d = state[name]
            data, at, got_frames, got_v = b"".join(frames), 0, [], []
            while at < len(data):   # the classifier frames and decides; its verdicts must be the recording's
                arena, alen, o, lens = pack([data[at:]])
                v, _, cons = d.e.classify(arena[:alen], o, lens, [0])
                if v[0] not in (ALLOW, DENY):
                    break
                got_frames.append(data[at:at + int(cons[0])])
                got_v.append(int(v[0]))
                at += int(cons[0])
            assert (got_frames, got_v) == (frames, verdicts), name
            act, _ = d.forward(got_frames, [0] * len(frames), got_v)
            text, binary = _lib.mc_denied_message(False), _lib.mc_denied_message(True)
            inj = b"".join(bytes([fr[0] | 0x81]) + binary[1:] if fr[0] >= 0x80 else text
                           for fr, a in zip(frames, act) if a == 3)
            return act.tolist(), inj
        return f

    def replies(name):
        def r(data, max_ops):
            ops, result, _, _ = state[name].replies([data], [0], max_ops)[0]   # (compared with the device's inside)
            return [(o, n) for o, n, _ in ops], result, injected(ops)
        return r

    replay_golden(forward, replies)
    sengine.update_policy(gen.mc_policy())


# ------------------------------------------------------------------ 2. parity with the shim
def shim_script(binary, nconn, seed):
    """Per connection: rounds of (request frames with verdicts decided by the
    policy, reply bytes).  Text replies answer the requests that owe one."""
    rng = np.random.default_rng(seed)
    reqs = [r for r in gen.memcache_requests(40 * nconn, seed) if (r[0] >= 0x80) == binary]
    out = []
    for c in range(nconn):
        mine = reqs[c * 6:(c + 1) * 6]
        rounds = [mine[:2], mine[2:3], mine[3:]]
        out.append(rounds)
    return out, rng


@pytest.mark.parametrize("binary", [False, True], ids=["text", "binary"])
def test_parity_with_the_shim(sengine, binary):
    """The same scripted calls through proxylib OnData and through the batch
    calls, 64 connections: PASS / DROP, reply ops, results, injected bytes."""
    nconn = 64
    script, rng = shim_script(binary, nconn, 11 if binary else 12)
    pol = gen.mc_policy()
    mid = P.open_module([("access-log-path", "/tmp/l7g-access.sock")])
    assert mid != 0
    try:
        P.policy_update(mid, pol)
        shim = [P.Connection(mid, "memcache", 7000 + c, True, 3000 + c % 128, 7, "1.1.1.1:1",
                             "2.2.2.2:%d" % gen.MC_PORT, "10.0.0.5", 4096) for c in range(nconn)]
        assert all(s.result == P.OK for s in shim)
        d = Dev(sengine, mc_conns(nconn, flags=2 if binary else 1), 16, device=True)
        for rnd in range(3):
            frames, conn, verdicts, shim_inj = [], [], [], {}
            for c in range(nconn):
                batch = script[c][rnd]
                res, ops = shim[c].on_data(False, [b"".join(batch)], 2 * len(batch) + 2)
                assert res == P.OK
                assert [n for o, n in ops[:len(batch)]] == [len(b) for b in batch] and all(
                    o in (P.PASS, P.DROP) for o, _ in ops[:len(batch)]), (c, ops)
                frames += batch
                conn += [c] * len(batch)
                verdicts += [ALLOW if o == P.PASS else DENY for o, _ in ops[:len(batch)]]
                shim_inj[c] = shim[c].take_inject(True)
            act, inj = d.forward(frames, conn, verdicts)
            for c in range(nconn):
                assert b"".join(b for b, k in zip(inj, conn) if k == c) == shim_inj[c], c
            # replies: what a server would answer to the passed requests that owe one, one line or a retrieval
            streams = []
            for c in range(nconn):
                if binary:
                    n = sum(1 for a, k in zip(act, conn) if k == c and a == 1)
                    streams.append(gen.mc_bin(0, magic=0x81, value=b"v" * c) * n)
                else:
                    q = d.m.parsers[c].reply_queue if d.m.parsers[c] else []
                    s = b""
                    for cmd, denied, _ in q:
                        if not denied:
                            s += b"VALUE k 0 1\r\nx\r\nEND\r\n" if model.is_retrieval(cmd) or cmd == b"stats" else b"OK\r\n"
                    streams.append(s)
            want = d.replies(streams, list(range(nconn)), max_ops=12)
            for c in range(nconn):
                res, ops = shim[c].on_data(True, [streams[c]] if streams[c] else [], 12)
                assert res == (P.OK if want[c][1] == OK else P.PARSER_ERROR), c
                assert ops == [(o, n) for o, n, _ in want[c][0]], c
                assert shim[c].take_inject(True) == want[c][3] == injected(want[c][0]), c
        for s in shim:
            s.close()
    finally:
        P.close_module(mid)


# ------------------------------------------------------------------ 3. random interleavings
TEXT_COMMANDS = [b"get", b"gets", b"gat", b"gats", b"getx", b"gatling", b"set", b"add", b"replace", b"append", b"prepend",
                 b"cas", b"delete", b"incr", b"decr", b"touch", b"slabs", b"lru", b"lru_crawler", b"stats", b"version",
                 b"misbehave", b"flush_all", b"cache_memlimit", b"quit", b"watch"]
SPACES = [b" ", b" ", b" ", b"\t", b"  ", b"\xc2\xa0", b"\xe2\x80\x83", b"\xe3\x80\x80", b"\xc2\x85", b"\xe1\x9a\x80"]


def random_text_request(rng):
    cmd = TEXT_COMMANDS[int(rng.integers(0, len(TEXT_COMMANDS)))]
    if cmd == b"watch" and rng.random() < 0.7:
        cmd = b"get"
    sp = lambda: SPACES[int(rng.integers(0, len(SPACES)))]
    noreply = rng.random() < 0.3
    key = [b"user:%d" % int(rng.integers(0, 50)), b"tmp", b"cache:x", b"counter", b"session:0123abcd"][
        int(rng.integers(0, 5))]
    if model.is_retrieval(cmd):
        t = [cmd] + ([b"5"] if cmd.startswith(b"gat") else []) + [key] * int(rng.integers(1, 3))
    elif cmd in model.STORAGE:
        t = [cmd, key, b"0", b"0", b"1"] + ([b"7"] if cmd == b"cas" else []) + ([b"noreply"] if noreply else [])
    elif cmd == b"delete":
        t = [cmd, key] + ([b"noreply"] if noreply else [])
    elif cmd in (b"incr", b"decr", b"touch"):
        t = [cmd, key, b"3"] + ([b"noreply"] if noreply else [])
    elif cmd in (b"flush_all", b"cache_memlimit"):
        t = [cmd] + ([b"9"] if rng.random() < 0.5 else []) + ([b"noreply"] if noreply else [])
    elif cmd == b"lru_crawler":
        t = [cmd, b"metadump", b"all"]
    else:
        t = [cmd]
    line = (sp() if rng.random() < 0.1 else b"") + t[0]
    for x in t[1:]:
        line += sp() + x
    line += (sp() if rng.random() < 0.1 else b"") + b"\r\n"
    return line + (b"x\r\n" if cmd in model.STORAGE else b"")


def random_text_reply(rng, queue):
    """Bytes for a text connection whose queue (model's) is `queue`."""
    s = b""
    for cmd, denied, _ in queue[:int(rng.integers(0, 4))]:
        if denied:
            continue
        r = rng.random()
        if r < 0.15:
            s += [b"ERROR\r\n", b"CLIENT_ERROR x y\r\n", b"SERVER_ERROR oom\r\n"][int(rng.integers(0, 3))]
        elif model.is_retrieval(cmd) or cmd == b"stats":
            s += b"END\r\n" if r < 0.3 else b"VALUE k 0 3\r\nabc\r\nEND\r\n"
        elif cmd == b"lru_crawler":
            s += b"OK\r\n" if r < 0.5 else b"key=a\r\nEND\r\n"
        else:
            s += b"STORED\r\n"
    r = rng.random()
    if r < 0.08:
        s += b"\r\n"                # a blank line
    elif r < 0.16:
        s += b"STOR"                # a partial line
    elif r < 0.24:
        s += b"STORED\r"            # ... ending in CR
    elif r < 0.30:
        s += b"STORED\r\n"          # a reply nobody asked for (unless something is still queued)
    return s


def random_binary_reply(rng, owed):
    s = b""
    for _ in range(int(rng.integers(0, owed + 2))):
        r = rng.random()
        if r < 0.08:
            s += gen.mc_bin(0, magic=0x01)                       # bit 7 clear
            break
        if r < 0.16:
            s += gen.mc_bin(0, key=b"abcdef", magic=0x81)[:27]   # key bytes missing
            break
        if r < 0.24:
            s += gen.mc_bin(0, magic=0x81)[:int(rng.integers(1, 24))]   # a short header
            break
        s += gen.mc_bin(int(rng.integers(0, 20)), magic=0x81, value=b"v" * int(rng.integers(0, 40)))
    return s


@WAYS
def test_random_interleavings_against_the_model(sengine, device):
    rng = np.random.default_rng(20260 + device)
    nconn = 300
    conns = mc_conns(nconn, other=(5, 77))
    for c in range(nconn):
        conns["flags"][c] = (0, 0, 1, 2)[c % 4]
    d = Dev(sengine, conns, 2, device)
    binary = [c % 4 == 3 or (c % 4 < 2 and c % 2 == 1) for c in range(nconn)]
    bin_reqs = [r for r in gen.memcache_requests(3000, 5) if r[0] >= 0x80]
    seen_acts, seen_kinds, errors = set(), set(), 0
    for rnd in range(20):
        frames, conn = [], []
        for _ in range(600):
            c = int(rng.integers(0, nconn + 3))     # (some past the table)
            b = binary[c] if c < nconn else False
            if rng.random() < 0.02:
                b = not b                            # a request of the other kind
            frames.append(bin_reqs[int(rng.integers(0, len(bin_reqs)))] if b else random_text_request(rng))
            conn.append(c)
        arena, alen, o, lens = pack(frames)
        verdict = d.e.classify(arena[:alen], o, lens, np.minimum(np.asarray(conn, np.uint32), nconn - 1))[0]
        act, _ = d.forward(frames, conn, verdict)
        seen_acts |= set(act.tolist())
        streams, sconn = [], []
        for c in rng.permutation(nconn)[:200].tolist():
            p = d.m.parsers[c]
            if p is None:
                s = b"" if rng.random() < 0.5 else b"STORED\r\n"
            elif p.kind == 1:
                s = random_text_reply(rng, p.reply_queue)
            else:
                s = random_binary_reply(rng, max(0, p.request_count - p.reply_count))
            streams.append(s)
            sconn.append(c)
        want = d.replies(streams, sconn, max_ops=6)
        for ops, result, _, _ in want:
            seen_kinds |= {k for k, _, _ in ops}
            errors += result == PARSER_ERROR
    assert seen_acts == {0, 1, 2, 3, 4, 5, 6, 7}
    assert seen_kinds == {0, 1, 3, 4} and errors > 0
    st = d.check_stats()
    assert all(st[k] > 0 for k in ("queued", "sessions", "full", "mismatch", "inject_now", "inject_queued", "passed"))


# ------------------------------------------------------------------ 4. batch order
@pytest.mark.parametrize("binary", [False, True], ids=["text", "binary"])
def test_batch_order_decides(sengine, binary):
    """One connection's 200 requests scattered through 5,000 on other
    connections, in several permutations of the others: index order decides."""
    rng = np.random.default_rng(9)
    nconn = 40
    if binary:
        mine = [gen.mc_bin(0, key=b"k%d" % i) for i in range(200)]
        # an open run of immediate injects: two unanswered... none; replies lead by 3 (unsolicited), so the run
        # starts at position 4 and ends at the first ALLOW after it
        v_mine = [ALLOW, DENY, ALLOW] + [DENY] * 9 + [ALLOW] + [DENY if i % 3 else ALLOW for i in range(187)]
        others = [gen.mc_bin(1, key=b"o", extras=bytes(8), value=b"v") for _ in range(4800)]
    else:
        mine = [b"delete k%d\r\n" % i for i in range(200)]
        v_mine = [DENY] * 7 + [ALLOW] + [DENY if i % 2 else ALLOW for i in range(192)]
        others = [b"get o%d\r\n" % i for i in range(4800)]
    expect = None
    for perm in range(3):
        d = Dev(sengine, mc_conns(nconn, flags=2 if binary else 1), 256, device=True)
        if binary:
            d.replies([gen.mc_bin(0, magic=0x81) * 3], [0])      # replies - requests = 3
        pos = np.sort(rng.permutation(5000)[:200])
        frames, conn, verdict = [None] * 5000, [0] * 5000, [0] * 5000
        oc = rng.integers(1, nconn, size=5000)
        ov = rng.integers(0, 2, size=5000)
        k = 0
        for j in range(5000):
            if k < 200 and j == pos[k]:
                frames[j], conn[j], verdict[j] = mine[k], 0, v_mine[k]
                k += 1
            else:
                frames[j], conn[j], verdict[j] = others[j % 4800], int(oc[j]), int(ov[j])
        act, _ = d.forward(frames, conn, verdict)
        got = act[pos].tolist()
        if binary:
            assert got[:13] == [1, 4, 1, 3, 3, 3, 3, 3, 3, 3, 3, 3, 1] and 3 not in got[13:]
        else:
            assert got[:8] == [3] * 7 + [1] and 3 not in got[8:]     # the prefix ends at the first ALLOW that owes a reply
        assert expect is None or got == expect
        expect = got


# ------------------------------------------------------------------ 5. window edges
@WAYS
def test_window_edges(sengine, device):
    """One stream per offset 0 .. 2W + 16 of the END of a retrieval reply, the
    CRLF of a one-line reply and a second frame's first byte."""
    n = 2 * W + 17
    d = Dev(sengine, mc_conns(3 * n, flags=1), 4, device)
    frames = [b"get a\r\n"] * n + [b"delete a\r\n"] * n + [b"delete a\r\n", b"delete b\r\n"] * n
    conn = list(range(n)) + list(range(n, 2 * n)) + [c for c in range(2 * n, 3 * n) for _ in (0, 1)]
    d.forward(frames, conn, [ALLOW] * len(frames))
    streams = []
    for k in range(n):      # streams lie back to back, so every alignment of every edge occurs as well
        streams.append(b"VALUE a 0 %d\r\n" % k + b"v" * k + b"\r\nEND\r\n")
    for k in range(n):
        streams.append(b"N" * (k + 1) + b"\r\n")
    for k in range(n):
        streams.append(b"D" * (k + 1) + b"\r\nNOT_FOUND\r\n")
    want = d.replies(streams, list(range(3 * n)), max_ops=4)
    assert all(len(w[0]) == (2 if s >= 2 * n else 1) and w[1] == OK for s, w in enumerate(want))
    assert d.check_stats()["queued"] == 0


# ------------------------------------------------------------------ 6. the ring
@WAYS
def test_ring_wraps_fills_and_drains(sengine, device):
    d = Dev(sengine, mc_conns(2, flags=1), 4, device)
    for k in range(7):      # the head wraps: three pushes, three pops, seven times
        act, _ = d.forward([b"delete a\r\n", b"get b\r\n", b"delete c\r\n"], [0, 0, 0], [ALLOW, ALLOW, DENY],
                           tags=[10 * k + 1, 10 * k + 2, 10 * k + 3])
        assert act.tolist() == [1, 1, 4]
        want = d.replies([b"DELETED\r\nEND\r\n"], [0])      # DELETED, then a retrieval miss waits
        assert [o[:2] for o in want[0][0]] == [(PASS, 9), (MORE, 1)]
        want = d.replies([b"VALUE b 0 1\r\nx\r\nEND\r\n"], [0])
        assert want[0][0] == [(PASS, 21, 10 * k + 2), (INJECT, 28, 0)]
    # full: exactly from the push that finds count == capacity; noreply requests still go through
    frames = [b"get a\r\n"] * 3 + [b"delete x\r\n", b"set k 0 0 1 noreply\r\nx\r\n", b"get b\r\n", b"delete y noreply\r\n",
                                   b"delete z\r\n"]
    act, _ = d.forward(frames, [0] * 8, [ALLOW, ALLOW, ALLOW, DENY, ALLOW, ALLOW, DENY, DENY])
    assert act.tolist() == [1, 1, 1, 4, 2, 6, 5, 6]
    act, _ = d.forward([b"get c\r\n", b"quit\r\n"], [0, 0], [ALLOW, ALLOW])
    assert act.tolist() == [6, 2]
    st = d.check_stats()
    assert st["full"] == 3 and st["queued"] == 4
    # after the replies drain the ring, pushes succeed again
    want = d.replies([b"VALUE a 0 1\r\nx\r\nEND\r\n" * 3], [0])
    assert [o[:2] for o in want[0][0]] == [(PASS, 21)] * 3 + [(INJECT, 28)]
    act, _ = d.forward([b"get c\r\n"] * 5, [0] * 5, [ALLOW] * 5)
    assert act.tolist() == [1, 1, 1, 1, 6]


# ------------------------------------------------------------------ 7. max_ops
@WAYS
def test_max_ops_continues_from_taken(sengine, device):
    reqs = [(b"get k%d\r\n" % i, ALLOW) if i % 3 else (b"delete k%d\r\n" % i, DENY if i % 2 else ALLOW)
            for i in range(1, 61)]
    stream = b"".join(b"VALUE k 0 1\r\nx\r\nEND\r\n" if r.startswith(b"get") else b"DELETED\r\n"
                      for r, v in reqs if v == ALLOW)
    assert sum(v == ALLOW for _, v in reqs) == 50
    whole = None
    for max_ops in (64, 3, 1):
        d = Dev(sengine, mc_conns(1, flags=1), 64, device)
        d.forward([r for r, _ in reqs], [0] * len(reqs), [v for _, v in reqs])
        ops, at = [], 0
        while True:
            o, result, taken, _ = d.replies([stream[at:]], [0], max_ops)[0]
            assert result == OK
            ops += o
            at += taken
            if len(o) < max_ops:
                break
        if whole is None:
            whole = ops
            assert sum(k == PASS for k, _, _ in ops) == 50 and any(k == INJECT for k, _, _ in ops)
        assert ops == whole and at == len(stream)
    # binary: 40 frames, and an ERROR 2 that fills what is left
    bstream = b"".join(gen.mc_bin(0, magic=0x81, value=b"v" * i) for i in range(40)) + gen.mc_bin(0, magic=0x01)
    for max_ops in (64, 3, 1):
        d = Dev(sengine, mc_conns(1, flags=2), 4, device)
        ops, at = [], 0
        for _ in range(45 if max_ops == 1 else 15 if max_ops == 3 else 1):
            o, result, taken, _ = d.replies([bstream[at:]], [0], max_ops)[0]
            ops += o
            at += taken
        assert [k for k, _, _ in ops[:40]] == [PASS] * 40 and at == len(bstream) - 24
        assert all(o == (4, 2, 0) for o in ops[40:]) and len(ops) > 40


# ------------------------------------------------------------------ 8. resets and switches
def test_resets_and_switches(sengine):
    conns = mc_conns(6, flags=1, other=(4,))
    d = Dev(sengine, conns, 8)
    owed = lambda: d.forward([b"get a\r\n"] * 6, list(range(6)), [ALLOW] * 6)[0].tolist()
    assert owed() == [1, 1, 1, 1, 0, 1]                     # connection 4 is not memcached
    assert d.check_stats()["queued"] == 5
    # l7g_conn_update: that session alone
    d.e.conn_update(1, {k: int(conns[k][1]) for k in ("policy", "port", "ingress", "proto", "src_id", "dst_id")})
    d.m.reset(1)
    d.m.flags[1] = 0
    want = d.replies([b"END\r\n"] * 2, [0, 1])
    assert want[0][0] == [(MORE, 1, 0)] and want[1][1] == PARSER_ERROR
    # l7g_mc_session_reset: the named ones
    d.e.mc_session_reset([0, 2])
    d.m.reset(0)
    d.m.reset(2)
    assert d.check_stats()["queued"] == 2
    # l7g_conns_set: all
    d.e.set_connections(conns)
    d.m.set_connections(conns)
    assert d.check_stats() == dict.fromkeys(d.e.MC_SESSION_STATS, 0) | {
        k: d.m.counts[k] for k in d.m.counts}
    assert owed() == [1, 1, 1, 1, 0, 1]
    # a stream on a connection that is not memcached, one past the table, one outside the arena, an empty one
    want = d.replies([b"OK\r\n", b"OK\r\n", b"OK\r\n", b""], [4, 99, 0, 5], offs=[0, 4, 1 << 40, 12])
    assert [w[1] for w in want] == [2, 2, 2, 0]
    # a request outside the arena takes no part
    act, _ = d.forward([b"get a\r\n", b"get b\r\n"], [0, 0], [ALLOW, ALLOW], offs=[0, 1 << 33])
    assert act.tolist() == [1, 0]
    # a policy update resets nothing
    d.e.update_policy(gen.mc_policy())
    assert d.check_stats()["queued"] == 6
    # enabling again: every session empty, the counters too
    d2 = Dev(sengine, conns, 8)
    assert d2.check_stats() == dict.fromkeys(d2.e.MC_SESSION_STATS, 0)
    assert d2.replies([b""], [0])[0][1] == 3                # no parser yet, nothing to make one from
    # off: the calls answer hipErrorNotReady
    sengine.mc_sessions(0)
    with pytest.raises(RuntimeError, match=f"HIP error {HIP_ERROR_NOT_READY}"):
        sengine.mc_forward(np.frombuffer(b"get a\r\n", np.uint8), [0], [7], [0], [ALLOW])
    with pytest.raises(RuntimeError, match=f"HIP error {HIP_ERROR_NOT_READY}"):
        sengine.mc_replies(np.frombuffer(b"END\r\n", np.uint8), [0], [5], [0])
    with pytest.raises(RuntimeError, match=f"HIP error {HIP_ERROR_NOT_READY}"):
        sengine.mc_session_reset([0])
    assert sengine.mc_session_stats() == dict.fromkeys(sengine.MC_SESSION_STATS, 0)


# ------------------------------------------------------------------ 9. a batch past the grid cap
def test_forward_past_the_grid_cap(sengine):
    """4096 workgroups of 256 lanes: one request more than every forward kernel
    covers before it takes its grid-stride a second time.  The model walks a
    request at a time through Python's bytes.Fields; at this size the
    expectation is the text parser's request rule over three fixed frames,
    written out below and held to the model on the batch's first 20,000."""
    n = 4096 * 256 + 1
    nconn, cap = 512, 1024
    rng = np.random.default_rng(3)
    kinds = [b"get a\r\n", b"delete a\r\n", b"set a 0 0 1 noreply\r\nx\r\n"]
    pick = rng.integers(0, 3, size=n)
    conn = rng.integers(0, nconn, size=n).astype(np.uint32)
    verdict = (rng.random(n) < 0.9).astype(np.uint8)
    count, want, full, now = [0] * nconn, np.zeros(n, np.uint8), 0, 0
    for i, (k, c, v) in enumerate(zip(pick.tolist(), conn.tolist(), verdict.tolist())):
        if k == 2:
            want[i] = 2 if v else 5
        elif not v and count[c] == 0:
            want[i] = 3
            now += 1
        elif count[c] < cap:
            count[c] += 1
            want[i] = 1 if v else 4
        else:
            want[i] = 6
            full += 1
    head = model.Sessions(mc_conns(nconn, flags=1), cap)
    assert head.forward([kinds[k] for k in pick[:20000].tolist()], conn[:20000], verdict[:20000])[0].tolist() == \
        want[:20000].tolist()
    assert set(want.tolist()) == {1, 2, 3, 4, 5, 6}
    import torch
    sengine.mc_sessions(cap)
    sengine.set_connections(mc_conns(nconn, flags=1))
    lens = np.array([len(k) for k in kinds], np.uint32)[pick]
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    arena = np.frombuffer(b"".join(kinds), np.uint8)[
        np.repeat(np.array([0, 7, 17], np.int64)[pick] - offs.astype(np.int64), lens) + np.arange(int(lens.sum()))]
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(a).to(dev) for a in (np.concatenate([arena, np.zeros(16, np.uint8)]), offs.view(np.int64),
                                               lens.view(np.int32), conn.view(np.int32), verdict)]
    out = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    sengine.mc_forward_device(t[0].data_ptr(), len(arena), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                              t[4].data_ptr(), 0, n, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    st = sengine.mc_session_stats()
    assert (st["queued"], st["sessions"], st["full"], st["inject_now"]) == (sum(count), nconn, full, now)

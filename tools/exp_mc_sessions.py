"""What the memcached sessions cost (GPU box): ms per call of l7g_mc_forward
for 1M device-resident memcached requests of cfg5's generator over 4096
connections, and of l7g_mc_replies over the 4096 reply streams that answer
them -- a unique stream of n / copies requests whose arena is replicated on the
device (gen.tile_offsets, as bench.py does).  Connections 0..1023 carry the
binary requests and the others the text ones (a connection speaks one
protocol), and the policy allows all but a few percent.

First the outputs are checked against the model (tests/mc_sessions_py.py):
l7g_classify's verdicts go through l7g_mc_forward and every act is compared;
the reply streams are built from the model's queues (a one-line reply, a
retrieval with one value, or a binary reply per request that owes one), go
through l7g_mc_replies, and the ops, op_aux, result and taken of a sample of
2,000 streams are compared.  Then 3 warm-up rounds and `rounds` windows of
`reps` rounds; a round is one forward and one replies call that drains every
queue again, each between its own pair of HIP events, and a window's figure is
the mean of its calls; the median window is reported.

Beside them the existing host path on one core for the reply direction: the
proxylib shim's OnData(reply) over the same 4096 streams, its connections
brought to the same state through OnData(request) first (not timed; those
calls classify on the device).  The timed calls are the C entry alone, their
arguments built beforehand.  That is the baseline, not the new code; it does
not include copying the streams home over PCIe.
usage: python tools/exp_mc_sessions.py [n] [copies] [rounds]"""
import ctypes as C
import functools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cilium_amd import Engine, api, gen  # noqa: E402
from cilium_amd import proxylib as P  # noqa: E402
import mc_sessions_py as model  # noqa: E402

SAMPLE = 2000
NCONNS, NBIN = 4096, 1024
MAX_PENDING, MAX_OPS = 1024, 1024
POLICY_NAME = "10.0.0.5"


def policy():
    rules = [{"command": "get"}, {"command": "gat"}, {"command": "storage"}, {"command": "touch"}, {"command": "stats"},
             {"command": "version"}, {"command": "noop"}, {"command": "flush_all"},
             {"command": "delete", "keyPrefix": "user:"}]
    group = [api.port_rule(l7proto="memcache", l7=rules)]
    return api.policy_set(api.network_policy(POLICY_NAME, 5, ingress=[(gen.MC_PORT, group), (0, group)]))


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    reps, u = 10, n // k
    dev = torch.device("cuda", 0)
    w = gen.memcache_workload(u, nconns=NCONNS)
    uniq = [w.arena[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(w.offsets, w.lengths)]
    binary = np.array([f[0] >= 0x80 for f in uniq])
    w.conn_ids = np.where(binary, w.conn_ids % NBIN, NBIN + w.conn_ids % (NCONNS - NBIN)).astype(np.uint32)
    w.conns["flags"] = np.where(np.arange(NCONNS) < NBIN, 2, 1)
    eng = Engine(0)
    eng.update_policy(policy())
    eng.set_connections(w.conns)
    eng.mc_sessions(MAX_PENDING)
    offs, lens, cids = gen.tile_offsets(w, k)
    nn = len(offs)
    d_arena = torch.from_numpy(np.tile(w.arena, k)).to(dev)
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (offs.view(np.int64), lens.view(np.int32),
                                                                     cids.view(np.int32))]
    verdict = torch.zeros(nn, dtype=torch.uint8, device=dev)
    rule = torch.zeros(nn, dtype=torch.int32, device=dev)
    consumed = torch.zeros(nn, dtype=torch.int32, device=dev)
    tags = torch.arange(1, nn + 1, dtype=torch.int64, device=dev)
    act = torch.zeros(nn, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    eng.classify_device(d_arena.data_ptr(), d_arena.numel(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), nn,
                        verdict.data_ptr(), rule.data_ptr(), consumed.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    h_verdict = verdict.cpu().numpy()
    assert set(h_verdict.tolist()) <= {0, 1}, "cfg5's generator makes whole, valid requests"

    def forward():
        eng.mc_forward_device(d_arena.data_ptr(), d_arena.numel(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                              verdict.data_ptr(), tags.data_ptr(), nn, act.data_ptr(), stream=stream)

    # ---- the check, request direction: every act
    model.fields = functools.lru_cache(maxsize=None)(model.fields)   # (the unique requests repeat `copies` times)
    m = model.Sessions(w.conns, MAX_PENDING)
    want_act, _ = m.forward(uniq * k, cids, h_verdict, np.arange(1, nn + 1, dtype=np.uint64))
    forward()
    torch.cuda.synchronize()
    h_act = act.cpu().numpy()
    assert np.array_equal(h_act, want_act)
    assert not (h_act == 6).any() and not (h_act == 7).any() and not (h_act == 0).any()

    # ---- the matching reply streams, from the model's queues
    streams = []
    for c in range(NCONNS):
        p = m.parsers[c]
        if p is None:
            streams.append(b"")
        elif p.kind == 2:
            streams.append(gen.mc_bin(0, magic=0x81, value=b"12345678") * int(((cids == c) & (h_act == 1)).sum()))
        else:
            streams.append(b"".join(
                b"" if denied else b"VALUE k 0 5\r\nhello\r\nEND\r\n" if model.is_retrieval(cmd) or cmd == b"stats"
                else b"STORED\r\n" for cmd, denied, _ in p.reply_queue))
    s_arena, s_off, s_len = gen.pack(streams)
    ds = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (
        np.concatenate([s_arena, np.zeros(16, np.uint8)]), s_off.view(np.int64), s_len.view(np.int32),
        np.arange(NCONNS, dtype=np.int32))]
    ro = [torch.zeros(shape, dtype=t, device=dev) for shape, t in (
        ((NCONNS, MAX_OPS), torch.uint8), ((NCONNS, MAX_OPS), torch.int32), ((NCONNS, MAX_OPS), torch.int64),
        ((NCONNS,), torch.int32), ((NCONNS,), torch.uint8), ((NCONNS,), torch.int64))]

    def replies():
        eng.mc_replies_device(ds[0].data_ptr(), len(s_arena), ds[1].data_ptr(), ds[2].data_ptr(), ds[3].data_ptr(),
                              NCONNS, MAX_OPS, *[t.data_ptr() for t in ro], stream=stream)

    want = m.replies(streams, np.arange(NCONNS), MAX_OPS)
    replies()
    torch.cuda.synchronize()
    kind, opn, aux, nops, res, taken = [t.cpu().numpy() for t in ro]
    pick = np.random.default_rng(7).choice(NCONNS, size=min(SAMPLE, NCONNS), replace=False)
    for c in pick.tolist():
        j = int(nops[c])
        got = list(zip(kind[c, :j].tolist(), opn[c, :j].view(np.uint32).tolist(), aux[c, :j].view(np.uint64).tolist()))
        assert (got, int(res[c]), int(taken[c])) == want[c][:3], c
        assert int(taken[c]) == len(streams[c]) and j < MAX_OPS, c
    st = eng.mc_session_stats()
    assert st == m.stats() and st["queued"] == 0, st
    out = {"n": nn, "unique": u, "copies": k, "connections": NCONNS, "binary_connections": NBIN, "reps": reps,
           "rounds": rounds, "max_pending": MAX_PENDING, "max_ops": MAX_OPS, "acts_checked": nn,
           "streams_checked": int(len(pick)), "denied_share": round(float((h_verdict == 0).mean()), 4),
           "reply_stream_bytes": int(len(s_arena)), "reply_ops": int(nops.sum()),
           "acts": {str(a): int((h_act == a).sum()) for a in range(8)}}

    # ---- the windows
    def window():
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
        for e in ev:
            e[0].record()
            forward()
            e[1].record()
            e[2].record()
            replies()
            e[3].record()
        torch.cuda.synchronize()
        return (sum(e[0].elapsed_time(e[1]) for e in ev) / reps, sum(e[2].elapsed_time(e[3]) for e in ev) / reps)

    for _ in range(3):
        forward()
        replies()
    torch.cuda.synchronize()
    t = {"forward": [], "replies": []}
    for _ in range(rounds):
        a, b = window()
        t["forward"].append(a)
        t["replies"].append(b)
    assert eng.mc_session_stats()["queued"] == 0 and np.array_equal(ro[4].cpu().numpy(), res)
    for name in t:
        out[f"{name}_ms_per_call"] = round(float(np.median(t[name])), 4)
        out[f"{name}_windows_ms"] = [round(x, 4) for x in t[name]]
    eng.mc_sessions(0)
    eng.close()

    # ---- the host path on one core, reply direction: the shim's OnData(reply) over the same streams
    mid = P.open_module([("access-log-path", "/tmp/l7g-access.sock")])
    assert mid != 0
    P.policy_update(mid, policy())
    order = np.argsort(cids, kind="stable")
    bounds = np.searchsorted(cids[order], np.arange(NCONNS + 1)).tolist()
    frames = uniq * k
    shim = []
    for c in range(NCONNS):
        s = P.Connection(mid, "memcache", 100000 + c, True, int(w.conns["src_id"][c]), int(w.conns["dst_id"][c]),
                         "1.1.1.1:1", "2.2.2.2:%d" % int(w.conns["port"][c]), POLICY_NAME, 1 << 14)
        assert s.result == P.OK
        idx = order[bounds[c]:bounds[c + 1]].tolist()
        res_c, ops = s.on_data(False, [b"".join(frames[i] for i in idx)], len(idx) + 2)
        assert res_c == P.OK and [o == P.PASS for o, _ in ops[:len(idx)]] == [bool(h_verdict[i]) for i in idx], c
        s.take_inject(True)
        shim.append(s)
    lib = P.lib()
    keep = [C.create_string_buffer(s, len(s)) for s in streams]
    slices = [(P.GoSlice * 1)(P.GoSlice(C.cast(b, C.c_void_p), len(s), len(s))) for b, s in zip(keep, streams)]
    data = [P.GoSlice(C.cast(sl, C.c_void_p), 1 if s else 0, 1) for sl, s in zip(slices, streams)]
    ops_mem = (C.c_int64 * (2 * MAX_OPS))()
    results = []
    t0 = time.perf_counter()
    for c in range(NCONNS):
        ops = P.GoSlice(C.cast(ops_mem, C.c_void_p), 0, MAX_OPS)
        results.append((lib.OnData(100000 + c, 1, 0, C.byref(data[c]), C.byref(ops)), ops.len))
    rep_s = time.perf_counter() - t0
    for c in pick.tolist():
        assert results[c] == (P.OK, len(want[c][0])), c
    for s in shim:
        s.close()
    P.close_module(mid)
    out["host_one_core"] = {"replies_ms": round(1e3 * rep_s, 3),
                            "note": "the proxylib shim's OnData(reply), one call per connection, over the same 4096 "
                                    "streams; ctypes call overhead of 4096 calls included, PCIe not included"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

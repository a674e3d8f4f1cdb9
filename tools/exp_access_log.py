"""What the access-log records cost (GPU box): ms per call of l7g_classify
against l7g_classify_logged for 1M cfg2 HTTP, 1M cfg3 Kafka and 1M mixed (cfg5)
requests, device-resident: a unique stream of n / copies requests whose arena
is replicated on the device (gen.tile_offsets, as bench.py does).
Every record is checked first: the first copy's against a re-parse on the host
(HTTP: the head split at its SPs and CRLFs; Kafka: tests/kafka_topics_py.py),
every other copy's against the first copy's.  Then each leg: 3 warm-up calls
and `rounds` windows of `reps` calls between two HIP events, the two calls
alternated; the median window is reported.  Alongside: the arena bytes
http_log_kernel fetches per HTTP request (16-byte chunks of 256-byte windows up
to the empty line), from the records.  Its own time comes from a kernel trace of
this tool (rocprofv3 --kernel-trace, tools/kernel_resources.py).
usage: python tools/exp_access_log.py [n] [copies] [rounds]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kafka_topics_py  # noqa: E402
from cilium_amd import Engine, gen  # noqa: E402
from cilium_amd._lib import ALLOW, DENY, PROTO_HTTP, PROTO_KAFKA  # noqa: E402
from cilium_amd.engine import LOGREC_DTYPE  # noqa: E402

STRIDE = 4


def http_fields(data):
    """(method_len, path_len, flags, host_off, host_len, head_len, nheaders, version) of a well-formed head."""
    head_len = data.index(b"\r\n\r\n") + 4
    lines = data[:head_len - 4].split(b"\r\n")
    m, p, ver = lines[0].split(b" ")
    flags = host_off = host_len = 0
    at = len(lines[0]) + 2
    for ln in lines[1:]:
        if not flags and ln[:5].lower() == b"host:":
            v = ln[5:]
            lead = len(v) - len(v.lstrip(b" \t"))
            flags, host_off, host_len = 1, at + 5 + lead, len(v.strip(b" \t"))
        at += len(ln) + 2
    return (len(m), len(p), flags, host_off, host_len, head_len, len(lines) - 1, (ver[5] - 48) << 4 | (ver[7] - 48))


def check_records(w, k, v, rec, topics):
    """The first copy against the host re-parse, the other copies against the first."""
    u = w.n
    raw = rec.view(np.uint32).reshape(k, u, 8)
    done = ((v == ALLOW) | (v == DENY)).reshape(k, u)
    assert (done == done[0]).all()
    assert (raw[:, done[0]] == raw[0, done[0]]).all()
    proto = w.conns["proto"][w.conn_ids]
    ks = done[0] & (proto == PROTO_KAFKA)
    t = topics.reshape(k, u, STRIDE, 2)
    r0 = rec[:u]
    assert (r0["kind"][done[0] & (proto == PROTO_HTTP)] == 1).all() and (r0["kind"][ks] == 2).all()
    assert (r0["kind"][done[0] & (proto != PROTO_HTTP) & (proto != PROTO_KAFKA)] == 0).all()
    arena = w.arena.tobytes()
    for i in np.nonzero(done[0])[0]:
        data = arena[int(w.offsets[i]):int(w.offsets[i]) + int(w.lengths[i])]
        r = r0[i]
        if proto[i] == PROTO_HTTP:
            got = (r["method_len"], r["path_len"], r["flags"] & 1, r["host_off"] if r["flags"] & 1 else 0,
                   r["host_len"], r["head_len"], r["nheaders"], r["api_key"])
            assert tuple(int(x) for x in got) == http_fields(data), (i, got)
        elif proto[i] == PROTO_KAFKA:
            p = kafka_topics_py.parse(data)
            nt = len(p["topics"])
            assert (r["api_key"], r["api_version"], r["correlation_id"], r["ntopics"], r["flags"] & 1) == \
                (p["api_key"], p["api_version"], p["correlation_id"], nt, int(nt > STRIDE)), i
            m = min(nt, STRIDE)
            assert [tuple(x) for x in t[0, i, :m].tolist()] == p["topics"][:m], i
            assert (t[1:, i, :m] == t[0, i, :m]).all(), i
    return int(done.sum())


def fetched_bytes(w, k, v, rec):
    """Arena bytes http_log_kernel loads per HTTP request answered ALLOW / DENY."""
    proto = np.tile(w.conns["proto"][w.conn_ids], k)
    sel = ((v == ALLOW) | (v == DENY)) & (proto == PROTO_HTTP)
    if not sel.any():
        return None
    offs, lens, _ = gen.tile_offsets(w, k)
    lead = (offs[sel] & np.uint64(15)).astype(np.int64)
    qend = lead + lens[sel].astype(np.int64)
    windows = (lead + rec["head_len"][sel].astype(np.int64) - 2) // 256 + 1
    chunks = np.minimum((qend + 15) // 16, windows * 16)
    return {"requests": int(sel.sum()), "mean_bytes_fetched": round(float(16 * chunks.mean()), 1),
            "mean_head_bytes": round(float(rec["head_len"][sel].mean()), 1),
            "mean_request_bytes": round(float(lens[sel].mean()), 1)}


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    reps, u = 10, n // k
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    out = {"n": u * k, "unique": u, "copies": k, "reps": reps, "rounds": rounds, "topic_stride": STRIDE}
    for name, w in (("cfg2_http", gen.http_workload(2, u)), ("cfg3_kafka", gen.kafka_workload(u)),
                    ("cfg5_mixed", gen.mixed_workload(u))):
        eng.update_policy(w.policy)
        eng.set_connections(w.conns)
        offs, lens, cids = gen.tile_offsets(w, k)
        nn = len(offs)
        d_arena = torch.from_numpy(w.arena).to(dev).repeat(k)
        d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
             for a in (offs.view(np.int64), lens.view(np.int32), cids.view(np.int32))]
        o = [torch.full((nn,), 7, dtype=t, device=dev) for t in (torch.uint8, torch.int32, torch.int32)]
        rec = torch.zeros((nn, 8), dtype=torch.int32, device=dev)
        top = torch.zeros((nn, STRIDE, 2), dtype=torch.int32, device=dev)
        args = (d_arena.data_ptr(), d_arena.numel(), *[t.data_ptr() for t in d], nn, *[t.data_ptr() for t in o])

        def call(logged):
            s = torch.cuda.current_stream().cuda_stream
            if logged:
                eng.classify_logged_device(*args, rec.data_ptr(), top.data_ptr(), STRIDE, stream=s)
            else:
                eng.classify_device(*args, stream=s)

        def window(logged):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                call(logged)
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / reps

        call(False)
        torch.cuda.synchronize()
        plain = [t.cpu().numpy().copy() for t in o]
        call(True)
        torch.cuda.synchronize()
        assert all(np.array_equal(a, t.cpu().numpy()) for a, t in zip(plain, o)), name
        v = plain[0]
        h_rec = rec.cpu().numpy().view(LOGREC_DTYPE).reshape(nn)
        checked = check_records(w, k, v, h_rec, top.cpu().numpy().view(np.uint32))
        legs = {"plain": [], "logged": []}
        for logged in (False, True):
            for _ in range(3):
                call(logged)
        torch.cuda.synchronize()
        for _ in range(rounds):
            legs["plain"].append(window(False))
            legs["logged"].append(window(True))
        mp, ml = float(np.median(legs["plain"])), float(np.median(legs["logged"]))
        out[name] = {"records_checked": checked, "verdicts": np.bincount(v, minlength=5).tolist(),
                     "plain_ms_per_call": round(mp, 4), "logged_ms_per_call": round(ml, 4),
                     "logging_ms": round(ml - mp, 4), "logging_pct": round(100 * (ml - mp) / mp, 2),
                     "plain_windows_ms": [round(x, 4) for x in legs["plain"]],
                     "logged_windows_ms": [round(x, 4) for x in legs["logged"]],
                     "http_log_kernel": fetched_bytes(w, k, v, h_rec)}
        del d_arena, d, o, rec, top
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()

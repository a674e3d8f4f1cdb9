"""What the Kafka sessions cost (GPU box): ms per call of l7g_kafka_forward and
l7g_kafka_responses for 1M device-resident cfg3 Kafka requests over 4096
connections, all ALLOW -- a unique stream of n / copies requests whose arena is
replicated on the device (gen.tile_offsets, as bench.py does).

First the outputs are checked: every new id against the model's numbering
(rank in a stable sort by connection), and for a sample of 2,000 requests the
rewritten bytes, the restored response bytes and the reported entry.  Then 3
warm-up rounds and `rounds` windows of `reps` rounds; a round is one forward
(1M inserts) and one responses call answering all of them (1M hits), each
between its own pair of HIP events, and a window's figure is the mean of its
calls; the median window is reported.  The response frames are rebuilt from
new_id between the two calls and the table is collected between windows,
neither inside a timed interval.  l7g_kafka_session_gc is timed once, by the
host clock (it synchronises), over a table at half occupancy (1M live entries
in 2M slots, none expired).

Beside them the existing host path on one core for the same requests: 4096
l7g_kafka_corr caches, the batch grouped by connection (one stable argsort,
timed apart), one l7g_kafka_corr_requests / _responses call per connection
over a host copy of the bytes, ctypes call overhead (2 x 4096 calls) included.
That is the baseline, not the new code; it does not include copying the batch
home over PCIe.
usage: python tools/exp_kafka_sessions.py [n] [copies] [rounds]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cilium_amd import Engine, _lib, gen  # noqa: E402

SAMPLE = 2000
NCONNS = 4096


def be32_at(arena, at):
    b = [arena[at + k].astype(np.uint32) for k in range(4)]
    return b[0] << 24 | b[1] << 16 | b[2] << 8 | b[3]


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    reps, u = 10, n // k
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    w = gen.kafka_workload(u, nconns=NCONNS)
    eng.update_policy(w.policy)
    eng.set_connections(w.conns)
    offs, lens, cids = gen.tile_offsets(w, k)
    nn = len(offs)
    eng.kafka_sessions(nn)
    assert int(lens.min()) >= 12
    h_arena = np.tile(w.arena, k)
    d_arena = torch.from_numpy(h_arena).to(dev)
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (offs.view(np.int64), lens.view(np.int32),
                                                                     cids.view(np.int32))]
    verdict = torch.ones(nn, dtype=torch.uint8, device=dev)
    tags = torch.arange(1, nn + 1, dtype=torch.int64, device=dev)
    fwd = torch.zeros(nn, dtype=torch.uint8, device=dev)
    new_id = torch.zeros(nn, dtype=torch.int32, device=dev)
    # responses: 8-byte frames, a size prefix and the id
    r_arena = torch.zeros((nn, 8), dtype=torch.uint8, device=dev)
    r_arena[:, 3] = 4
    r_off = torch.arange(nn, dtype=torch.int64, device=dev) * 8
    r_len = torch.full((nn,), 8, dtype=torch.int32, device=dev)
    ro = [torch.zeros(nn, dtype=t, device=dev) for t in (torch.uint8, torch.int32, torch.int16, torch.int16, torch.int64)]
    stream = torch.cuda.current_stream().cuda_stream
    now = [0]

    def forward():
        now[0] += 1
        eng.kafka_forward_device(d_arena.data_ptr(), d_arena.numel(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                 verdict.data_ptr(), tags.data_ptr(), nn, now[0], fwd.data_ptr(), new_id.data_ptr(),
                                 stream=stream)

    def fill_responses():
        r_arena[:, 4:] = new_id.view(torch.uint8).reshape(nn, 4).flip(1)

    def responses():
        eng.kafka_responses_device(r_arena.data_ptr(), r_arena.numel(), r_off.data_ptr(), r_len.data_ptr(),
                                   d[2].data_ptr(), nn, *[t.data_ptr() for t in ro], stream=stream)

    # ---- the check: the whole numbering, and a sample's bytes and entries
    forward()
    torch.cuda.synchronize()
    order = np.argsort(cids, kind="stable")
    sc = cids[order]
    want_id = np.zeros(nn, np.uint32)
    want_id[order] = (np.arange(nn) - np.searchsorted(sc, sc, side="left") + 1).astype(np.uint32)
    assert np.array_equal(new_id.cpu().numpy().view(np.uint32), want_id) and bool((fwd == 1).all())
    pick = np.random.default_rng(7).choice(nn, size=min(SAMPLE, nn), replace=False)
    got_arena = d_arena.cpu().numpy()
    o = offs.astype(np.int64)
    corr = be32_at(h_arena, o + 8)
    for i in pick.tolist():
        a, b = int(o[i]), int(o[i]) + int(lens[i])
        want = bytearray(h_arena[a:b].tobytes())
        want[8:12] = int(want_id[i]).to_bytes(4, "big")
        assert got_arena[a:b].tobytes() == bytes(want), i
    fill_responses()
    responses()
    torch.cuda.synchronize()
    found, orig, key, ver, tag = [t.cpu().numpy() for t in ro]
    assert bool(found.all())
    hr = r_arena.cpu().numpy()
    for i in pick.tolist():
        assert int(orig.view(np.uint32)[i]) == int(corr[i]) and int(tag[i]) == i + 1, i
        assert int(key[i]) == int(h_arena[o[i] + 4]) << 8 | int(h_arena[o[i] + 5]), i
        assert int(ver[i]) == int(h_arena[o[i] + 6]) << 8 | int(h_arena[o[i] + 7]), i
        assert hr[i].tobytes() == b"\x00\x00\x00\x04" + int(corr[i]).to_bytes(4, "big"), i
    st = eng.kafka_session_stats()
    assert (st["live"], st["forwarded"], st["found"], st["dropped"], st["missed"]) == (0, nn, nn, 0, 0), st
    out = {"n": nn, "unique": u, "copies": k, "connections": NCONNS, "reps": reps, "rounds": rounds,
           "table_slots": 1 << (2 * nn - 1).bit_length(), "ids_checked": nn, "sample_checked": int(len(pick))}

    # ---- the windows
    def window():
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
        for e in ev:
            e[0].record()
            forward()
            e[1].record()
            fill_responses()
            e[2].record()
            responses()
            e[3].record()
        torch.cuda.synchronize()
        return (sum(e[0].elapsed_time(e[1]) for e in ev) / reps, sum(e[2].elapsed_time(e[3]) for e in ev) / reps)

    for _ in range(3):
        forward()
        fill_responses()
        responses()
    torch.cuda.synchronize()
    t = {"forward": [], "responses": []}
    for _ in range(rounds):
        eng.kafka_session_gc(now[0], 1 << 40)
        a, b = window()
        t["forward"].append(a)
        t["responses"].append(b)
    assert bool((fwd == 1).all()) and bool((ro[0] == 1).all())
    for name in t:
        out[f"{name}_ms_per_call"] = round(float(np.median(t[name])), 4)
        out[f"{name}_windows_ms"] = [round(x, 4) for x in t[name]]
    out["used_slots_after_window"] = eng.kafka_session_stats()["used_slots"]

    # ---- the collection, once, at half occupancy
    eng.kafka_session_gc(now[0], 1 << 40)
    forward()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gone = eng.kafka_session_gc(now[0], 1 << 40)
    out["gc_ms_half_occupancy"] = round(1e3 * (time.perf_counter() - t0), 4)
    st = eng.kafka_session_stats()
    assert gone == 0 and st["live"] == st["used_slots"] == nn, st
    eng.kafka_sessions(0)

    # ---- the host path on one core: one cache per connection, the batch grouped by connection
    lib = _lib.load()
    t0 = time.perf_counter()
    order = np.argsort(cids, kind="stable")
    g_off = np.ascontiguousarray(offs[order])
    g_len = np.ascontiguousarray(lens[order])
    bounds = np.searchsorted(cids[order], np.arange(NCONNS + 1)).tolist()
    group_s = time.perf_counter() - t0
    caches = [lib.l7g_kafka_corr_create() for _ in range(NCONNS)]
    host_arena = h_arena.copy()
    ids = np.zeros(nn, np.uint32)
    ap, op, lp, ip = host_arena.ctypes.data, g_off.ctypes.data, g_len.ctypes.data, ids.ctypes.data
    t0 = time.perf_counter()
    for c in range(NCONNS):
        a, b = bounds[c], bounds[c + 1]
        lib.l7g_kafka_corr_requests(caches[c], ap, op + 8 * a, lp + 4 * a, b - a, ip + 4 * a)
    req_s = time.perf_counter() - t0
    assert np.array_equal(ids, want_id[order])
    h_r = np.zeros((nn, 8), np.uint8)
    h_r[:, 3] = 4
    h_r[:, 4:] = ids.byteswap().view(np.uint8).reshape(nn, 4)
    h_roff = np.arange(nn, dtype=np.uint64) * 8
    h_rlen = np.full(nn, 8, np.uint32)
    h_found = np.zeros(nn, np.uint8)
    rp, rop, rlp, fp = h_r.ctypes.data, h_roff.ctypes.data, h_rlen.ctypes.data, h_found.ctypes.data
    t0 = time.perf_counter()
    for c in range(NCONNS):
        a, b = bounds[c], bounds[c + 1]
        lib.l7g_kafka_corr_responses(caches[c], rp, rop + 8 * a, rlp + 4 * a, b - a, fp + a)
    rep_s = time.perf_counter() - t0
    assert bool(h_found.all())
    for c in caches:
        lib.l7g_kafka_corr_destroy(c)
    out["host_one_core"] = {"requests_ms": round(1e3 * req_s, 3), "responses_ms": round(1e3 * rep_s, 3),
                            "group_by_connection_ms": round(1e3 * group_s, 3),
                            "note": "4096 l7g_kafka_corr caches, one call per connection and direction; ctypes call "
                                    "overhead included, the argsort that groups the batch timed apart, PCIe not included"}
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()

"""What every parser's access-log records cost (GPU box): ms per call of
l7g_classify, l7g_classify_logged and l7g_classify_logged_all for 1M memcached,
1M r2d2, 1M cassandra and 1M mixed (cfg5) requests, device-resident: a unique
stream of n / copies requests whose arena is replicated on the device
(gen.tile_offsets, as bench.py does; every copy on connections of its own, so
that a cassandra USE of one copy does not reach the next).
The records are checked first: the three calls give the same verdicts, the
first copy's records and rows equal tests/generic_log_py.py (memcached, r2d2)
and the oracle's parser walked per connection (cassandra), every other copy's
equal the first copy's, and HTTP / Kafka records equal l7g_classify_logged's.
Then each leg: 3 warm-up calls and `rounds` windows of `reps` calls between two
HIP events, the three calls alternated; the median window is reported.
usage: python tools/exp_generic_log.py [n] [copies] [rounds]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import generic_log_py as G  # noqa: E402
import refpy  # noqa: E402
from cilium_amd import Engine, gen  # noqa: E402
from cilium_amd._lib import (ALLOW, DENY, PROTO_CASSANDRA, PROTO_HTTP, PROTO_KAFKA, PROTO_MEMCACHE,  # noqa: E402
                             PROTO_R2D2, cass_action_name)
from cilium_amd.engine import LOGREC_DTYPE  # noqa: E402

SPAN_STRIDE, TEXT_STRIDE = 4, 64
KEYWORDS = ("alter", "create", "drop", "truncate", "list")


def check_first_copy(w, v, rec, spans, text):
    """The first copy's generic records against the restatement / the oracle."""
    pol = refpy.Policy(w.policy)
    refs = {}
    proto = w.conns["proto"][w.conn_ids]
    arena = w.arena.tobytes()
    kinds = {3: 0, 4: 0, 5: 0, 6: 0}
    for i in range(w.n):
        data = arena[int(w.offsets[i]):int(w.offsets[i]) + int(w.lengths[i])]
        ci = int(w.conn_ids[i])
        path = None
        if proto[i] == PROTO_CASSANDRA:  # (every request: the parser's keyspace moves with each USE)
            if ci not in refs:
                refs[ci] = refpy.Cassandra(pol, w.conns[ci:ci + 1])
            path = refs[ci].request(data)[3]
        if v[i] not in (ALLOW, DENY) or proto[i] in (PROTO_HTTP, PROTO_KAFKA):
            continue
        r = rec[i]
        if proto[i] == PROTO_MEMCACHE:
            e = G.memcached(data, int(w.conns[ci]["flags"]))
            if e["proto"] == "textmemcached":
                nk = len(e["keys"])
                assert (r["kind"], r["mc_cmd_off"], r["mc_cmd_len"], r["mc_nkeys"], r["flags"]) == \
                    (3, *e["cmd"], nk, int(nk > SPAN_STRIDE)), i
                assert [tuple(x) for x in spans[i, :min(nk, SPAN_STRIDE)].tolist()] == e["keys"][:SPAN_STRIDE], i
            else:
                assert (r["kind"], r["api_key"], r["mcb_key_off"], r["mcb_key_len"]) == (4, e["opcode"], *e["key"]), i
        elif proto[i] == PROTO_R2D2:
            e = G.r2d2(data)
            assert (r["kind"], r["r2_cmd_len"], r["r2_file_off"], r["r2_file_len"], r["r2_nfields"]) == \
                (5, e["cmd_len"], *e["file"], e["nfields"]), i
        else:
            e = G.cassandra_path(path)
            assert r["kind"] == 6 and bool(r["flags"] & 2) == (e is not None), (i, path)
            if e is not None:
                table = e["fields"]["query_table"]
                m = min(len(table), TEXT_STRIDE)
                assert r["cass_table_len"] == len(table) and text[i, :m].tobytes() == table[:m], (i, path)
                a = int(r["api_key"])
                if a >= 0:
                    name = cass_action_name(a).encode()
                else:
                    word = data[int(r["cass_word_off"]):int(r["cass_word_off"]) + int(r["cass_word_len"])].lower()
                    name = KEYWORDS[int(r["cass_keyword"])].encode() + b"-" + word + \
                        (b"-view" if word == b"materialized" else b"")
                assert name == e["fields"]["query_action"], (i, path)
        kinds[int(r["kind"])] += 1
    return kinds


def own_connections(w, k):
    """k copies of w's requests, copy j on connections [j * nconns, (j + 1) * nconns)."""
    offs, lens, cids = gen.tile_offsets(w, k)
    nc = len(w.conns)
    cids = (cids.reshape(k, -1) + (np.arange(k, dtype=np.uint32) * np.uint32(nc))[:, None]).reshape(-1)
    return offs, lens, cids.astype(np.uint32), np.tile(w.conns, k)


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    reps, u = 10, n // k
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    out = {"n": u * k, "unique": u, "copies": k, "reps": reps, "rounds": rounds, "span_stride": SPAN_STRIDE,
           "text_stride": TEXT_STRIDE}
    for name, w in (("memcached", gen.memcache_workload(u)), ("r2d2", gen.r2d2_workload(u)),
                    ("cassandra", gen.cassandra_workload(u)), ("cfg5_mixed", gen.mixed_workload(u))):
        offs, lens, cids, conns = own_connections(w, k)
        eng.update_policy(w.policy)
        eng.set_connections(conns)
        nn = len(offs)
        d_arena = torch.from_numpy(w.arena).to(dev).repeat(k)
        d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
             for a in (offs.view(np.int64), lens.view(np.int32), cids.view(np.int32))]
        o = [torch.full((nn,), 7, dtype=t, device=dev) for t in (torch.uint8, torch.int32, torch.int32)]
        rec = torch.zeros((nn, 8), dtype=torch.int32, device=dev)
        spans = torch.zeros((nn, SPAN_STRIDE, 2), dtype=torch.int32, device=dev)
        text = torch.zeros((nn, TEXT_STRIDE), dtype=torch.uint8, device=dev)
        args = (d_arena.data_ptr(), d_arena.numel(), *[t.data_ptr() for t in d], nn, *[t.data_ptr() for t in o])

        def call(leg):
            s = torch.cuda.current_stream().cuda_stream
            if leg == "all":
                eng.classify_logged_all_device(*args, rec.data_ptr(), spans.data_ptr(), SPAN_STRIDE, text.data_ptr(),
                                               TEXT_STRIDE, stream=s)
            elif leg == "logged":
                eng.classify_logged_device(*args, rec.data_ptr(), spans.data_ptr(), SPAN_STRIDE, stream=s)
            else:
                eng.classify_device(*args, stream=s)

        def window(leg):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                call(leg)
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / reps

        def outputs(leg):
            call(leg)
            torch.cuda.synchronize()
            return [t.cpu().numpy().copy() for t in o], rec.cpu().numpy().view(np.uint32).reshape(nn, 8).copy(), \
                spans.cpu().numpy().view(np.uint32).copy()

        plain, _, _ = outputs("plain")
        lo, lrec, lspans = outputs("logged")
        spans.zero_()
        ao, arec, aspans = outputs("all")
        assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(plain, lo, ao)), name
        v = plain[0]
        done = (v == ALLOW) | (v == DENY)
        proto = np.tile(w.conns["proto"][w.conn_ids], k)
        hk = (proto == PROTO_HTTP) | (proto == PROTO_KAFKA)
        assert np.array_equal(arec[done & hk], lrec[done & hk]) and np.array_equal(aspans[hk], lspans[hk]), name
        # every copy as the first
        d2 = done.reshape(k, u)
        assert (d2 == d2[0]).all()
        r3 = arec.reshape(k, u, 8)
        assert (r3[:, d2[0]] == r3[0, d2[0]]).all(), name
        h_text = text.cpu().numpy()
        assert (aspans.reshape(k, u, -1) == aspans.reshape(k, u, -1)[0]).all(), name
        assert (h_text.reshape(k, u, -1) == h_text.reshape(k, u, -1)[0]).all(), name
        kinds = check_first_copy(w, v[:u], arec[:u].view(LOGREC_DTYPE).reshape(u), aspans.reshape(nn, SPAN_STRIDE, 2)[:u],
                                 h_text[:u])
        legs = {"plain": [], "logged": [], "all": []}
        for leg in legs:
            for _ in range(3):
                call(leg)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for leg in legs:
                legs[leg].append(window(leg))
        med = {leg: float(np.median(x)) for leg, x in legs.items()}
        out[name] = {"records_checked_per_copy": kinds, "verdicts": np.bincount(v, minlength=5).tolist(),
                     "plain_ms_per_call": round(med["plain"], 4), "logged_ms_per_call": round(med["logged"], 4),
                     "logged_all_ms_per_call": round(med["all"], 4),
                     "all_minus_plain_ms": round(med["all"] - med["plain"], 4),
                     "all_minus_logged_ms": round(med["all"] - med["logged"], 4),
                     "all_over_plain_pct": round(100 * (med["all"] - med["plain"]) / med["plain"], 2),
                     **{leg + "_windows_ms": [round(x, 4) for x in xs] for leg, xs in legs.items()}}
        del d_arena, d, o, rec, spans, text
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()

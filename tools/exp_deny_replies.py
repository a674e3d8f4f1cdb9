"""What the deny replies cost (GPU box): ms per call of l7g_deny_replies for
1M device-resident requests -- a unique stream of n / copies requests whose
arena is replicated on the device (gen.tile_offsets, as bench.py does) -- over
three legs: (a) cfg3 Kafka under a policy that denies about 1 %, (b) the same
requests under a policy that denies them all, (c) the cfg5 mix with about 1 %
denied.  Each leg first checks the replies of a sample of denied requests
against the host function (Kafka) or the template (HTTP), and that every copy's
lengths equal the first copy's.  Then 3 warm-up calls and `rounds` windows of
`reps` calls between two HIP events; the median window is reported.  One call =
sizes and bytes, into a buffer of exactly total[0] bytes.
Beside each: l7g_classify of the same batch, timed the same way, and the time
one CPU core takes to call l7g_kafka_deny_response for the same denied Kafka
requests (the path the call replaces: a comparison, not a target; it does not
include copying the requests back over PCIe).
usage: python tools/exp_deny_replies.py [n] [copies] [rounds]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cilium_amd import Engine, _lib, api, gen  # noqa: E402
from cilium_amd._lib import DENY, PROTO_HTTP, PROTO_KAFKA  # noqa: E402

SAMPLE = 2000


def one_percent_policy():
    """cfg3's generator names 1000 topics and, one time in ten, one of 1000
    "other-" topics: every topic allowed but the last 40 others."""
    rules = [api.PortRuleKafka(topic=t) for t in gen.kafka_topics()]
    rules += [api.PortRuleKafka(topic=f"other-{j:04d}") for j in range(960)]
    rules += [api.PortRuleKafka(api_key=k) for k in ("metadata", "apiversions", "heartbeat")]
    return api.policy_set(api.network_policy("k1", 3, ingress=[(9092, [api.port_rule(kafka=rules)])]))


def deny_all_policy():
    return api.policy_set(api.network_policy("k0", 3, ingress=[(9092, [api.port_rule(
        kafka=[api.PortRuleKafka(api_key="produce", topic="zz-nomatch")])])]))


def mixed_one_percent(u):
    """cfg5 with every 64th connection under its cfg5 policy and the others
    under one without L7 restrictions."""
    w = gen.mixed_workload(u)
    ports = sorted({int(p) for p in w.conns["port"]})
    wide = [(p, [api.port_rule(kafka=[api.PortRuleKafka()]) if p == 9092 else api.port_rule()]) for p in ports]
    pol = {"policies": w.policy["policies"] + [api.network_policy("open", 21, ingress=wide, egress=wide)]}
    conns = w.conns.copy()
    strict = np.arange(len(conns)) % 64 == 0
    conns["policy"][~strict] = len(pol["policies"]) - 1
    return gen.Workload("cfg5-1pct", w.arena, w.offsets, w.lengths, w.conn_ids, conns, pol, w.meta)


def cpu_kafka_replies(reqs):
    """Seconds one core takes to call l7g_kafka_deny_response for reqs, and the
    bytes it wrote (ctypes call overhead included)."""
    lib = _lib.load()
    out = C.create_string_buffer(1 << 20)
    n = C.c_size_t(0)
    ref = C.byref(n)
    fn = lib.l7g_kafka_deny_response
    total = 0
    t0 = time.perf_counter()
    for r in reqs:
        if fn(r, len(r), out, 1 << 20, ref) == 0:
            total += n.value
    return time.perf_counter() - t0, total


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    reps, u = 10, n // k
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    out = {"n": u * k, "unique": u, "copies": k, "reps": reps, "rounds": rounds}
    kw = gen.kafka_workload(u)
    legs = (("a_cfg3_one_percent", kw, one_percent_policy()), ("b_cfg3_all_denied", kw, deny_all_policy()),
            ("c_cfg5_one_percent", None, None))
    for name, w, pol in legs:
        if w is None:
            w = mixed_one_percent(u)
            pol = w.policy
        eng.update_policy(pol)
        eng.set_connections(w.conns)
        offs, lens, cids = gen.tile_offsets(w, k)
        nn = len(offs)
        d_arena = torch.from_numpy(w.arena).to(dev).repeat(k)
        d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
             for a in (offs.view(np.int64), lens.view(np.int32), cids.view(np.int32))]
        o = [torch.full((nn,), 7, dtype=t, device=dev) for t in (torch.uint8, torch.int32, torch.int32)]
        ro = torch.zeros(nn, dtype=torch.int64, device=dev)
        rl = torch.zeros(nn, dtype=torch.int32, device=dev)
        tot = torch.zeros(2, dtype=torch.int64, device=dev)
        args = (d_arena.data_ptr(), d_arena.numel(), *[t.data_ptr() for t in d], nn)

        def classify():
            eng.classify_device(*args, *[t.data_ptr() for t in o], stream=torch.cuda.current_stream().cuda_stream)

        classify()
        eng.deny_replies_device(*args, o[0].data_ptr(), 0, 0, ro.data_ptr(), rl.data_ptr(), tot.data_ptr(),
                                stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        total, nreplies = [int(x) for x in tot.cpu().numpy().view(np.uint64)]
        buf = torch.zeros(max(total, 1), dtype=torch.uint8, device=dev)

        def replies():
            eng.deny_replies_device(*args, o[0].data_ptr(), buf.data_ptr(), total, ro.data_ptr(), rl.data_ptr(),
                                    tot.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)

        def window(fn):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / reps

        replies()
        torch.cuda.synchronize()
        # ---- the sample, and every copy against the first
        v = o[0].cpu().numpy()
        h_len = rl.cpu().numpy().view(np.uint32)
        h_off = ro.cpu().numpy().view(np.uint64)
        h_buf = buf.cpu().numpy()
        assert (h_len.reshape(k, u) == h_len[:u]).all() and (v.reshape(k, u) == v[:u]).all()
        assert np.array_equal(h_off[1:], np.cumsum(h_len.astype(np.uint64))[:-1]) and h_off[0] == 0
        proto = w.conns["proto"][w.conn_ids]
        arena = w.arena.tobytes()
        req = lambda i: arena[int(w.offsets[i]):int(w.offsets[i]) + int(w.lengths[i])]  # noqa: E731
        denied = np.nonzero(v == DENY)[0]
        pick = np.random.default_rng(7).choice(denied, size=min(SAMPLE, len(denied)), replace=False)
        for i in pick.tolist():
            j = i % u
            got = h_buf[int(h_off[i]):int(h_off[i]) + int(h_len[i])].tobytes()
            if proto[j] == PROTO_KAFKA:
                want = _lib.kafka_deny_response(req(j)) or b""
            elif proto[j] == PROTO_HTTP:
                want = _lib.deny_reply_template(PROTO_HTTP)
            else:
                want = b""
            assert got == want, (name, i)
        # ---- the windows
        res = {"verdicts": np.bincount(v, minlength=5).tolist(), "denied_pct": round(100 * len(denied) / nn, 3),
               "replies": nreplies, "reply_bytes": total, "sample_checked": int(len(pick))}
        t = {"classify": [], "deny_replies": []}
        for fn in (classify, replies):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            t["classify"].append(window(classify))
            t["deny_replies"].append(window(replies))
        res["classify_ms_per_call"] = round(float(np.median(t["classify"])), 4)
        res["deny_replies_ms_per_call"] = round(float(np.median(t["deny_replies"])), 4)
        res["classify_windows_ms"] = [round(x, 4) for x in t["classify"]]
        res["deny_replies_windows_ms"] = [round(x, 4) for x in t["deny_replies"]]
        # ---- one CPU core over the same denied Kafka requests (the first copy's, scaled by the copies)
        kd = [req(j) for j in np.nonzero((v[:u] == DENY) & (proto == PROTO_KAFKA))[0].tolist()]
        secs, wrote = cpu_kafka_replies(kd)
        res["cpu_one_core"] = {"kafka_requests": len(kd) * k, "ms": round(1e3 * secs * k, 3),
                               "us_per_request": round(1e6 * secs / max(len(kd), 1), 3), "reply_bytes": wrote * k,
                               "note": "first copy timed, scaled by copies; ctypes call overhead included"}
        out[name] = res
        del d_arena, d, o, ro, rl, tot, buf
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()

"""Throughput of the cassandra session path (GPU box): a 1M-request batch over
4096 connections, device-resident, through l7g_classify --
  execute/sessions   every request an EXECUTE of a bound id (sessions on);
  query/sessions     the same statement as a plain QUERY, sessions on (the
                     marks, two sorts and the commit launches, no lookup);
  query/stateless    the same QUERYs with sessions off (the stateless kernel).
Each leg: 3 warm-up calls, then `reps` calls between two HIP events; the
median of `rounds` such windows, legs alternated.  Every leg's answers are
checked (all ALLOW, by the ^ks1\\. rule) before anything is timed.
usage: python tools/exp_cass_sessions.py [n] [nconns]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cilium_amd import Engine, gen  # noqa: E402


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    nconns = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    reps, rounds = 10, 5
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    eng.update_policy(gen.cassandra_policy())
    conns = gen.make_conns(nconns, 0, gen.CASS_PORT, True, gen.PROTO_CASSANDRA, [100] * nconns)
    rng = np.random.default_rng(gen.SEED_BASE + 32)
    cid = rng.integers(0, nconns, size=n).astype(np.uint32)
    ids = [b"stmt%04d" % (c % 7) for c in range(nconns)]
    every = np.arange(nconns, dtype=np.uint32)

    def open_sessions():
        eng.set_connections(conns)
        for frames, reply in (([gen.cass_query_frame("use ks1")] * nconns, False),
                              ([gen.cass_query_frame("select * from users", 0x09, stream=1)] * nconns, False),
                              ([gen.cass_prepared_reply(ids[c], 1) for c in range(nconns)], True)):
            arena, offs, lens = gen.pack(frames)
            (eng.cass_replies if reply else eng.classify)(arena, offs, lens, every)

    def batch(frames):
        arena, offs, lens = gen.pack(frames)
        d = [torch.from_numpy(a).to(dev) for a in (arena, offs.view(np.int64), lens.view(np.int32), cid.view(np.int32))]
        o = [torch.full((n,), 7, dtype=t, device=dev) for t in (torch.uint8, torch.int32, torch.int32)]
        return d, o

    def call(b):
        d, o = b
        eng.classify_device(d[0].data_ptr(), d[0].numel(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n,
                            o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                            stream=torch.cuda.current_stream().cuda_stream)

    def window(b):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            call(b)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / reps

    ex = batch([gen.cass_execute_frame(ids[int(c)], stream=2) for c in cid])
    qy = batch([gen.cass_query_frame("select * from ks1.users", stream=2)] * n)
    legs = {"execute/sessions": [], "query/sessions": [], "query/stateless": []}
    verdicts = {}
    for r in range(rounds + 1):  # round 0 warms every leg up and checks its answers
        for name in legs:
            if name.endswith("stateless"):
                eng.cass_sessions(0)
                eng.set_connections(conns)
            else:
                eng.cass_sessions(1 << 16)
                open_sessions()
            b = ex if name.startswith("execute") else qy
            for _ in range(3):
                call(b)
            torch.cuda.synchronize()
            if r == 0:
                v = b[1][0].cpu().numpy()
                verdicts[name] = np.bincount(v, minlength=5).tolist()
                assert verdicts[name][1] == n, (name, verdicts[name])  # ks1.users: ALLOW by the ^ks1\. rule
            else:
                legs[name].append(window(b))
            if name == "execute/sessions":
                st = eng.cass_session_stats()  # (of this leg: enabling sessions again starts them anew)
    out = {"n": n, "nconns": nconns, "reps": reps, "rounds": rounds, "verdicts": verdicts, "session_stats": st}
    for name, ms in legs.items():
        m = float(np.median(ms))
        out[name] = {"ms_per_call": round(m, 4), "requests_per_s": round(n / m * 1e3), "windows_ms": [round(x, 4) for x in ms]}
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()

"""The Kafka / memcached leg of each step of a run (measurement tool): from a
rocprofv3 --kernel-trace CSV, per step, the end of the Kafka kernel's main
grid, the start and end of the memcached kernel beside it, of the second
(helper) Kafka grid behind that when there is one, and of the inflate kernel,
in ms from the main grid's start; then memcached end - main Kafka end
(negative: memcached is done first) and the leg's length (to the last end).
usage: python tools/leg_timeline.py TRACE.csv [steps to skip at the front]"""
import csv
import statistics
import sys


def main():
    rows = [r for r in csv.DictReader(open(sys.argv[1])) if "l7::" in r["Kernel_Name"]]
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows)
    kafka = [e for e in ev if "kafka_classify_kernel" in e[2]]
    mcs = [e for e in ev if "memcache_classify" in e[2]]
    zfs = [e for e in ev if "kafka_inflate" in e[2]]
    print("step  kafka_end  mc_start  mc_end  helper_start  helper_end  inflate_start  inflate_end  inflate_ms  "
          "mc_end-kafka_end  leg_ms  (ms from the Kafka main grid's start)")
    gaps, legs = [], []
    for i, (m0, m1, _) in enumerate(mcs):
        nxt = mcs[i + 1][0] if i + 1 < len(mcs) else 1 << 62
        before = [e for e in kafka if e[0] <= m0]
        if not before:
            continue
        k0, k1, _ = before[-1]  # the main grid: launched just before the memcached kernel
        later = [e for e in kafka if m0 < e[0] < nxt]
        if i + 1 < len(mcs) and later:
            later = later[:-1]  # (the next step's main grid)
        helper = later[0] if later else None
        zf = [e for e in zfs if k0 <= e[0] < nxt]
        if not zf:
            continue
        ms = lambda t: (t - k0) / 1e6  # noqa: E731
        z0, z1 = zf[0][0], zf[0][1]
        leg = max(k1, m1, z1, helper[1] if helper else 0)
        h = f"{ms(helper[0]):12.3f}  {ms(helper[1]):10.3f}" if helper else f"{'-':>12s}  {'-':>10s}"
        print(f"{i:4d}  {ms(k1):9.3f}  {ms(m0):8.3f}  {ms(m1):6.3f}  {h}  {ms(z0):13.3f}  {ms(z1):11.3f}  "
              f"{(z1 - z0) / 1e6:10.4f}  {(m1 - k1) / 1e6:16.3f}  {ms(leg):6.3f}")
        if i >= skip:
            gaps.append((m1 - k1) / 1e6)
            legs.append(ms(leg))
    if gaps:
        print(f"steps {skip}..: median mc_end-kafka_end {statistics.median(gaps):.3f} ms (max {max(gaps):.3f}), "
              f"median leg {statistics.median(legs):.3f} ms")


if __name__ == "__main__":
    main()

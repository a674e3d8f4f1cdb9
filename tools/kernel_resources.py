"""Per-kernel resources (measurement tool), from either of two inputs.

A rocprofv3 --kernel-trace CSV of a run: each kernel's first dispatch -- LDS
bytes per workgroup, scratch bytes per lane, VGPRs (the trace's VGPR_Count is
in units of 2 registers on this ROCm: 128 = 256 VGPRs; the 'vgprs' column
doubles it), SGPRs, workgroup size -- and its dispatch count and mean duration.

A gfx950 code object (no GPU needed): the same columns from the kernels'
metadata notes, plus the spill counts, read with llvm-readelf.  One is made with
  hipcc -O3 -std=c++17 --offload-arch=gfx950 -mcode-object-version=5 -munsafe-fp-atomics \\
        --offload-device-only --no-gpu-bundle-output -c KERNEL.hip -o KERNEL.co
usage: python tools/kernel_resources.py TRACE.csv|KERNEL.co [pattern]"""
import collections
import csv
import os
import re
import subprocess
import sys


def from_trace(path, pat):
    first, durs = {}, collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        k = r["Kernel_Name"]
        if pat not in k:
            continue
        durs[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
        first.setdefault(k, r)
    print(f"{'kernel':70s} {'lds_B':>7s} {'scratch_B':>9s} {'vgprs':>5s} {'sgprs':>5s} {'wg':>5s} {'calls':>5s} {'mean_ms':>9s}")
    for k, r in sorted(first.items(), key=lambda kv: -sum(durs[kv[0]])):
        print(f"{k[:70]:70s} {int(r['LDS_Block_Size']):7d} {int(r['Scratch_Size']):9d} {2 * int(r['VGPR_Count']):5d} "
              f"{int(r['SGPR_Count']):5d} {int(r['Workgroup_Size_X']):5d} {len(durs[k]):5d} {sum(durs[k]) / len(durs[k]):9.4f}")


def _tool(name):
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm") + "/llvm/bin", "/opt/rocm/llvm/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return name


def from_code_object(path, pat):
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", path], capture_output=True, text=True, check=True).stdout
    rows = []
    for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        f = dict(re.findall(r"\.(\w+):\s+'?([^'\n]+)'?", ".agpr_count:" + blk))
        if "name" not in f or "vgpr_count" not in f:
            continue
        name = f["name"]
        for filt in (_tool("llvm-cxxfilt"), "c++filt"):
            try:
                name = subprocess.run([filt, f["name"]], capture_output=True, text=True).stdout.strip() or name
                break
            except OSError:
                pass
        name = re.sub(r"^void ", "", name).split("(")[0]
        if pat in name or pat.replace("::", "") in f["name"]:
            rows.append((name, f))
    print(f"{'kernel':70s} {'lds_B':>7s} {'scratch_B':>9s} {'vgprs':>5s} {'sgprs':>5s} {'wg':>5s} {'vspill':>6s} {'sspill':>6s}")
    for name, f in sorted(rows, key=lambda r: (r[0], r[1]["name"])):  # (two kernels may print one name)
        print(f"{name[:70]:70s} {int(f['group_segment_fixed_size']):7d} {int(f['private_segment_fixed_size']):9d} "
              f"{int(f['vgpr_count']):5d} {int(f['sgpr_count']):5d} {int(f['max_flat_workgroup_size']):5d} "
              f"{int(f.get('vgpr_spill_count', 0)):6d} {int(f.get('sgpr_spill_count', 0)):6d}")


def main():
    path = sys.argv[1]
    pat = sys.argv[2] if len(sys.argv) > 2 else "l7::"
    if path.endswith(".csv"):
        from_trace(path, pat)
    else:
        from_code_object(path, pat)


if __name__ == "__main__":
    main()

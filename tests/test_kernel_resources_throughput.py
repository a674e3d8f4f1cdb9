"""Compiled resources of the throughput classifiers (no GPU needed).

kafka_classify.hip is cross-compiled for gfx950 with the command in
tools/kernel_resources.py's docstring and its kernels' metadata notes are read
through that tool, as profiles/no_scratch/kernel_resources.txt was made.

Of the three parts built (profiles/no_scratch/ab_cfg5.txt) only the Kafka one
made the cfg5 step faster and was kept, so it is the one pinned here:

  * kafka_classify_kernel<{5, 6}, false>: at most 12 bytes of scratch per lane,
    the round-3 value (they had 8 and 56), at the waves per SIMD they are
    built for (5: at most 96 VGPRs, 6: at most 80) and with the CRC tables'
    and staging slots' 24 KiB of LDS;
  * kafka_classify_kernel<4, true>, the logged build, no worse than it was:
    no scratch, no spilled VGPR, at most its earlier 118 VGPRs.

The HTTP kernels that stage an image in LDS and memcache_classify_kernel<1>
keep the scratch the table shows (80 and 28 bytes): without it the step was
not faster, and those changes were left out; nothing is asserted of them, so
their sources (a minute and more of compiling) are not built here.
"""
import concurrent.futures as cf
import contextlib
import io
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "cilium_amd", "csrc", "kernels")
SOURCES = ("kafka_classify",)


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def _compile(hipcc, name, out):
    co = os.path.join(out, name + ".co")
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-mcode-object-version=5", "-munsafe-fp-atomics",
           "--offload-device-only", "--no-gpu-bundle-output", "-c", os.path.join(KERNELS, name + ".hip"), "-o", co]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return co


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{kernel name: {column: value}} of the sources' kernels (compiled once, side by side)."""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc is not installed: the kernels cannot be cross-compiled")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    out = str(tmp_path_factory.mktemp("co"))
    with cf.ThreadPoolExecutor(len(SOURCES)) as ex:
        cos = list(ex.map(lambda s: _compile(hipcc, s, out), SOURCES))
    rows = {}
    for co in cos:
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            kernel_resources.from_code_object(co, "l7::")
        lines = buf.getvalue().splitlines()
        cols = lines[0].split()[1:]
        for ln in lines[1:]:
            f = ln.rsplit(None, len(cols))
            rows[f[0].strip()] = dict(zip(cols, map(int, f[1:])))
    return rows


KAFKA = {"l7::kafka_classify_kernel<5, false>": 96, "l7::kafka_classify_kernel<6, false>": 80}


@pytest.mark.parametrize("kernel", sorted(KAFKA))
def test_kafka_scratch_at_most_round3(resources, kernel):
    r = resources[kernel]
    print(kernel, r)
    assert r["scratch_B"] <= 12, r


@pytest.mark.parametrize("kernel", sorted(KAFKA))
def test_kafka_keeps_its_occupancy_and_lds(resources, kernel):
    r = resources[kernel]
    assert r["vgprs"] <= KAFKA[kernel] and r["lds_B"] == 24576 and r["wg"] == 256, r


def test_kafka_logged_build_is_no_worse(resources):
    r = resources["l7::kafka_classify_kernel<4, true>"]
    print(r)
    assert r["scratch_B"] == 0 and r["vspill"] == 0 and r["vgprs"] <= 118 and r["lds_B"] == 24576, r

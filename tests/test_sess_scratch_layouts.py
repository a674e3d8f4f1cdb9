"""The scratch layouts of the session calls on the host
(tests/native/sess_scratch_main.cc over cilium_amd/csrc/kernels/sess_scratch.h):
for n in {1, 255, 256, 257, 2^20, 2^31 - 1}, nconns in {0, 1, 4096, 2^32 - 1}
and several temp-storage sizes, every layout's regions are 256-byte aligned,
in order and disjoint, and every offset and total equals the formula the
sizing functions and launchers used to spell out each on their own."""
import json
import subprocess

from cilium_amd import build as b


def test_layouts_are_aligned_ordered_disjoint_and_as_before():
    exe = [x for x in b.build_test_natives() if x.endswith("sess_scratch_main")][0]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["bad"] == 0, r.stderr
    assert d["checked"] == 6 * 4 * 8 * 5, d  # every point, every layout

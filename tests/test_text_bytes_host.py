"""The White_Space rune rule the text kernels and the host scan share
(cilium_amd/csrc/kernels/text_bytes.h: ws_rune_len), on the host
(tests/native/text_bytes_main.cc): over all 2^24 three-byte values with 1, 2
and 3 of the bytes present, the accepted sequences are exactly the UTF-8
encodings of Unicode White_Space (unicode.IsSpace, what bytes.Fields splits
on), the width never exceeds what is present, depends only on the bytes it
covers, and is 0 where the rune is cut short; and proxylib/shim.cc's SpaceLen
agrees with the rule on every accepted sequence and on the near misses of the
memcached generators."""
import json
import subprocess

import mc_edge_cases
from cilium_amd import build as b
from cilium_amd import gen

# Unicode White_Space, spelled out (not taken from the header)
WHITE_SPACE = [0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680,
               0x2000, 0x2001, 0x2002, 0x2003, 0x2004, 0x2005, 0x2006, 0x2007, 0x2008, 0x2009, 0x200A,
               0x2028, 0x2029, 0x202F, 0x205F, 0x3000]


def test_rune_rule_over_every_three_bytes_and_the_host_scan():
    exe = [x for x in b.build_test_natives() if x.endswith("text_bytes_main")][0]
    near = sorted(set(gen._MC_NOT_SPACES) | set(mc_edge_cases.NEAR))
    r = subprocess.run([exe], input="".join(s.hex() + "\n" for s in near), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    want = {chr(cp).encode("utf-8") for cp in WHITE_SPACE}
    assert len(want) == 25
    got = {bytes.fromhex(h): w for h, w in d["accepted"]}
    assert set(got) == want, (sorted(set(got) ^ want))
    assert len(d["accepted"]) == 25 and all(len(s) == w for s, w in got.items())
    assert d["violations"] == 0, r.stderr
    assert d["near"] == len(near) and d["spacelen_calls"] > 3 * (25 + len(near))
    assert d["spacelen_disagree"] == 0, r.stderr
    assert d["points"] == 3 * 2 ** 24

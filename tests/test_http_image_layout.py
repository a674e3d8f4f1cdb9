"""The HTTP rule-set image as the branch-free DFA step needs it (no GPU):
every image carries the null DFA behind its header, every slot of every
compiled rule set has a class table, row 0 of every transition table loops
back to state 0, and a tables image exported by a build with the previous
layout is refused by l7g_tables_import because of its tag."""
import os
import struct

import pytest

import cilium_amd
from cilium_amd import gen
from http_image import (DEV_DFA, H_DFA_OFF, H_NDFA, H_SLOT_DFA, LDS_IMAGE_BYTES, NULL_DFA_BYTES, NULL_DFA_OFF, NUM_SLOTS,
                        http_images)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _check_image(img):
    assert len(img) >= NULL_DFA_OFF + NULL_DFA_BYTES
    assert img[NULL_DFA_OFF:NULL_DFA_OFF + NULL_DFA_BYTES] == bytes(NULL_DFA_BYTES)
    ndfa = img[H_NDFA]
    slot_dfa = img[H_SLOT_DFA:H_SLOT_DFA + NUM_SLOTS + 1]
    (dfa_off,) = struct.unpack_from("<I", img, H_DFA_OFF)
    assert dfa_off >= NULL_DFA_OFF + NULL_DFA_BYTES  # nothing overlaps the null DFA
    assert slot_dfa[NUM_SLOTS] == ndfa
    walked = 0
    for s in range(NUM_SLOTS):
        lo, hi = slot_dfa[s], slot_dfa[s + 1]
        assert lo <= hi <= ndfa
        # a slot without a DFA walks the null DFA (checked above); the others:
        for d in range(lo, hi):
            cls_off, trans_off, mask_off, ncls, start, absorb, _ = struct.unpack_from("<IIIHHII", img, dfa_off + DEV_DFA * d)
            assert cls_off + 256 <= len(img) and mask_off != 0
            cls = img[cls_off:cls_off + 256]
            assert max(cls) < ncls
            row0 = struct.unpack_from(f"<{ncls}H", img, trans_off)
            assert row0 == (0,) * ncls, "state 0 must loop back to itself"
            assert 1 <= absorb and start < 65536 and 2 * ncls < 65536
            walked += 1
    assert walked == ndfa
    return ndfa


@pytest.mark.parametrize("cfg", ["cfg1", "cfg2", "cfg4"])
def test_every_slot_has_class_table_and_looping_dead_row(cfg):
    if cfg == "cfg4":
        w = gen.cfg4_workload(64, nids=64, rules_total=64 * 20)
    else:
        w = gen.http_workload(int(cfg[3]), 64)
    e = cilium_amd.Engine(-1)
    e.update_policy(w.policy)
    e.set_connections(w.conns)
    imgs = http_images(e.export_tables())
    assert len(imgs) >= (64 if cfg == "cfg4" else 1)
    assert sum(_check_image(img) for img in imgs) >= 1
    for img in imgs:
        assert len(img) <= LDS_IMAGE_BYTES  # these rule sets stay stageable in LDS (kLdsImageBytes)
    e.close()


def test_previous_layout_export_is_refused():
    """tests/golden/http_tables_layout2.bin: l7g_tables_export of the cfg1
    policy by the build before the null DFA (layout tag 2)."""
    with open(os.path.join(GOLDEN, "http_tables_layout2.bin"), "rb") as f:
        old = f.read()
    e = cilium_amd.Engine(-1)
    e.update_policy(gen.cfg1_policy())
    cur = e.export_tables()
    assert old[:8] == cur[:8] and old[8:16] != cur[8:16]  # same magic, another tag
    assert old[15] == 2 and cur[15] == 3
    with pytest.raises(cilium_amd.PolicyError, match="layout"):
        e.import_tables(old)
    e.import_tables(cur)
    e.close()

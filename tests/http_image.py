"""Reading HTTP rule-set images out of an l7g_tables_export buffer (test helper;
the layout is cilium_amd/csrc/device_tables.h and engine/serial.h)."""
import struct

# ImgHeader (80 B) field offsets
IMG_HEADER = 80
H_NDFA = 3                 # u8
H_SLOT_DFA = 4             # u8[NUM_SLOTS + 1]
H_MAX_SLOT_DFAS = 16       # u8: most DFAs on one slot = framing passes
H_DFA_OFF = 24             # u32: DevDfa[ndfa]
NUM_SLOTS = 11
DEV_DFA = 24               # sizeof(DevDfa)
NULL_DFA_OFF, NULL_DFA_BYTES = IMG_HEADER, 256   # kImgNullDfaOff, kImgNullDfaBytes
LDS_IMAGE_BYTES = 32 * 1024                      # kLdsImageBytes


def http_images(export):
    """[magic | layout tag | form | px | policy source | DevRuleset[] | images | ...] -> the rule sets' images."""
    (srclen,) = struct.unpack_from("<Q", export, 32)
    at = 40 + srclen
    (nrs,) = struct.unpack_from("<Q", export, at)
    rs = [struct.unpack_from("<II", export, at + 8 + 8 * i) for i in range(nrs)]
    at += 8 + 8 * nrs
    (nbytes,) = struct.unpack_from("<Q", export, at)
    images = export[at + 8:at + 8 + nbytes]
    assert len(images) == nbytes
    return [images[off:off + ln] for off, ln in rs]

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


# ---- the DFAs of an image (DevDfa: cls_off, trans_off, mask_off u32; ncls, start u16; absorb, pad u32)
H_NCHUNKS, H_NHDR = 0, 1   # u8
H_RULE_OFF = 36            # u32: i32[nchunks * 64] global rule ids
H_HDR_OFF = 40             # u32: DevHdrName[nhdr] (hash u32, len u16, pad u16, name_off u32)
H_TOTAL_STATES = 44        # u32
H_NFA_OFF, H_NNFA = 64, 68  # u32: DevNfaRef[nnfa] (nfa u64, mask_off u32, slot u8, pad); u8
SLOT_NAMES = [":method", ":path", ":authority"]
TOKEN_BYTES = [9] + [b for b in range(0x20, 0x100) if b != 0x7F]   # HT, SP, VCHAR, obs-text


class Dfa:
    """One serialized DFA: class table, transition rows, mask rows (one int per
    state: chunk c in bits [64c, 64c + 64))."""

    def __init__(self, img, off, nchunks):
        cls_off, trans_off, mask_off, self.ncls, self.start, self.absorb, _ = struct.unpack_from("<IIIHHII", img, off)
        self.cls = img[cls_off:cls_off + 256]
        assert len(self.cls) == 256 and max(self.cls) < self.ncls
        # every state of a subset construction is reached from the start state (and 0 is the dead one)
        rows, todo = {}, [0, self.start]
        while todo:
            s = todo.pop()
            if s in rows:
                continue
            rows[s] = struct.unpack_from(f"<{self.ncls}H", img, trans_off + 2 * self.ncls * s)
            todo.extend(t for t in set(rows[s]) if t not in rows)
        self.nstates = max(rows) + 1
        assert len(rows) == self.nstates, "a state number no walk reaches"
        self.rows = [rows[s] for s in range(self.nstates)]
        self.masks = []
        for s in range(self.nstates):
            words = struct.unpack_from(f"<{nchunks}Q", img, mask_off + 8 * nchunks * s)
            self.masks.append(sum(w << (64 * c) for c, w in enumerate(words)))

    def walk(self, data):
        s = self.start
        for b in data:
            s = self.rows[s][self.cls[b]]
        return s

    def loops(self, s):
        """State s leads back to itself on every header-token byte."""
        return all(self.rows[s][self.cls[b]] == s for b in TOKEN_BYTES)


def http_image_rule_ids(img):
    """The global ids of an image's rules, in evaluation order."""
    (rule_off,) = struct.unpack_from("<I", img, H_RULE_OFF)
    ids = list(struct.unpack_from(f"<{64 * img[H_NCHUNKS]}i", img, rule_off))
    while ids and ids[-1] == -1:
        ids.pop()
    return ids


def http_image_tables(img):
    """{"ids": global rule ids in evaluation order, "slots": {header name: [Dfa]},
    "nfa": [(header name, rejected mask, accepted mask)], "total_states"}."""
    nchunks, nhdr, ndfa = img[H_NCHUNKS], img[H_NHDR], img[H_NDFA]
    ids = http_image_rule_ids(img)
    (hdr_off,) = struct.unpack_from("<I", img, H_HDR_OFF)
    names = list(SLOT_NAMES)
    for k in range(nhdr):
        _, ln, _, name_off = struct.unpack_from("<IHHI", img, hdr_off + 12 * k)
        names.append(img[name_off:name_off + ln].decode())
    (dfa_off,) = struct.unpack_from("<I", img, H_DFA_OFF)
    slot_dfa = img[H_SLOT_DFA:H_SLOT_DFA + NUM_SLOTS + 1]
    slots = {}
    for s, name in enumerate(names):
        slots[name] = [Dfa(img, dfa_off + DEV_DFA * d, nchunks) for d in range(slot_dfa[s], slot_dfa[s + 1])]
    (nfa_off,) = struct.unpack_from("<I", img, H_NFA_OFF)
    nfa = []
    for k in range(img[H_NNFA]):
        _, mask_off, slot = struct.unpack_from("<QIB", img, nfa_off + 16 * k)
        words = struct.unpack_from(f"<{2 * nchunks}Q", img, mask_off)
        rows = [sum(w << (64 * c) for c, w in enumerate(words[a * nchunks:(a + 1) * nchunks])) for a in range(2)]
        nfa.append((names[slot], rows[0], rows[1]))
    (total,) = struct.unpack_from("<I", img, H_TOTAL_STATES)
    assert sum(len(v) for v in slots.values()) == ndfa
    return {"ids": ids, "slots": slots, "nfa": nfa, "total_states": total, "nchunks": nchunks}


# ---- the other compilers' images in an export (capi.cc l7g_tables_export: the HTTP, Kafka, memcached,
# r2d2 and cassandra compilers' Save(), engine/*_compile.h)
def _vec(export, at, size):
    (n,) = struct.unpack_from("<Q", export, at)
    return at + 8 + n * size, export[at + 8:at + 8 + n * size]


def _skip_cache(export, at):
    (n,) = struct.unpack_from("<Q", export, at)
    at += 8
    for _ in range(n):
        at, _ = _vec(export, at, 4)
        at += 16
    return at


def _skip_strmap(export, at):
    (n,) = struct.unpack_from("<Q", export, at)
    at += 8
    for _ in range(n):
        at, _ = _vec(export, at, 1)
        at += 8
    return at


def _images(export, at, tail_words, lower=False):
    at, rs = _vec(export, at, 8)
    at, images = _vec(export, at, 1)
    at, _ = _vec(export, at, 1)            # NFA pool
    at = _skip_strmap(export, _skip_cache(export, at))
    if lower:                              # cassandra: the unicode.ToLower pairs
        at, _ = _vec(export, at, 4)
    imgs = [images[off:off + ln] for off, ln in struct.iter_unpack("<II", rs)]
    return at + 8 * tail_words, imgs


def export_images(export):
    """{"http" | "memcache" | "r2d2" | "cassandra": that compiler's rule-set images}."""
    (srclen,) = struct.unpack_from("<Q", export, 32)
    at, out = 40 + srclen, {}
    at, out["http"] = _images(export, at, 4)
    for size in (36, 24, 4, 32, 32, 1):    # Kafka: rule sets, rules, index, topic and client slots, strings
        at, _ = _vec(export, at, size)
    at = _skip_cache(export, _skip_strmap(export, _skip_strmap(export, at + 24)))
    at, out["memcache"] = _images(export, at, 5)
    at, out["r2d2"] = _images(export, at, 3)
    at, out["cassandra"] = _images(export, at, 3, lower=True)
    assert at == len(export), (at, len(export))
    return out


def generic_image_tables(img, proto):
    """A memcached / r2d2 / cassandra image (McImgHeader, R2ImgHeader, CassImgHeader): {"ids", "dfas":
    [Dfa] (a rule's bit in the end state's mask row: its regex accepts), "nfa": mask of the rules each
    NFA evaluates, "nchunks"}."""
    nchunks, ndfa = img[0], img[2]
    if proto == "memcache":
        rule_off, dfa_off, _, nfa_off, nnfa = struct.unpack_from("<IIIII", img, 20)
    else:
        nnfa = img[3]
        rule_off, dfa_off, nfa_off = struct.unpack_from("<III", img, 12)
    ids = list(struct.unpack_from(f"<{64 * nchunks}i", img, rule_off))
    while ids and ids[-1] == -1:
        ids.pop()
    nfa = []
    for k in range(nnfa):
        _, mask_off = struct.unpack_from("<QI", img, nfa_off + 16 * k)
        nfa.append(sum(w << (64 * c) for c, w in enumerate(struct.unpack_from(f"<{nchunks}Q", img, mask_off))))
    return {"ids": ids, "dfas": [Dfa(img, dfa_off + DEV_DFA * d, nchunks) for d in range(ndfa)], "nfa": nfa,
            "nchunks": nchunks}

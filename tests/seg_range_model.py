"""Range decode of the segmented container (hc_seg_decompress_range*, include/hcodec.h) restated
in Python: which segments a byte range covers, and the statuses, by the documented precedence,
of decoding those alone with the oracle. Also the cases and the ranges the range tests share.
Test infrastructure only."""
import struct
import zlib

import oracle
import seg_check_cases as cases_mod
import seg_check_model as scm
import seg_model
from seg_model import NO_SEGMENT, SEG_HEADER, SEG_SIZE, CAPACITY

ARG, DEVICE, SEG_CHECK = 71, 70, 72
BIG = 16 * 2049 + 5  # 2050 segments at seg_bytes 16: more than one 1024-entry tile of the index scan


def header(container):
    """the fields of a container whose 48 header bytes pass every header rule (hc_seg_info's) for
    its length, or None; the index entries are not looked at"""
    c = bytes(container)
    if len(c) < 48 or c[:8] != seg_model.MAGIC or c[9] > 1 or any(c[10:16]) or c[8] & 0x3F:
        return None
    flags, check = c[8], c[9]
    raw_len, seg_bytes, width, n = struct.unpack_from("<4Q", c, 16)
    adapt = bool(flags & seg_model.FLAG_ADAPT)
    if not adapt and width != 0:
        return None
    if 48 + (12 if check else 8) * n > len(c) or raw_len > 520 * len(c):
        return None
    segs = seg_model.cuts(raw_len, adapt, width, seg_bytes)
    if segs is None or len(segs) != n:
        return None
    return dict(flags=flags, raw_len=raw_len, seg_bytes=seg_bytes, width=width, n_segments=n, cuts=segs, check=check)


def covered(fields, offset, length):
    """(first, count) of the segments that hold raw bytes [offset, offset + length)"""
    if length == 0:
        return 0, 0
    n = fields["n_segments"]
    if n == 1:
        return 0, 1
    full = fields["cuts"][0][1]  # every cut but the last has this length
    k0 = min(offset // full, n - 1)
    k1 = min((offset + length - 1) // full, n - 1)
    return k0, k1 - k0 + 1


def decode_range(container, offset, length, out_cap=None, device=True):
    """(status, bad_segment, bytes, out_len) of a ranged read; out_len and bad_segment are None
    where the call does not set them. device=False: the host call on a host without a device."""
    f = header(container)
    if f is None:
        return SEG_HEADER, NO_SEGMENT, b"", 0
    if offset > f["raw_len"] or length > f["raw_len"] - offset:
        return ARG, None, b"", None
    p = scm.parse(container)
    if p is None:
        return SEG_HEADER, NO_SEGMENT, b"", 0
    if not device:
        return DEVICE, NO_SEGMENT, b"", 0
    if out_cap is not None and out_cap < length:
        return CAPACITY, NO_SEGMENT, b"", length
    f, place, crcs = p
    k0, count = covered(f, offset, length)
    out = bytearray()
    for k in range(k0, k0 + count):
        o, m = place[k]
        b, want = f["cuts"][k]
        st, dec = oracle.decompress(container[o:o + m])
        if st:
            return st, k, b"", 0
        if len(dec) != want:
            return SEG_SIZE, k, b"", 0
        if crcs is not None and zlib.crc32(dec) != crcs[k]:
            return SEG_CHECK, k, b"", 0
        out += dec[max(offset, b) - b:min(offset + length, b + want) - b]
    assert len(out) == length
    return 0, NO_SEGMENT, bytes(out), length


def span(container, offset, length):
    """the encoded bytes [s0, s1) of the covered segments of a valid container"""
    f, place, _ = scm.parse(container)
    k0, count = covered(f, offset, length)
    if count == 0:
        return place[0][0], place[0][0]
    return place[k0][0], place[k0 + count - 1][0] + place[k0 + count - 1][1]


def ranges(cuts, raw_len):
    """the (offset, length) ranges every case is read at; those that do not fit it are dropped"""
    F = cuts[0][1]
    n = len(cuts)
    out = [(0, 0), (raw_len, 0), (0, raw_len), (0, 1), (raw_len - 1, 1)]
    if F < raw_len:  # more than one segment
        out += [
            (F, cuts[1][1]),         # one whole segment
            (F + 1, 3),              # an unaligned sliver inside one segment
            (F + 4, 2 * F),          # aligned, partial edges, three segments or more
            (F + 5, 2 * F + 7),      # unaligned over three segments or more
            (cuts[-1][0] - 1, raw_len - cuts[-1][0] + 1),  # from one byte before the last cut to the end
        ]
        if raw_len > n * F:  # the last band took leftover rows: wholly in those, offset / full >= n
            out.append((n * F, raw_len - n * F))
            out.append((n * F + 1, raw_len - n * F - 2))
    seen, kept = set(), []
    for o, m in out:
        if o < 0 or m < 0 or o > raw_len or m > raw_len - o or (o, m) in seen:
            continue
        seen.add((o, m))
        kept.append((o, m))
    return kept


# (raw input, use_adapt, width, seg_bytes, use_diff, checked): the small shapes of the container tests
CASES = [(f"rng:256:{n}", False, 512, 16, d, False) for n in (0, 1, 17, BIG) for d in (False, True)]
CASES += [(f"rng:4:{w * h}", True, w, seg, d, False) for w, h, seg in ((16, 19, 128), (16, 15, 128), (9, 32, 80))
          for d in (False, True)]
PHOTO = [("photo:64:200", False, 512, 4096), ("photo:64:200", True, 64, 4096)]
CASES += [p + (d, k) for p in PHOTO for d in (False, True) for k in (False, True)]
# ranges of the 2050-segment case alone: across the edge of the first index tile, and the last 5 bytes
BIG_RANGES = [(16 * 1020, 16 * 11), (BIG - 5, 5)]

_built = {}


def case_id(c):
    return f"{c[0]}-{'a' if c[1] else 'c'}{'m' if c[4] else ''}-w{c[2]}-s{c[3]}{'-k' if c[5] else ''}"


def built(case):
    """(raw, the model's container, its fields, the case's ranges), built once"""
    if case not in _built:
        name, adapt, w, seg, diff, check = case
        raw = cases_mod.raw(name)
        c = scm.build(raw, diff, adapt, w, seg, check=check)
        f = scm.parse(c)[0]
        rs = ranges(f["cuts"], len(raw))
        if name == f"rng:256:{BIG}":
            rs = rs + BIG_RANGES
        _built[case] = (raw, c, f, rs)
    return _built[case]


def index_mutants(c):
    """{name: container} of the container-level errors that the index decides (the header is
    intact): forged enc_len entries, a truncated container, trailing bytes"""
    c = bytes(c)
    f, place, _ = scm.parse(c)
    n = f["n_segments"]

    def index(k, v):
        return c[:48 + 8 * k] + struct.pack("<Q", v % 2**64) + c[56 + 8 * k:]

    return {
        "enc_len_wraps": index(1, 2**64 - 8),
        "enc_len_wraps_first": index(0, 2**64 - 8),
        "enc_len_past_end": index(n - 1, len(c)),
        "enc_len_longer": index(0, place[0][1] + 16),
        "enc_len_shorter": index(n - 1, place[n - 1][1] - 1),
        "trailing_byte": c + b"\x00",
        "last_byte_cut": c[:-1],
        "payload_cut": c[:place[1][0] + 3],
    }


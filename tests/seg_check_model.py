"""The checked segmented container (HCSEG1 with header byte 9 = 1, include/hcodec.h) restated in
Python: seg_model's cuts, streams and precedence, plus a zlib.crc32 of every segment's raw bytes
behind the index. check=False is seg_model itself. Test infrastructure only.
"""
import struct
import zlib

import oracle
import seg_model
from seg_model import MAGIC, NO_SEGMENT, SEG_HEADER, SEG_SIZE, CAPACITY, align16, cuts

SEG_CHECK = 72
CHECK_CRC32 = 0x100  # HC_SEG_CHECK_CRC32: the encoders' flag, and SegInfo.flags of a checked container


def build(raw, use_diff=False, use_adapt=False, width=512, seg_bytes=seg_model.DEFAULT_BYTES, check=True):
    """the container the encoder must write, byte for byte"""
    plain = seg_model.build(raw, use_diff, use_adapt, width, seg_bytes)
    if not check:
        return plain
    raw = bytes(raw)
    f, _ = seg_model.parse(plain)
    n = f["n_segments"]
    out = bytearray(plain[:9] + b"\x01" + plain[10:48 + 8 * n])
    out += b"".join(struct.pack("<I", zlib.crc32(raw[o:o + m])) for o, m in f["cuts"])
    for s in seg_model.segments(plain):
        out += bytes(align16(len(out)) - len(out))
        out += s
    return bytes(out)


def parse(container):
    """(fields, [(offset, enc_len)], crcs or None) of a container of either kind, or None when a
    container-level rule fails"""
    c = bytes(container)
    if len(c) < 10 or c[9] == 0:
        p = seg_model.parse(c)
        return None if p is None else (dict(p[0], check=0), p[1], None)
    if len(c) < 48 or c[:8] != MAGIC or c[9] != 1 or any(c[10:16]) or c[8] & 0x3F:
        return None
    flags = c[8]
    raw_len, seg_bytes, width, n = struct.unpack_from("<4Q", c, 16)
    adapt = bool(flags & seg_model.FLAG_ADAPT)
    if not adapt and width != 0:
        return None
    if 48 + 12 * n > len(c) or raw_len > 520 * len(c):
        return None
    segs = cuts(raw_len, adapt, width, seg_bytes)
    if segs is None or len(segs) != n:
        return None
    lens = struct.unpack_from(f"<{n}Q", c, 48)
    crcs = struct.unpack_from(f"<{n}I", c, 48 + 8 * n)
    off, place = align16(48 + 12 * n), []
    for m in lens:
        if off > len(c) or m > len(c) - off:
            return None
        place.append((off, m))
        end = off + m
        off = align16(end)
    if end != len(c):
        return None
    return dict(flags=flags, raw_len=raw_len, seg_bytes=seg_bytes, width=width, n_segments=n, cuts=segs,
                check=1), place, list(crcs)


def segments(container):
    """the segments' streams of a valid container"""
    _, place, _ = parse(container)
    return [bytes(container[o:o + m]) for o, m in place]


def repack(container, streams):
    """the container with its segments' streams replaced (same header fields, same crc words)"""
    c = bytes(container)
    f, _, crcs = parse(c)
    out = bytearray(c[:48]) + b"".join(struct.pack("<Q", len(s)) for s in streams)
    if crcs is not None:
        out += b"".join(struct.pack("<I", v) for v in crcs)
    for s in streams:
        out += bytes(align16(len(out)) - len(out)) + s
    return bytes(out)


def decode(container, out_cap=None):
    """(status, bad_segment, bytes): the lowest failing segment decides, whether its coder failed,
    its length is wrong or, in a checked container, its checksum differs"""
    p = parse(container)
    if p is None:
        return SEG_HEADER, NO_SEGMENT, b""
    f, place, crcs = p
    if out_cap is not None and f["raw_len"] > out_cap:
        return CAPACITY, NO_SEGMENT, b""
    out = bytearray()
    for k, ((o, m), (_, want)) in enumerate(zip(place, f["cuts"])):
        st, dec = oracle.decompress(container[o:o + m])
        if st:
            return st, k, b""
        if len(dec) != want:
            return SEG_SIZE, k, b""
        if crcs is not None and zlib.crc32(dec) != crcs[k]:
            return SEG_CHECK, k, b""
        out += dec
    return 0, NO_SEGMENT, bytes(out)

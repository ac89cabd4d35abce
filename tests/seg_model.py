"""The segmented container (HCSEG1, include/hcodec.h) restated in Python on top of the oracle.

Every segment is a complete reference stream, so the model needs no coder of its own: build()
puts oracle.compress outputs behind a header and an index, decode() hands each segment to
oracle.decompress and applies the container's status precedence. Test infrastructure only.
"""
import struct

import oracle

MAGIC = bytes([0x48, 0x43, 0x53, 0x45, 0x47, 0x31, 0x00, 0xFF])
FLAG_DIFF, FLAG_ADAPT = 0x80, 0x40
DEFAULT_BYTES = 65536
SEG_HEADER, SEG_SIZE, CAPACITY = 68, 69, 64
NO_SEGMENT = 2**64 - 1


def align16(x):
    return (x + 15) & ~15


def cuts(raw_len, use_adapt, width, seg_bytes):
    """[(offset, length)] of the segments, or None for arguments the format does not allow"""
    if seg_bytes == 0 or seg_bytes % 16:
        return None
    if not use_adapt:
        n = max(1, -(-raw_len // seg_bytes))
        return [(k * seg_bytes, min((k + 1) * seg_bytes, raw_len) - k * seg_bytes) for k in range(n)]
    if width < 8 or raw_len % width or raw_len // width < 8:
        return None
    height = raw_len // width
    rows = max(8, (seg_bytes // width) // 4 * 4)
    out, row = [], 0
    while row < height:
        take = rows
        if height - (row + take) < 8:  # too few rows would remain for a matrix (or none)
            take = height - row
        out.append((row * width, take * width))
        row += take
    return out


def build(raw, use_diff=False, use_adapt=False, width=512, seg_bytes=DEFAULT_BYTES):
    """the container the encoder must write, byte for byte"""
    raw = bytes(raw)
    segs = cuts(len(raw), use_adapt, width, seg_bytes)
    assert segs is not None
    streams = []
    for off, n in segs:
        st, enc = oracle.compress(raw[off:off + n], use_diff, use_adapt, width)
        assert st == 0, st
        streams.append(enc)
    flags = (FLAG_DIFF if use_diff else 0) | (FLAG_ADAPT if use_adapt else 0)
    out = bytearray(MAGIC + bytes([flags]) + bytes(7))
    out += struct.pack("<4Q", len(raw), seg_bytes, width if use_adapt else 0, len(segs))
    out += b"".join(struct.pack("<Q", len(s)) for s in streams)
    for s in streams:
        out += bytes(align16(len(out)) - len(out))
        out += s
    return bytes(out)


def parse(container):
    """(fields, [(offset, enc_len)]) of a container, or None when a container-level rule fails"""
    c = bytes(container)
    if len(c) < 48 or c[:8] != MAGIC or any(c[9:16]) or c[8] & 0x3F:
        return None
    flags = c[8]
    raw_len, seg_bytes, width, n = struct.unpack_from("<4Q", c, 16)
    adapt = bool(flags & FLAG_ADAPT)
    if not adapt and width != 0:
        return None
    # (the cheap rules first: a forged raw_len would otherwise make cuts() list 2^40 segments)
    if 48 + 8 * n > len(c) or raw_len > 520 * len(c):
        return None
    segs = cuts(raw_len, adapt, width, seg_bytes)
    if segs is None or len(segs) != n:
        return None
    lens = struct.unpack_from(f"<{n}Q", c, 48)
    off, place = align16(48 + 8 * n), []
    for k, m in enumerate(lens):
        if off > len(c) or m > len(c) - off:
            return None
        place.append((off, m))
        end = off + m
        off = align16(end)
    if end != len(c):
        return None
    return dict(flags=flags, raw_len=raw_len, seg_bytes=seg_bytes, width=width, n_segments=n, cuts=segs), place


def segments(container):
    """the segments' streams of a valid container"""
    _, place = parse(container)
    return [bytes(container[o:o + m]) for o, m in place]


def decode(container, out_cap=None):
    """(status, bad_segment, bytes) by the decoder's precedence rules"""
    p = parse(container)
    if p is None:
        return SEG_HEADER, NO_SEGMENT, b""
    f, place = p
    if out_cap is not None and f["raw_len"] > out_cap:
        return CAPACITY, NO_SEGMENT, b""
    out = bytearray()
    for k, ((o, m), (_, want)) in enumerate(zip(place, f["cuts"])):
        st, dec = oracle.decompress(container[o:o + m])
        if st:
            return st, k, b""
        if len(dec) != want:
            return SEG_SIZE, k, b""
        out += dec
    return 0, NO_SEGMENT, bytes(out)


def header_mutants(c):
    """{name: container} of every container-level error that the 48 header bytes decide"""
    c = bytes(c)
    f, _ = parse(c)
    adapt = bool(f["flags"] & 0x40)

    def field(k, v):
        return c[:16 + 8 * k] + struct.pack("<Q", v % 2**64) + c[24 + 8 * k:]

    m = {
        "short": c[:47],
        "magic": bytes([c[0] ^ 1]) + c[1:],
        "magic_end": c[:7] + b"\xfe" + c[8:],
        "reserved": c[:12] + b"\x01" + c[13:],
        "low_flag": c[:8] + bytes([c[8] | 0x01]) + c[9:],
        "seg_bytes_0": field(1, 0),
        "seg_bytes_odd": field(1, f["seg_bytes"] + 8),
        "n_more": field(3, f["n_segments"] + 1),
        "n_less": field(3, f["n_segments"] - 1),
        "n_huge": field(3, 2**61),           # 48 + 8 n wraps to 48
        "index_cut": c[:48 + 8 * f["n_segments"] - 1],
        "raw_huge": field(0, f["raw_len"] + f["seg_bytes"] * 2**40),
    }
    if adapt:
        m["width_0"] = field(2, 0)
        m["width_odd"] = field(2, f["width"] + 1) if f["raw_len"] % (f["width"] + 1) else field(2, f["width"] + 3)
        m["width_small"] = field(2, 4)
        m["height_small"] = field(2, f["raw_len"] // 4)
    else:
        m["width_set"] = field(2, 8)
    return m

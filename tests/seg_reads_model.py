"""List read of the segmented container (hc_seg_decompress_ranges*, include/hcodec.h) restated in
Python on seg_range_model and seg_check_model: the list rules, need, the covered union, the
oracle's decode of every covered segment once, the statuses by the documented precedence, and the
destination bytes. Also the host plan's records, the work bound's formula, the rectangle helper and
the read lists the tests share. Test infrastructure only."""
import zlib

import oracle
import seg_check_model as scm
import seg_range_model as srm
from seg_model import NO_SEGMENT, SEG_HEADER, SEG_SIZE, CAPACITY, FLAG_ADAPT, align16

ARG, DEVICE, SEG_CHECK = srm.ARG, srm.DEVICE, srm.SEG_CHECK
FILL = 0xA5  # what a destination buffer holds where no read writes


def reads_ok(raw_len, reads):
    """the read list's rules over (offset, length, dst_off) triples"""
    prev = 0
    for o, m, d in reads:
        if o < 0 or m < 0 or d < 0 or o > raw_len or m > raw_len - o or o < prev:
            return False
        prev = o
        if o >= 2**64 or m >= 2**64 or d >= 2**64 or d + m >= 2**64:
            return False
    return True


def need(reads):
    """the highest dst_off + length over the reads of length > 0"""
    return max([d + m for o, m, d in reads if m], default=0)


def covered(fields, reads):
    """the container indices of the segments a valid list covers, ascending, each once"""
    ks = set()
    for o, m, _ in reads:
        k0, count = srm.covered(fields, o, m)
        ks.update(range(k0, k0 + count))
    return sorted(ks)


def records(fields, reads):
    """per read of a valid list, what the host plan hands the device: (k0, cnt, e0, src, length,
    dst_off): the segments it covers, the rank of the first of them among the covered segments, and
    where its bytes start in the staging region (covered entry c at c full). An empty read covers
    nothing and carries the k0 and e0 of the read before it (0, 0 when it is the first)."""
    cuts = fields["cuts"]
    full = cuts[0][1]
    rank = {k: i for i, k in enumerate(covered(fields, reads))}
    out, k0, e0 = [], 0, 0
    for o, m, d in reads:
        a, count = srm.covered(fields, o, m)
        if count:
            k0, e0 = a, rank[a]
            # its segments are consecutive entries, so its bytes are one run of the staging region
            assert [rank[k] for k in range(a, a + count)] == list(range(e0, e0 + count))
            out.append((k0, count, e0, e0 * full + (o - cuts[a][0]), m, d))
        else:
            out.append((k0, 0, e0, 0, m, d))
    return out


def work_bound(fields, in_len, reads, adapt_decompress_work_bound):
    """the header's formula of hc_seg_decompress_ranges_work_bound;
    adapt_decompress_work_bound(in_len, raw, count) is hc_adapt_decompress_work_bound"""
    P = len(reads)
    ks = covered(fields, reads)
    C, W = len(ks), sum(fields["cuts"][k][1] for k in ks)
    t = align16(48 * P) + 3 * align16(8 * P) + 6 * align16(8 * C) + align16(4 * C) + 16 + align16(W)
    if fields["check"]:
        t += align16(4 * C)
    if fields["flags"] & FLAG_ADAPT and C:
        t += align16(adapt_decompress_work_bound(in_len, W, C))
    return t


def rect_reads(raw_len, pitch, x, y, w, h):
    """hc_seg_rect_reads: the (offset, length, dst_off) reads of a rectangle's rows, or None"""
    if pitch == 0 or x + w > pitch:
        return None
    end = (y + h - 1) * pitch + x + w  # the last row's
    if h and (max(end, h * w) >= 2**64 or (w and end > raw_len)):
        return None
    return [((y + r) * pitch + x, w, r * w) for r in range(h)]


def decode_reads(container, reads, out_cap=None, device=True):
    """(status, bad_segment, out[:need] over FILL bytes, out_len) of a list read; out_len and
    bad_segment are None where the call does not set them. Every covered segment is decoded once.
    device=False: the host call on a host without a device."""
    c = bytes(container)
    f = srm.header(c)
    if f is None:
        return SEG_HEADER, NO_SEGMENT, b"", 0
    if not reads_ok(f["raw_len"], reads):
        return ARG, None, b"", None
    p = scm.parse(c)
    if p is None:
        return SEG_HEADER, NO_SEGMENT, b"", 0
    if not device:
        return DEVICE, NO_SEGMENT, b"", 0
    top = need(reads)
    if out_cap is not None and out_cap < top:
        return CAPACITY, NO_SEGMENT, b"", top
    f, place, crcs = p
    raws = {}
    for k in covered(f, reads):
        o, m = place[k]
        st, dec = oracle.decompress(c[o:o + m])
        if st:
            return st, k, b"", 0
        if len(dec) != f["cuts"][k][1]:
            return SEG_SIZE, k, b"", 0
        if crcs is not None and zlib.crc32(dec) != crcs[k]:
            return SEG_CHECK, k, b"", 0
        raws[k] = dec
    out = bytearray([FILL]) * top
    for o, m, d in reads:
        k0, count = srm.covered(f, o, m)
        got = b"".join(raws[k] for k in range(k0, k0 + count))
        at = o - f["cuts"][k0][0] if count else 0
        out[d:d + m] = got[at:at + m]
    return 0, NO_SEGMENT, bytes(out), top


def read_sets(case):
    """{name: [(offset, length, dst_off)]} of the read lists a case is read at: every range of the
    range tests as the one-read list, and the lists that only a list can be"""
    raw, c, f, rs = srm.built(case)
    cuts, n, L = f["cuts"], f["n_segments"], len(raw)
    F = cuts[0][1]
    sets = {f"range_{o}_{m}": [(o, m, 0)] for o, m in rs}
    sets["none"] = []
    sets["empties"] = [(0, 0, 5), (L, 0, 0), (L, 0, 2**64 - 1)]
    if F >= 8 and L >= F:
        # inside one segment, destinations in reverse order with a gap; then overlapping sources
        sets["two_in_one"] = [(1, 2, 9), (F - 3, 3, 1)]
        sets["overlap"] = [(1, 5, 20), (1, 5, 3), (3, F - 4, 30)]
    if n >= 2 and L >= cuts[1][0] + 2:
        b1 = cuts[1][0]
        sets["across_cut_twice"] = [(b1 - 2, 4, 7), (b1 - 1, 2, 1)]
    if n >= 3:
        # rank differs from segment index: segments 0 and n - 1, destinations in reverse order
        sets["first_and_last"] = [(1, 3, cuts[-1][1] + 4), (cuts[-1][0], cuts[-1][1], 1)]
        sets["long_then_short"] = [(0, 0, 0), (1, L - 1, 17), (F + 1, 2, 3), (L - 1, 1, 0)]
    if n >= 4 and L >= 3 * F + 3:
        sets["skip_one"] = [(F - 1, 1, 2), (F, 0, 0), (2 * F + 1, F + 2, 5)]  # segments 0, 2, 3
    if n >= 2 and cuts[-1][1] < F:
        sets["ends_in_short_last"] = [(cuts[-1][0] - 1, cuts[-1][1] + 1, 3)]
    if L > n * F:  # the last band took leftover rows
        sets["leftover_rows"] = [(0, 3, 100), (n * F + 1, L - n * F - 2, 0)]
        sets["spans_bands"] = [(F - 5, 9, 40), (n * F - 1, 3, 1)]
    return sets

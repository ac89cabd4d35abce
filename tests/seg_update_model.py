"""Range write of the segmented container (hc_seg_update*, include/hcodec.h) restated in Python on
seg_check_model: the patch rules, the covered and the decoded segments, the oracle's decode of the
decoded segments alone, the overlay, the oracle's streams of the covered cuts, the splice, and the
statuses by the documented precedence. Also the patch sets the update tests share. Test
infrastructure only."""
import struct
import zlib

import numpy as np

import oracle
import seg_check_model as scm
import seg_range_model as srm
from seg_model import NO_SEGMENT, SEG_HEADER, SEG_SIZE, CAPACITY, FLAG_ADAPT, FLAG_DIFF, align16

ARG, DEVICE, SEG_CHECK = srm.ARG, srm.DEVICE, srm.SEG_CHECK


def patches_ok(raw_len, patches, data_len=None):
    """the patch list's rules over (offset, length, src_off) triples"""
    prev_end = 0
    for o, m, s in patches:
        if o < 0 or m < 0 or o > raw_len or m > raw_len - o or o < prev_end:
            return False
        prev_end = o + m
        if data_len is not None and (s > data_len or m > data_len - s):
            return False
    return True


def plan(fields, patches):
    """(covered, decoded): the container indices of the segments a valid patch list covers, and of
    those among them that are decoded first: every one whose cut does not lie inside ONE patch"""
    cuts = fields["cuts"]
    covered, whole = [], set()
    for o, m, _ in patches:
        k0, count = srm.covered(fields, o, m)
        for k in range(k0, k0 + count):
            if not covered or covered[-1] < k:
                covered.append(k)
            b, n = cuts[k]
            if o <= b and o + m >= b + n:
                whole.add(k)
    return covered, [k for k in covered if k not in whole]


def records(fields, patches):
    """per patch of a valid list, what the host plan hands the device: (cnt, k0 or None, e0, d0,
    dmask, dst): the segments it newly covers (a shared one belongs to the first patch) from entry
    e0 of the covered array, which of their two ends go to the decoder from entry d0 of the decoded
    array, and where its bytes go in the staging region (covered entry c at c full)"""
    cuts = fields["cuts"]
    full = cuts[0][1]
    covered, decoded = plan(fields, patches)
    entry = {k: i for i, k in enumerate(covered)}
    seen, n_dec, out = set(), 0, []
    for o, m, _ in patches:
        a, count = srm.covered(fields, o, m)
        new = [k for k in range(a, a + count) if k not in seen]
        dmask = 0
        if new and new[0] in decoded:
            dmask |= 1
        if len(new) > 1 and new[-1] in decoded:
            dmask |= 2
        dst = entry[a] * full + (o - cuts[a][0]) if count else 0
        out.append((len(new), new[0] if new else None, len(seen), n_dec, dmask, dst))
        seen.update(new)
        n_dec += (dmask & 1) + (dmask >> 1)
    return out


def triples(patches):
    """[(offset, bytes)] -> ([(offset, length, src_off)], patch_data), the sources back to back"""
    out, data = [], bytearray()
    for o, b in patches:
        out.append((o, len(b), len(data)))
        data += b
    return out, bytes(data)


def patched(raw, patches):
    """the raw bytes with [(offset, bytes)] laid over them"""
    raw = bytearray(raw)
    for o, b in patches:
        raw[o:o + len(b)] = b
    return bytes(raw)


def update_bound(fields, in_len, patches, compress_bound):
    """hc_seg_update_bound: compress_bound(n, adapt) is hc_compress_bound"""
    adapt = bool(fields["flags"] & FLAG_ADAPT)
    covered, _ = plan(fields, patches)
    return in_len + sum(align16(compress_bound(fields["cuts"][k][1], adapt)) for k in covered)


def update(container, patches, out_cap=None, device=True, data_len=None):
    """(status, bad_segment, bytes, out_len) of a range write with [(offset, bytes)] patches;
    out_len and bad_segment are None where the call does not set them"""
    c = bytes(container)
    f = srm.header(c)
    if f is None:
        return SEG_HEADER, NO_SEGMENT, b"", 0
    tri, data = triples(patches)
    if not patches_ok(f["raw_len"], tri, len(data) if data_len is None else data_len):
        return ARG, None, b"", None
    p = scm.parse(c)
    if p is None:
        return SEG_HEADER, NO_SEGMENT, b"", 0
    if not device:
        return DEVICE, NO_SEGMENT, b"", 0
    f, place, crcs = p
    covered, decoded = plan(f, tri)
    adapt, diff = bool(f["flags"] & FLAG_ADAPT), bool(f["flags"] & FLAG_DIFF)
    raws = {}
    for k in decoded:
        o, m = place[k]
        st, dec = oracle.decompress(c[o:o + m])
        if st:
            return st, k, b"", 0
        if len(dec) != f["cuts"][k][1]:
            return SEG_SIZE, k, b"", 0
        if crcs is not None and zlib.crc32(dec) != crcs[k]:
            return SEG_CHECK, k, b"", 0
        raws[k] = bytearray(dec)
    for k in covered:
        raws.setdefault(k, bytearray(f["cuts"][k][1]))
    for o, b in patches:  # the overlay, cut by cut
        for k in covered:
            s, n = f["cuts"][k]
            lo, hi = max(o, s), min(o + len(b), s + n)
            if lo < hi:
                raws[k][lo - s:hi - s] = b[lo - o:hi - o]
    streams = [c[o:o + m] for o, m in place]
    for k in covered:
        st, enc = oracle.compress(bytes(raws[k]), diff, adapt, f["width"] if adapt else 512)
        assert st == 0, st
        streams[k] = enc
        if crcs is not None:
            crcs[k] = zlib.crc32(bytes(raws[k]))
    n = f["n_segments"]
    out = bytearray(c[:48]) + b"".join(struct.pack("<Q", len(s)) for s in streams)
    if crcs is not None:
        out += b"".join(struct.pack("<I", v) for v in crcs)
    for k, s in enumerate(streams):
        at = align16(len(out))
        if k - 1 in raws:
            out += bytes(at - len(out))  # zero padding after a recoded segment
        else:  # the old padding goes along with the index or the uncovered segment it follows
            old_end = place[k - 1][0] + place[k - 1][1] if k else 48 + (12 if crcs is not None else 8) * n
            out += c[old_end:place[k][0]]
        assert len(out) == at
        out += s
    assert len(streams) == n
    if out_cap is not None and len(out) > out_cap:
        return CAPACITY, NO_SEGMENT, b"", len(out)
    return 0, NO_SEGMENT, bytes(out), len(out)


def fill(spans, kind, seed=7):
    """[(offset, length)] -> [(offset, bytes)]: zero bytes (the streams shrink) or pseudo-random
    ones (they grow)"""
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return [(o, bytes(m)) for o, m in spans]
    return [(o, rng.integers(0, 256, m, dtype=np.uint8).tobytes()) for o, m in spans]


KINDS = ("zero", "random")


def patch_sets(case):
    """{name: [(offset, length)]} of the patch lists a case is written at"""
    raw, c, f, rs = srm.built(case)
    cuts, n, L = f["cuts"], f["n_segments"], len(raw)
    sets = {f"range_{o}_{m}": [(o, m)] for o, m in rs}
    sets["none"] = []
    F = cuts[0][1]
    if F >= 4 and L >= F:
        sets["two_in_one"] = [(1, 1), (F - 2, 2)]
        sets["adjacent_fill"] = [(0, F // 2), (F // 2, F - F // 2)]  # together the whole cut: decoded all the same
    if n >= 2:
        b1 = cuts[1][0]
        sets["meet_on_cut"] = [(b1 - 2, 2), (b1, min(3, cuts[1][1]))]
    if n >= 3:
        sets["first_and_last"] = [(0, cuts[0][1]), (cuts[-1][0], cuts[-1][1])]  # two runs: the middle block shifts
        sets["edges_partial"] = [(1, 2), (cuts[-1][0] + 1, 1), (L, 0)]
    if case[0] == f"rng:256:{srm.BIG}":
        sets["many_small"] = [(100 + 160 * i, 1) for i in range(200)]  # more than one descriptor launch
    return sets

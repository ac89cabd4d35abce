"""Append to the segmented container (hc_seg_append*, include/hcodec.h) restated in Python on
seg_check_model and seg_range_model: the first coded segment, the oracle's decode of the one
decoded segment, the oracle's streams of the coded cuts, the result's layout, and the statuses by
the documented precedence. Also the cases and the add lengths the append tests share. Test
infrastructure only."""
import struct
import zlib

import numpy as np

import oracle
import seg_check_model as scm
import seg_model
import seg_range_model as srm
from seg_model import NO_SEGMENT, SEG_HEADER, SEG_SIZE, CAPACITY, FLAG_ADAPT, FLAG_DIFF, align16

ARG, DEVICE, SEG_CHECK, MATRIX_SIZE = srm.ARG, srm.DEVICE, srm.SEG_CHECK, 6
MAX_CODED = 2**31 - 1


def plan(fields, add_len):
    """(status, K, new cuts, decoded): the first coded segment, the cuts of raw_len + add_len, and
    whether old segment n - 1 is decoded first (0 or 1); K and the rest None on a non-zero status"""
    raw_len, n, old = fields["raw_len"], fields["n_segments"], fields["cuts"]
    adapt = bool(fields["flags"] & FLAG_ADAPT)
    if raw_len + add_len >= 2**64:
        return ARG, None, None, None
    if adapt and add_len % fields["width"]:
        return MATRIX_SIZE, None, None, None
    new = seg_model.cuts(raw_len + add_len, adapt, fields["width"], fields["seg_bytes"])
    assert new is not None and len(new) >= n and new[:n - 1] == old[:n - 1]
    k = n if add_len == 0 or (len(new) > n - 1 and new[n - 1] == old[n - 1]) else n - 1
    if len(new) - k > MAX_CODED:
        return ARG, None, None, None
    return 0, k, new, int(k == n - 1 and old[n - 1][1] > 0)


def entry_bytes(fields):
    return 12 if fields["check"] else 8


def append_bound(fields, in_len, add_len, compress_bound):
    """hc_seg_append_bound: compress_bound(n, adapt) is hc_compress_bound"""
    st, k, new, _ = plan(fields, add_len)
    if st:
        return 0
    adapt = bool(fields["flags"] & FLAG_ADAPT)
    slots = sum(align16(compress_bound(m, adapt)) for _, m in new[k:])
    return in_len + align16(entry_bytes(fields) * (len(new) - fields["n_segments"])) + 16 + slots


def work_bound(fields, in_len, add_len, compress_bound, adapt_enc_bound, adapt_dec_bound):
    """hc_seg_append_work_bound by the formula of include/hcodec.h; the last two are the library's
    hc_adapt_compress_work_bound and hc_adapt_decompress_work_bound"""
    st, k, new, dec = plan(fields, add_len)
    if st:
        return 0
    adapt, check = bool(fields["flags"] & FLAG_ADAPT), bool(fields["check"])
    C = len(new) - k
    full, last = fields["cuts"][0][1], fields["cuts"][-1][1]
    stage = add_len + (fields["raw_len"] - k * full if k < fields["n_segments"] else 0)  # the open tail, then the added bytes
    total = 9 * align16(8 * C) + align16(4 * C) + 3 * align16(8 * (2 * C + 1)) + 160
    if check:
        total += align16(4 * C) + 16
    total += align16(stage) + sum(align16(compress_bound(m, adapt)) for _, m in new[k:])
    if adapt:
        e = adapt_enc_bound(stage, C) if C else 0
        d = adapt_dec_bound(min(in_len, compress_bound(last, True)), last, 1) if dec else 0
        total += align16(max(e, d))
    return total


def append(container, add, out_cap=None, device=True):
    """(status, bad_segment, bytes, out_len) of an append; out_len and bad_segment are None where
    the call does not set them. device=False: the host call on a host without a device."""
    c, add = bytes(container), bytes(add)
    f = srm.header(c)
    if f is None:
        return SEG_HEADER, NO_SEGMENT, b"", 0
    st, K, new, dec = plan(f, len(add))
    if st:
        return st, None, b"", None
    p = scm.parse(c)
    if p is None:
        return SEG_HEADER, NO_SEGMENT, b"", 0
    if not device:
        return DEVICE, NO_SEGMENT, b"", 0
    f, place, crcs = p
    n, n2 = f["n_segments"], len(new)
    adapt, diff = bool(f["flags"] & FLAG_ADAPT), bool(f["flags"] & FLAG_DIFF)
    tail = b""
    if dec:
        o, m = place[n - 1]
        st, got = oracle.decompress(c[o:o + m])
        if st:
            return st, n - 1, b"", 0
        if len(got) != f["cuts"][n - 1][1]:
            return SEG_SIZE, n - 1, b"", 0
        if crcs is not None and zlib.crc32(got) != crcs[n - 1]:
            return SEG_CHECK, n - 1, b"", 0
        tail = got
    staged = tail + add  # raw bytes [K full, raw_len + add_len)
    base = new[K][0] if K < n2 else 0
    streams, new_crcs = [], []
    for o, m in new[K:]:
        cut = staged[o - base:o - base + m]
        assert len(cut) == m
        st, enc = oracle.compress(cut, diff, adapt, f["width"] if adapt else 512)
        assert st == 0, st
        streams.append(enc)
        new_crcs.append(zlib.crc32(cut))
    out = bytearray(c[:16]) + struct.pack("<4Q", f["raw_len"] + len(add), f["seg_bytes"], f["width"], n2)
    out += c[48:48 + 8 * K] + b"".join(struct.pack("<Q", len(s)) for s in streams)
    if crcs is not None:
        out += c[48 + 8 * n:48 + 8 * n + 4 * K] + b"".join(struct.pack("<I", v) for v in new_crcs)
    out += bytes(align16(len(out)) - len(out))
    if K:  # the kept block: old padding between kept segments included
        out += c[place[0][0]:place[K - 1][0] + place[K - 1][1]]
    for s in streams:
        out += bytes(align16(len(out)) - len(out)) + s
    if out_cap is not None and len(out) > out_cap:
        return CAPACITY, NO_SEGMENT, b"", len(out)
    return 0, NO_SEGMENT, bytes(out), len(out)


def add_bytes(n, seed=11):
    """the n pseudo-random bytes every test appends"""
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


# the checked forms of the two small plain cases: 12-byte index entries, n -> n + 1 for odd and even n
EXTRA_CASES = [(f"rng:256:{n}", False, 512, 16, False, True) for n in (1, 17)]
CASES = srm.CASES + EXTRA_CASES


def add_lengths(case):
    """the add lengths a case is appended at (all valid for it)"""
    name, adapt, w, seg, diff, check = case
    raw_len = len(srm.built(case)[0])
    adds = [0]
    if name.startswith("rng:256:"):
        adds += {0: [1, 16, 17], 1: [15, 16], 17: [15, 16], srm.BIG: [5, 16 * 3]}[raw_len]
    elif name.startswith("rng:4:"):
        rows = {(16, 19): [1, 5, 13], (16, 15): [1], (9, 32): [3, 8]}[(w, raw_len // w)]
        adds += [r * w for r in rows]
    elif adapt:
        adds += [9 * w]
    else:
        adds += [seg + 100]
    return adds

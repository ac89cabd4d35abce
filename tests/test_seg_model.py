"""The segmented container without a device: the format model against the oracle, and the
library's host-only entry points (hc_seg_count, hc_seg_compress_bound, hc_seg_info, the
host-decided statuses) against the model."""
import ctypes
import struct

import numpy as np
import pytest

import seg_model

# (width, height, seg_bytes) -> band rows, checked with the oracle (bands decode back to their rows)
ADAPT_CUTS = [
    (16, 19, 128, [8, 11]),
    (16, 15, 128, [15]),
    (9, 32, 80, [8, 8, 8, 8]),
    (64, 200, 4096, [64, 64, 64, 8]),
]
# plain inputs (_plain) at seg_bytes 16: length -> (segment lengths, container length without -m)
PLAIN_CUTS = {0: ([0], 73), 1: ([1], 74), 15: ([15], 95), 16: ([16], 96), 17: ([16, 1], 106)}


def _plain(n):
    return np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8).tobytes()


def _matrix(w, h, seed=5):
    return np.random.default_rng(seed).integers(0, 4, w * h, dtype=np.uint8).tobytes()


def _cases(oracle_mod):
    """(raw, use_diff, use_adapt, width, seg_bytes) of every shape above, with and without -m"""
    out = []
    for diff in (False, True):
        for n in PLAIN_CUTS:
            out.append((_plain(n), diff, False, 512, 16))
        out.append((oracle_mod.synth("photo", 3, 64, 200).tobytes(), diff, False, 512, 4096))
        for w, h, seg, _ in ADAPT_CUTS:
            out.append((_matrix(w, h), diff, True, w, seg))
    return out


def test_cut_rule():
    for w, h, seg, rows in ADAPT_CUTS:
        c = seg_model.cuts(w * h, True, w, seg)
        assert [n // w for _, n in c] == rows and all(n % w == 0 for _, n in c)
        assert [o for o, _ in c] == [sum(rows[:k]) * w for k in range(len(rows))]
        assert all(o % 4 == 0 for o, _ in c)
    for n, (lens, _) in PLAIN_CUTS.items():
        assert [m for _, m in seg_model.cuts(n, False, 0, 16)] == lens
    assert seg_model.cuts(64, False, 0, 24) is None and seg_model.cuts(64, False, 0, 0) is None
    assert seg_model.cuts(16 * 7, True, 16, 128) is None and seg_model.cuts(7 * 16, True, 7, 128) is None


def test_plain_container_lengths(oracle_mod):
    for n, (lens, total) in PLAIN_CUTS.items():
        for diff in (False, True):
            c = seg_model.build(_plain(n), diff, False, 512, 16)
            if not diff:
                assert len(c) == total
            f, place = seg_model.parse(c)
            assert f["n_segments"] == len(lens) and f["raw_len"] == n and f["width"] == 0
            assert all(o % 16 == 0 for o, _ in place)


def test_model_round_trip(oracle_mod):
    for raw, diff, adapt, w, seg in _cases(oracle_mod):
        c = seg_model.build(raw, diff, adapt, w, seg)
        f, _ = seg_model.parse(c)
        # every segment is a complete reference stream, decodable alone
        for (off, n), s in zip(f["cuts"], seg_model.segments(c)):
            assert oracle_mod.decompress(s) == (0, raw[off:off + n])
        assert seg_model.decode(c) == (0, seg_model.NO_SEGMENT, raw)
        # and no reference stream is a container: the magic reads as a count above 2^63
        assert oracle_mod.decompress(c)[0] == 9
    assert oracle_mod.decompress(seg_model.MAGIC)[0] == 8


def test_count_and_bound(hc, oracle_mod):
    for raw, diff, adapt, w, seg in _cases(oracle_mod):
        c = seg_model.build(raw, diff, adapt, w, seg)
        want = len(seg_model.cuts(len(raw), adapt, w, seg))
        assert hc.seg_count(len(raw), seg, adapt, w) == want
        assert hc.seg_compress_bound(len(raw), seg, adapt, w) >= len(c)
    assert hc.seg_count(100, 24) == 0 and hc.seg_compress_bound(100, 24) == 0
    assert hc.seg_count(16 * 7, 128, True, 16) == 0 and hc.seg_count(100, 128, True, 0) == 0
    # seg_bytes 0 is the default size
    assert hc.seg_count(3 * 65536 + 1, 0) == 4 == hc.seg_count(3 * 65536 + 1, hc.HC_SEG_DEFAULT_BYTES)
    assert hc.HC_SEG_DEFAULT_BYTES == seg_model.DEFAULT_BYTES == 65536


def test_info_matches_model(hc, oracle_mod):
    for raw, diff, adapt, w, seg in _cases(oracle_mod):
        c = seg_model.build(raw, diff, adapt, w, seg)
        st, info = hc.seg_info(c)
        f, _ = seg_model.parse(c)
        assert st == 0
        assert (info.raw_len, info.seg_bytes, info.width, info.n_segments, info.flags) == (
            f["raw_len"], f["seg_bytes"], f["width"], f["n_segments"], f["flags"])
        # the header and the index are all it reads
        assert hc.seg_info(c[:48 + 8 * f["n_segments"]])[0] == 0


def test_info_rejects_header_mutants(hc, oracle_mod):
    plain = seg_model.build(_plain(100), True, False, 512, 32)
    adapt = seg_model.build(_matrix(16, 35), False, True, 16, 128)
    assert seg_model.parse(plain)[0]["n_segments"] == 4 and seg_model.parse(adapt)[0]["n_segments"] == 4
    for c in (plain, adapt):
        for name, bad in seg_model.header_mutants(c).items():
            assert seg_model.parse(bad) is None, name
            st, info = hc.seg_info(bad)
            assert st == hc.HC_ERR_SEG_HEADER and info is None, name
    # 520 bytes per container byte is the most a valid one holds: one more is rejected, the edge is not
    head = plain[:16] + struct.pack("<4Q", 520 * 72, 520 * 72 + 16, 0, 1) + bytes(8)
    assert hc.seg_info(head + bytes(16))[0] == 0
    head = plain[:16] + struct.pack("<4Q", 520 * 72 + 1, 520 * 72 + 16, 0, 1) + bytes(8)
    assert hc.seg_info(head + bytes(16))[0] == hc.HC_ERR_SEG_HEADER
    assert hc.lib().hc_seg_info(None, 0, None) == hc.HC_ERR_ARG


def test_host_decided_statuses(hc):
    L = hc.lib()
    n = ctypes.c_uint64(0)
    buf = ctypes.create_string_buffer(4096)
    out = ctypes.cast(buf, ctypes.c_void_p)
    data = ctypes.cast(ctypes.c_char_p(bytes(112)), ctypes.c_void_p)
    # HC_ERR_ARG first: null pointers, a segment size that is no multiple of 16
    assert L.hc_seg_compress(None, 3, 0, 0, 512, 16, out, 4096, ctypes.byref(n)) == hc.HC_ERR_ARG
    assert L.hc_seg_compress(data, 3, 0, 0, 512, 16, out, 4096, None) == hc.HC_ERR_ARG
    assert L.hc_seg_compress(data, 3, 0, 0, 0, 24, out, 4096, ctypes.byref(n)) == hc.HC_ERR_ARG
    assert L.hc_seg_decompress(None, 3, out, 4096, ctypes.byref(n), None) == hc.HC_ERR_ARG
    assert L.hc_seg_decompress(data, 3, out, 4096, None, None) == hc.HC_ERR_ARG
    assert L.hc_seg_decompress_alloc(data, 3, None, ctypes.byref(n), None) == hc.HC_ERR_ARG
    # then hc_compress's own, in its order
    assert hc.seg_compress(b"abc", width=0, seg_bytes=16)[0] == hc.HC_ERR_WIDTH
    assert hc.seg_compress(b"abcde", use_adapt=True, width=2, seg_bytes=16)[0] == hc.HC_ERR_MATRIX_SIZE
    assert hc.seg_compress(bytes(49), use_adapt=True, width=7, seg_bytes=16)[0] == hc.HC_ERR_DIMS
    assert hc.seg_compress(bytes(16 * 7), use_adapt=True, width=16, seg_bytes=16)[0] == hc.HC_ERR_DIMS
    # a bad container never needs the device
    assert hc.seg_decompress(b"")[0] == hc.HC_ERR_SEG_HEADER
    assert hc.seg_decompress(seg_model.MAGIC + bytes(40), full=True) == (hc.HC_ERR_SEG_HEADER, b"", 0, hc.NO_SEGMENT)
    # the device entry points check their arguments before any launch
    one = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(264)
    null = ctypes.c_void_p(0)
    assert L.hc_seg_compress_dev(one, 64, 0, 512, 16, one, 4096, one, one, null, 1 << 30, null) == hc.HC_ERR_ARG
    assert L.hc_seg_compress_dev(odd, 64, 0, 512, 16, one, 4096, one, one, one, 1 << 30, null) == hc.HC_ERR_ARG
    assert L.hc_seg_compress_dev(one, 64, 0x01, 512, 16, one, 4096, one, one, one, 1 << 30, null) == hc.HC_ERR_ARG
    assert L.hc_seg_compress_dev(one, 64, 0, 512, 24, one, 4096, one, one, one, 1 << 30, null) == hc.HC_ERR_ARG
    assert L.hc_seg_compress_dev(one, 64, 0, 0, 16, one, 4096, one, one, one, 1 << 30, null) == hc.HC_ERR_WIDTH
    assert L.hc_seg_compress_dev(one, 64, 0x40, 5, 16, one, 4096, one, one, one, 1 << 30, null) == hc.HC_ERR_MATRIX_SIZE
    assert L.hc_seg_compress_dev(one, 64, 0x40, 4, 16, one, 4096, one, one, one, 1 << 30, null) == hc.HC_ERR_DIMS
    need = int(L.hc_seg_compress_work_bound(64, 16, 0, 512))
    assert need > 4 * hc.compress_bound(16)
    assert L.hc_seg_compress_dev(one, 64, 0, 512, 16, one, 4096, one, one, one, need - 1, null) == hc.HC_ERR_ARG
    assert L.hc_seg_decompress_dev(one, 64, None, one, 64, one, one, one, one, 1 << 30, null) == hc.HC_ERR_ARG


def test_no_cpu_fallback(hc):
    import torch
    st, out = hc.seg_compress(b"abc", seg_bytes=16)
    if not torch.cuda.is_available():
        # needs the device: fails loudly instead of falling back to the CPU
        assert (st, out) == (hc.HC_ERR_DEVICE, b"")
        c = seg_model.MAGIC + bytes(8) + struct.pack("<4Q", 0, 16, 0, 1) + struct.pack("<Q", 9) + bytes(8) + bytes(9)
        assert seg_model.parse(c) is not None
        assert hc.seg_decompress(c)[0] == hc.HC_ERR_DEVICE
    else:
        assert st == 0 and seg_model.parse(out) is not None

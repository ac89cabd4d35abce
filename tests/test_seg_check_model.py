"""The checked segmented container without a device: the format model (tests/seg_check_model.py)
against the oracle and zlib, and the library's host-only entry points against the model."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

import seg_check_cases as cases
import seg_check_model as scm
import seg_model

# (raw input, use_diff, use_adapt, width, seg_bytes): n = 1, 2, 3, 4 and 7 segments, so every
# padding of the 12 n index bytes up to a multiple of 16 (0, 4, 8 and 12 bytes)
SHAPES = [("rng:256:0", False, False, 512, 16), ("rng:256:17", True, False, 512, 16),
          ("rng:256:40", False, False, 512, 16), ("rng:256:100", True, False, 512, 32),
          ("rng:256:100", False, False, 512, 16), ("photo:64:200", True, False, 512, 4096),
          ("photo:64:200", True, True, 64, 4096), ("rng:4:288", False, True, 9, 80)]


def _both(shape):
    name, diff, adapt, w, seg = shape
    raw = cases.raw(name)
    return raw, seg_model.build(raw, diff, adapt, w, seg), scm.build(raw, diff, adapt, w, seg)


def test_model_format(oracle_mod):
    pads = set()
    for shape in SHAPES:
        raw, plain, c = _both(shape)
        assert scm.build(raw, *shape[1:], check=False) == plain
        f, place, crcs = scm.parse(c)
        g, gplace = seg_model.parse(plain)
        n = f["n_segments"]
        assert f["check"] == 1 and c[9] == 1 and c[:9] == plain[:9] and c[10:48 + 8 * n] == plain[10:48 + 8 * n]
        assert {k: f[k] for k in g} == g
        assert crcs == [zlib.crc32(raw[o:o + m]) for o, m in f["cuts"]]
        assert place[0][0] == seg_model.align16(48 + 12 * n) and all(o % 16 == 0 for o, _ in place)
        assert not any(c[48 + 12 * n:place[0][0]])
        pads.add(place[0][0] - (48 + 12 * n))
        assert scm.segments(c) == seg_model.segments(plain)
        # the unchecked parser does not take a checked container, and the other way round it is seg_model's
        assert seg_model.parse(c) is None
        assert scm.parse(plain) == (dict(g, check=0), gplace, None)
    assert pads == {0, 4, 8, 12}
    assert scm.parse(scm.build(b"", check=True))[2] == [0]  # the CRC of an empty segment


def test_model_round_trip(oracle_mod):
    for shape in SHAPES:
        raw, plain, c = _both(shape)
        assert scm.decode(c) == (0, scm.NO_SEGMENT, raw) == scm.decode(plain)
        assert scm.decode(c, out_cap=len(raw)) == (0, scm.NO_SEGMENT, raw)
        if raw:
            assert scm.decode(c, out_cap=len(raw) - 1) == (scm.CAPACITY, scm.NO_SEGMENT, b"")
        assert scm.decode(c + b"\x00")[0] == scm.SEG_HEADER and scm.decode(c[:-1])[0] == scm.SEG_HEADER
        assert oracle_mod.decompress(c)[0] == 9  # still no reference stream
        # a wrong crc word fails exactly its segment
        n = scm.parse(c)[0]["n_segments"]
        k = n - 1
        at = 48 + 8 * n + 4 * k
        bad = c[:at] + bytes([c[at] ^ 1]) + c[at + 1:]
        assert scm.decode(bad) == (scm.SEG_CHECK, k, b"")


@pytest.mark.parametrize("case", cases.SILENT_FLIPS, ids=cases.FLIP_IDS)
def test_silent_flips_through_the_model(oracle_mod, case):
    name, diff, adapt, w, seg, byte, bit = case
    raw = cases.raw(name)
    plain, c = seg_model.build(raw, diff, adapt, w, seg), scm.build(raw, diff, adapt, w, seg)
    o, m = seg_model.parse(plain)[0]["cuts"][1]
    # unchecked: status 0, the right length, other bytes, and only in segment 1
    st, k, got = scm.decode(cases.flip(plain, 1, byte, bit))
    assert (st, k, len(got)) == (0, scm.NO_SEGMENT, len(raw)) and got != raw
    assert got[:o] == raw[:o] and got[o + m:] == raw[o + m:]
    assert zlib.crc32(got[o:o + m]) != zlib.crc32(raw[o:o + m])
    assert seg_model.decode(cases.flip(plain, 1, byte, bit)) == (0, scm.NO_SEGMENT, got)
    # checked: the segment is named
    assert scm.decode(cases.flip(c, 1, byte, bit)) == (scm.SEG_CHECK, 1, b"")


def test_info_reports_the_check(hc, oracle_mod):
    assert hc.HC_SEG_CHECK_CRC32 == scm.CHECK_CRC32 == 0x100 and hc.HC_ERR_SEG_CHECK == scm.SEG_CHECK == 72
    for shape in SHAPES:
        raw, plain, c = _both(shape)
        f, _, _ = scm.parse(c)
        n = f["n_segments"]
        st, info = hc.seg_info(c)
        assert st == 0
        assert (info.raw_len, info.seg_bytes, info.width, info.n_segments, info.flags) == (
            f["raw_len"], f["seg_bytes"], f["width"], n, f["flags"] | hc.HC_SEG_CHECK_CRC32)
        assert hc.seg_info(plain)[1].flags == f["flags"]
        # the header and the whole index are what it asks for
        assert hc.seg_info(c[:48 + 12 * n])[0] == 0
        assert hc.seg_info(c[:48 + 12 * n - 1])[0] == hc.HC_ERR_SEG_HEADER
        # check kinds above 1 and the bytes after it stay invalid
        assert hc.seg_info(c[:9] + b"\x02" + c[10:])[0] == hc.HC_ERR_SEG_HEADER
        assert hc.seg_info(c[:9] + b"\xff" + c[10:])[0] == hc.HC_ERR_SEG_HEADER
        assert hc.seg_info(c[:10] + b"\x01" + c[11:])[0] == hc.HC_ERR_SEG_HEADER
        assert hc.seg_info(c[:15] + b"\x01" + c[16:])[0] == hc.HC_ERR_SEG_HEADER
        assert hc.seg_info(plain[:10] + b"\x01" + plain[11:])[0] == hc.HC_ERR_SEG_HEADER
        for name, bad in seg_model.header_mutants(plain).items():
            # the same mutation of the checked container's header (index_cut: of its own index)
            if name == "short":
                bad = c[:47]
            elif name == "index_cut":
                bad = c[:48 + 12 * n - 1]
            else:
                bad = bad[:9] + b"\x01" + bad[10:48] + c[48:]
            assert scm.parse(bad) is None, name
            assert hc.seg_info(bad) == (hc.HC_ERR_SEG_HEADER, None), name


def test_bounds(hc, oracle_mod):
    L = hc.lib()
    K = hc.HC_SEG_CHECK_CRC32
    for shape in SHAPES:
        name, diff, adapt, w, seg = shape
        raw, plain, c = _both(shape)
        n = len(raw)
        fl = (hc.HC_FLAG_DIFF if diff else 0) | (hc.HC_FLAG_ADAPT if adapt else 0)
        for f in (fl, fl & hc.HC_FLAG_ADAPT):
            assert L.hc_seg_compress_bound2(n, seg, f, w) == L.hc_seg_compress_bound(n, seg, int(adapt), w) > 0
            assert L.hc_seg_compress_work_bound2(n, seg, f, w) == L.hc_seg_compress_work_bound(n, seg, int(adapt), w) > 0
        assert L.hc_seg_compress_bound2(n, seg, fl | K, w) >= len(c) >= len(plain)
        assert hc.seg_compress_bound(n, seg, adapt, w, check=True) == L.hc_seg_compress_bound2(n, seg, fl | K, w)
        assert hc.seg_compress_bound(n, seg, adapt, w) == L.hc_seg_compress_bound(n, seg, int(adapt), w)
        # the checked encoder's workspace also holds the n crc words
        k = len(seg_model.cuts(n, adapt, w, seg))
        assert L.hc_seg_compress_work_bound2(n, seg, fl | K, w) >= L.hc_seg_compress_work_bound2(n, seg, fl, w) + 4 * k
    # invalid arguments: 0, as for the old functions; so is an unknown flag bit
    assert L.hc_seg_compress_bound2(100, 24, K, 512) == 0 == L.hc_seg_compress_work_bound2(100, 24, K, 512)
    assert L.hc_seg_compress_bound2(100, 16, 0x01, 512) == 0 == L.hc_seg_compress_work_bound2(100, 16, 0x200, 512)


def test_argument_checks(hc):
    import torch
    L = hc.lib()
    K = hc.HC_SEG_CHECK_CRC32
    n = ctypes.c_uint64(0)
    buf = ctypes.create_string_buffer(4096)
    out = ctypes.cast(buf, ctypes.c_void_p)
    data = ctypes.cast(ctypes.c_char_p(bytes(112)), ctypes.c_void_p)
    # hc_seg_compress2: HC_ERR_ARG first (null pointers, unknown flag bits, the segment size), then hc_compress's own
    assert L.hc_seg_compress2(None, 3, K, 512, 16, out, 4096, ctypes.byref(n)) == hc.HC_ERR_ARG
    assert L.hc_seg_compress2(data, 3, K, 512, 16, out, 4096, None) == hc.HC_ERR_ARG
    assert L.hc_seg_compress2(data, 3, K, 512, 16, None, 4096, ctypes.byref(n)) == hc.HC_ERR_ARG
    assert L.hc_seg_compress2(data, 3, K | 0x01, 512, 16, out, 4096, ctypes.byref(n)) == hc.HC_ERR_ARG
    assert L.hc_seg_compress2(data, 3, 0x200, 512, 16, out, 4096, ctypes.byref(n)) == hc.HC_ERR_ARG
    assert L.hc_seg_compress2(data, 3, K, 512, 24, out, 4096, ctypes.byref(n)) == hc.HC_ERR_ARG
    assert L.hc_seg_compress2(data, 3, K, 0, 16, out, 4096, ctypes.byref(n)) == hc.HC_ERR_WIDTH
    assert L.hc_seg_compress2(data, 5, K | 0x40, 2, 16, out, 4096, ctypes.byref(n)) == hc.HC_ERR_MATRIX_SIZE
    assert L.hc_seg_compress2(data, 49, K | 0x40, 7, 16, out, 4096, ctypes.byref(n)) == hc.HC_ERR_DIMS
    assert hc.seg_compress(b"abc", width=0, seg_bytes=16, check=True)[0] == hc.HC_ERR_WIDTH
    # hc_seg_compress_dev: the check bit is a flag now, bit 0 is still none, and the bit asks for its own bound
    one = ctypes.c_void_p(256)
    null = ctypes.c_void_p(0)
    assert L.hc_seg_compress_dev(one, 64, 0x01, 512, 16, one, 4096, one, one, one, 1 << 30, null) == hc.HC_ERR_ARG
    assert L.hc_seg_compress_dev(one, 64, K | 0x01, 512, 16, one, 4096, one, one, one, 1 << 30, null) == hc.HC_ERR_ARG
    assert L.hc_seg_compress_dev(one, 64, K, 512, 16, one, 4096, one, one, null, 1 << 30, null) == hc.HC_ERR_ARG
    assert L.hc_seg_compress_dev(one, 64, K, 0, 16, one, 4096, one, one, one, 1 << 30, null) == hc.HC_ERR_WIDTH
    need = int(L.hc_seg_compress_work_bound2(64, 16, K, 512))
    plain = int(L.hc_seg_compress_work_bound(64, 16, 0, 512))
    assert need >= plain + 16
    assert L.hc_seg_compress_dev(one, 64, K, 512, 16, one, 4096, one, one, one, need - 1, null) == hc.HC_ERR_ARG
    assert L.hc_seg_compress_dev(one, 64, K, 512, 16, one, 4096, one, one, one, plain, null) == hc.HC_ERR_ARG
    # hc_crc32_batch: no ranges is no work, whatever the pointers; otherwise every pointer is needed
    assert L.hc_crc32_batch(null, null, null, 0, null, null) == 0
    for bad in range(4):
        args = [null if k == bad else one for k in range(4)]
        assert L.hc_crc32_batch(args[0], args[1], args[2], 1, args[3], null) == hc.HC_ERR_ARG
    if not torch.cuda.is_available():
        # valid arguments need the device: loud failures, no CPU path
        assert hc.seg_compress(b"abc", seg_bytes=16, check=True) == (hc.HC_ERR_DEVICE, b"")
        assert L.hc_seg_compress2(data, 3, K, 512, 16, out, 4096, ctypes.byref(n)) == hc.HC_ERR_DEVICE
        assert L.hc_crc32_batch(one, one, one, 1, one, null) == hc.HC_ERR_DEVICE
        c = scm.build(b"abc", seg_bytes=16)
        assert hc.seg_decompress(c, full=True)[0] == hc.HC_ERR_DEVICE
    else:
        st, c = hc.seg_compress(b"abc", seg_bytes=16, check=True)
        assert st == 0 and scm.parse(c)[2] == [zlib.crc32(b"abc")]

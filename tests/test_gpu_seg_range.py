"""Range decode of the segmented container on the GPU: hc_seg_decompress_range (host buffers, the
compact upload) and hc_seg_decompress_range_dev against the range model (tests/seg_range_model.py:
the oracle on the covered segments alone, the documented precedence)."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import gpu_batch
import seg_check_cases as cases
import seg_check_model as scm
import seg_model
import seg_range_model as srm

pytestmark = pytest.mark.gpu

NO_SEG = srm.NO_SEGMENT
FRONT, GUARD = 16, 64  # 0xA5 bytes in front of out[0] and behind out[length]
MUTANT_CASES = [("rng:256:100", False, 512, 32, True, False), ("rng:4:560", True, 16, 128, False, False)]
# the photo cases with -m, unchecked and checked: 4 segments, cuts at 4096, 8192 and 12288 of 12800 bytes
PHOTO_M = [c for c in srm.CASES if c[0] == "photo:64:200" and c[4]]
PHOTO_MK = [c for c in PHOTO_M if c[5]]
EDGES = (4100, 8192)   # segments 1 .. 3: 1 and 3 partly covered (staged), 2 whole and in place
WHOLE = (4096, 8192)   # segments 1 and 2, both whole and in place


def _upload(torch, container):
    host = np.zeros(gpu_batch.align(max(len(container), 1)), dtype=np.uint8)
    host[:len(container)] = np.frombuffer(bytes(container), dtype=np.uint8)
    return torch.from_numpy(host).cuda()


def dev_range(hc, torch, container, offset, length, out_cap=None, info=None):
    """seg_decompress_range_dev into a 16-byte-offset view of a 0xA5 buffer ->
    (status, out_len, bad_segment, out[:length], every byte around it is still 0xA5)"""
    inp = _upload(torch, container)
    backing = torch.full((FRONT + length + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = backing[FRONT:]
    olen = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    bad = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hc.seg_decompress_range_dev(inp, out, olen, st, offset, length, bad_segment=bad, info=info, in_len=len(container),
                                out_cap=length if out_cap is None else out_cap)
    torch.cuda.synchronize()
    got = backing.cpu().numpy().tobytes()
    clean = got[:FRONT] == b"\xa5" * FRONT and got[FRONT + length:] == b"\xa5" * GUARD
    return int(st.item()), int(olen.item()), int(bad.item()) % 2**64, got[FRONT:FRONT + length], clean


def both(hc, torch, container, offset, length):
    """the host and the device call, which must agree: (status, bad_segment, bytes, out_len); the
    guards around the device output are intact whatever the status"""
    st, got, n, bad = hc.seg_decompress_range(container, offset, length, full=True)
    dst, dn, dbad, out, clean = dev_range(hc, torch, container, offset, length)
    assert clean, (offset, length)
    assert (dst, dn, dbad) == (st, n, bad), (offset, length)
    if st == 0:
        assert out == got, (offset, length)
    return st, bad, got, n


@pytest.mark.parametrize("case", srm.CASES, ids=srm.case_id)
def test_matches_model(hc, gpu, case):
    raw, c, f, rs = srm.built(case)
    for o, m in rs:
        want = srm.decode_range(c, o, m)
        assert want == (0, NO_SEG, raw[o:o + m], m)
        assert both(hc, gpu, c, o, m) == want, (o, m)
    # the whole range is the whole decoder, in all four results
    st, got, n, bad = hc.seg_decompress(c, full=True)
    assert hc.seg_decompress_range(c, 0, len(raw), full=True) == (st, got, n, bad) == (0, raw, len(raw), NO_SEG)


def _raw_call(hc, torch, container, offset, length, work_bytes):
    """hc_seg_decompress_range_dev through ctypes with a workspace of exactly work_bytes bytes:
    (return value, status, out_len, bytes)"""
    L = hc.lib()
    inp = _upload(torch, container)
    st, info = hc.seg_info(container)
    assert st == 0
    out = torch.full((length + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    olen = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    stt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    work = torch.empty(max(work_bytes, 16), dtype=torch.uint8, device="cuda")
    rc = L.hc_seg_decompress_range_dev(inp.data_ptr(), len(container), ctypes.byref(info), offset, length, out.data_ptr(),
                                       length, olen.data_ptr(), stt.data_ptr(), None, work.data_ptr(), work_bytes,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = out.cpu().numpy().tobytes()
    assert got[length:] == b"\xa5" * GUARD
    return rc, int(stt.item()), int(olen.item()), got[:length]


@pytest.mark.parametrize("case", [c for c in srm.CASES if c[4] and c[0] != "rng:256:0"], ids=srm.case_id)
def test_work_bound(hc, gpu, case):
    raw, c, f, rs = srm.built(case)
    L = hc.lib()
    st, info = hc.seg_info(c)
    for o, m in rs:
        need = int(L.hc_seg_decompress_range_work_bound(ctypes.byref(info), len(c), o, m))
        assert need >= 16
        # exactly the bound is enough; a byte less is refused before any launch
        assert _raw_call(hc, gpu, c, o, m, need) == (0, 0, m, raw[o:o + m]), (o, m)
        rc, st, n, got = _raw_call(hc, gpu, c, o, m, need - 1)
        assert (rc, st, n) == (hc.HC_ERR_ARG, -1, -1) and got == b"\xa5" * m, (o, m)


def test_work_bound_follows_the_range(hc, gpu):
    raw, c, f, rs = srm.built((f"rng:256:{srm.BIG}", False, 512, 16, False, False))
    L = hc.lib()
    st, info = hc.seg_info(c)
    bound = lambda o, m: int(L.hc_seg_decompress_range_work_bound(ctypes.byref(info), len(c), o, m))
    aligned, unaligned = bound(16 * 1020, 16 * 11), bound(16 * 1020 + 1, 16 * 11)
    assert srm.covered(f, 16 * 1020, 16 * 11) == (1020, 11) and srm.covered(f, 16 * 1020 + 1, 16 * 11) == (1020, 12)
    # two slots against one per covered segment; arrays for the covered segments, not for all 2050
    assert aligned < unaligned
    assert aligned < int(L.hc_seg_decompress_work_bound(ctypes.byref(info), len(c))) + len(raw)
    # (44 bytes per covered segment, 24 per slot, the slots, 16 of control, 15 of rounding per array)
    assert aligned <= 11 * 44 + 2 * 24 + 2 * 16 + 16 + 11 * 15
    assert unaligned >= 12 * 16
    # the whole range costs what the whole decoder costs; partly covered edges add a slot each
    whole = int(L.hc_seg_decompress_work_bound(ctypes.byref(info), len(c)))
    assert bound(0, len(raw)) == whole
    assert aligned < bound(16 * 1020 + 4, 16 * 11) < unaligned  # 12 segments, 2 slots against 12


@pytest.mark.parametrize("case", PHOTO_M + [(f"rng:256:{srm.BIG}", False, 512, 16, True, False),
                                            ("rng:4:304", True, 16, 128, True, False)], ids=srm.case_id)
def test_capacity(hc, gpu, case):
    raw, c, f, rs = srm.built(case)
    for o, m in rs:
        if m == 0:
            continue
        # one byte short: the needed length, and nothing written at all
        assert srm.decode_range(c, o, m, out_cap=m - 1) == (hc.HC_ERR_CAPACITY, NO_SEG, b"", m)
        st, n, bad, got, clean = dev_range(hc, gpu, c, o, m, out_cap=m - 1)
        assert (st, n, bad) == (hc.HC_ERR_CAPACITY, m, NO_SEG) and clean and got == b"\xa5" * m, (o, m)
        assert hc.seg_decompress_range(c, o, m, full=True, cap=m - 1) == (hc.HC_ERR_CAPACITY, b"", m, NO_SEG), (o, m)
        # room for the range and not for the container: what the whole decoder rejects
        if m + 1 < len(raw):
            cap = m + 1
            st, n, bad, got, clean = dev_range(hc, gpu, c, o, m, out_cap=cap)
            assert (st, n, bad, got) == (0, m, NO_SEG, raw[o:o + m]) and clean, (o, m)
            assert hc.seg_decompress_range(c, o, m, full=True, cap=cap) == (0, raw[o:o + m], m, NO_SEG), (o, m)
            buf = ctypes.create_string_buffer(len(raw))
            k = ctypes.c_uint64(0)
            src = ctypes.cast(ctypes.c_char_p(c), ctypes.c_void_p)
            assert hc.lib().hc_seg_decompress(src, len(c), ctypes.cast(buf, ctypes.c_void_p), cap, ctypes.byref(k),
                                              None) == hc.HC_ERR_CAPACITY


@pytest.mark.parametrize("case", PHOTO_M, ids=srm.case_id)
def test_damage(hc, gpu, case):
    import oracle
    name, adapt, w, seg, diff, check = case
    raw, good, f, rs = srm.built(case)
    streams = scm.segments(good)
    assert len(streams) == 4 and srm.covered(f, *EDGES) == (1, 3) and srm.covered(f, *WHOLE) == (1, 2)
    st, short = oracle.compress(raw[:512], diff, adapt, w)  # a valid stream of another length than a 4096-byte cut
    assert st == 0

    def cut(k):
        return streams[k][:len(streams[k]) // 2]

    def damaged(repl):
        return scm.repack(good, [repl.get(k, s) for k, s in enumerate(streams)])

    def check_range(bad, o, m, want_bad):
        want = srm.decode_range(bad, o, m)
        assert want[1] == want_bad and (want[0] == 0) == (want_bad == NO_SEG)
        if want[0] == 0:
            assert want[2] == raw[o:o + m]
        assert both(hc, gpu, bad, o, m) == want, (o, m)

    o, m = EDGES
    for repl in (cut, lambda k: short):  # the coder's own status (8 or 9), and HC_ERR_SEG_SIZE
        assert srm.decode_range(damaged({1: repl(1)}), o, m)[0] in ((8, 9) if repl is cut else (hc.HC_ERR_SEG_SIZE,))
        check_range(damaged({1: repl(1)}), o, m, 1)                    # a staged edge segment
        check_range(damaged({2: repl(2)}), o, m, 2)                    # an in-place interior segment
        check_range(damaged({2: repl(2), 3: cut(3)}), o, m, 2)         # two covered: the lower one
        check_range(damaged({1: repl(1), 2: cut(2)}), o, m, 1)
        check_range(damaged({0: repl(0), 2: repl(2)}), o, m, 2)        # one below the range, one inside
        check_range(damaged({0: repl(0)}), o, m, NO_SEG)               # outside the range only
        check_range(damaged({0: repl(0), 3: cut(3)}), *WHOLE, NO_SEG)
        check_range(damaged({2: repl(2)}), *WHOLE, 2)
        check_range(damaged({2: repl(2)}), 0, 4096, NO_SEG)
    # the last, short segment staged and damaged: its container index, not its place in the range
    check_range(damaged({3: cut(3)}), 12287, 513, 3)
    check_range(damaged({3: cut(3)}), 12290, 7, 3)


def _set_crc(c, k, value):
    n = scm.parse(c)[0]["n_segments"]
    at = 48 + 8 * n + 4 * k
    return c[:at] + struct.pack("<I", value) + c[at + 4:]


@pytest.mark.parametrize("case", PHOTO_MK, ids=srm.case_id)
def test_checked_containers(hc, gpu, case):
    name, adapt, w, seg, diff, check = case
    raw, good, f, rs = srm.built(case)
    crcs = scm.parse(good)[2]
    flip = next(x for x in cases.SILENT_FLIPS if (x[0], x[2]) == (name, adapt))
    flipped = cases.flip(good, 1, flip[5], flip[6])  # segment 1 decodes cleanly, to its length, to other bytes
    assert scm.decode(flipped) == (hc.HC_ERR_SEG_CHECK, 1, b"")
    for o, m in (EDGES, (4097, 3), (8191, 2)):  # segment 1 staged
        assert srm.decode_range(flipped, o, m) == (hc.HC_ERR_SEG_CHECK, 1, b"", 0)
        assert both(hc, gpu, flipped, o, m) == (hc.HC_ERR_SEG_CHECK, 1, b"", 0), (o, m)
    for o, m in (WHOLE, (4096, 4096), (0, 12800)):  # segment 1 in place
        assert both(hc, gpu, flipped, o, m) == (hc.HC_ERR_SEG_CHECK, 1, b"", 0), (o, m)
    for o, m in ((8192, 100), (8193, 4607), (0, 4096), (1, 4095)):  # segment 1 not covered
        assert both(hc, gpu, flipped, o, m) == (0, NO_SEG, raw[o:o + m], m), (o, m)
    # a forged crc word fails its segment when it is covered, staged or in place, and only then
    for k in range(4):
        forged = _set_crc(good, k, crcs[k] ^ 0x80000000)
        b, n = f["cuts"][k]
        for o, m in ((b, n), (b + 1, n - 1), (0, 12800)):
            assert both(hc, gpu, forged, o, m) == (hc.HC_ERR_SEG_CHECK, k, b"", 0), (k, o, m)
        o, m = (0, b) if k else (n, 12800 - n)
        assert both(hc, gpu, forged, o, m) == (0, NO_SEG, raw[o:o + m], m), (k, o, m)
        assert both(hc, gpu, forged, o, 0) == (0, NO_SEG, b"", 0)
    two = _set_crc(_set_crc(good, 3, 0), 1, 0)
    assert both(hc, gpu, two, *EDGES) == (hc.HC_ERR_SEG_CHECK, 1, b"", 0)
    assert both(hc, gpu, two, 8192, 4608) == (hc.HC_ERR_SEG_CHECK, 3, b"", 0)


@pytest.mark.parametrize("case", MUTANT_CASES, ids=srm.case_id)
def test_container_mutants(hc, gpu, case):
    raw, good, f, rs = srm.built(case)
    assert f["n_segments"] == 4
    st, info = hc.seg_info(good)
    index = srm.index_mutants(good)
    for o, m in ((0, 0), (5, 70)):
        for name, bad in list(seg_model.header_mutants(good).items()) + list(index.items()):
            assert srm.decode_range(bad, o, m) == (hc.HC_ERR_SEG_HEADER, NO_SEG, b"", 0), name
            assert both(hc, gpu, bad, o, m) == (hc.HC_ERR_SEG_HEADER, NO_SEG, b"", 0), name
            _, _, _, out, clean = dev_range(hc, gpu, bad, o, m)
            assert clean and out == b"\xa5" * m, name  # and nothing was decoded
        # index mutants whose header is intact: the same verdict with the caller's own (valid) info
        for name in ("enc_len_wraps", "enc_len_longer", "enc_len_shorter"):
            st, n, k, out, clean = dev_range(hc, gpu, index[name], o, m, info=info)
            assert (st, n, k) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG) and clean and out == b"\xa5" * m, name
        # an info that is valid for this length but is not what the device bytes say
        other = hc.seg_info(good)[1]
        other.flags ^= hc.HC_FLAG_DIFF
        st, n, k, out, clean = dev_range(hc, gpu, good, o, m, info=other)
        assert (st, n, k) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG) and clean and out == b"\xa5" * m
    # a range outside raw_len: the argument error of both calls
    assert hc.seg_decompress_range(good, len(raw), 1)[0] == hc.HC_ERR_ARG
    with pytest.raises(hc.HCodecError):
        dev_range(hc, gpu, good, len(raw), 1)


def test_batch_cli(hc, gpu, tmp_path):
    raw = cases.raw("photo:64:200")
    good = scm.build(raw, True, False, 512, 4096)
    (tmp_path / "a.bin.huf").write_bytes(good)
    for o, m in (EDGES, (4097, 3), (0, 12800), (12800, 0)):
        r = subprocess.run([hc.BATCH_CLI_PATH, "-d", "-r", f"{o}:{m}", str(tmp_path / "a.bin.huf")], capture_output=True)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "a.bin").read_bytes() == raw[o:o + m]  # exactly the slice, under the usual name
        os.remove(tmp_path / "a.bin")
    # a plain stream has no index to read a range by
    st, stream = hc.compress(raw[:5000], True)
    assert st == 0
    (tmp_path / "p.bin.huf").write_bytes(stream)
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d", "-r", "0:16", str(tmp_path / "p.bin.huf"), str(tmp_path / "a.bin.huf")],
                       capture_output=True)
    assert r.returncode == hc.HC_ERR_UNSUPPORTED == 65
    assert b"p.bin.huf: -r needs a segmented container\n" in r.stderr
    assert not os.path.exists(tmp_path / "p.bin") and (tmp_path / "a.bin").read_bytes() == raw[:16]
    os.remove(tmp_path / "a.bin")
    # a range past the end
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d", "-r", "12800:1", str(tmp_path / "a.bin.huf")], capture_output=True)
    assert r.returncode == hc.HC_ERR_ARG == 71 and not os.path.exists(tmp_path / "a.bin")
    # a damaged covered segment is named by its container index; one outside the range is not noticed
    streams = scm.segments(good)
    (tmp_path / "bad.huf").write_bytes(scm.repack(good, streams[:2] + [streams[2][:8]] + streams[3:]))
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d", "-r", "4100:8192", str(tmp_path / "bad.huf")], capture_output=True)
    assert r.returncode == 8 and b"bad.huf: segment 2: ERROR: invalid or missing Huffman coding header" in r.stderr
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d", "-r", "4:4000", str(tmp_path / "bad.huf")], capture_output=True)
    assert r.returncode == 0 and (tmp_path / "bad").read_bytes() == raw[4:4004]
    # -r belongs to -d, and takes OFFSET:LENGTH: anything else is the usage error, before any file is touched
    for args in (["-c", "-r", "0:16"], ["-r", "0:16"], ["-d", "-r", "16"], ["-d", "-r", "0:"], ["-d", "-r", ":4"],
                 ["-d", "-r", "0:4:4"], ["-d", "-r", "0x10:4"], ["-d", "-r", "-1:4"]):
        r = subprocess.run([hc.BATCH_CLI_PATH] + args + [str(tmp_path / "a.bin.huf")], capture_output=True)
        assert r.returncode == 2 and b"ERROR: unrecognized option used" in r.stderr, args
    assert not os.path.exists(tmp_path / "a.bin") and not os.path.exists(tmp_path / "a.bin.huf.huf")

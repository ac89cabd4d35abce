"""List read of the segmented container without a device: the read model (tests/seg_reads_model.py)
against the raw bytes, the library's host-only entry points (hc_seg_reads_segments,
hc_seg_rect_reads, hc_seg_decompress_ranges_work_bound, the host-decided statuses of
hc_seg_decompress_ranges) against the model, the host plan under the sanitizers, and the usage
errors of the batch CLI's -R."""
import ctypes
import os
import shutil
import subprocess

import pytest

import seg_check_model as scm
import seg_model
import seg_range_model as srm
import seg_reads_model as srd

NO_SEG = srm.NO_SEGMENT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUTANT_CASES = [("rng:256:100", False, 512, 32, True, False), ("rng:4:560", True, 16, 128, False, False)]
LEFTOVER = ("rng:4:304", True, 16, 128, False, False)
RECTS = [(12800, 64, 5, 3, 20, 150), (12800, 64, 0, 0, 64, 200), (12800, 64, 63, 199, 1, 1), (12800, 64, 64, 0, 0, 7),
         (12800, 64, 0, 200, 5, 0), (100, 7, 2, 1, 3, 13), (0, 1, 0, 0, 0, 0), (2**64 - 1, 2**32, 1, 2**32 - 2, 2**32 - 1, 1)]
BAD_RECTS = {
    "pitch_0": (12800, 0, 0, 0, 0, 0),
    "wider_than_pitch": (12800, 64, 60, 0, 5, 1),
    "x_w_wraps": (12800, 64, 2**64 - 1, 0, 2, 1),
    "below_the_end": (12800, 64, 0, 199, 1, 2),
    "last_row_past_end": (12799, 64, 0, 199, 64, 1),
    "row_wraps": (12800, 64, 0, 2**64 - 2, 1, 3),
    "product_wraps": (2**64 - 1, 2**33, 0, 2**31, 1, 1),
    "sum_wraps": (2**64 - 1, 2**32, 2**32 - 1, 2**32 - 1, 1, 1),
    "area_wraps": (2**64 - 1, 2**33, 0, 0, 2**33, 2**31),
}


def bad_lists(raw_len):
    """{name: [(offset, length, dst_off)]} of the lists the rules refuse"""
    bad = {
        "past_end": [(raw_len, 1, 0)],
        "offset_past_end": [(raw_len + 1, 0, 0)],
        "wraps": [(1, 2**64 - 1, 0)],
        "wraps_offset": [(2**64 - 1, 2, 0)],
        "dst_wraps_empty": [(0, 0, 0), (raw_len, 0, 2**64 - 1), (raw_len + 1, 0, 0)],
    }
    if raw_len >= 8:
        bad["unsorted"] = [(4, 2, 0), (0, 2, 2)]
        bad["unsorted_empty"] = [(4, 2, 0), (3, 0, 2)]
        bad["dst_wraps"] = [(0, 2, 2**64 - 1)]
        bad["dst_wraps_far"] = [(0, 1, 0), (2, 6, 2**64 - 3)]
    return bad


def test_read_sets_list():
    case = ("photo:64:200", False, 512, 4096, True, False)
    raw, c, f, rs = srm.built(case)
    sets = srd.read_sets(case)
    assert sets["range_0_12800"] == [(0, 12800, 0)] and sets["none"] == []
    assert sets["two_in_one"] == [(1, 2, 9), (4093, 3, 1)] and srd.covered(f, sets["two_in_one"]) == [0]
    assert srd.covered(f, sets["overlap"]) == [0] and srd.need(sets["overlap"]) == 30 + 4092
    assert srd.covered(f, sets["first_and_last"]) == [0, 3] and srd.covered(f, sets["skip_one"]) == [0, 2, 3]
    assert sets["ends_in_short_last"] == [(12287, 513, 3)] and srd.covered(f, sets["ends_in_short_last"]) == [2, 3]
    assert srd.covered(f, sets["empties"]) == [] and srd.need(sets["empties"]) == 0
    # the records: the rank of a read's first segment, and one run of the staging region per read
    assert srd.records(f, sets["skip_one"]) == [(0, 1, 0, 4095, 1, 2), (0, 0, 0, 0, 0, 0), (2, 2, 1, 4097, 4098, 5)]
    assert srd.records(f, sets["long_then_short"]) == [(0, 0, 0, 0, 0, 0), (0, 4, 0, 1, 12799, 17), (1, 1, 1, 4097, 2, 3),
                                                       (3, 1, 3, 12799, 1, 0)]
    raw, c, f, rs = srm.built(LEFTOVER)
    sets = srd.read_sets(LEFTOVER)
    assert f["cuts"] == [(0, 128), (128, 176)]  # the last band took three leftover rows: last > full
    assert sets["leftover_rows"] == [(0, 3, 100), (257, 46, 0)] and srd.covered(f, sets["leftover_rows"]) == [0, 1]
    assert srd.records(f, sets["leftover_rows"])[1] == (1, 1, 1, 128 + 129, 46, 0)
    assert srd.covered(f, [(257, 46, 0)]) == [1] and srd.records(f, [(257, 46, 0)]) == [(1, 1, 0, 129, 46, 0)]
    assert srd.records(f, sets["spans_bands"]) == [(0, 2, 0, 123, 9, 40), (1, 1, 1, 255, 3, 1)]


@pytest.mark.parametrize("case", srm.CASES, ids=srm.case_id)
def test_model_against_raw_bytes(oracle_mod, case):
    raw, c, f, rs = srm.built(case)
    for sname, reads in srd.read_sets(case).items():
        st, bad, out, n = srd.decode_reads(c, reads)
        assert (st, bad, n) == (0, NO_SEG, srd.need(reads)), sname
        want = bytearray([srd.FILL]) * n
        for o, m, d in reads:
            want[d:d + m] = raw[o:o + m]
        assert out == bytes(want), sname
        assert srd.decode_reads(c, reads, out_cap=n) == (0, NO_SEG, out, n), sname
        if n:
            assert srd.decode_reads(c, reads, out_cap=n - 1) == (srd.CAPACITY, NO_SEG, b"", n), sname
        if len(reads) == 1 and reads[0][2] == 0:  # the one-read list (o, m, 0) is the ranged read
            o, m, d = reads[0]
            assert (st, bad, out, n) == srm.decode_range(c, o, m), sname
    for lname, bad in bad_lists(len(raw)).items():
        assert not srd.reads_ok(len(raw), bad), lname
        assert srd.decode_reads(c, bad) == (srd.ARG, None, b"", None), lname


@pytest.mark.parametrize("case", srm.CASES, ids=srm.case_id)
def test_library_counts_and_bound(hc, oracle_mod, case):
    raw, c, f, rs = srm.built(case)
    st, info = hc.seg_info(c)
    assert st == 0
    awb = lambda n, r, k: int(hc.lib().hc_adapt_decompress_work_bound(n, r, k))
    for sname, reads in srd.read_sets(case).items():
        ks = srd.covered(f, reads)
        assert hc.seg_reads_segments(info, len(c), reads) == (0, len(ks), srd.need(reads)), sname
        bound = hc.seg_decompress_ranges_work_bound(info, len(c), reads)
        assert bound == srd.work_bound(f, len(c), reads, awb) >= 16, sname
        # naming a segment again costs a record and nothing else: ten times the same read
        if reads and reads[-1][1]:
            o, m, d = reads[-1]
            more = reads + [(o, m, d + 1000 * (i + 1)) for i in range(10)]
            assert hc.seg_reads_segments(info, len(c), more)[1] == len(ks), sname
            again = hc.seg_decompress_ranges_work_bound(info, len(c), more)
            assert again == srd.work_bound(f, len(c), more, awb), sname
            assert again - bound == srd.align16(48 * len(more)) + 3 * srd.align16(8 * len(more)) \
                - srd.align16(48 * len(reads)) - 3 * srd.align16(8 * len(reads)), sname
    for lname, bad in bad_lists(len(raw)).items():
        assert hc.seg_reads_segments(info, len(c), bad)[0] == hc.HC_ERR_ARG, lname
        assert hc.seg_decompress_ranges_work_bound(info, len(c), bad) == 0, lname
    # an info that is not valid for this length, and null pointers
    assert hc.seg_reads_segments(info, 47, [])[0] == hc.HC_ERR_ARG
    assert hc.seg_decompress_ranges_work_bound(info, 47, []) == 16
    assert hc.seg_reads_segments(None, len(c), [])[0] == hc.HC_ERR_ARG
    assert hc.seg_decompress_ranges_work_bound(None, len(c), []) == 0
    n = ctypes.c_uint64(0)
    L = hc.lib()
    assert L.hc_seg_reads_segments(ctypes.byref(info), len(c), None, 0, None, ctypes.byref(n)) == hc.HC_ERR_ARG
    assert L.hc_seg_reads_segments(ctypes.byref(info), len(c), None, 0, ctypes.byref(n), None) == hc.HC_ERR_ARG
    assert L.hc_seg_reads_segments(ctypes.byref(info), len(c), None, 1, ctypes.byref(n), ctypes.byref(n)) == hc.HC_ERR_ARG


def test_work_bound_does_not_grow_with_n(hc, oracle_mod):
    """the same covered cuts in a container of 7 and of 2050 segments: the same bound, to the byte"""
    awb = lambda n, r, k: int(hc.lib().hc_adapt_decompress_work_bound(n, r, k))
    reads = [(17, 3, 0), (19, 40, 9), (80, 5, 3)]  # segments 1 .. 3 and 5
    bounds = []
    for n_bytes in (100, srm.BIG):
        raw, c, f, rs = srm.built((f"rng:256:{n_bytes}", False, 512, 16, False, False))
        st, info = hc.seg_info(c)
        assert st == 0 and srd.covered(f, reads) == [1, 2, 3, 5]
        bounds.append(hc.seg_decompress_ranges_work_bound(info, len(c), reads))
        assert bounds[-1] == srd.work_bound(f, len(c), reads, awb)
    assert bounds[0] == bounds[1] == 144 + 3 * 32 + 6 * 32 + 16 + 16 + 64
    # and 200 reads that all name segment 1021 of the 2050: C is 1
    many = [(16 * 1021 + (i % 13), 3, 3 * i) for i in sorted(range(200), key=lambda i: i % 13)]
    assert hc.seg_reads_segments(info, len(c), many) == (0, 1, 600)
    assert hc.seg_decompress_ranges_work_bound(info, len(c), many) == 9600 + 3 * 1600 + 6 * 16 + 16 + 16 + 16


def test_rect_reads(hc):
    for args in RECTS:
        want = srd.rect_reads(*args)
        assert want is not None, args
        assert hc.seg_rect_reads(*args) == (0, want), args
        assert srd.reads_ok(args[0], want) or args[4] == 0, args
    assert hc.seg_rect_reads(12800, 64, 5, 3, 20, 150)[1][:2] == [(197, 20, 0), (261, 20, 20)]
    for name, args in BAD_RECTS.items():
        assert srd.rect_reads(*args) is None, name
        if args[5] < 2**20:
            assert hc.seg_rect_reads(*args) == (hc.HC_ERR_ARG, []), name
    L = hc.lib()
    assert L.hc_seg_rect_reads(12800, 64, 0, 0, 1, 1, None) == hc.HC_ERR_ARG  # rows and nowhere to write them
    assert L.hc_seg_rect_reads(12800, 64, 0, 0, 1, 0, None) == hc.HC_OK


def _call(hc, container, reads, cap=1 << 16, out=True, out_len=True):
    """hc_seg_decompress_ranges with sentinels in *out_len and *bad_segment: (rc, out_len, bad_segment)"""
    L = hc.lib()
    buf = ctypes.create_string_buffer(max(cap, 1))
    n = ctypes.c_uint64(12345)
    bad = ctypes.c_uint64(777)
    src = ctypes.cast(ctypes.c_char_p(bytes(container)), ctypes.c_void_p) if container is not None else None
    rc = L.hc_seg_decompress_ranges(src, len(container) if container is not None else 3, hc.seg_reads(reads), len(reads),
                                    ctypes.cast(buf, ctypes.c_void_p) if out else None, cap,
                                    ctypes.byref(n) if out_len else None, ctypes.byref(bad))
    return rc, n.value, bad.value


@pytest.mark.parametrize("case", MUTANT_CASES, ids=srm.case_id)
def test_host_decided_statuses(hc, oracle_mod, case):
    import torch
    raw, good, f, rs = srm.built(case)
    ok_lists = ([], [(0, 0, 0)], [(5, 40, 3), (5, 1, 0)])
    # 1: null pointers, before anything is looked at and with nothing set
    assert _call(hc, None, []) == (hc.HC_ERR_ARG, 12345, 777)
    assert _call(hc, good, [], out=False) == (hc.HC_ERR_ARG, 12345, 777)
    assert _call(hc, good, [], out_len=False)[0] == hc.HC_ERR_ARG
    n = ctypes.c_uint64(12345)
    src = ctypes.cast(ctypes.c_char_p(good), ctypes.c_void_p)
    assert hc.lib().hc_seg_decompress_ranges(src, len(good), None, 1, src, 0, ctypes.byref(n), None) == hc.HC_ERR_ARG
    assert n.value == 12345  # a count without a list
    head, index = seg_model.header_mutants(good), srm.index_mutants(good)
    for reads in ok_lists:
        # 2: the header fails; 4: the index fails: the verdict does not depend on the list
        for name, bad in list(head.items()) + list(index.items()):
            assert srd.decode_reads(bad, reads)[:2] == (hc.HC_ERR_SEG_HEADER, NO_SEG), name
            assert _call(hc, bad, reads) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG), name
    # 3: a list that fails its rules: after the header (2 wins), before the index (3 wins), nothing set
    for lname, bad in bad_lists(len(raw)).items():
        assert _call(hc, good, bad) == (hc.HC_ERR_ARG, 12345, 777), lname
        assert _call(hc, head["magic"], bad) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG), lname
        assert _call(hc, index["enc_len_longer"], bad) == (hc.HC_ERR_ARG, 12345, 777), lname
    # the device call's host-decided answers need no device either
    L = hc.lib()
    st, info = hc.seg_info(good)
    one, odd, null = ctypes.c_void_p(256), ctypes.c_void_p(264), ctypes.c_void_p(0)
    big = 1 << 30
    dev = L.hc_seg_decompress_ranges_dev
    args = lambda **kw: [kw.get("inp", one), len(good), kw.get("info", ctypes.byref(info)), kw.get("reads", None),
                         kw.get("n", 0), kw.get("out", one), 4096, one, one, one, kw.get("work", one), kw.get("wb", big), null]
    assert dev(*args(info=None)) == hc.HC_ERR_ARG
    assert dev(*args(work=null)) == hc.HC_ERR_ARG and dev(*args(out=null)) == hc.HC_ERR_ARG
    assert dev(*args(out=odd)) == hc.HC_ERR_ARG and dev(*args(inp=odd)) == hc.HC_ERR_ARG and dev(*args(work=odd)) == hc.HC_ERR_ARG
    assert dev(*args(n=1)) == hc.HC_ERR_ARG                      # a count without a list
    for lname, bad in bad_lists(len(raw)).items():
        assert dev(*args(reads=hc.seg_reads(bad), n=len(bad))) == hc.HC_ERR_ARG, lname
    assert dev(*args(reads=hc.seg_reads([(5, 40, 3)]), n=1, wb=16)) == hc.HC_ERR_ARG  # below the work bound
    if not torch.cuda.is_available():
        # 5: a valid container and a valid list need the device: no CPU path
        for reads in ok_lists:
            assert srd.decode_reads(good, reads, device=False)[:2] == (hc.HC_ERR_DEVICE, NO_SEG)
            assert _call(hc, good, reads) == (hc.HC_ERR_DEVICE, 0, NO_SEG)
        assert _call(hc, good, [(5, 40, 3)], cap=1) == (hc.HC_ERR_DEVICE, 0, NO_SEG)  # before the capacity


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    """tests/seg_reads_plan_check.cpp built with AddressSanitizer and UBSan (host code only, its own main)"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/seg_reads_plan_check.cpp")
    exe = str(tmp_path_factory.mktemp("seg_reads") / "seg_reads_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "huffman-codec_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "seg_reads_plan_check.cpp")], check=True)
    return exe


def test_host_plan_under_sanitizers(plan_check, oracle_mod):
    def run(args):
        r = subprocess.run([plan_check] + [str(a) for a in args], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr  # a sanitizer report ends the program with another status
        assert r.stderr == ""
        return [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]

    def plan(case, reads):
        name, adapt, w, seg, diff, check = case
        raw_len = len(srm.built(case)[0])
        return run([raw_len, seg, int(adapt), w if adapt else 0] + [f"{o}:{m}:{d}" for o, m, d in reads])

    big = [(32 * i + 3, 1, i) for i in range(1025)]
    for case in srm.CASES:
        if case[4] or case[5]:
            continue  # (the plan does not depend on the diff model or the check)
        raw, c, f, rs = srm.built(case)
        sets = dict(srd.read_sets(case))
        if case[0] == f"rng:256:{srm.BIG}":
            sets["every_other_1025"] = big
        for sname, reads in sets.items():
            ks = srd.covered(f, reads)
            got = plan(case, reads)
            W = sum(f["cuts"][k][1] for k in ks)
            base = srd.work_bound(dict(f, flags=0, check=0), len(c), reads, None)
            assert got[0] == (0, len(ks), W, srd.need(reads), ks[0] if ks else 0, ks[-1] if ks else 0, base), (case, sname)
            assert got[1:] == srd.records(f, reads), (case, sname)
        for lname, bad in bad_lists(len(raw)).items():
            assert plan(case, bad) == [(71, 0, 0, 0, 0, 0, 0)], (case, lname)
    for args in RECTS:
        want = srd.rect_reads(*args)
        assert run(["rect"] + list(args)) == [(0, args[5])] + want, args
    for name, args in BAD_RECTS.items():
        assert run(["rect"] + list(args)) == [(71, 0)], name
    assert run(["rect", 2**64 - 1, 1, 0, 0, 0, 2**64 - 1]) == [(0, 0)]  # rows without bytes: the rules alone


def test_batch_cli_usage(hc, oracle_mod, tmp_path):
    """-R goes with -d alone, once, and takes X:Y:W:H: anything else is the usage error, before any
    file is touched; a FILE that is no container, a header that fails and a rectangle outside the
    container need no device to say so"""
    raw, good, f, rs = srm.built(("photo:64:200", False, 512, 4096, True, False))
    (tmp_path / "a.bin.huf").write_bytes(good)
    (tmp_path / "p").write_bytes(b"xy")
    R = ["-R", "5:3:20:150"]
    for args in (R, ["-c"] + R, ["-d", "-r", "0:4"] + R, ["-d"] + R + R, ["-d"] + R + ["-u", f"1:{tmp_path / 'p'}"],
                 R + ["-u", f"1:{tmp_path / 'p'}"], ["-d"] + R + ["-e", str(tmp_path / "p")], R + ["-e", str(tmp_path / "p")],
                 ["-d", "-R", "5:3:20"], ["-d", "-R", "5:3:20:150:1"], ["-d", "-R", "5:3:20:"], ["-d", "-R", ":3:20:150"],
                 ["-d", "-R", "5::20:150"], ["-d", "-R", "0x5:3:20:150"], ["-d", "-R", "5:3:-20:150"], ["-d", "-R", ""],
                 ["-d", "-R", "5:3:20:18446744073709551616"]):
        r = subprocess.run([hc.BATCH_CLI_PATH] + args + [str(tmp_path / "a.bin.huf")], capture_output=True)
        assert r.returncode == 2 and b"ERROR: unrecognized option used" in r.stderr, args
    assert not os.path.exists(tmp_path / "a.bin") and not os.path.exists(tmp_path / "a.bin.huf.upd")
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d", "-R"], capture_output=True)
    assert r.returncode == 1 and b"ERROR: missing additional argument" in r.stderr
    r = subprocess.run([hc.BATCH_CLI_PATH, "-h"], capture_output=True)
    assert r.returncode == 0 and b"-R X:Y:W:H" in r.stdout and b"-r OFFSET:LENGTH" in r.stdout and b"-u OFFSET:PATCHFILE" in r.stdout
    (tmp_path / "plain.huf").write_bytes(b"not a container")
    (tmp_path / "head.huf").write_bytes(seg_model.header_mutants(good)["n_more"])
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d"] + R + ["-w", "64", str(tmp_path / "plain.huf"), str(tmp_path / "head.huf")],
                       capture_output=True)
    assert r.returncode == 65 and b"plain.huf: -R needs a segmented container\n" in r.stderr
    assert b"head.huf: " in r.stderr and not os.path.exists(tmp_path / "plain") and not os.path.exists(tmp_path / "head")
    # outside the container: what -r reports for a range outside it; at -w's default the pitch is 512
    for args in (["-w", "64", "-R", "5:3:20:198"], ["-w", "64", "-R", "45:0:20:1"], ["-R", "5:3:20:150"], ["-w", "0", "-R", "0:0:0:0"]):
        r = subprocess.run([hc.BATCH_CLI_PATH, "-d"] + args + [str(tmp_path / "a.bin.huf")], capture_output=True)
        assert r.returncode == hc.HC_ERR_ARG == 71 and not os.path.exists(tmp_path / "a.bin"), args
    want = subprocess.run([hc.BATCH_CLI_PATH, "-d", "-r", "12800:1", str(tmp_path / "a.bin.huf")], capture_output=True)
    assert want.returncode == 71 and r.stderr.splitlines()[0] == want.stderr.splitlines()[0]

"""Range decode of the segmented container without a device: the range model
(tests/seg_range_model.py) against the whole-container model, the library's host-only entry
points (hc_seg_range_segments, the host-decided statuses of hc_seg_decompress_range, whose index
scan runs on the host) against the range model, and that host scan under the sanitizers."""
import ctypes
import os
import shutil
import subprocess

import pytest

import seg_check_model as scm
import seg_model
import seg_range_model as srm

NO_SEG = srm.NO_SEGMENT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the 4-segment containers of the container tests' mutants: (raw, use_adapt, width, seg_bytes, use_diff, checked)
MUTANT_CASES = [("rng:256:100", False, 512, 32, True, False), ("rng:4:560", True, 16, 128, False, False)]

_whole = {}


def whole(case):
    """seg_check_model.decode of the case's container, computed once"""
    if case not in _whole:
        _whole[case] = scm.decode(srm.built(case)[1])
    return _whole[case]


def mutants(case):
    """(header mutants, index mutants) of a case's container"""
    good = srm.built(case)[1]
    return seg_model.header_mutants(good), srm.index_mutants(good)


def test_ranges_list():
    # the shared list has every kind of range the cases call for
    raw, c, f, rs = srm.built(("photo:64:200", False, 512, 4096, True, False))
    assert rs == [(0, 0), (12800, 0), (0, 12800), (0, 1), (12799, 1), (4096, 4096), (4097, 3), (4100, 8192),
                  (4101, 8199), (12287, 513)]
    raw, c, f, rs = srm.built(("rng:4:304", True, 16, 128, False, False))
    assert f["cuts"] == [(0, 128), (128, 176)] and (256, 48) in rs and (257, 46) in rs  # the leftover rows
    assert srm.covered(f, 256, 48) == (1, 1) and 256 // 128 >= f["n_segments"]
    raw, c, f, rs = srm.built(("rng:256:17", False, 512, 16, False, False))
    assert rs == [(0, 0), (17, 0), (0, 17), (0, 1), (16, 1), (15, 2)]
    raw, c, f, rs = srm.built((f"rng:256:{srm.BIG}", False, 512, 16, False, False))
    assert f["n_segments"] == 2050 and (16 * 1020, 16 * 11) in rs and (srm.BIG - 5, 5) in rs
    assert srm.covered(f, 16 * 1020, 16 * 11) == (1020, 11)  # segments 1020 .. 1030: across entry 1024


@pytest.mark.parametrize("case", srm.CASES, ids=srm.case_id)
def test_covered_is_the_byte_map(case):
    raw, c, f, rs = srm.built(case)
    owner = [k for k, (_, m) in enumerate(f["cuts"]) for _ in range(m)]  # byte -> segment, from the cuts
    assert len(owner) == len(raw)
    for o, m in rs:
        want = (0, 0) if m == 0 else (owner[o], owner[o + m - 1] - owner[o] + 1)
        assert srm.covered(f, o, m) == want, (o, m)
    if len(raw) <= 20000:  # every offset, at a few lengths
        for o in range(len(raw)):
            for m in {1, min(2, len(raw) - o), min(17, len(raw) - o), len(raw) - o}:
                assert srm.covered(f, o, m) == (owner[o], owner[o + m - 1] - owner[o] + 1), (o, m)


@pytest.mark.parametrize("case", srm.CASES, ids=srm.case_id)
def test_model_is_the_slice(oracle_mod, case):
    raw, c, f, rs = srm.built(case)
    assert whole(case) == (0, NO_SEG, raw)
    for o, m in rs:
        assert srm.decode_range(c, o, m) == (0, NO_SEG, raw[o:o + m], m), (o, m)
        assert srm.decode_range(c, o, m, out_cap=m) == (0, NO_SEG, raw[o:o + m], m), (o, m)
        if m:
            assert srm.decode_range(c, o, m, out_cap=m - 1) == (srm.CAPACITY, NO_SEG, b"", m), (o, m)
    # outside raw_len: the argument error, even for the empty range
    for o, m in ((len(raw) + 1, 0), (0, len(raw) + 1), (len(raw), 1), (2**64 - 1, 2)):
        assert srm.decode_range(c, o, m)[0] == srm.ARG, (o, m)


@pytest.mark.parametrize("case", srm.CASES, ids=srm.case_id)
def test_range_segments_matches_model(hc, oracle_mod, case):
    raw, c, f, rs = srm.built(case)
    st, info = hc.seg_info(c)
    assert st == 0
    for o, m in rs:
        assert hc.seg_range_segments(info, len(c), o, m) == (0,) + srm.covered(f, o, m), (o, m)
    for o, m in ((len(raw) + 1, 0), (0, len(raw) + 1), (len(raw), 1), (2**64 - 1, 2)):
        assert hc.seg_range_segments(info, len(c), o, m)[0] == hc.HC_ERR_ARG, (o, m)
    # an info that is not valid for this length, and null pointers
    assert hc.seg_range_segments(info, 47, 0, 0)[0] == hc.HC_ERR_ARG
    info.n_segments += 1
    assert hc.seg_range_segments(info, len(c), 0, 0)[0] == hc.HC_ERR_ARG
    assert hc.seg_range_segments(None, len(c), 0, 0)[0] == hc.HC_ERR_ARG
    n = ctypes.c_uint64(0)
    info.n_segments -= 1
    assert hc.lib().hc_seg_range_segments(ctypes.byref(info), len(c), 0, 0, None, ctypes.byref(n)) == hc.HC_ERR_ARG
    assert hc.lib().hc_seg_range_segments(ctypes.byref(info), len(c), 0, 0, ctypes.byref(n), None) == hc.HC_ERR_ARG


def _call(hc, container, offset, length, cap=None, out=True, out_len=True):
    """hc_seg_decompress_range with sentinels in *out_len and *bad_segment: (rc, out_len, bad_segment)"""
    L = hc.lib()
    cap = min(length, 1 << 16) if cap is None else cap  # (no valid range of these tests is longer)
    buf = ctypes.create_string_buffer(max(cap, 1))
    n = ctypes.c_uint64(12345)
    bad = ctypes.c_uint64(777)
    src = ctypes.cast(ctypes.c_char_p(bytes(container)), ctypes.c_void_p) if container is not None else None
    rc = L.hc_seg_decompress_range(src, len(container) if container is not None else 3, offset, length,
                                   ctypes.cast(buf, ctypes.c_void_p) if out else None, cap,
                                   ctypes.byref(n) if out_len else None, ctypes.byref(bad))
    return rc, n.value, bad.value


@pytest.mark.parametrize("case", MUTANT_CASES, ids=srm.case_id)
def test_host_decided_statuses(hc, oracle_mod, case):
    import torch
    raw, good, f, rs = srm.built(case)
    assert f["n_segments"] == 4
    # 1: null pointers, before anything is looked at and with nothing set
    assert _call(hc, None, 0, 0) == (hc.HC_ERR_ARG, 12345, 777)
    assert _call(hc, good, 0, 4, out=False) == (hc.HC_ERR_ARG, 12345, 777)
    assert _call(hc, good, 0, 4, out_len=False)[0] == hc.HC_ERR_ARG
    assert _call(hc, seg_model.header_mutants(good)["magic"], 0, 4, out_len=False)[0] == hc.HC_ERR_ARG
    head, index = mutants(case)
    for o, m in ((0, 0), (5, 70)):
        # 2: the header fails; 4: the index fails: the verdict does not depend on the range
        for name, bad in list(head.items()) + list(index.items()):
            assert srm.decode_range(bad, o, m) == (hc.HC_ERR_SEG_HEADER, NO_SEG, b"", 0), name
            assert _call(hc, bad, o, m) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG), name
            assert hc.seg_decompress_range(bad, o, m, full=True) == (hc.HC_ERR_SEG_HEADER, b"", 0, NO_SEG), name
    # 3: a range outside raw_len: after the header (2 wins), before the index (3 wins), nothing set
    for o, m in ((len(raw) + 1, 0), (0, len(raw) + 1), (len(raw), 1), (2**64 - 1, 2), (1, 2**64 - 1)):
        assert srm.decode_range(good, o, m)[0] == hc.HC_ERR_ARG
        assert _call(hc, good, o, m) == (hc.HC_ERR_ARG, 12345, 777), (o, m)
        assert _call(hc, head["magic"], o, m) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG), (o, m)
        assert srm.decode_range(index["enc_len_longer"], o, m)[0] == hc.HC_ERR_ARG
        assert _call(hc, index["enc_len_longer"], o, m) == (hc.HC_ERR_ARG, 12345, 777), (o, m)
    # the work bound's own answers need no device either
    L = hc.lib()
    st, info = hc.seg_info(good)
    assert L.hc_seg_decompress_range_work_bound(None, len(good), 0, 0) == 0
    assert L.hc_seg_decompress_range_work_bound(ctypes.byref(info), len(good), len(raw), 1) == 0
    assert L.hc_seg_decompress_range_work_bound(ctypes.byref(info), len(good), 0, len(raw)) > 16
    assert L.hc_seg_decompress_range_work_bound(ctypes.byref(info), 47, 0, 0) == 16
    one, odd, null = ctypes.c_void_p(256), ctypes.c_void_p(264), ctypes.c_void_p(0)
    big = 1 << 30
    dev = L.hc_seg_decompress_range_dev
    assert dev(one, len(good), None, 0, 4, one, 4, one, one, one, one, big, null) == hc.HC_ERR_ARG
    assert dev(one, len(good), ctypes.byref(info), 0, 4, one, 4, one, one, one, null, big, null) == hc.HC_ERR_ARG
    assert dev(one, len(good), ctypes.byref(info), 0, 4, odd, 4, one, one, one, one, big, null) == hc.HC_ERR_ARG
    if not torch.cuda.is_available():
        # 5: a valid container and a valid range need the device: no CPU path
        for o, m in rs:
            assert srm.decode_range(good, o, m, device=False) == (hc.HC_ERR_DEVICE, NO_SEG, b"", 0)
            assert _call(hc, good, o, m) == (hc.HC_ERR_DEVICE, 0, NO_SEG), (o, m)
        # ... before the capacity is looked at
        assert _call(hc, good, 0, 8, cap=7) == (hc.HC_ERR_DEVICE, 0, NO_SEG)


@pytest.fixture(scope="module")
def index_check(tmp_path_factory):
    """tests/seg_index_check.cpp built with AddressSanitizer and UBSan (host code only, its own main)"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/seg_index_check.cpp")
    exe = str(tmp_path_factory.mktemp("seg_index") / "seg_index_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "huffman-codec_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "seg_index_check.cpp")], check=True)
    return exe


def test_host_index_scan_under_sanitizers(index_check, oracle_mod, tmp_path):
    def run(args):
        r = subprocess.run([index_check] + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr  # a sanitizer report ends the program with another status
        assert r.stderr == ""
        return [tuple(line.split()) for line in r.stdout.splitlines()]

    # the valid containers, at every range of their case
    for i, case in enumerate(srm.CASES):
        raw, c, f, rs = srm.built(case)
        path = tmp_path / f"good{i}"
        path.write_bytes(c)
        args, want = [], []
        for o, m in rs:
            args += [f"{o}:{m}", str(path)]
            want.append((path.name, "0") + tuple(str(v) for v in srm.covered(f, o, m) + srm.span(c, o, m)))
        args += ["all", str(path), f"{len(raw) + 1}:0", str(path), f"0:{len(raw) + 1}", str(path)]
        s0, s1 = srm.span(c, 0, len(raw))
        n = f["n_segments"]
        want.append((path.name, "0", "0", str(n if raw else 0), str(s0), str(s1)))
        want += [(path.name, "71", "0", "0", "0", "0")] * 2
        assert run(args) == want, srm.case_id(case)
    # every header and index mutant: the model's verdict, for the whole range and for a part
    for j, case in enumerate(MUTANT_CASES + [c for c in srm.CASES if c[0] == "photo:64:200" and c[4]]):
        raw, good, f, rs = srm.built(case)
        head = seg_model.header_mutants(good) if not case[5] else {}
        names = []
        for name, bad in list(head.items()) + list(srm.index_mutants(good).items()):
            assert srm.decode_range(bad, 0, 0)[0] == 68, name
            (tmp_path / f"m{j}_{name}").write_bytes(bad)
            names.append(f"m{j}_{name}")
        paths = [str(tmp_path / nm) for nm in names]
        want = [(nm, "68", "0", "0", "0", "0") for nm in names]
        assert run(paths) == want
        assert run(["0:0"] + paths) == want
        assert run(["5:70"] + paths) == want
    # an empty file and a header alone
    (tmp_path / "empty").write_bytes(b"")
    (tmp_path / "head").write_bytes(srm.built(srm.CASES[0])[1][:48])
    assert run([str(tmp_path / "empty"), str(tmp_path / "head")]) == [("empty", "68", "0", "0", "0", "0"),
                                                                      ("head", "68", "0", "0", "0", "0")]

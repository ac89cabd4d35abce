"""Range write of the segmented container without a device: the update model
(tests/seg_update_model.py) against the container model of the patched raw bytes, the library's
host-only entry points (hc_seg_update_segments, hc_seg_update_bound, the host-decided statuses of
hc_seg_update) against the update model, and the host plan under the sanitizers."""
import ctypes
import os
import shutil
import subprocess

import pytest

import seg_check_model as scm
import seg_model
import seg_range_model as srm
import seg_update_model as sup

NO_SEG = srm.NO_SEGMENT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUTANT_CASES = [("rng:256:100", False, 512, 32, True, False), ("rng:4:560", True, 16, 128, False, False)]
PHOTO = ("photo:64:200", False, 512, 4096, True, True)


def bad_lists(raw_len):
    """{name: [(offset, length, src_off)]} of the lists the rules refuse, for a data length of 64"""
    bad = {
        "past_end": [(raw_len, 1, 0)],
        "offset_past_end": [(raw_len + 1, 0, 0)],
        "wraps": [(1, 2**64 - 1, 0)],
        "wraps_offset": [(2**64 - 1, 2, 0)],
        "src_past_data": [(0, 1, 64)],
        "src_wraps": [(0, 1, 2**64 - 1)],
    }
    if raw_len >= 8:
        bad["unsorted"] = [(4, 2, 0), (0, 2, 2)]
        bad["overlap"] = [(0, 4, 0), (3, 2, 4)]
        bad["empty_inside_one"] = [(0, 4, 0), (2, 0, 0)]
        bad["src_long"] = [(0, 8, 57)]
    return bad


def test_patch_sets_list():
    sets = sup.patch_sets(("photo:64:200", False, 512, 4096, True, False))
    assert sets["adjacent_fill"] == [(0, 2048), (2048, 2048)] and sets["meet_on_cut"] == [(4094, 2), (4096, 3)]
    assert sets["first_and_last"] == [(0, 4096), (12288, 512)] and sets["range_0_12800"] == [(0, 12800)]
    raw, c, f, rs = srm.built(("photo:64:200", False, 512, 4096, True, False))
    plan = lambda spans: sup.plan(f, [(o, m, 0) for o, m in spans])
    assert plan(sets["adjacent_fill"]) == ([0], [0])          # the rule is per patch
    assert plan(sets["meet_on_cut"]) == ([0, 1], [0, 1])
    assert plan(sets["first_and_last"]) == ([0, 3], [])
    assert plan(sets["range_0_12800"]) == ([0, 1, 2, 3], [])  # nothing is decoded
    assert plan([(4100, 8192)]) == ([1, 2, 3], [1, 3]) and plan([(0, 0), (12800, 0)]) == ([], [])
    big = sup.patch_sets((f"rng:256:{srm.BIG}", False, 512, 16, False, False))
    assert len(big["many_small"]) == 200 and [(16 * 1020, 16 * 11)] in big.values()
    raw, c, f, rs = srm.built(("rng:4:304", True, 16, 128, False, False))
    assert sup.plan(f, [(256, 48, 0)]) == ([1], [1]) and sup.plan(f, [(128, 176, 0)]) == ([1], [])  # the leftover rows


@pytest.mark.parametrize("case", srm.CASES, ids=srm.case_id)
def test_model_is_the_container_of_the_patched_bytes(oracle_mod, case):
    name, adapt, w, seg, diff, check = case
    raw, c, f, rs = srm.built(case)
    for sname, spans in sup.patch_sets(case).items():
        for kind in sup.KINDS:
            patches = sup.fill(spans, kind)
            want = scm.build(sup.patched(raw, patches), diff, adapt, w, seg, check=check)
            assert sup.update(c, patches) == (0, NO_SEG, want, len(want)), (sname, kind)
            assert sup.update(c, patches, out_cap=len(want)) == (0, NO_SEG, want, len(want)), (sname, kind)
            assert sup.update(c, patches, out_cap=len(want) - 1) == (sup.CAPACITY, NO_SEG, b"", len(want)), sname
        # the bytes already there: the container itself
        same = [(o, raw[o:o + m]) for o, m in spans]
        assert sup.update(c, same) == (0, NO_SEG, c, len(c)), sname
    for lname, bad in bad_lists(len(raw)).items():
        assert not sup.patches_ok(len(raw), bad, 64), lname


@pytest.mark.parametrize("case", srm.CASES, ids=srm.case_id)
def test_library_counts_and_bound(hc, oracle_mod, case):
    raw, c, f, rs = srm.built(case)
    st, info = hc.seg_info(c)
    assert st == 0
    for sname, spans in sup.patch_sets(case).items():
        tri = [(o, m, 0) for o, m in spans]
        covered, decoded = sup.plan(f, tri)
        assert hc.seg_update_segments(info, len(c), tri) == (0, len(covered), len(decoded)), sname
        assert hc.seg_update_bound(info, len(c), tri) == sup.update_bound(f, len(c), tri, hc.compress_bound), sname
        assert hc.seg_update_work_bound(info, len(c), tri) >= 32, sname
    for lname, bad in bad_lists(len(raw)).items():
        if lname.startswith("src_"):
            continue  # (these three calls do not see the patch data's length)
        assert hc.seg_update_segments(info, len(c), bad)[0] == hc.HC_ERR_ARG, lname
        assert hc.seg_update_bound(info, len(c), bad) == 0 and hc.seg_update_work_bound(info, len(c), bad) == 0, lname
    # an info that is not valid for this length, and null pointers
    assert hc.seg_update_segments(info, 47, [])[0] == hc.HC_ERR_ARG
    assert hc.seg_update_bound(info, 47, []) == 0 and hc.seg_update_work_bound(info, 47, []) == 16
    assert hc.seg_update_segments(None, len(c), [])[0] == hc.HC_ERR_ARG
    assert hc.seg_update_bound(None, len(c), []) == 0 and hc.seg_update_work_bound(None, len(c), []) == 0
    n = ctypes.c_uint64(0)
    L = hc.lib()
    assert L.hc_seg_update_segments(ctypes.byref(info), len(c), None, 0, None, ctypes.byref(n)) == hc.HC_ERR_ARG
    assert L.hc_seg_update_segments(ctypes.byref(info), len(c), None, 0, ctypes.byref(n), None) == hc.HC_ERR_ARG
    assert L.hc_seg_update_segments(ctypes.byref(info), len(c), None, 1, ctypes.byref(n), ctypes.byref(n)) == hc.HC_ERR_ARG
    assert hc.seg_update_bound(info, len(c), []) == len(c)


def _call(hc, container, tri, data, cap=1 << 16, out=True, out_len=True):
    """hc_seg_update with sentinels in *out_len and *bad_segment: (rc, out_len, bad_segment)"""
    L = hc.lib()
    buf = ctypes.create_string_buffer(max(cap, 1))
    n = ctypes.c_uint64(12345)
    bad = ctypes.c_uint64(777)
    src = ctypes.cast(ctypes.c_char_p(bytes(container)), ctypes.c_void_p) if container is not None else None
    pd = ctypes.cast(ctypes.c_char_p(bytes(data)), ctypes.c_void_p) if data else None
    rc = L.hc_seg_update(src, len(container) if container is not None else 3, hc.seg_patches(tri), len(tri), pd, len(data),
                         ctypes.cast(buf, ctypes.c_void_p) if out else None, cap, ctypes.byref(n) if out_len else None,
                         ctypes.byref(bad))
    return rc, n.value, bad.value


@pytest.mark.parametrize("case", MUTANT_CASES, ids=srm.case_id)
def test_host_decided_statuses(hc, oracle_mod, case):
    import torch
    raw, good, f, rs = srm.built(case)
    data = bytes(64)
    ok_lists = ([], [(0, 0, 0)], [(5, 40, 3)])
    # 1: null pointers, before anything is looked at and with nothing set
    assert _call(hc, None, [], data) == (hc.HC_ERR_ARG, 12345, 777)
    assert _call(hc, good, [], data, out=False) == (hc.HC_ERR_ARG, 12345, 777)
    assert _call(hc, good, [], data, out_len=False)[0] == hc.HC_ERR_ARG
    head, index = seg_model.header_mutants(good), srm.index_mutants(good)
    for tri in ok_lists:
        # 2: the header fails; 4: the index fails: the verdict does not depend on the patches
        for name, bad in list(head.items()) + list(index.items()):
            assert sup.update(bad, [(o, data[s:s + m]) for o, m, s in tri])[:2] == (hc.HC_ERR_SEG_HEADER, NO_SEG), name
            assert _call(hc, bad, tri, data) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG), name
    # 3: a list that fails its rules: after the header (2 wins), before the index (3 wins), nothing set
    for lname, bad in bad_lists(len(raw)).items():
        assert _call(hc, good, bad, data) == (hc.HC_ERR_ARG, 12345, 777), lname
        assert _call(hc, head["magic"], bad, data) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG), lname
        assert _call(hc, index["enc_len_longer"], bad, data) == (hc.HC_ERR_ARG, 12345, 777), lname
    # the device call's host-decided answers need no device either
    L = hc.lib()
    st, info = hc.seg_info(good)
    one, odd, null = ctypes.c_void_p(256), ctypes.c_void_p(264), ctypes.c_void_p(0)
    far = ctypes.c_void_p(1 << 20)
    big = 1 << 30
    dev = L.hc_seg_update_dev
    args = lambda **kw: [kw.get("inp", one), len(good), kw.get("info", ctypes.byref(info)), kw.get("tri", None),
                         kw.get("n", 0), one, 64, kw.get("out", far), kw.get("cap", 4096), one, one, one,
                         kw.get("work", one), kw.get("wb", big), null]
    assert dev(*args(info=None)) == hc.HC_ERR_ARG
    assert dev(*args(work=null)) == hc.HC_ERR_ARG
    assert dev(*args(out=odd)) == hc.HC_ERR_ARG and dev(*args(inp=odd)) == hc.HC_ERR_ARG
    assert dev(*args(n=1)) == hc.HC_ERR_ARG                      # a count without a list
    assert dev(*args(out=ctypes.c_void_p(256 + 16))) == hc.HC_ERR_ARG    # out begins inside in
    assert dev(*args(inp=far, out=one, cap=(1 << 20) - 256 + 1)) == hc.HC_ERR_ARG  # in begins inside out
    for lname, bad in bad_lists(len(raw)).items():
        assert dev(*args(tri=hc.seg_patches(bad), n=len(bad))) == hc.HC_ERR_ARG, lname
    assert dev(*args(tri=hc.seg_patches([(5, 40, 3)]), n=1, wb=16)) == hc.HC_ERR_ARG  # below the work bound
    if not torch.cuda.is_available():
        # 5: a valid container and a valid list need the device: no CPU path
        for tri in ok_lists:
            assert sup.update(good, [(o, data[s:s + m]) for o, m, s in tri], device=False)[:2] == (hc.HC_ERR_DEVICE, NO_SEG)
            assert _call(hc, good, tri, data) == (hc.HC_ERR_DEVICE, 0, NO_SEG)
        assert _call(hc, good, [(5, 40, 3)], data, cap=1) == (hc.HC_ERR_DEVICE, 0, NO_SEG)  # before the capacity


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    """tests/seg_update_plan_check.cpp built with AddressSanitizer and UBSan (host code only, its own main)"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/seg_update_plan_check.cpp")
    exe = str(tmp_path_factory.mktemp("seg_update") / "seg_update_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "huffman-codec_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "seg_update_plan_check.cpp")], check=True)
    return exe


def test_host_plan_under_sanitizers(plan_check, oracle_mod):
    def run(case, tri, data_len):
        name, adapt, w, seg, diff, check = case
        raw_len = len(srm.built(case)[0])
        r = subprocess.run([plan_check, str(raw_len), str(seg), str(int(adapt)), str(w if adapt else 0), str(data_len)]
                           + [f"{o}:{m}:{s}" for o, m, s in tri], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr  # a sanitizer report ends the program with another status
        assert r.stderr == ""
        return [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]

    for case in srm.CASES:
        if case[4] or case[5]:
            continue  # (the plan does not depend on the diff model or the check)
        raw, c, f, rs = srm.built(case)
        for sname, spans in sup.patch_sets(case).items():
            tri, at = [], 3
            for o, m in spans:
                tri.append((o, m, at))
                at += m
            covered, decoded = sup.plan(f, tri)
            got = run(case, tri, at)
            raw_of = lambda ks: sum(f["cuts"][k][1] for k in ks)
            assert got[0] == (0, len(covered), len(decoded), raw_of(covered), raw_of(decoded)), (case, sname)
            want = sup.records(f, tri)
            assert len(got) == 1 + len(tri)
            for (k0, cnt, e0, d0, dmask, dst), (wcnt, wk0, we0, wd0, wmask, wdst) in zip(got[1:], want):
                assert (cnt, e0, d0, dmask, dst) == (wcnt, we0, wd0, wmask, wdst), (case, sname)
                assert wk0 is None or k0 == wk0, (case, sname)
            # a source range that ends one byte past the data
            if at > 3:
                assert run(case, tri, at - 1) == [(71, 0, 0, 0, 0)], (case, sname)
        for lname, bad in bad_lists(len(raw)).items():
            assert run(case, bad, 64) == [(71, 0, 0, 0, 0)], (case, lname)


def test_batch_cli_usage(hc, oracle_mod, tmp_path):
    """-u goes with none of the coding options and takes OFFSET:PATCHFILE: anything else is the
    usage error, before any file is touched; a FILE that is no container needs no device to say so"""
    raw, good, f, rs = srm.built(MUTANT_CASES[0])
    (tmp_path / "a.huf").write_bytes(good)
    (tmp_path / "p").write_bytes(b"xy")
    u = ["-u", f"1:{tmp_path / 'p'}"]
    for args in (["-c"] + u, ["-d"] + u, ["-m"] + u, ["-a"] + u, u + ["-s", "64"], u + ["-k"], u + ["-r", "0:4"],
                 ["-u", "1"], ["-u", "1:"], ["-u", f":{tmp_path / 'p'}"], ["-u", f"0x1:{tmp_path / 'p'}"],
                 ["-u", f"-1:{tmp_path / 'p'}"]):
        r = subprocess.run([hc.BATCH_CLI_PATH] + args + [str(tmp_path / "a.huf")], capture_output=True)
        assert r.returncode == 2 and b"ERROR: unrecognized option used" in r.stderr, args
    assert not os.path.exists(tmp_path / "a.huf.upd")
    r = subprocess.run([hc.BATCH_CLI_PATH, "-h"], capture_output=True)
    assert r.returncode == 0 and b"-u OFFSET:PATCHFILE" in r.stdout
    (tmp_path / "plain").write_bytes(b"not a container")
    r = subprocess.run([hc.BATCH_CLI_PATH] + u + [str(tmp_path / "plain")], capture_output=True)
    assert r.returncode == 65 and b"plain: -u needs a segmented container\n" in r.stderr
    r = subprocess.run([hc.BATCH_CLI_PATH, "-u", f"1:{tmp_path / 'missing'}", str(tmp_path / "a.huf")], capture_output=True)
    assert r.returncode == 5 and b"missing: ERROR: given input file does not exist" in r.stderr

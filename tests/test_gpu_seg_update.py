"""Range write of the segmented container on the GPU: hc_seg_update (host buffers) and
hc_seg_update_dev against the update model (tests/seg_update_model.py: the oracle on the decoded
and the covered segments alone, the documented precedence), whose result for a container of this
library is the container of the patched raw bytes."""
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
import seg_update_model as sup

pytestmark = pytest.mark.gpu

NO_SEG = srm.NO_SEGMENT
FRONT, GUARD = 16, 64  # 0xA5 bytes in front of out[0] and behind out[out_cap]
MUTANT_CASES = [("rng:256:100", False, 512, 32, True, False), ("rng:4:560", True, 16, 128, False, False)]
PHOTO_M = [c for c in srm.CASES if c[0] == "photo:64:200" and c[4]]
PHOTO_MK = [c for c in PHOTO_M if c[5]]
BIG_CASE = (f"rng:256:{srm.BIG}", False, 512, 16, True, False)
EDGES = (4100, 8192)   # segments 1 .. 3: 1 and 3 decoded, 2 covered whole
# the seal's piece scan past one 1024-entry tile: 520 segments covered in part by one byte each (1041
# pieces, 11 descriptor launches, a segment in every old block between them), and 520 covered whole by
# one patch (nothing decoded, empty old blocks between them)
TILE_CASES = [(f"rng:256:{srm.BIG}", False, 512, 16, False, k) for k in (False, True)]
TILE_SETS = {"partial_520": [(32 * i + 3, 1) for i in range(520)], "whole_520": [(16 * 700, 16 * 520)]}


def _upload(torch, data, front=0):
    """the bytes at `front` of a zeroed device buffer whose length is a multiple of 16"""
    host = np.zeros(gpu_batch.align(front + max(len(data), 1)), dtype=np.uint8)
    host[front:front + len(data)] = np.frombuffer(bytes(data), dtype=np.uint8)
    return torch.from_numpy(host).cuda()


def dev_update(hc, torch, container, patches, out_cap=None, info=None, work_bytes=None):
    """hc_seg_update_dev into a 16-byte-offset view of a 0xA5 buffer, the patch bytes at an odd
    address -> (status, out_len, bad_segment, out[:out_cap], every byte around it is still 0xA5).
    work_bytes: through ctypes with a workspace of exactly that many bytes, the return value first."""
    tri, data = sup.triples(patches)
    tri = [(o, m, s + 1) for o, m, s in tri]
    pd = _upload(torch, data, front=1)
    inp = _upload(torch, container)
    if out_cap is None:
        st, i = hc.seg_info(container)
        out_cap = hc.seg_update_bound(i, len(container), tri) if st == 0 else 64
    backing = torch.full((FRONT + out_cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = backing[FRONT:]
    olen = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    bad = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    rc = None
    if work_bytes is None:
        hc.seg_update_dev(inp, tri, pd, out, olen, st, bad_segment=bad, info=info, in_len=len(container), out_cap=out_cap,
                          patch_data_len=1 + len(data))
    else:
        if info is None:
            info = hc.seg_info(container)[1]
        work = torch.empty(max(work_bytes, 16), dtype=torch.uint8, device="cuda")
        rc = hc.lib().hc_seg_update_dev(inp.data_ptr(), len(container), ctypes.byref(info), hc.seg_patches(tri), len(tri),
                                        pd.data_ptr(), 1 + len(data), out.data_ptr(), out_cap, olen.data_ptr(),
                                        st.data_ptr(), bad.data_ptr(), work.data_ptr(), work_bytes,
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = backing.cpu().numpy().tobytes()
    clean = got[:FRONT] == b"\xa5" * FRONT and got[FRONT + out_cap:] == b"\xa5" * GUARD
    res = (int(st.item()), int(olen.item()), int(bad.item()) % 2**64, got[FRONT:FRONT + out_cap], clean)
    return (rc,) + res if work_bytes is not None else res


def both(hc, torch, container, patches, want):
    """the device and the host call against the model's (status, bad_segment, bytes, out_len); on
    a non-zero status the device output is untouched; the guards are intact whatever the status"""
    wst, wbad, wbytes, wlen = want
    st, n, bad, out, clean = dev_update(hc, torch, container, patches)
    assert clean
    assert (st, n, bad) == (wst, wlen, wbad)
    if st == 0:
        assert out[:n] == wbytes and out[n:] == b"\xa5" * (len(out) - n)
    else:
        assert out == b"\xa5" * len(out)
    assert hc.seg_update(container, patches, full=True) == (wst, wbytes, wlen, wbad)


@pytest.mark.parametrize("case", srm.CASES, ids=srm.case_id)
def test_matches_model(hc, gpu, case):
    name, adapt, w, seg, diff, check = case
    raw, c, f, rs = srm.built(case)
    for sname, spans in sup.patch_sets(case).items():
        for kind in sup.KINDS:
            patches = sup.fill(spans, kind)
            want = sup.update(c, patches)
            new_raw = sup.patched(raw, patches)
            assert want[0] == 0, (sname, kind)
            both(hc, gpu, c, patches, want)
            assert hc.seg_decompress(want[2], full=True) == (0, new_raw, len(raw), NO_SEG), (sname, kind)
            if spans == [(0, len(raw))]:  # nothing is decoded: the encoder's own output for the patch
                assert sup.plan(f, sup.triples(patches)[0])[1] == []
                assert hc.seg_compress(new_raw, diff, adapt, w, seg, check=check) == (0, want[2]), (sname, kind)


@pytest.mark.parametrize("sname", TILE_SETS)
@pytest.mark.parametrize("case", TILE_CASES, ids=srm.case_id)
def test_pieces_across_a_scan_tile(hc, gpu, case, sname):
    """more pieces than the seal scans in one tile: 520 covered segments are 1041 pieces"""
    name, adapt, w, seg, diff, check = case
    raw, c, f, rs = srm.built(case)
    tri = [(o, m, 0) for o, m in TILE_SETS[sname]]
    covered, decoded = sup.plan(f, tri)
    assert len(covered) == 520 and 2 * len(covered) + 1 > 1024
    assert len(decoded) == (520 if sname == "partial_520" else 0)
    # every old block between two covered segments holds a segment, or none does
    assert all(b - a == (2 if sname == "partial_520" else 1) for a, b in zip(covered, covered[1:]))
    patches = sup.fill(TILE_SETS[sname], "random")
    want = sup.update(c, patches)
    assert want[0] == 0
    both(hc, gpu, c, patches, want)
    assert hc.seg_compress(sup.patched(raw, patches), diff, adapt, w, seg, check=check) == (0, want[2])


@pytest.mark.parametrize("case", PHOTO_M, ids=srm.case_id)
def test_damage(hc, gpu, case):
    import oracle
    name, adapt, w, seg, diff, check = case
    raw, good, f, rs = srm.built(case)
    streams = scm.segments(good)
    st, short = oracle.compress(raw[:1024], diff, adapt, w)  # a valid stream of another length than any cut
    assert st == 0 and len(streams) == 4

    def cut(k):
        return streams[k][:len(streams[k]) // 2]

    def damaged(repl):
        return scm.repack(good, [repl.get(k, s) for k, s in enumerate(streams)])

    patches = sup.fill([EDGES], "random")  # segments 1 and 3 decoded, 2 covered whole, 0 not covered
    new_raw = sup.patched(raw, patches)
    assert sup.plan(f, sup.triples(patches)[0]) == ([1, 2, 3], [1, 3])
    for repl in (cut, lambda k: short):  # the coder's own status (8 or 9), and HC_ERR_SEG_SIZE
        for bad_in, want_bad in (({1: repl(1)}, 1), ({3: repl(3)}, 3), ({1: repl(1), 3: cut(3)}, 1),
                                 ({2: repl(2), 3: repl(3)}, 3), ({0: repl(0), 3: repl(3)}, 3)):
            bad = damaged(bad_in)
            want = sup.update(bad, patches)
            assert want[0] != 0 and want[1:] == (want_bad, b"", 0)
            both(hc, gpu, bad, patches, want)
        assert sup.update(damaged({1: repl(1)}), patches)[0] in ((8, 9) if repl is cut else (hc.HC_ERR_SEG_SIZE,))
        # in a segment covered whole: repaired
        bad = damaged({2: repl(2)})
        want = sup.update(bad, patches)
        assert want[0] == 0 and want[2] == scm.build(new_raw, diff, adapt, w, seg, check=check)
        both(hc, gpu, bad, patches, want)
        # in an uncovered segment: carried over verbatim, and the result's decoder names it
        bad = damaged({0: repl(0)})
        want = sup.update(bad, patches)
        assert want[0] == 0 and scm.segments(want[2])[0] == repl(0)
        both(hc, gpu, bad, patches, want)
        st, _, _, k = hc.seg_decompress(want[2], full=True)
        assert st != 0 and k == 0
    # a forged enc_len of a decoded segment: one that still tiles the container cuts the stream short,
    # one that does not fails the index
    forge = lambda v: good[:48 + 8] + struct.pack("<Q", v) + good[48 + 16:]
    if len(streams[1]) % 16 != 1:
        both(hc, gpu, forge(len(streams[1]) - 1), patches, sup.update(forge(len(streams[1]) - 1), patches))
    both(hc, gpu, forge(len(streams[1]) + 16), patches, (hc.HC_ERR_SEG_HEADER, NO_SEG, b"", 0))


@pytest.mark.parametrize("case", PHOTO_MK, ids=srm.case_id)
def test_checked_containers(hc, gpu, case):
    name, adapt, w, seg, diff, check = case
    raw, good, f, rs = srm.built(case)
    flip = next(x for x in cases.SILENT_FLIPS if (x[0], x[2]) == (name, adapt))
    flipped = cases.flip(good, 1, flip[5], flip[6])  # segment 1 decodes cleanly, to its length, to other bytes
    assert scm.decode(flipped) == (hc.HC_ERR_SEG_CHECK, 1, b"")
    for spans in ([EDGES], [(4097, 3)], [(5000, 1), (8191, 2)]):  # segment 1 decoded
        patches = sup.fill(spans, "random")
        want = sup.update(flipped, patches)
        assert want == (hc.HC_ERR_SEG_CHECK, 1, b"", 0)
        both(hc, gpu, flipped, patches, want)
    for spans in ([(4096, 4096)], [(0, 12800)], [(8192, 100)], [(1, 4095)]):  # covered whole, or not covered
        patches = sup.fill(spans, "random")
        want = sup.update(flipped, patches)
        assert want[0] == 0
        both(hc, gpu, flipped, patches, want)
    # the new crc words are those of the new raw bytes
    patches = sup.fill([EDGES], "zero")
    want = sup.update(good, patches)
    assert scm.parse(want[2])[2] == scm.parse(scm.build(sup.patched(raw, patches), diff, adapt, w, seg, check=True))[2]
    both(hc, gpu, good, patches, want)


@pytest.mark.parametrize("case", MUTANT_CASES, ids=srm.case_id)
def test_container_mutants(hc, gpu, case):
    raw, good, f, rs = srm.built(case)
    assert f["n_segments"] == 4
    st, info = hc.seg_info(good)
    index = srm.index_mutants(good)
    sets = sup.patch_sets(case)
    assert sets["none"] == [] and [(0, 0)] in sets.values() and [(0, len(raw))] in sets.values()
    for spans in sets.values():  # every patch set, the empty one included
        patches = sup.fill(spans, "random")
        for name, bad in list(seg_model.header_mutants(good).items()) + list(index.items()):
            want = sup.update(bad, patches)
            assert want == (hc.HC_ERR_SEG_HEADER, NO_SEG, b"", 0), name
            st, n, k, out, clean = dev_update(hc, gpu, bad, patches, out_cap=2 * len(good))
            assert (st, n, k) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG) and clean and out == b"\xa5" * len(out), name
            assert hc.seg_update(bad, patches, full=True, cap=2 * len(good)) == (hc.HC_ERR_SEG_HEADER, b"", 0, NO_SEG), name
        # index mutants whose header is intact: the same verdict with the caller's own (valid) info
        for name in ("enc_len_wraps", "enc_len_longer", "enc_len_shorter"):
            st, n, k, out, clean = dev_update(hc, gpu, index[name], patches, info=info)
            assert (st, n, k) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG) and clean and out == b"\xa5" * len(out), name
        # an info that is valid for this length but is not what the device bytes say
        other = hc.seg_info(good)[1]
        other.flags ^= hc.HC_FLAG_DIFF
        st, n, k, out, clean = dev_update(hc, gpu, good, patches, info=other)
        assert (st, n, k) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG) and clean and out == b"\xa5" * len(out)


@pytest.mark.parametrize("case", PHOTO_M + [BIG_CASE, ("rng:4:304", True, 16, 128, True, False)], ids=srm.case_id)
def test_capacity(hc, gpu, case):
    raw, c, f, rs = srm.built(case)
    st, info = hc.seg_info(c)
    sets = sup.patch_sets(case)
    for sname in [s for s in ("none", "first_and_last", "range_0_1", f"range_0_{len(raw)}") if s in sets]:
        for kind in sup.KINDS:
            patches = sup.fill(sets[sname], kind)
            want = sup.update(c, patches)
            m = want[3]
            # one byte short: the needed length, and nothing written at all
            assert sup.update(c, patches, out_cap=m - 1) == (hc.HC_ERR_CAPACITY, NO_SEG, b"", m)
            st, n, bad, out, clean = dev_update(hc, gpu, c, patches, out_cap=m - 1)
            assert (st, n, bad) == (hc.HC_ERR_CAPACITY, m, NO_SEG) and clean and out == b"\xa5" * (m - 1), (sname, kind)
            assert hc.seg_update(c, patches, full=True, cap=m - 1) == (hc.HC_ERR_CAPACITY, b"", m, NO_SEG), (sname, kind)
            # exactly the length
            st, n, bad, out, clean = dev_update(hc, gpu, c, patches, out_cap=m)
            assert (st, n, bad, out) == (0, m, NO_SEG, want[2]) and clean, (sname, kind)
            assert hc.seg_update(c, patches, full=True, cap=m) == (0, want[2], m, NO_SEG), (sname, kind)
            # hc_seg_update_bound (dev_update's and seg_update's default)
            assert m <= hc.seg_update_bound(info, len(c), sup.triples(patches)[0])
            both(hc, gpu, c, patches, want)


@pytest.mark.parametrize("case", [c for c in srm.CASES if c[4] and c[0] != "rng:256:0"], ids=srm.case_id)
def test_work_bound(hc, gpu, case):
    raw, c, f, rs = srm.built(case)
    st, info = hc.seg_info(c)
    sets = sup.patch_sets(case)
    for sname in [s for s in ("none", "range_0_1", f"range_0_{len(raw)}", "meet_on_cut", "first_and_last", "many_small")
                  if s in sets]:
        patches = sup.fill(sets[sname], "random")
        want = sup.update(c, patches)
        tri = [(o, m, s + 1) for o, m, s in sup.triples(patches)[0]]
        need = hc.seg_update_work_bound(info, len(c), tri)
        assert need >= 32
        # exactly the bound is enough; a byte less is refused before any launch
        rc, st, n, bad, out, clean = dev_update(hc, gpu, c, patches, work_bytes=need)
        assert (rc, st, n, bad) == (0, 0, want[3], NO_SEG) and out[:n] == want[2] and clean, sname
        rc, st, n, bad, out, clean = dev_update(hc, gpu, c, patches, work_bytes=need - 1)
        assert (rc, st, n, bad) == (hc.HC_ERR_ARG, -1, -1, 7) and out == b"\xa5" * len(out) and clean, sname


def test_work_bound_follows_the_patches(hc, gpu):
    raw, c, f, rs = srm.built((f"rng:256:{srm.BIG}", False, 512, 16, False, False))
    L = hc.lib()
    st, info = hc.seg_info(c)
    bound = lambda tri: hc.seg_update_work_bound(info, len(c), tri)
    one, whole = bound([(16, 16, 0)]), bound([(0, len(raw), 0)])
    assert one < whole
    assert one < int(L.hc_seg_decompress_work_bound(ctypes.byref(info), len(c))) + len(raw)
    # not with n: a segment of 16 bytes costs a few hundred bytes of arrays, its staging and its slot
    assert one <= 1024 + hc.compress_bound(16)
    assert bound([]) < one < bound([(16, 16, 0), (64, 1, 0)]) < whole


@pytest.mark.parametrize("case", MUTANT_CASES, ids=srm.case_id)
def test_argument_errors(hc, gpu, case):
    raw, good, f, rs = srm.built(case)
    st, info = hc.seg_info(good)
    data = bytes(64)
    L = hc.lib()
    inp = _upload(gpu, good)
    pd = _upload(gpu, data)
    out = gpu.full((4 * len(good) + 4096,), 0xA5, dtype=gpu.uint8, device="cuda")
    res = gpu.full((4,), -1, dtype=gpu.int64, device="cuda")
    work = gpu.empty((1 << 20,), dtype=gpu.uint8, device="cuda")
    stream = ctypes.c_void_p(gpu.cuda.current_stream().cuda_stream)

    def call(tri, inp_ptr=None, out_ptr=None, work_ptr=None, cap=None):
        rc = L.hc_seg_update_dev(inp.data_ptr() if inp_ptr is None else inp_ptr, len(good), ctypes.byref(info),
                                 hc.seg_patches(tri), len(tri), pd.data_ptr(), len(data),
                                 out.data_ptr() if out_ptr is None else out_ptr, out.numel() if cap is None else cap,
                                 res.data_ptr(), res.data_ptr() + 8, res.data_ptr() + 16,
                                 work.data_ptr() if work_ptr is None else work_ptr, work.numel() - 16, stream)
        gpu.cuda.synchronize()
        untouched = bool((out == 0xA5).all().item()) and bool((res == -1).all().item())
        return rc, untouched

    lists = {
        "unsorted": [(8, 2, 0), (0, 2, 2)],
        "overlap": [(0, 4, 0), (3, 2, 4)],
        "outside_raw_len": [(len(raw), 1, 0)],
        "length_wraps": [(1, 2**64 - 1, 0)],
        "src_past_data": [(0, 8, 57)],
        "src_wraps": [(0, 1, 2**64 - 1)],
    }
    for name, tri in lists.items():
        assert call(tri) == (hc.HC_ERR_ARG, True), name
        patches = [(o, bytes(min(m, 8))) for o, m, s in tri]
        if name in ("unsorted", "overlap"):
            assert hc.seg_update(good, patches, full=True, cap=4096) == (hc.HC_ERR_ARG, b"", 0, NO_SEG), name
    ok = [(5, 40, 3)]
    assert call(ok, inp_ptr=inp.data_ptr() + 8) == (hc.HC_ERR_ARG, True)
    assert call(ok, out_ptr=out.data_ptr() + 4) == (hc.HC_ERR_ARG, True)
    assert call(ok, work_ptr=work.data_ptr() + 8) == (hc.HC_ERR_ARG, True)
    assert call(ok, out_ptr=inp.data_ptr() + 16, cap=16) == (hc.HC_ERR_ARG, True)   # out inside in
    # and the same list is fine with its arguments in order
    rc, untouched = call(ok)
    assert rc == 0 and not untouched and res.cpu().numpy()[1].astype(np.int32) == 0


def test_batch_cli(hc, gpu, tmp_path):
    raw = cases.raw("photo:64:200")
    good = scm.build(raw, True, False, 512, 4096, check=True)
    (tmp_path / "a.huf").write_bytes(good)
    (tmp_path / "b.huf").write_bytes(good)
    patches = sup.fill([(1, 2), (4100, 8192)], "random")
    for k, (o, b) in enumerate(patches):
        (tmp_path / f"p{k}").write_bytes(b)
    want = sup.update(good, patches)[2]
    # several -u in any order, several files; FILE itself is never touched
    r = subprocess.run([hc.BATCH_CLI_PATH, "-u", f"4100:{tmp_path / 'p1'}", "-u", f"1:{tmp_path / 'p0'}",
                        str(tmp_path / "a.huf"), str(tmp_path / "b.huf")], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "a.huf.upd").read_bytes() == want == (tmp_path / "b.huf.upd").read_bytes()
    assert (tmp_path / "a.huf").read_bytes() == good
    os.mkdir(tmp_path / "o")
    r = subprocess.run([hc.BATCH_CLI_PATH, "-u", f"1:{tmp_path / 'p0'}", "-o", str(tmp_path / "o"), str(tmp_path / "a.huf")],
                       capture_output=True)
    assert r.returncode == 0 and (tmp_path / "o" / "a.huf.upd").read_bytes() == sup.update(good, patches[:1])[2]
    # a plain stream is no container; the container beside it is still written
    st, stream = hc.compress(raw[:5000], True)
    (tmp_path / "p.huf").write_bytes(stream)
    os.remove(tmp_path / "a.huf.upd")
    r = subprocess.run([hc.BATCH_CLI_PATH, "-u", f"1:{tmp_path / 'p0'}", str(tmp_path / "p.huf"), str(tmp_path / "a.huf")],
                       capture_output=True)
    assert r.returncode == hc.HC_ERR_UNSUPPORTED == 65 and b"p.huf: -u needs a segmented container\n" in r.stderr
    assert not os.path.exists(tmp_path / "p.huf.upd") and os.path.exists(tmp_path / "a.huf.upd")
    # overlapping patches, and one past the end
    for args in (["-u", f"1:{tmp_path / 'p0'}", "-u", f"2:{tmp_path / 'p0'}"], ["-u", f"12799:{tmp_path / 'p0'}"]):
        os.remove(tmp_path / "a.huf.upd")
        r = subprocess.run([hc.BATCH_CLI_PATH] + args + [str(tmp_path / "a.huf")], capture_output=True)
        assert r.returncode == hc.HC_ERR_ARG == 71 and not os.path.exists(tmp_path / "a.huf.upd")
        (tmp_path / "a.huf.upd").write_bytes(b"")
    # a damaged segment that must be decoded is named; one that is overwritten whole is repaired
    streams = scm.segments(good)
    (tmp_path / "bad.huf").write_bytes(scm.repack(good, streams[:2] + [streams[2][:8]] + streams[3:]))
    r = subprocess.run([hc.BATCH_CLI_PATH, "-u", f"8200:{tmp_path / 'p0'}", str(tmp_path / "bad.huf")], capture_output=True)
    assert r.returncode == 8 and b"bad.huf: segment 2: ERROR: invalid or missing Huffman coding header" in r.stderr
    (tmp_path / "seg2").write_bytes(bytes(4096))
    r = subprocess.run([hc.BATCH_CLI_PATH, "-u", f"8192:{tmp_path / 'seg2'}", str(tmp_path / "bad.huf")], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert hc.seg_decompress((tmp_path / "bad.huf.upd").read_bytes()) == (0, raw[:8192] + bytes(4096) + raw[12288:])

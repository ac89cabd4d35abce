"""List read of the segmented container on the GPU: hc_seg_decompress_ranges (host buffers, the
compact upload) and hc_seg_decompress_ranges_dev against the read model (tests/seg_reads_model.py:
the oracle on every covered segment once, the documented precedence). The device call writes into
a 16-byte-offset view of a 0xA5 buffer: the guards around it and the gaps between the destination
ranges must still be 0xA5 afterwards."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gpu_batch
import seg_check_cases as cases
import seg_check_model as scm
import seg_model
import seg_range_model as srm
import seg_reads_model as srd

pytestmark = pytest.mark.gpu

NO_SEG = srm.NO_SEGMENT
FRONT, GUARD = 16, 64  # 0xA5 bytes in front of out[0] and behind out[out_cap]
A5 = b"\xa5"
MUTANT_CASES = [("rng:256:100", False, 512, 32, True, False), ("rng:4:560", True, 16, 128, False, False)]
PHOTO = [c for c in srm.CASES if c[0] == "photo:64:200"]
PHOTO_M = [c for c in PHOTO if c[4]]
PHOTO_MK = [c for c in PHOTO_M if c[5]]
BIG_CASES = [(f"rng:256:{srm.BIG}", False, 512, 16, True, k) for k in (False, True)]
LEFTOVER = ("rng:4:304", True, 16, 128, True, False)
# x, y, w, h at pitch 64: 150 reads, unaligned sources and destinations; rows 3 .. 152 end at byte 9792, in the
# third of the four 4096-byte segments
RECT = (5, 3, 20, 150)
# segments 1 and 3, named in reverse destination order; segment 2 between them is not covered
TWO = [(4100, 8, 40), (12300, 20, 3)]


def _upload(torch, data):
    host = np.zeros(gpu_batch.align(max(len(data), 1)), dtype=np.uint8)
    host[:len(data)] = np.frombuffer(bytes(data), dtype=np.uint8)
    return torch.from_numpy(host).cuda()


def dev_reads(hc, torch, container, reads, out_cap=None, info=None, work_bytes=None, room=None, graph=False):
    """hc_seg_decompress_ranges_dev into a 16-byte-offset view of a 0xA5 buffer of `room` bytes
    (default: out_cap; out_cap default: need) -> (status, out_len, bad_segment, out[:room], every
    byte around it is still 0xA5). work_bytes: through ctypes with a workspace of exactly that many
    bytes and 64 guard bytes behind it, the return value first and the guard's state last.
    graph: captured with torch.cuda.graph and replayed once."""
    inp = _upload(torch, container)
    if out_cap is None:
        out_cap = srd.need(reads)
    if room is None:
        room = out_cap
    backing = torch.full((FRONT + room + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = backing[FRONT:]
    olen = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    bad = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    rc = wguard = None
    if work_bytes is not None:
        if info is None:
            info = hc.seg_info(container)[1]
        size = gpu_batch.align(max(work_bytes, 16))
        work = torch.full((size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        rc = hc.lib().hc_seg_decompress_ranges_dev(inp.data_ptr(), len(container), ctypes.byref(info), hc.seg_reads(reads),
                                                   len(reads), out.data_ptr(), out_cap, olen.data_ptr(), st.data_ptr(),
                                                   bad.data_ptr(), work.data_ptr(), work_bytes,
                                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        wguard = work[work_bytes:].cpu().numpy().tobytes() == A5 * (size + GUARD - work_bytes)
    elif graph:
        if info is None:
            info = hc.seg_info(container)[1]
        work = torch.empty(max(hc.seg_decompress_ranges_work_bound(info, len(container), reads), 16), dtype=torch.uint8,
                           device="cuda")
        # warm up outside the capture (library init, lazy module loads), then wipe what that call wrote
        hc.seg_decompress_ranges_dev(inp, reads, out, olen, st, bad_segment=bad, info=info, in_len=len(container),
                                     out_cap=out_cap, work=work)
        torch.cuda.synchronize()
        backing.fill_(0xA5)
        work.fill_(0)
        olen.fill_(-1)
        bad.fill_(7)
        st.fill_(-1)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            hc.seg_decompress_ranges_dev(inp, reads, out, olen, st, bad_segment=bad, info=info, in_len=len(container),
                                         out_cap=out_cap, work=work, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert int(st.item()) == -1 and backing.cpu().numpy().tobytes() == A5 * len(backing)  # captured, not run
        g.replay()
    else:
        hc.seg_decompress_ranges_dev(inp, reads, out, olen, st, bad_segment=bad, info=info, in_len=len(container),
                                     out_cap=out_cap)
    torch.cuda.synchronize()
    got = backing.cpu().numpy().tobytes()
    clean = got[:FRONT] == A5 * FRONT and got[FRONT + room:] == A5 * GUARD
    res = (int(st.item()), int(olen.item()), int(bad.item()) % 2**64, got[FRONT:FRONT + room], clean)
    return (rc,) + res + (wguard,) if work_bytes is not None else res


def both(hc, torch, container, reads, want=None):
    """the device and the host call against the model's (status, bad_segment, bytes, out_len): on
    HC_OK every destination range holds its bytes and every gap is still 0xA5, on the device and on the
    host; the guards are intact whatever the status. Returns the model's answer."""
    if want is None:
        want = srd.decode_reads(container, reads)
    wst, wbad, wbytes, wlen = want
    st, n, bad, out, clean = dev_reads(hc, torch, container, reads)
    assert clean
    assert (st, n, bad) == (wst, wlen, wbad)
    if st == 0:
        assert out == wbytes
    assert hc.seg_decompress_ranges(container, reads, full=True, fill=srd.FILL) == (wst, wbytes, wlen, wbad)
    return want


@pytest.mark.parametrize("case", srm.CASES, ids=srm.case_id)
def test_matches_model(hc, gpu, case):
    raw, c, f, rs = srm.built(case)
    for sname, reads in srd.read_sets(case).items():
        want = both(hc, gpu, c, reads)
        assert want[0] == 0 and want[3] == srd.need(reads), sname
        for o, m, d in reads:
            assert want[2][d:d + m] == raw[o:o + m], sname
        if len(reads) == 1 and reads[0][2] == 0:
            # the one-read list is the ranged read, host and device, in all four outputs
            o, m, d = reads[0]
            assert hc.seg_decompress_ranges(c, reads, full=True) == hc.seg_decompress_range(c, o, m, full=True), sname
            inp = _upload(gpu, c)
            res = []
            for call in (lambda *a, **k: hc.seg_decompress_range_dev(*a, o, m, **k),
                         lambda i, *a, **k: hc.seg_decompress_ranges_dev(i, reads, *a, **k)):
                out = gpu.full((m + GUARD,), 0xA5, dtype=gpu.uint8, device="cuda")
                meta = [gpu.full((1,), -1, dtype=dt, device="cuda") for dt in (gpu.int64, gpu.int32, gpu.int64)]
                call(inp, out, meta[0], meta[1], bad_segment=meta[2], in_len=len(c), out_cap=m)
                gpu.cuda.synchronize()
                res.append((out.cpu().numpy().tobytes(), [int(t.item()) for t in meta]))
            assert res[0] == res[1], sname


def test_leftover_rows(hc, gpu):
    """width 16, seg_bytes 128, 19 rows: band 1 took three leftover rows (last > full), and offsets at
    and past n full belong to it"""
    raw, c, f, rs = srm.built(LEFTOVER)
    assert f["cuts"] == [(0, 128), (128, 176)]
    for reads in ([(257, 46, 0)], [(300, 4, 0)], [(123, 9, 40), (255, 3, 1)], [(0, 3, 100), (257, 46, 0)],
                  [(120, 184, 7), (256, 48, 200), (303, 1, 0)]):
        want = both(hc, gpu, c, reads)
        assert want[0] == 0
        for o, m, d in reads:
            assert want[2][d:d + m] == raw[o:o + m], reads


@pytest.mark.parametrize("case", PHOTO, ids=srm.case_id)
def test_rectangle(hc, gpu, case, tmp_path):
    name, adapt, w, seg, diff, check = case
    raw, c, f, rs = srm.built(case)
    x, y, rw, rh = RECT
    st, reads = hc.seg_rect_reads(len(raw), 64, x, y, rw, rh)
    assert st == 0 and reads == srd.rect_reads(len(raw), 64, x, y, rw, rh) and len(reads) == 150
    assert srd.covered(f, reads) == [0, 1, 2]
    tile = np.frombuffer(raw, dtype=np.uint8).reshape(200, 64)[y:y + rh, x:x + rw].tobytes()
    want = both(hc, gpu, c, reads)
    assert want == (0, NO_SEG, tile, rw * rh)
    # the batch CLI: the adaptive container's own width is the pitch, the plain one's comes from -w
    (tmp_path / "a.bin.huf").write_bytes(c)
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d", "-R", "5:3:20:150"] + ([] if adapt else ["-w", "64"])
                       + [str(tmp_path / "a.bin.huf")], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "a.bin").read_bytes() == tile


def test_batch_cli(hc, gpu, tmp_path):
    raw = cases.raw("photo:64:200")
    good = scm.build(raw, True, False, 512, 4096, check=True)
    img = np.frombuffer(raw, dtype=np.uint8).reshape(200, 64)
    (tmp_path / "a.bin.huf").write_bytes(good)
    (tmp_path / "b.huf").write_bytes(good)
    os.mkdir(tmp_path / "o")
    for x, y, w, h in ((0, 0, 64, 200), (63, 199, 1, 1), (7, 100, 0, 5), (7, 100, 5, 0)):
        r = subprocess.run([hc.BATCH_CLI_PATH, "-d", "-w", "64", "-R", f"{x}:{y}:{w}:{h}", "-o", str(tmp_path / "o"),
                            str(tmp_path / "a.bin.huf"), str(tmp_path / "b.huf")], capture_output=True)
        assert r.returncode == 0, r.stderr
        tile = img[y:y + h, x:x + w].tobytes()
        assert (tmp_path / "o" / "a.bin").read_bytes() == tile == (tmp_path / "o" / "b").read_bytes(), (x, y, w, h)
    # -r keeps its behaviour
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d", "-r", "4100:8192", str(tmp_path / "a.bin.huf")], capture_output=True)
    assert r.returncode == 0 and (tmp_path / "a.bin").read_bytes() == raw[4100:4100 + 8192]
    os.remove(tmp_path / "a.bin")
    # a damaged covered segment is named by its container index; one that holds no row is not noticed
    streams = scm.segments(good)
    (tmp_path / "bad.huf").write_bytes(scm.repack(good, streams[:2] + [streams[2][:8]] + streams[3:]))
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d", "-w", "64", "-R", "5:60:20:100", str(tmp_path / "bad.huf")],
                       capture_output=True)
    assert r.returncode == 8 and b"bad.huf: segment 2: ERROR: invalid or missing Huffman coding header" in r.stderr
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d", "-w", "64", "-R", "5:3:20:100", str(tmp_path / "bad.huf")],
                       capture_output=True)
    assert r.returncode == 0 and (tmp_path / "bad").read_bytes() == img[3:103, 5:25].tobytes()


@pytest.mark.parametrize("case", BIG_CASES, ids=srm.case_id)
def test_large_counts(hc, gpu, case):
    """more than one descriptor chunk and more than one scan tile: 1025 one-byte reads, every other
    segment of 2050; and 200 reads that all name segment 1021"""
    raw, c, f, rs = srm.built(case)
    st, info = hc.seg_info(c)
    reads = [(32 * i + 3, 1, 2 * (1024 - i)) for i in range(1025)]  # destinations in reverse order, a gap after each
    assert srd.covered(f, reads) == list(range(0, 2050, 2))
    assert hc.seg_reads_segments(info, len(c), reads) == (0, 1025, 2049)
    want = both(hc, gpu, c, reads)
    assert want[0] == 0 and want[2][0::2] == bytes(raw[32 * i + 3] for i in reversed(range(1025)))
    assert want[2][1::2] == A5 * 1024
    many = [(16 * 1021 + (i % 13), 3, 4 * i) for i in sorted(range(200), key=lambda i: i % 13)]
    # C == 1 through the work bound: 200 records, and the arrays, the staging and the crc of ONE segment
    assert hc.seg_decompress_ranges_work_bound(info, len(c), many) == 9600 + 3 * 1600 + 6 * 16 + 16 + 16 + 16 \
        + (16 if case[5] else 0)
    want = both(hc, gpu, c, many)
    assert want[0] == 0 and all(want[2][4 * i:4 * i + 3] == raw[16 * 1021 + i % 13:][:3] for i in range(200))
    # a damaged segment among the 1025, past the first scan tile and the first chunks; its neighbour is not covered
    streams = scm.segments(c)
    for k, covered in ((2046, True), (2047, False)):
        bad = scm.repack(c, streams[:k] + [streams[k][:1]] + streams[k + 1:])
        want = both(hc, gpu, bad, reads)
        assert (want[0] != 0, want[1]) == (covered, 2046 if covered else NO_SEG)


@pytest.mark.parametrize("case", PHOTO_M, ids=srm.case_id)
def test_damage(hc, gpu, case):
    import oracle
    name, adapt, w, seg, diff, check = case
    raw, good, f, rs = srm.built(case)
    streams = scm.segments(good)
    assert len(streams) == 4 and srd.covered(f, TWO) == [1, 3]
    st, short = oracle.compress(raw[:1024], diff, adapt, w)  # a valid stream of another length than any cut
    assert st == 0

    def cut(k):
        return streams[k][:len(streams[k]) // 2]

    def damaged(repl):
        return scm.repack(good, [repl.get(k, s) for k, s in enumerate(streams)])

    for repl in (cut, lambda k: short):  # the coder's own status (8 or 9), and HC_ERR_SEG_SIZE
        for bad_in, want_bad in (({1: repl(1)}, 1), ({3: repl(3)}, 3), ({1: repl(1), 3: cut(3)}, 1),
                                 ({3: repl(3), 1: cut(1)}, 1), ({0: repl(0), 3: repl(3)}, 3), ({2: repl(2), 3: cut(3)}, 3)):
            want = both(hc, gpu, damaged(bad_in), TWO)
            assert want[0] != 0 and want[1:] == (want_bad, b"", 0)
        assert srd.decode_reads(damaged({1: repl(1)}), TWO)[0] in ((8, 9) if repl is cut else (hc.HC_ERR_SEG_SIZE,))
        # in segments that no read covers: not noticed
        want = both(hc, gpu, damaged({0: repl(0), 2: repl(2)}), TWO)
        assert want == (0, NO_SEG, want[2], 48) and want[2][40:48] == raw[4100:4108] and want[2][3:23] == raw[12300:12320]
        # every list of a damaged container whose reads stay off the damage
        assert both(hc, gpu, damaged({2: repl(2)}), [])[0] == 0
        assert both(hc, gpu, damaged({2: repl(2)}), [(8192, 0, 0), (12288, 0, 9)])[0] == 0
        assert both(hc, gpu, damaged({2: repl(2)}), [(8191, 2, 0)])[:2] == (srd.decode_reads(damaged({2: repl(2)}), [(8191, 2, 0)])[0], 2)


@pytest.mark.parametrize("case", PHOTO_MK, ids=srm.case_id)
def test_checked_containers(hc, gpu, case):
    name, adapt, w, seg, diff, check = case
    raw, good, f, rs = srm.built(case)
    flip = next(x for x in cases.SILENT_FLIPS if (x[0], x[2]) == (name, adapt))
    flipped = cases.flip(good, 1, flip[5], flip[6])  # segment 1 decodes cleanly, to its length, to other bytes
    assert scm.decode(flipped) == (hc.HC_ERR_SEG_CHECK, 1, b"")
    for reads in (TWO, [(4097, 3, 0)], [(0, 1, 9), (8191, 2, 0)], [(0, 12800, 0)], [(5000, 1, 1), (5000, 1, 0)]):
        assert both(hc, gpu, flipped, reads) == (hc.HC_ERR_SEG_CHECK, 1, b"", 0), reads
    for reads in ([(0, 4096, 0), (8192, 100, 5000)], [(4095, 1, 0)], [(4096, 0, 0)]):  # segment 1 not covered
        assert both(hc, gpu, flipped, reads)[0] == 0, reads
    # two forged crc words, named in reverse destination order: the lower segment
    n = f["n_segments"]
    two = bytearray(good)
    for k in (1, 3):
        two[48 + 8 * n + 4 * k] ^= 0x80
    assert both(hc, gpu, bytes(two), TWO) == (hc.HC_ERR_SEG_CHECK, 1, b"", 0)
    assert both(hc, gpu, bytes(two), TWO[1:]) == (hc.HC_ERR_SEG_CHECK, 3, b"", 0)
    assert both(hc, gpu, bytes(two), [(0, 4096, 0), (8192, 4096, 4096)])[0] == 0


@pytest.mark.parametrize("case", MUTANT_CASES, ids=srm.case_id)
def test_container_mutants(hc, gpu, case):
    raw, good, f, rs = srm.built(case)
    assert f["n_segments"] == 4
    st, info = hc.seg_info(good)
    index = srm.index_mutants(good)
    sets = srd.read_sets(case)
    assert sets["none"] == [] and "empties" in sets and "skip_one" in sets
    for sname, reads in sets.items():  # every list, the empty one included
        room = srd.need(reads)
        for name, bad in list(seg_model.header_mutants(good).items()) + list(index.items()):
            want = srd.decode_reads(bad, reads)
            assert want == (hc.HC_ERR_SEG_HEADER, NO_SEG, b"", 0), name
            st, n, k, out, clean = dev_reads(hc, gpu, bad, reads)
            assert (st, n, k) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG) and clean and out == A5 * room, (sname, name)
            assert hc.seg_decompress_ranges(bad, reads, full=True, cap=room) == (hc.HC_ERR_SEG_HEADER, b"", 0, NO_SEG), name
        # index mutants whose header is intact: the same verdict with the caller's own (valid) info
        for name in ("enc_len_wraps", "enc_len_longer", "enc_len_shorter"):
            st, n, k, out, clean = dev_reads(hc, gpu, index[name], reads, info=info)
            assert (st, n, k) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG) and clean and out == A5 * room, (sname, name)
        # an info that is valid for this length but is not what the device bytes say
        other = hc.seg_info(good)[1]
        other.flags ^= hc.HC_FLAG_DIFF
        st, n, k, out, clean = dev_reads(hc, gpu, good, reads, info=other)
        assert (st, n, k) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG) and clean and out == A5 * room, sname
    # the index's verdict comes before the capacity's
    st, n, k, out, clean = dev_reads(hc, gpu, index["enc_len_longer"], sets["skip_one"], out_cap=1, room=64, info=info)
    assert (st, n, k) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG) and clean and out == A5 * 64
    # a list that fails its rules: the argument error of both calls
    assert hc.seg_decompress_ranges(good, [(len(raw), 1, 0)], cap=8)[0] == hc.HC_ERR_ARG
    assert hc.seg_decompress_ranges(good, [(4, 1, 0), (3, 1, 1)], cap=8)[0] == hc.HC_ERR_ARG
    with pytest.raises(hc.HCodecError):
        dev_reads(hc, gpu, good, [(4, 1, 0), (3, 1, 1)])


@pytest.mark.parametrize("case", PHOTO_M + BIG_CASES[:1] + [LEFTOVER], ids=srm.case_id)
def test_capacity(hc, gpu, case):
    raw, c, f, rs = srm.built(case)
    for sname, reads in srd.read_sets(case).items():
        m = srd.need(reads)
        if m == 0 or m > 2**32:
            continue
        want = srd.decode_reads(c, reads)
        # one byte short: the needed length, and nothing written at all, not even where there is room
        assert srd.decode_reads(c, reads, out_cap=m - 1) == (hc.HC_ERR_CAPACITY, NO_SEG, b"", m)
        st, n, bad, out, clean = dev_reads(hc, gpu, c, reads, out_cap=m - 1, room=m)
        assert (st, n, bad) == (hc.HC_ERR_CAPACITY, m, NO_SEG) and clean and out == A5 * m, sname
        assert hc.seg_decompress_ranges(c, reads, full=True, cap=m - 1) == (hc.HC_ERR_CAPACITY, b"", m, NO_SEG), sname
        # more room than the reads reach: only the destination ranges are written
        st, n, bad, out, clean = dev_reads(hc, gpu, c, reads, out_cap=m + 9, room=m + 9)
        assert (st, n, bad, out) == (0, m, NO_SEG, want[2] + A5 * 9) and clean, sname
        assert hc.seg_decompress_ranges(c, reads, full=True, cap=m + 9, fill=srd.FILL) == (0, want[2], m, NO_SEG), sname


@pytest.mark.parametrize("case", [c for c in srm.CASES if c[4] and c[0] != "rng:256:0"] + BIG_CASES[1:], ids=srm.case_id)
def test_work_bound(hc, gpu, case):
    raw, c, f, rs = srm.built(case)
    st, info = hc.seg_info(c)
    sets = srd.read_sets(case)
    names = ("none", "range_0_1", f"range_0_{len(raw)}", "overlap", "first_and_last", "skip_one", "leftover_rows")
    for sname in [s for s in names if s in sets]:
        reads = sets[sname]
        want = srd.decode_reads(c, reads)
        need = hc.seg_decompress_ranges_work_bound(info, len(c), reads)
        assert need >= 16
        # exactly the bound is enough, and no byte behind it is touched; a byte less is refused before any launch
        rc, st, n, bad, out, clean, wguard = dev_reads(hc, gpu, c, reads, work_bytes=need)
        assert (rc, st, n, bad, out) == (0, 0, want[3], NO_SEG, want[2]) and clean and wguard, sname
        rc, st, n, bad, out, clean, wguard = dev_reads(hc, gpu, c, reads, work_bytes=need - 1)
        assert (rc, st, n, bad) == (hc.HC_ERR_ARG, -1, -1, 7) and out == A5 * len(out) and clean and wguard, sname


@pytest.mark.parametrize("case", PHOTO_MK, ids=srm.case_id)
def test_graph_capture(hc, gpu, case):
    """one replay of the captured device call: a single chain of launches, no parallel branches"""
    raw, c, f, rs = srm.built(case)
    st, reads = hc.seg_rect_reads(len(raw), 64, *RECT)
    want = srd.decode_reads(c, reads)
    st, n, bad, out, clean = dev_reads(hc, gpu, c, reads, graph=True)
    assert (st, n, bad, out) == (0, want[3], NO_SEG, want[2]) and clean

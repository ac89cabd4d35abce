"""Append to the segmented container on the GPU: hc_seg_append (host buffers) and hc_seg_append_dev
against the append model (tests/seg_append_model.py: the oracle on the decoded and the coded
segments alone, the documented precedence), whose result for a container of this library is the
container of the concatenated raw bytes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gpu_batch
import seg_append_model as sam
import seg_check_cases as cases
import seg_check_model as scm
import seg_model
import seg_range_model as srm

pytestmark = pytest.mark.gpu

NO_SEG = srm.NO_SEGMENT
FRONT, GUARD = 16, 64  # 0xA5 bytes in front of out[0] and behind out[out_cap]
MUTANT_CASES = [("rng:256:100", False, 512, 32, True, False), ("rng:4:560", True, 16, 128, False, False)]
PHOTO_M = [c for c in srm.CASES if c[0] == "photo:64:200" and c[4]]
BIG_CASE = (f"rng:256:{srm.BIG}", False, 512, 16, True, False)


def _upload(torch, data, front=0):
    """the bytes at `front` of a zeroed device buffer whose length is a multiple of 16"""
    host = np.zeros(gpu_batch.align(front + max(len(data), 1)), dtype=np.uint8)
    host[front:front + len(data)] = np.frombuffer(bytes(data), dtype=np.uint8)
    return torch.from_numpy(host).cuda()


def dev_append(hc, torch, container, add, out_cap=None, info=None, work_bytes=None):
    """hc_seg_append_dev into a 16-byte-offset view of a 0xA5 buffer, the added bytes at an odd
    address -> (status, out_len, bad_segment, out[:out_cap], every byte around it is still 0xA5).
    work_bytes: through ctypes with a workspace of exactly that many bytes, the return value first."""
    ad = _upload(torch, add, front=1)[1:]
    inp = _upload(torch, container)
    if out_cap is None:
        st, i = hc.seg_info(container)
        out_cap = hc.seg_append_bound(i, len(container), len(add)) if st == 0 else 64
        out_cap = out_cap or 64  # (arguments that the call refuses)
    backing = torch.full((FRONT + out_cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = backing[FRONT:]
    olen = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    bad = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    rc = None
    if work_bytes is None:
        hc.seg_append_dev(inp, ad, out, olen, st, bad_segment=bad, info=info, in_len=len(container), out_cap=out_cap,
                          add_len=len(add))
    else:
        if info is None:
            info = hc.seg_info(container)[1]
        work = torch.empty(max(work_bytes, 16), dtype=torch.uint8, device="cuda")
        rc = hc.lib().hc_seg_append_dev(inp.data_ptr(), len(container), ctypes.byref(info), ad.data_ptr(), len(add),
                                        out.data_ptr(), out_cap, olen.data_ptr(), st.data_ptr(), bad.data_ptr(),
                                        work.data_ptr(), work_bytes,
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = backing.cpu().numpy().tobytes()
    clean = got[:FRONT] == b"\xa5" * FRONT and got[FRONT + out_cap:] == b"\xa5" * GUARD
    res = (int(st.item()), int(olen.item()), int(bad.item()) % 2**64, got[FRONT:FRONT + out_cap], clean)
    return (rc,) + res if work_bytes is not None else res


def both(hc, torch, container, add, want):
    """the device and the host call against the model's (status, bad_segment, bytes, out_len); on
    a non-zero status the device output is untouched; the guards are intact whatever the status"""
    wst, wbad, wbytes, wlen = want
    st, n, bad, out, clean = dev_append(hc, torch, container, add)
    assert clean
    assert (st, n, bad) == (wst, wlen, wbad)
    if st == 0:
        assert out[:n] == wbytes and out[n:] == b"\xa5" * (len(out) - n)
    else:
        assert out == b"\xa5" * len(out)
    assert hc.seg_append(container, add, full=True) == (wst, wbytes, wlen, wbad)


@pytest.mark.parametrize("case", sam.CASES, ids=srm.case_id)
def test_matches_model(hc, gpu, case):
    name, adapt, w, seg, diff, check = case
    raw, c, f, rs = srm.built(case)
    for add in sam.add_lengths(case):
        t = sam.add_bytes(add)
        want = sam.append(c, t)
        assert want[0] == 0, add
        both(hc, gpu, c, t, want)
        assert hc.seg_compress(raw + t, diff, adapt, w, seg, check=check) == (0, want[2]), add
        assert hc.seg_decompress(want[2], full=True) == (0, raw + t, len(raw) + add, NO_SEG), add
    if adapt:  # the added bytes must be whole rows: decided on the host, nothing launched
        inp, ad = _upload(gpu, c), _upload(gpu, bytes(w + 1))
        out = gpu.full((4096,), 0xA5, dtype=gpu.uint8, device="cuda")
        olen = gpu.full((1,), -1, dtype=gpu.int64, device="cuda")
        st = gpu.full((1,), -1, dtype=gpu.int32, device="cuda")
        with pytest.raises(hc.HCodecError, match=f"failed: {hc.HC_ERR_MATRIX_SIZE}"):
            hc.seg_append_dev(inp, ad, out, olen, st, in_len=len(c), add_len=w + 1)
        gpu.cuda.synchronize()
        assert bool((out == 0xA5).all().item()) and int(olen.item()) == -1 and int(st.item()) == -1
        assert hc.seg_append(c, bytes(w + 1), full=True, cap=4096)[0] == hc.HC_ERR_MATRIX_SIZE


@pytest.mark.parametrize("check", (False, True), ids=("plain", "checked"))
def test_coded_entries_across_a_scan_tile(hc, gpu, check):
    """more coded segments than the seal scans in one tile, behind a decoded open tail of one byte;
    the device call and the host call (which gathers the coded streams alone)"""
    case = ("rng:256:17", False, 512, 16, False, check)
    name, adapt, w, seg, diff, check = case
    raw, c, f, rs = srm.built(case)
    t = sam.add_bytes(16 * 1030)
    st, K, new, dec = sam.plan(f, len(t))
    assert (st, K, dec) == (0, 1, 1) and len(new) - K == 1031 > 1024
    want = sam.append(c, t)
    assert want[0] == 0
    both(hc, gpu, c, t, want)
    assert hc.seg_compress(raw + t, diff, adapt, w, seg, check=check) == (0, want[2])


def test_chain(hc, gpu):
    """three appends of unequal lengths from the empty container: one ends inside a segment, one on
    a cut, one spans three segments; the result is one seg_compress of the concatenation"""
    for diff, check in ((False, False), (True, True)):
        parts = [sam.add_bytes(40, seed=s) for s in (1, 2, 3)]
        parts = [parts[0][:21], parts[1][:11], parts[2][:37]]   # 21 (mid-segment), 32 (on a cut), 69 (three more)
        st, host = hc.seg_compress(b"", diff, False, 512, 16, check=check)
        assert st == 0
        dev, so_far = host, b""
        for t in parts:
            so_far += t
            st, host = hc.seg_append(host, t)
            assert st == 0
            st, n, bad, out, clean = dev_append(hc, gpu, dev, t)
            assert (st, bad, clean) == (0, NO_SEG, True)
            dev = out[:n]
            assert host == dev == hc.seg_compress(so_far, diff, False, 512, 16, check=check)[1]
        assert scm.parse(host)[0]["n_segments"] == 5 and hc.seg_decompress(host) == (0, so_far)


@pytest.mark.parametrize("case", PHOTO_M, ids=srm.case_id)
def test_damage(hc, gpu, case):
    import oracle
    name, adapt, w, seg, diff, check = case
    raw, good, f, rs = srm.built(case)
    streams = scm.segments(good)
    st, short = oracle.compress(raw[:1024], diff, adapt, w)  # a valid stream of another length than any cut
    assert st == 0 and len(streams) == 4
    t = sam.add_bytes(sam.add_lengths(case)[1])
    assert sam.plan(f, len(t))[1::2] == (3, 1)  # K == 3: segment 3 is decoded

    def cut(k):
        return streams[k][:len(streams[k]) // 2]

    def damaged(c, repl):
        s = scm.segments(c)
        return scm.repack(c, [repl.get(k, x) for k, x in enumerate(s)])

    for repl in (cut, lambda k: short):  # the coder's own status, and HC_ERR_SEG_SIZE
        bad = damaged(good, {3: repl(3)})
        want = sam.append(bad, t)
        assert want[0] != 0 and want[1:] == (3, b"", 0)
        assert want[0] in ((8, 9, 10, 11, 13, 14, 15) if repl is cut else (hc.HC_ERR_SEG_SIZE,))
        both(hc, gpu, bad, t, want)
        # the decoded segment decides, whatever the kept ones hold
        bad = damaged(good, {0: repl(0), 3: repl(3)})
        both(hc, gpu, bad, t, sam.append(bad, t))
        # a damaged kept segment is carried over verbatim, and the result's decoder names it
        bad = damaged(good, {1: repl(1)})
        want = sam.append(bad, t)
        assert want[0] == 0 and scm.segments(want[2])[1] == repl(1)
        both(hc, gpu, bad, t, want)
        st, _, _, k = hc.seg_decompress(want[2], full=True)
        assert st != 0 and k == 1
    if check:  # the right length, other bytes than the index's crc word says
        n = f["n_segments"]
        at = 48 + 8 * n + 4 * (n - 1)
        bad = good[:at] + bytes([good[at] ^ 1]) + good[at + 1:]
        want = sam.append(bad, t)
        assert want == (hc.HC_ERR_SEG_CHECK, 3, b"", 0)
        both(hc, gpu, bad, t, want)
    # raw_len on a cut (K == n): the old last segment is kept, so damage in it is not noticed
    whole = raw[:2 * f["cuts"][0][1]]
    c2 = scm.build(whole, diff, adapt, w, seg, check=check)
    f2 = scm.parse(c2)[0]
    t2 = sam.add_bytes(9 * w if adapt else 100)
    assert f2["n_segments"] == 2 and sam.plan(f2, len(t2))[1::2] == (2, 0)
    s2 = scm.segments(c2)
    bad = damaged(c2, {1: s2[1][:len(s2[1]) // 2]})
    want = sam.append(bad, t2)
    assert want[0] == 0 and scm.segments(want[2])[1] == s2[1][:len(s2[1]) // 2]
    both(hc, gpu, bad, t2, want)
    want = scm.build(whole + t2, diff, adapt, w, seg, check=check)
    both(hc, gpu, c2, t2, (0, NO_SEG, want, len(want)))


@pytest.mark.parametrize("case", MUTANT_CASES, ids=srm.case_id)
def test_container_mutants(hc, gpu, case):
    name, adapt, w, seg, diff, check = case
    raw, good, f, rs = srm.built(case)
    assert f["n_segments"] == 4
    st, info = hc.seg_info(good)
    index = srm.index_mutants(good)
    for add in (0, w if adapt else 1, 5 * w if adapt else 70):  # A == 0 and A > 0: the same verdict
        t = sam.add_bytes(add)
        for mname, bad in list(seg_model.header_mutants(good).items()) + list(index.items()):
            want = sam.append(bad, t)
            assert want == (hc.HC_ERR_SEG_HEADER, NO_SEG, b"", 0), mname
            st, n, k, out, clean = dev_append(hc, gpu, bad, t, out_cap=2 * len(good))
            assert (st, n, k) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG) and clean and out == b"\xa5" * len(out), mname
            assert hc.seg_append(bad, t, full=True, cap=2 * len(good)) == (hc.HC_ERR_SEG_HEADER, b"", 0, NO_SEG), mname
        # index mutants whose header is intact: the same verdict with the caller's own (valid) info
        for mname in ("enc_len_wraps", "enc_len_longer", "enc_len_shorter"):
            st, n, k, out, clean = dev_append(hc, gpu, index[mname], t, info=info)
            assert (st, n, k) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG) and clean and out == b"\xa5" * len(out), mname
        # an info that is valid for this length but is not what the device bytes say
        other = hc.seg_info(good)[1]
        other.flags ^= hc.HC_FLAG_DIFF
        st, n, k, out, clean = dev_append(hc, gpu, good, t, info=other)
        assert (st, n, k) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG) and clean and out == b"\xa5" * len(out)


@pytest.mark.parametrize("case", PHOTO_M + [BIG_CASE, ("rng:4:304", True, 16, 128, True, False)], ids=srm.case_id)
def test_capacity(hc, gpu, case):
    raw, c, f, rs = srm.built(case)
    st, info = hc.seg_info(c)
    for add in sam.add_lengths(case):
        t = sam.add_bytes(add)
        want = sam.append(c, t)
        m = want[3]
        # one byte short: the needed length, and nothing written at all
        assert sam.append(c, t, out_cap=m - 1) == (hc.HC_ERR_CAPACITY, NO_SEG, b"", m)
        st, n, bad, out, clean = dev_append(hc, gpu, c, t, out_cap=m - 1)
        assert (st, n, bad) == (hc.HC_ERR_CAPACITY, m, NO_SEG) and clean and out == b"\xa5" * (m - 1), add
        assert hc.seg_append(c, t, full=True, cap=m - 1) == (hc.HC_ERR_CAPACITY, b"", m, NO_SEG), add
        # exactly the length
        st, n, bad, out, clean = dev_append(hc, gpu, c, t, out_cap=m)
        assert (st, n, bad, out) == (0, m, NO_SEG, want[2]) and clean, add
        assert hc.seg_append(c, t, full=True, cap=m) == (0, want[2], m, NO_SEG), add
        # hc_seg_append_bound (dev_append's and seg_append's default) is never reached
        assert m < hc.seg_append_bound(info, len(c), add)


@pytest.mark.parametrize("case", [c for c in sam.CASES if (c[4] or c[5]) and c[0] != "rng:256:0"], ids=srm.case_id)
def test_work_bound(hc, gpu, case):
    raw, c, f, rs = srm.built(case)
    st, info = hc.seg_info(c)
    for add in sam.add_lengths(case):
        t = sam.add_bytes(add)
        want = sam.append(c, t)
        need = hc.seg_append_work_bound(info, len(c), add)
        assert need >= 32
        # exactly the bound is enough; 16 bytes less are refused before any launch
        rc, st, n, bad, out, clean = dev_append(hc, gpu, c, t, work_bytes=need)
        assert (rc, st, n, bad) == (0, 0, want[3], NO_SEG) and out[:n] == want[2] and clean, add
        rc, st, n, bad, out, clean = dev_append(hc, gpu, c, t, work_bytes=need - 16)
        assert (rc, st, n, bad) == (hc.HC_ERR_ARG, -1, -1, 7) and out == b"\xa5" * len(out) and clean, add


def test_batch_cli(hc, gpu, tmp_path):
    raw = cases.raw("photo:64:200")
    a = scm.build(raw, True, False, 512, 4096, check=True)
    b = scm.build(raw[:8192], False, False, 512, 4096, check=False)
    (tmp_path / "a.huf").write_bytes(a)
    (tmp_path / "b.huf").write_bytes(b)
    t = sam.add_bytes(5000)
    (tmp_path / "t").write_bytes(t)
    # two containers of different kinds in one process; FILE itself is never touched
    r = subprocess.run([hc.BATCH_CLI_PATH, "-e", str(tmp_path / "t"), str(tmp_path / "a.huf"), str(tmp_path / "b.huf")],
                       capture_output=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "a.huf.app").read_bytes() == hc.seg_compress(raw + t, True, False, 512, 4096, check=True)[1]
    assert (tmp_path / "b.huf.app").read_bytes() == hc.seg_compress(raw[:8192] + t, False, False, 512, 4096)[1]
    assert (tmp_path / "a.huf").read_bytes() == a
    os.mkdir(tmp_path / "o")
    r = subprocess.run([hc.BATCH_CLI_PATH, "-e", str(tmp_path / "t"), "-o", str(tmp_path / "o"), str(tmp_path / "b.huf")],
                       capture_output=True)
    assert r.returncode == 0 and (tmp_path / "o" / "b.huf.app").read_bytes() == (tmp_path / "b.huf.app").read_bytes()
    # a plain stream is no container; the container beside it is still written
    st, stream = hc.compress(raw[:5000], True)
    (tmp_path / "p.huf").write_bytes(stream)
    os.remove(tmp_path / "a.huf.app")
    r = subprocess.run([hc.BATCH_CLI_PATH, "-e", str(tmp_path / "t"), str(tmp_path / "p.huf"), str(tmp_path / "a.huf")],
                       capture_output=True)
    assert r.returncode == hc.HC_ERR_UNSUPPORTED == 65 and b"p.huf: -e needs a segmented container\n" in r.stderr
    assert not os.path.exists(tmp_path / "p.huf.app") and os.path.exists(tmp_path / "a.huf.app")
    # a damaged open segment is named; a bad header is the container's error
    streams = scm.segments(a)
    (tmp_path / "bad.huf").write_bytes(scm.repack(a, streams[:3] + [streams[3][:8]]))
    r = subprocess.run([hc.BATCH_CLI_PATH, "-e", str(tmp_path / "t"), str(tmp_path / "bad.huf")], capture_output=True)
    assert r.returncode == 8 and b"bad.huf: segment 3: ERROR: invalid or missing Huffman coding header" in r.stderr
    assert not os.path.exists(tmp_path / "bad.huf.app")
    (tmp_path / "cut.huf").write_bytes(a[:-1])
    r = subprocess.run([hc.BATCH_CLI_PATH, "-e", str(tmp_path / "t"), str(tmp_path / "cut.huf")], capture_output=True)
    assert r.returncode == hc.HC_ERR_SEG_HEADER == 68 and not os.path.exists(tmp_path / "cut.huf.app")

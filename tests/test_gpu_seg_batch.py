"""The batched segmented coders on the GPU (hc_seg_*_batch_dev, hc_seg_*_host_batch,
huffman-codec-batch): every item of a call against the batch model (tests/seg_batch_model.py: the
single models per item) and against the single device calls, 0xA5 guards around every output. The
shapes are the container tests' smallest: an empty segment, one byte, 17 bytes, 2050 segments
(two scan tiles), adaptive bands with leftover rows, checked and unchecked photo containers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import seg_batch_model as sbm
import seg_check_cases as cases
import seg_check_model as scm
import seg_model
import seg_range_model as srm

pytestmark = pytest.mark.gpu

NO_SEG = srm.NO_SEGMENT
WHOLE = sbm.WHOLE
GUARD = 32  # 0xA5 bytes in front of the first output and behind every one (up to the next 16-byte boundary, and these)
A5 = b"\xa5"
CHUNK = 32  # at least the larger of the implementation's descriptor chunks (32 encoder, 16 decoder items)

_models = {}


def model(name, use_diff, use_adapt, width, seg, check):
    """(raw, the model's container), built once"""
    key = (name, use_diff, use_adapt, width, seg, check)
    if key not in _models:
        raw = cases.raw(name)
        _models[key] = (raw, scm.build(raw, use_diff, use_adapt, width, seg, check=check))
    return _models[key]


def _a16(x):
    return (x + 15) & ~15


def _place(blobs):
    """distinct byte strings -> (one host buffer with each at a 16-byte offset, {id: offset})"""
    offs, at = {}, 0
    for b in blobs:
        if id(b) not in offs:
            offs[id(b)] = at
            at += _a16(len(b)) + 16
    host = np.zeros(max(at, 16), dtype=np.uint8)
    seen = set()
    for b in blobs:
        if id(b) not in seen and len(b):
            seen.add(id(b))
            host[offs[id(b)]:offs[id(b)] + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    return host, offs


def _outs(sizes):
    """out_off of every item in a buffer of 0xA5: GUARD bytes, then each output followed by GUARD bytes"""
    offs, at = [], GUARD
    for s in sizes:
        offs.append(at)
        at += _a16(s + GUARD)
    return offs, at


def _guards_intact(got, offs, sizes, total):
    edges = [(0, GUARD)] + [(o + s, offs[k + 1] if k + 1 < len(offs) else total)
                            for k, (o, s) in enumerate(zip(offs, sizes))]
    return all(got[a:b] == A5 * (b - a) for a, b in edges)


def enc_batch(hc, torch, raws, widths, caps=None, work_bytes=None, **opts):
    """seg_compress_batch_dev over host inputs -> (rc, [(status, out_len, the item's whole output
    region)], guards intact); work_bytes: a workspace of exactly that size"""
    flags = hc._seg_flags(opts.get("use_diff"), opts.get("use_adapt"), opts.get("check"))
    seg = opts.get("seg_bytes", 0)
    if caps is None:
        caps = [int(hc.lib().hc_seg_compress_bound2(len(r), seg, flags, w)) or 64 for r, w in zip(raws, widths)]
    host, in_offs = _place(raws)
    out_offs, total = _outs(caps)
    items = [(in_offs[id(r)], len(r), w, o, c) for r, w, o, c in zip(raws, widths, out_offs, caps)]
    n = len(items)
    inp = torch.from_numpy(host).cuda()
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    lens = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")[:n]
    st = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")[:n]
    arr = hc.seg_enc_items(items)
    need = int(hc.lib().hc_seg_compress_batch_work_bound(arr, n, flags, seg))
    wb = need if work_bytes is None else work_bytes
    work = torch.empty(max(wb, 16), dtype=torch.uint8, device="cuda")
    rc = hc.lib().hc_seg_compress_batch_dev(inp.data_ptr(), out.data_ptr(), arr, n, flags, seg, lens.data_ptr(),
                                            st.data_ptr(), work.data_ptr(), wb,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = out.cpu().numpy().tobytes()
    res = [(int(s), int(m), got[o:o + c]) for s, m, o, c in zip(st.tolist(), lens.tolist(), out_offs, caps)]
    return rc, res, _guards_intact(got, out_offs, caps, total), need


def check_encoded(res, want):
    """res of enc_batch against [(status, container, out_len)] of the model"""
    for k, ((st, n, region), (wst, wc, wn)) in enumerate(zip(res, want)):
        assert (st, n) == (wst, wn), k
        if st == 0:
            assert region[:n] == wc, k
        elif st != 0:  # nothing of a failed item reaches its output
            assert region == A5 * len(region), k


def dec_batch(hc, torch, specs, work_bytes=None, infos=None):
    """seg_decompress_batch_dev over (container, offset, length, out_cap or None) -> (rc, [(status,
    bad_segment, bytes, out_len)] as the model gives them, guards intact, [every byte of a failed
    item's output is still 0xA5]). The output region of an item is its `length` bytes (a whole
    item: raw_len, or out_cap when that is less); the same container is uploaded once."""
    conts = [s[0] for s in specs]
    host, in_offs = _place(conts)
    sizes, items_info = [], []
    for k, (c, o, m, cap) in enumerate(specs):
        info = infos[k] if infos and infos[k] is not None else hc.seg_info(c)[1]
        items_info.append(info)
        if (o, m) == (0, WHOLE):
            raw_len = info.raw_len if info is not None else 0
            sizes.append(raw_len if cap is None else min(cap, raw_len))
        else:
            sizes.append(min(m, 1 << 20))
    out_offs, total = _outs(sizes)
    items = [(in_offs[id(c)], len(c), info, o, m, oo, size if cap is None else cap)
             for (c, o, m, cap), info, oo, size in zip(specs, items_info, out_offs, sizes)]
    n = len(items)
    inp = torch.from_numpy(host).cuda()
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    lens = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    bad = torch.full((n,), 7, dtype=torch.int64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    arr = hc.seg_dec_items(items)
    need = int(hc.lib().hc_seg_decompress_batch_work_bound(arr, n))
    wb = need if work_bytes is None else work_bytes
    work = torch.empty(max(wb, 16), dtype=torch.uint8, device="cuda")
    rc = hc.lib().hc_seg_decompress_batch_dev(inp.data_ptr(), out.data_ptr(), arr, n, lens.data_ptr(), st.data_ptr(),
                                              bad.data_ptr(), work.data_ptr(), wb,
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = out.cpu().numpy().tobytes()
    res, untouched = [], []
    for s, m, b, o, size in zip(st.tolist(), lens.tolist(), bad.tolist(), out_offs, sizes):
        res.append((int(s), int(b) % 2**64, got[o:o + m] if s == 0 else b"", int(m)))
        untouched.append(got[o:o + size] == A5 * size)
    return rc, res, _guards_intact(got, out_offs, sizes, total), untouched, need


def want_dec(specs):
    return [sbm.decode_item(c, o, m, cap) for c, o, m, cap in specs]


# --- 1. encode ---------------------------------------------------------------------------------
@pytest.mark.parametrize("use_diff,check", [(False, False), (True, False), (False, True), (True, True)])
def test_encode_plain(hc, gpu, use_diff, check):
    names = ["rng:256:0", "rng:256:1", "rng:256:17", f"rng:256:{srm.BIG}", "rng:256:17"]
    raws = [cases.raw(n) for n in names]
    rc, res, clean, _ = enc_batch(hc, gpu, raws, [512] * 5, use_diff=use_diff, check=check, seg_bytes=16)
    assert rc == 0 and clean
    want = [(0, c, len(c)) for c in (model(n, use_diff, False, 512, 16, check)[1] for n in names)]
    assert want[3][1][40:48] == (2050).to_bytes(8, "little")  # the tile-crossing item, between small ones
    check_encoded(res, want)
    assert want == [sbm.encode_item(r, 512, use_diff, False, 16, check) for r in raws]


@pytest.mark.parametrize("use_diff,check", [(False, False), (True, True)])
def test_encode_adaptive(hc, gpu, use_diff, check):
    # (name, width) at both segment sizes of the rng:4 cases: the widths differ inside a call; at 128
    # the 16 x 19 matrix is bands of 8 rows whose last took the 3 leftover rows, 16 x 15 is one band
    shapes = [("rng:4:304", 16), ("rng:4:240", 16), ("rng:4:288", 9), ("rng:4:304", 16)]
    for seg in (128, 80):
        raws = [cases.raw(n) for n, _ in shapes]
        widths = [w for _, w in shapes]
        rc, res, clean, _ = enc_batch(hc, gpu, raws, widths, use_diff=use_diff, use_adapt=True, check=check, seg_bytes=seg)
        assert rc == 0 and clean
        want = [(0, c, len(c)) for c in (model(n, use_diff, True, w, seg, check)[1] for n, w in shapes)]
        check_encoded(res, want)
    f = scm.parse(model("rng:4:304", use_diff, True, 16, 128, check)[1])[0]
    assert [m for _, m in f["cuts"]] == [128, 176]


# --- 2. decode: one call mixing every kind -----------------------------------------------------
MIX = [("rng:256:17", False, 512, 16, False, False), (f"rng:256:{srm.BIG}", False, 512, 16, True, False),
       ("rng:256:0", False, 512, 16, False, False),
       ("rng:4:304", True, 16, 128, False, False), ("rng:4:288", True, 9, 80, True, False),
       ("photo:64:200", False, 512, 4096, True, True), ("photo:64:200", False, 512, 4096, True, False),
       ("photo:64:200", True, 64, 4096, True, True), ("photo:64:200", True, 64, 4096, False, False)]


def mixed_specs():
    specs = []
    for case in MIX:
        raw, c, f, rs = srm.built(case)
        specs.append((c, 0, WHOLE, None))
        specs += [(c, o, m, None) for o, m in rs]
    return specs


def test_decode_mixed(hc, gpu):
    specs = mixed_specs()
    assert any(o % 4 and m > 0 for _, o, m, _ in specs) and len(specs) > 2 * CHUNK
    f = srm.built(MIX[3])[2]
    assert f["raw_len"] > f["n_segments"] * f["cuts"][0][1]  # the leftover-rows ranges are among them
    rc, res, clean, _, _ = dec_batch(hc, gpu, specs)
    assert rc == 0 and clean
    want = want_dec(specs)
    for k, (c, o, m, _) in enumerate(specs):
        raw_len = srm.header(c)["raw_len"]
        assert want[k][0] == 0 and want[k][3] == (raw_len if m == WHOLE else m), k
        assert res[k] == want[k], (k, o, m)


# --- 3. independence ---------------------------------------------------------------------------
def test_decode_independence(hc, gpu):
    import oracle
    goods = [(srm.built(MIX[5])[1], 4100, 8192, None), (srm.built(MIX[3])[1], 0, WHOLE, None)]
    good_want = want_dec(goods)
    assert all(w[0] == 0 for w in good_want)

    def between(spec, want_status, want_bad, want_len=0, info=None):
        specs = [goods[0], spec, goods[1]]
        rc, res, clean, untouched, _ = dec_batch(hc, gpu, specs, infos=[None, info, None])
        assert rc == 0 and clean
        assert [res[0], res[2]] == good_want
        assert res[1] == (want_status, want_bad, b"", want_len), res[1]
        if info is None:
            assert res[1] == sbm.decode_item(*spec)
        return untouched[1]

    for name, diff, adapt, w, seg, byte, bit in cases.SILENT_FLIPS:
        raw, good = model(name, diff, adapt, w, seg, True)
        f = scm.parse(good)[0]
        b1, n1 = f["cuts"][1]
        # the same length, other bytes: the checksum alone notices
        flipped = cases.flip(good, 1, byte, bit)
        between((flipped, b1 + 1, n1 - 1, None), hc.HC_ERR_SEG_CHECK, 1)
        between((flipped, 0, WHOLE, None), hc.HC_ERR_SEG_CHECK, 1)
        # another length
        streams = scm.segments(good)
        st, short = oracle.compress(raw[:n1 // 2 // w * w if adapt else n1 // 2], diff, adapt, w)
        assert st == 0
        resized = scm.repack(good, [short if k == 1 else s for k, s in enumerate(streams)])
        between((resized, b1, n1, None), hc.HC_ERR_SEG_SIZE, 1)
        # a damaged segment outside the range is not noticed, as in the single call
        for bad in (flipped, resized):
            specs = [goods[0], (bad, 0, b1, None), goods[1]]
            rc, res, clean, _, _ = dec_batch(hc, gpu, specs)
            assert rc == 0 and clean and res == [good_want[0], (0, NO_SEG, raw[:b1], b1), good_want[1]]

    raw, good, f, rs = srm.built(MIX[5])
    st, info = hc.seg_info(good)
    mutant = srm.index_mutants(good)["enc_len_longer"]
    assert between((mutant, 5, 70, None), hc.HC_ERR_SEG_HEADER, NO_SEG)
    assert between((mutant, 0, WHOLE, None), hc.HC_ERR_SEG_HEADER, NO_SEG)
    for name, bad in seg_model.header_mutants(srm.built(MIX[6])[1]).items():  # (of the unchecked container)
        assert between((bad, 5, 70, None), hc.HC_ERR_SEG_HEADER, NO_SEG), name
    other = hc.seg_info(good)[1]
    other.flags ^= hc.HC_FLAG_DIFF  # valid for this length, not what the device bytes say
    assert between((good, 5, 70, None), hc.HC_ERR_SEG_HEADER, NO_SEG, info=other)
    # out_cap one byte short: the needed length, nothing written
    assert between((good, 4100, 8192, 8191), hc.HC_ERR_CAPACITY, NO_SEG, 8192)
    assert between((good, 0, WHOLE, len(raw) - 1), hc.HC_ERR_CAPACITY, NO_SEG, len(raw))
    # a range outside raw_len
    assert between((good, len(raw), 1, None), hc.HC_ERR_ARG, NO_SEG)
    assert between((good, 1, len(raw), None), hc.HC_ERR_ARG, NO_SEG)
    assert between((good, 1, WHOLE, None), hc.HC_ERR_ARG, NO_SEG)


def test_encode_independence(hc, gpu):
    a, b = cases.raw("rng:4:304"), cases.raw("rng:4:288")
    good_want = [sbm.encode_item(a, 16, True, True, 128, True), sbm.encode_item(b, 9, True, True, 128, True)]
    for raw, w, status in ((a, 0, hc.HC_ERR_WIDTH), (a, 15, hc.HC_ERR_MATRIX_SIZE), (a[:112], 16, hc.HC_ERR_DIMS),
                           (a[:56], 7, hc.HC_ERR_DIMS), (b"", 16, hc.HC_ERR_DIMS)):
        want = [good_want[0], sbm.encode_item(raw, w, True, True, 128, True), good_want[1]]
        assert want[1] == (status, b"", 0)
        rc, res, clean, _ = enc_batch(hc, gpu, [a, raw, b], [16, w, 9], use_diff=True, use_adapt=True, check=True,
                                      seg_bytes=128)
        assert rc == 0 and clean
        check_encoded(res, want)
    # width 0 without -a, and a capacity one byte short: the needed length, nothing written
    c17 = model("rng:256:17", False, False, 512, 16, False)[1]
    r17 = cases.raw("rng:256:17")
    rc, res, clean, _ = enc_batch(hc, gpu, [r17, r17, r17, r17], [512, 0, 512, 512],
                                  caps=[len(c17), 64, len(c17) - 1, len(c17)], seg_bytes=16)
    assert rc == 0 and clean
    check_encoded(res, [(0, c17, len(c17)), (hc.HC_ERR_WIDTH, b"", 0), (hc.HC_ERR_CAPACITY, b"", len(c17)),
                        (0, c17, len(c17))])


# --- 4. more items than a descriptor chunk -----------------------------------------------------
def test_many_items(hc, gpu):
    n = max(130, 2 * CHUNK + 3)
    raw, c = model("rng:256:17", True, False, 512, 16, True)
    others = [model("rng:256:1", True, False, 512, 16, True), model("rng:256:0", True, False, 512, 16, True)]
    pick = lambda k: (raw, c) if k % 7 else others[(k // 7) % 2]  # every seventh item another size
    raws = [pick(k)[0] for k in range(n)]
    rc, res, clean, _ = enc_batch(hc, gpu, raws, [512] * n, use_diff=True, check=True, seg_bytes=16)
    assert rc == 0 and clean
    check_encoded(res, [(0, pick(k)[1], len(pick(k)[1])) for k in range(n)])
    # and back: each item's own bytes, every third one a range
    conts = [res[k][2][:res[k][1]] for k in range(n)]
    specs = [(conts[k], 1, len(raws[k]) - 1, None) if k % 3 == 0 and raws[k] else (conts[k], 0, WHOLE, None)
             for k in range(n)]
    rc, got, clean, _, _ = dec_batch(hc, gpu, specs)
    assert rc == 0 and clean
    for k, (cont, o, m, _) in enumerate(specs):
        want = raws[k] if m == WHOLE else raws[k][o:o + m]
        assert got[k] == (0, NO_SEG, want, len(want)), k


# --- 5. work bounds ----------------------------------------------------------------------------
def test_work_bounds(hc, gpu):
    names = ["rng:256:17", f"rng:256:{srm.BIG}", "rng:256:0"]
    raws = [cases.raw(n) for n in names]
    rc, res, clean, need = enc_batch(hc, gpu, raws, [512] * 3, use_diff=True, check=True, seg_bytes=16)
    assert rc == 0 and clean and need == sbm.encode_work_bound(hc, [(len(r), 512) for r in raws], False, 16, True)
    check_encoded(res, [(0, c, len(c)) for c in (model(n, True, False, 512, 16, True)[1] for n in names)])
    rc, res, clean, _ = enc_batch(hc, gpu, raws, [512] * 3, use_diff=True, check=True, seg_bytes=16, work_bytes=need - 1)
    assert rc == hc.HC_ERR_ARG and clean
    assert all((st, n, region) == (-1, -1, A5 * len(region)) for st, n, region in res)

    specs = [s for s in mixed_specs() if s[0] in (srm.built(MIX[1])[1], srm.built(MIX[7])[1], srm.built(MIX[3])[1])]
    rc, res, clean, _, need = dec_batch(hc, gpu, specs)
    assert rc == 0 and clean and need == sbm.decode_work_bound(hc, [s[:3] for s in specs])
    assert res == want_dec(specs)
    rc, res, clean, untouched, _ = dec_batch(hc, gpu, specs, work_bytes=need - 1)
    assert rc == hc.HC_ERR_ARG and clean and all(untouched)
    assert all(r == (-1, 7, b"", -1) for r in res)


# --- 6. the single device calls, directly ------------------------------------------------------
def _single_enc(hc, torch, raw, width, cap, **opts):
    inp = torch.from_numpy(np.frombuffer(bytes(raw) + bytes(16), dtype=np.uint8).copy()).cuda()
    out = torch.full((_a16(cap) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hc.seg_compress_dev(inp[:len(raw)], out, n, st, width=width, out_cap=cap, **opts)
    torch.cuda.synchronize()
    return int(st.item()), int(n.item()), out.cpu().numpy().tobytes()[:cap]


def test_equals_single_encode(hc, gpu):
    raws = [cases.raw("rng:4:304"), cases.raw("rng:4:288"), cases.raw("rng:4:240"), cases.raw("rng:4:304")]
    widths = [16, 9, 16, 16]
    opts = dict(use_diff=True, use_adapt=True, check=True, seg_bytes=128)
    caps = [int(hc.lib().hc_seg_compress_bound2(len(r), 128, hc._seg_flags(True, True, True), w))
            for r, w in zip(raws, widths)]
    caps[3] = 100  # too small: the needed length
    rc, res, clean, _ = enc_batch(hc, gpu, raws, widths, caps=caps, **opts)
    assert rc == 0 and clean
    for k in range(4):
        st, n, region = _single_enc(hc, gpu, raws[k], widths[k], caps[k], **opts)
        assert (res[k][0], res[k][1]) == (st, n), k
        assert res[k][2][:n] == region[:n] if st == 0 else res[k][2] == region == A5 * caps[k], k
    assert [r[0] for r in res] == [0, 0, 0, hc.HC_ERR_CAPACITY]


def test_equals_single_decode(hc, gpu):
    from test_gpu_seg_range import dev_range
    raw, good, f, rs = srm.built(MIX[5])
    streams = scm.segments(good)
    cut = scm.repack(good, streams[:2] + [streams[2][:8]] + streams[3:])
    adapt = srm.built(MIX[7])[1]
    specs = [(good, 4100, 8192, None), (cut, 4100, 8192, None), (cut, 4, 4000, None), (adapt, 4097, 3, None),
             (good, 0, 12800, 12799), (srm.index_mutants(good)["trailing_byte"], 0, 16, None), (adapt, 8192, 4608, None)]
    rc, res, clean, _, _ = dec_batch(hc, gpu, specs)
    assert rc == 0 and clean
    for k, (c, o, m, cap) in enumerate(specs):
        st, n, bad, out, ok = dev_range(hc, gpu, c, o, m, out_cap=cap)
        assert ok and res[k] == (st, bad, out if st == 0 else b"", n), k
    assert [r[0] for r in res] == [0, 8, 0, 0, hc.HC_ERR_CAPACITY, hc.HC_ERR_SEG_HEADER, 0]
    # a whole item against hc_seg_decompress_dev
    for c in (good, cut, srm.built(MIX[2])[1]):
        info = hc.seg_info(c)[1]
        inp = gpu.from_numpy(np.frombuffer(bytes(c) + bytes(16), dtype=np.uint8).copy()).cuda()
        out = gpu.full((_a16(info.raw_len) + 16,), 0xA5, dtype=gpu.uint8, device="cuda")
        n = gpu.full((1,), -1, dtype=gpu.int64, device="cuda")
        bad = gpu.full((1,), 7, dtype=gpu.int64, device="cuda")
        st = gpu.full((1,), -1, dtype=gpu.int32, device="cuda")
        hc.seg_decompress_dev(inp, out, n, st, bad_segment=bad, info=info, in_len=len(c), out_cap=info.raw_len)
        gpu.cuda.synchronize()
        rc, res, clean, _, _ = dec_batch(hc, gpu, [(c, 0, WHOLE, None)])
        single = (int(st.item()), int(bad.item()) % 2**64,
                  out.cpu().numpy().tobytes()[:int(n.item())] if int(st.item()) == 0 else b"", int(n.item()))
        assert rc == 0 and clean and res[0] == single


# --- 7. host calls -----------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", [None, 3000], ids=["one-call", "sub-batches"])
def test_host_batches(hc, gpu, monkeypatch, pipe):
    if pipe:  # several sub-batches, and the 2050-segment input (32789 bytes) above the limit alone
        monkeypatch.setenv("HC_PIPE_BYTES", str(pipe))
    names = ["rng:256:0", "rng:256:1", "rng:256:17", f"rng:256:{srm.BIG}", "rng:256:17"]
    raws = [cases.raw(n) for n in names] + [b"abc"]
    widths = [512] * 5 + [0]
    sts, outs, lens = hc.seg_compress_host_batch(raws, use_diff=True, widths=widths, seg_bytes=16, check=True)
    want = [sbm.encode_item(r, w, True, False, 16, True) for r, w in zip(raws, widths)]
    assert list(zip(sts, outs, lens)) == want and sts[5] == hc.HC_ERR_WIDTH
    a = [cases.raw("rng:4:304"), cases.raw("rng:4:288"), cases.raw("rng:4:240"), cases.raw("rng:4:304")[:112]]
    w = [16, 9, 16, 16]
    c304 = model("rng:4:304", False, True, 16, 128, False)[1]
    caps = [len(c304) - 1, 4096, 4096, 4096]
    sts, outs, lens = hc.seg_compress_host_batch(a, use_adapt=True, widths=w, seg_bytes=128, caps=caps)
    assert list(zip(sts, outs, lens)) == [sbm.encode_item(r, x, False, True, 128, False, cap)
                                          for r, x, cap in zip(a, w, caps)]
    assert sts == [hc.HC_ERR_CAPACITY, 0, 0, hc.HC_ERR_DIMS]

    specs = mixed_specs()
    raw, good, f, rs = srm.built(MIX[5])
    streams = scm.segments(good)
    cut = scm.repack(good, streams[:2] + [streams[2][:8]] + streams[3:])
    flip = cases.SILENT_FLIPS[0]
    flipped = cases.flip(model(flip[0], flip[1], flip[2], flip[3], flip[4], True)[1], 1, flip[5], flip[6])
    specs += [(cut, 4100, 8192, None), (cut, 4, 4000, None), (flipped, 0, WHOLE, None), (flipped, 0, 4096, None),
              (srm.index_mutants(good)["enc_len_longer"], 5, 70, None), (good, 12800, 1, None), (good, 4100, 8192, 8191),
              (good, 0, WHOLE, 12799), (b"", 0, 0, None)]
    blobs = [s[0] for s in specs]
    ranges = [(o, m) for _, o, m, _ in specs]
    caps = [cap if cap is not None else (srm.header(c)["raw_len"] if m == WHOLE else m) for c, o, m, cap in specs]
    want = [sbm.decode_item(c, o, m, cap) for (c, o, m, _), cap in zip(specs, caps)]
    sts, outs, lens, bad = hc.seg_decompress_host_batch(blobs, ranges=ranges, caps=caps)
    assert list(zip(sts, bad, outs, lens)) == want
    assert {hc.HC_ERR_SEG_CHECK, hc.HC_ERR_SEG_HEADER, hc.HC_ERR_ARG, hc.HC_ERR_CAPACITY, 8, 0} <= set(sts)
    # offsets and lengths both NULL: every item whole
    wholes = [s[0] for s in specs if s[2] == WHOLE and s[3] is None]
    sts, outs, lens, bad = hc.seg_decompress_host_batch(wholes)
    assert list(zip(sts, bad, outs, lens)) == [sbm.decode_item(c) for c in wholes]


# --- 8. huffman-codec-batch --------------------------------------------------------------------
def test_cli(hc, gpu, tmp_path):
    raws = {"a.bin": cases.raw("photo:64:200"), "b.bin": cases.raw(f"rng:256:{srm.BIG}"), "c.bin": b"",
            "d.bin": cases.raw("rng:256:17"), "e.bin": cases.raw("rng:4:304")}
    for name, raw in raws.items():
        (tmp_path / name).write_bytes(raw)
    files = [str(tmp_path / n) for n in raws]
    r = subprocess.run([hc.BATCH_CLI_PATH, "-c", "-m", "-s", "4096", "-k"] + files, capture_output=True)
    assert r.returncode == 0, r.stderr
    conts = {}
    for name, raw in raws.items():
        st, want = hc.seg_compress(raw, use_diff=True, seg_bytes=4096, check=True)
        conts[name] = (tmp_path / (name + ".huf")).read_bytes()
        assert st == 0 and conts[name] == want == scm.build(raw, True, False, 512, 4096, check=True), name
        os.remove(tmp_path / name)
    hufs = [f + ".huf" for f in files]
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d"] + hufs, capture_output=True)
    assert r.returncode == 0, r.stderr
    for name, raw in raws.items():
        assert (tmp_path / name).read_bytes() == raw == hc.seg_decompress(conts[name])[1], name
        os.remove(tmp_path / name)
    # ranges: inside all five only when empty; 4100:17 is inside two of them
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d", "-r", "0:0"] + hufs, capture_output=True)
    assert r.returncode == 0 and all((tmp_path / n).read_bytes() == b"" for n in raws)
    for n in raws:
        os.remove(tmp_path / n)
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d", "-r", "4100:17"] + hufs, capture_output=True)
    assert r.returncode == hc.HC_ERR_ARG and b"coded 2 of 5 files" in r.stderr
    for name, raw in raws.items():
        st, want = hc.seg_decompress_range(conts[name], 4100, 17)
        if st == 0:
            assert (tmp_path / name).read_bytes() == want == raw[4100:4117], name
            os.remove(tmp_path / name)
        else:
            assert st == hc.HC_ERR_ARG and not os.path.exists(tmp_path / name), name
    # one damaged file among them: its "segment K" message and exit code, the others written
    streams = scm.segments(conts["a.bin"])
    (tmp_path / "a.bin.huf").write_bytes(scm.repack(conts["a.bin"], streams[:2] + [streams[2][:8]] + streams[3:]))
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d"] + hufs, capture_output=True)
    assert r.returncode == 8 and b"a.bin.huf: segment 2: ERROR: invalid or missing Huffman coding header" in r.stderr
    assert b"coded 4 of 5 files" in r.stderr and not os.path.exists(tmp_path / "a.bin")
    assert all((tmp_path / n).read_bytes() == raw for n, raw in raws.items() if n != "a.bin")
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d", "-r", "4:4000", str(tmp_path / "a.bin.huf"), str(tmp_path / "b.bin.huf")],
                       capture_output=True)
    assert r.returncode == 0 and (tmp_path / "a.bin").read_bytes() == raws["a.bin"][4:4004]
    assert (tmp_path / "b.bin").read_bytes() == raws["b.bin"][4:4004]
    # a container that decodes to more than 8 times its size (and more than 64 KiB): -d sizes its
    # output by a guess first and by the header once the container has passed
    zeros = bytes(200000)
    (tmp_path / "z.bin").write_bytes(zeros)
    r = subprocess.run([hc.BATCH_CLI_PATH, "-c", "-s", "4096", str(tmp_path / "z.bin")], capture_output=True)
    z = (tmp_path / "z.bin.huf").read_bytes()
    assert r.returncode == 0 and z == scm.build(zeros, False, False, 512, 4096, check=False) and 8 * len(z) < len(zeros)
    os.remove(tmp_path / "z.bin")
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d", str(tmp_path / "z.bin.huf"), str(tmp_path / "d.bin.huf")],
                       capture_output=True)
    assert r.returncode == 0 and (tmp_path / "z.bin").read_bytes() == zeros
    assert (tmp_path / "d.bin").read_bytes() == raws["d.bin"]

"""The batched segmented coders without a device: the work bounds against their closed form
(tests/seg_batch_model.py), the statuses the host decides, the call-level argument errors, which
are all decided before any launch, and the ctypes structs against the header's."""
import ctypes
import subprocess

import pytest

import seg_batch_model as sbm
import seg_model
import seg_range_model as srm

ONE = ctypes.c_void_p(256)  # an aligned, non-null "device pointer" for calls that fail before any launch
NULL = ctypes.c_void_p(0)
PLAIN = ("rng:256:17", False, 512, 16, False, False)
PLAIN_M = (f"rng:256:{srm.BIG}", False, 512, 16, True, False)
ADAPT = ("rng:4:304", True, 16, 128, False, False)
PHOTO_AMK = ("photo:64:200", True, 64, 4096, True, True)


def _dec_items(hc, specs):
    """(container, offset, length) -> item tuples at in_off / out_off 0 with the container's own info"""
    return [(0, len(c), hc.seg_info(c)[1], o, m, 0, 0) for c, o, m in specs]


def test_new_symbols_are_declared_and_exported(hc):
    names = hc.header_symbols()
    L = hc.lib()
    for n in ("hc_seg_compress_batch_work_bound", "hc_seg_compress_batch_dev", "hc_seg_decompress_batch_work_bound",
              "hc_seg_decompress_batch_dev", "hc_seg_compress_host_batch", "hc_seg_decompress_host_batch"):
        assert n in names and hasattr(L, n), n
    out = subprocess.run(["nm", "-D", "--defined-only", hc.LIB_PATH], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {n for n in names if "seg" in n and "batch" in n} <= exported


def test_structs_match_the_header(hc, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hcodec.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(hc_seg_enc_item_t),'
                   ' sizeof(hc_seg_dec_item_t), sizeof(hc_seg_info_t), offsetof(hc_seg_dec_item_t, info),'
                   ' offsetof(hc_seg_dec_item_t, offset), offsetof(hc_seg_dec_item_t, out_cap),'
                   ' offsetof(hc_seg_enc_item_t, out_cap), HC_SEG_WHOLE == UINT64_MAX);return 0;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", hc.INCLUDE_DIR, str(src), "-o", str(tmp_path / "t")],
                   check=True)
    got = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()
    D, E = hc.SegDecItem, hc.SegEncItem
    assert [int(x) for x in got] == [ctypes.sizeof(E), ctypes.sizeof(D), ctypes.sizeof(hc.SegInfo), D.info.offset,
                                     D.offset.offset, D.out_cap.offset, E.out_cap.offset, 1]
    assert hc.HC_SEG_WHOLE == sbm.WHOLE == 2**64 - 1


@pytest.mark.parametrize("use_adapt,check", [(False, False), (False, True), (True, False), (True, True)])
def test_encode_work_bound(hc, use_adapt, check):
    seg = 128 if use_adapt else 16
    sets = ([(304, 16), (240, 16), (288, 9), (0, 16), (300, 16), (56, 7)] if use_adapt
            else [(0, 512), (1, 512), (17, 512), (srm.BIG, 512), (17, 0)])
    bound = lambda its: hc.seg_compress_batch_work_bound([(0, n, w, 0, 0) for n, w in its], use_adapt=use_adapt,
                                                         seg_bytes=seg, check=check)
    prev = -1
    for k in range(len(sets) + 1):  # monotone in the items, and the closed form at every step
        b = bound(sets[:k])
        assert b == sbm.encode_work_bound(hc, sets[:k], use_adapt, seg, check), k
        assert b > prev
        prev = b
    # at least what the single call needs for each item
    for n, w in sets:
        if sbm.host_status(n, use_adapt, w) == 0:
            flags = (hc.HC_FLAG_ADAPT if use_adapt else 0) | (hc.HC_SEG_CHECK_CRC32 if check else 0)
            assert bound([(n, w)]) >= int(hc.lib().hc_seg_compress_work_bound2(n, seg, flags, w)) > 0
    # refused arguments
    assert hc.seg_compress_batch_work_bound([(0, 17, 512, 0, 0)], seg_bytes=24) == 0
    assert int(hc.lib().hc_seg_compress_batch_work_bound(hc.seg_enc_items([(0, 17, 512, 0, 0)]), 1, 0x20, 16)) == 0
    assert hc.seg_compress_batch_work_bound([(0, 2**40, 512, 0, 0)], seg_bytes=16) == 0  # 2^36 segments
    assert hc.seg_compress_batch_work_bound([(0, 2**34, 512, 0, 0)] * 3, seg_bytes=16) == 0  # 3 * 2^30 in total


def test_decode_work_bound(hc):
    built = {c: srm.built(c) for c in (PLAIN, PLAIN_M, ADAPT, PHOTO_AMK)}
    specs = []
    for case, (raw, c, f, rs) in built.items():
        specs.append((c, 0, sbm.WHOLE))
        specs += [(c, o, m) for o, m in rs]
        specs.append((c, len(raw), 1))            # outside raw_len: nothing of it is counted
    specs.append((bytes(64), 0, sbm.WHOLE))       # no container at all
    L = hc.lib()
    bound = lambda sp: hc.seg_decompress_batch_work_bound(_dec_items(hc, sp))
    prev = -1
    for k in range(len(specs) + 1):
        b = bound(specs[:k])
        assert b == sbm.decode_work_bound(hc, specs[:k]), k
        assert b > prev
        prev = b
    # whole items: every array and the adaptive workspace of each single call fit
    for case, (raw, c, f, rs) in built.items():
        st, info = hc.seg_info(c)
        single = int(L.hc_seg_decompress_work_bound(ctypes.byref(info), len(c)))
        assert bound([(c, 0, sbm.WHOLE)]) >= single
        assert bound([(x[1], 0, sbm.WHOLE) for x in built.values()]) >= single
        for o, m in rs:
            assert bound([(c, o, m)]) >= int(L.hc_seg_decompress_range_work_bound(ctypes.byref(info), len(c), o, m))


def test_empty_batches(hc):
    L = hc.lib()
    assert L.hc_seg_compress_batch_dev(NULL, NULL, None, 0, 0, 0, NULL, NULL, NULL, 0, NULL) == 0
    assert L.hc_seg_decompress_batch_dev(NULL, NULL, None, 0, NULL, NULL, NULL, NULL, 0, NULL) == 0
    assert L.hc_seg_compress_host_batch(NULL, NULL, NULL, 0, 0, 0, NULL, NULL, NULL, NULL) == 0
    assert L.hc_seg_decompress_host_batch(NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL, NULL) == 0
    assert hc.seg_compress_host_batch([]) == ([], [], [])
    assert hc.seg_decompress_host_batch([]) == ([], [], [], [])


def test_encode_return_value_errors(hc):
    L = hc.lib()
    items = hc.seg_enc_items([(0, 17, 512, 0, 64), (32, 17, 512, 64, 64)])
    need = int(L.hc_seg_compress_batch_work_bound(items, 2, 0, 16))
    assert need > 0

    def call(inp=ONE, out=ONE, it=items, n=2, flags=0, seg=16, lens=ONE, st=ONE, work=ONE, wb=need):
        return L.hc_seg_compress_batch_dev(inp, out, it, n, flags, seg, lens, st, work, wb, NULL)

    for kw in (dict(inp=NULL), dict(out=NULL), dict(it=None), dict(lens=NULL), dict(st=NULL), dict(work=NULL),
               dict(inp=ctypes.c_void_p(264)), dict(out=ctypes.c_void_p(260)), dict(work=ctypes.c_void_p(257)),
               dict(it=hc.seg_enc_items([(0, 17, 512, 0, 64), (40, 17, 512, 64, 64)])),   # in_off
               dict(it=hc.seg_enc_items([(0, 17, 512, 0, 64), (32, 17, 512, 72, 64)])),   # out_off
               dict(flags=0x20), dict(flags=0x200), dict(seg=24), dict(wb=need - 1), dict(wb=0),
               dict(it=hc.seg_enc_items([(0, 2**40, 512, 0, 64), (32, 17, 512, 64, 64)]), wb=2**62)):
        assert call(**kw) == hc.HC_ERR_ARG, kw


def test_decode_return_value_errors(hc):
    L = hc.lib()
    raw, c, f, rs = srm.built(PLAIN)
    st, info = hc.seg_info(c)
    mk = lambda in_off=0, out_off=32: hc.seg_dec_items([(0, len(c), info, 0, sbm.WHOLE, 0, 17),
                                                        (in_off, len(c), info, 1, 5, out_off, 5)])
    items = mk()
    need = int(L.hc_seg_decompress_batch_work_bound(items, 2))
    assert need == sbm.decode_work_bound(hc, [(c, 0, sbm.WHOLE), (c, 1, 5)])

    def call(inp=ONE, out=ONE, it=items, n=2, lens=ONE, st=ONE, bad=ONE, work=ONE, wb=need):
        return L.hc_seg_decompress_batch_dev(inp, out, it, n, lens, st, bad, work, wb, NULL)

    for kw in (dict(inp=NULL), dict(out=NULL), dict(it=None), dict(lens=NULL), dict(st=NULL), dict(work=NULL),
               dict(inp=ctypes.c_void_p(264)), dict(out=ctypes.c_void_p(260)), dict(work=ctypes.c_void_p(257)),
               dict(it=mk(in_off=8)), dict(it=mk(out_off=36)), dict(wb=need - 1), dict(wb=0)):
        assert call(**kw) == hc.HC_ERR_ARG, kw
    # more segments in one container than a call takes: 2^32 cuts of 16 bytes, in an index of that size
    big = hc.SegInfo(raw_len=2**36, seg_bytes=16, width=0, n_segments=2**32, flags=0)
    it = hc.seg_dec_items([(0, 48 + 8 * 2**32 + 2**36, big, 0, 16, 0, 16)])
    assert L.hc_seg_decompress_batch_work_bound(it, 1) == 0
    assert call(it=it, n=1, wb=2**62) == hc.HC_ERR_ARG


def test_host_decided_statuses(hc):
    """what needs no device is decided per item before one is asked for; everything else, on a host
    without a device, is HC_ERR_DEVICE for that item alone"""
    import torch
    rest = None if torch.cuda.is_available() else hc.HC_ERR_DEVICE
    blobs = [bytes(range(64)), b"abcde", bytes(49), bytes(64), b""]
    widths = [8, 2, 7, 0, 8]
    want = [rest, hc.HC_ERR_MATRIX_SIZE, hc.HC_ERR_DIMS, hc.HC_ERR_WIDTH, hc.HC_ERR_DIMS]
    assert [sbm.host_status(len(b), True, w) or rest for b, w in zip(blobs, widths)] == want
    sts, outs, lens = hc.seg_compress_host_batch(blobs, use_adapt=True, widths=widths, seg_bytes=128)
    for k, w in enumerate(want):
        if w is not None:
            assert (sts[k], outs[k], lens[k]) == (w, b"", 0), k
            assert sbm.encode_item(blobs[k], widths[k], False, True, 128, False)[0] in (w, 0)
    with pytest.raises(hc.HCodecError, match="71"):
        hc.seg_compress_host_batch(blobs, seg_bytes=24, caps=[64] * 5)

    raw, c, f, rs = srm.built(PLAIN)
    hdr = seg_model.header_mutants(c)
    idx = srm.index_mutants(c)
    bad_hdr = next(iter(hdr.values()))
    blobs = [c, bad_hdr, c, idx["enc_len_longer"], c, c, b""]
    ranges = [(0, 17), (0, 1), (17, 1), (1, 5), (18, 0), (2, 9), (0, 0)]
    caps = [17, 1, 1, 5, 0, 8, 0]
    want = [rest, hc.HC_ERR_SEG_HEADER, hc.HC_ERR_ARG, hc.HC_ERR_SEG_HEADER, hc.HC_ERR_ARG,
            hc.HC_ERR_CAPACITY if rest is None else rest, hc.HC_ERR_SEG_HEADER]
    sts, outs, lens, bad = hc.seg_decompress_host_batch(blobs, ranges=ranges, caps=caps)
    for k, w in enumerate(want):
        if w is None:
            continue
        assert sts[k] == w and outs[k] == b"" and bad[k] == srm.NO_SEGMENT, k
        assert lens[k] == (9 if w == hc.HC_ERR_CAPACITY else 0), k
        if w != hc.HC_ERR_DEVICE:
            assert sbm.decode_item(blobs[k], *ranges[k], out_cap=caps[k])[:2] == (w, srm.NO_SEGMENT), k
    # whole items: the header on the host, the index on the device
    sts, outs, lens, bad = hc.seg_decompress_host_batch([bad_hdr, b"", c])
    assert sts[:2] == [hc.HC_ERR_SEG_HEADER] * 2 and lens[:2] == [0, 0] and bad[:2] == [srm.NO_SEGMENT] * 2
    assert rest is None or sts[2] == rest
    # one of offsets / lengths alone is no call
    L = hc.lib()
    arr = (ctypes.c_uint64 * 1)(0)
    p = ctypes.cast(arr, ctypes.c_void_p)
    assert L.hc_seg_decompress_host_batch(p, p, p, NULL, 1, p, p, p, p, NULL) == hc.HC_ERR_ARG
    assert L.hc_seg_decompress_host_batch(p, p, NULL, p, 1, p, p, p, p, NULL) == hc.HC_ERR_ARG

#!/usr/bin/env python3
"""Segmented container against whole-file coding on one large input.

The input is the synthetic 4096x4096 photo (hc.synth_batch, width 4096) in -m, -a -m and -a.
Each mode is coded through hc_seg_compress / hc_seg_decompress at 16, 64 and 256 KiB segments
and through hc_compress / hc_decompress (one stream, one wavefront) in the same process; every
call is a synchronous host-buffer call, timed with the host clock around it (copies included
on both sides), median of the repeats after warm-up. Prints one JSON line.

  scripts/seg_bench.py                       the sweep
  scripts/seg_bench.py --check               adds the checked container (a CRC-32 per segment,
                                             hc_seg_compress2 with HC_SEG_CHECK_CRC32) beside each
                                             unchecked figure
  scripts/seg_bench.py --no-whole --sizes 65536   the segmented calls alone, at the sizes named
  scripts/seg_bench.py --range               ranged reads (hc_seg_decompress_range, and
                                             hc_seg_decompress_range_dev under HIP events) against
                                             hc_seg_decompress plus a slice: 4 KiB inside one segment,
                                             1 MiB at a multiple of 4 and the same 1 MiB one byte on
                                             (every covered segment staged); --big adds a 16384x16384
                                             photo (4096 segments of 64 KiB)
  scripts/seg_bench.py --batch               many items per call (hc_seg_*_host_batch) against a loop of
                                             single calls in the same process: 4, 16 and 64 inputs of
                                             1 MiB (128 rows of a 8192x8192 photo each) at 64 KiB
                                             segments in -m and -a -m, encode and decode, and 64 ranged
                                             reads of 4 KiB out of one 4096x4096 container as one call
                                             against 64; with --trace-run the batch calls alone, twice
                                             at every N, so that a kernel's call count shows whether
                                             its launches grow with N (`rocprofv3 --kernel-trace --stats
                                             --output-format csv`, kernel trace alone, no counters)
  scripts/seg_bench.py --update              range writes (hc_seg_update, and hc_seg_update_dev under HIP
                                             events) into the -m container at 64 KiB segments: one 4 KiB
                                             patch in the middle and a 256 x 256 tile as 256 patches, each
                                             against what the other calls offer for the job (decode the
                                             whole, patch, code the whole), with the work bounds of both
                                             and the rate of the splice (an empty patch list: the whole
                                             container copied) beside a device copy; --big: the
                                             16384x16384 photo (4096 segments)
  scripts/seg_bench.py --trace-run           a few segmented calls only, to be run under
                                             `rocprofv3 --kernel-trace --stats -- python ...`
  scripts/seg_bench.py --glue-from STATS.csv adds the glue kernels' share of device time, read
                                             from that run's *_kernel_stats.csv
"""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "huffman-codec_amd", "python"))

import hcodec as hc  # noqa: E402

SIDE = 4096
MODES = {"-m": (1, 0), "-a -m": (1, 1), "-a": (0, 1)}
SIZES = (16384, 65536, 262144)
GLUE = ("seg_plan_kernel", "seg_seal_kernel", "seg_gather_kernel", "seg_open_kernel", "seg_close_kernel",
        "crc32_kernel", "pack_kernel", "seg_items_kernel")
BATCH_SIDE, BATCH_ITEM, BATCH_NS = 8192, 1 << 20, (4, 16, 64)


def photo(side=SIDE):
    import torch
    n = side * side
    raw = torch.empty(n, dtype=torch.uint8, device="cuda")
    hc.synth_batch("photo", 0, 1, side, side, raw, n)
    torch.cuda.synchronize()
    return raw.cpu().numpy().tobytes()


class Buffers:
    """host buffers allocated once, so that a timed call is the library call alone"""

    def __init__(self, raw):
        self.L = hc.lib()
        self.raw = raw
        self.src = ctypes.cast(ctypes.c_char_p(raw), ctypes.c_void_p)
        self.cap = max(hc.seg_compress_bound(len(raw), 16384, False, SIDE, check=True),
                       hc.seg_compress_bound(len(raw), 16384, True, SIDE, check=True),
                       hc.compress_bound(len(raw), True))
        self.enc = ctypes.create_string_buffer(self.cap)
        self.dec = ctypes.create_string_buffer(len(raw))
        self.n = ctypes.c_uint64(0)

    def p(self, b):
        return ctypes.cast(b, ctypes.c_void_p)

    def seg_encode(self, diff, adapt, seg, check=False):
        if check:
            flags = (hc.HC_FLAG_DIFF if diff else 0) | (hc.HC_FLAG_ADAPT if adapt else 0) | hc.HC_SEG_CHECK_CRC32
            rc = self.L.hc_seg_compress2(self.src, len(self.raw), flags, SIDE, seg, self.p(self.enc), self.cap,
                                         ctypes.byref(self.n))
        else:
            rc = self.L.hc_seg_compress(self.src, len(self.raw), diff, adapt, SIDE, seg, self.p(self.enc), self.cap,
                                        ctypes.byref(self.n))
        assert rc == 0, rc
        return self.n.value

    def seg_decode(self, enc_len):
        rc = self.L.hc_seg_decompress(self.p(self.enc), enc_len, self.p(self.dec), len(self.raw), ctypes.byref(self.n),
                                      None)
        assert rc == 0 and self.n.value == len(self.raw), rc

    def whole_encode(self, diff, adapt):
        rc = self.L.hc_compress(self.src, len(self.raw), diff, adapt, SIDE, self.p(self.enc), self.cap,
                                ctypes.byref(self.n))
        assert rc == 0, rc
        return self.n.value

    def whole_decode(self, enc_len):
        rc = self.L.hc_decompress(self.p(self.enc), enc_len, self.p(self.dec), len(self.raw), ctypes.byref(self.n))
        assert rc == 0 and self.n.value == len(self.raw), rc

    def exact(self):
        return self.dec.raw == self.raw


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)


def align16(x):
    return (x + 15) & ~15


def range_bench(raw, side, diff, adapt, seg, reps, device):
    """one container: the three ranges through the host call (against hc_seg_decompress plus a
    slice) and, with `device`, through the device call under HIP events"""
    import struct
    import torch
    L = hc.lib()
    st, enc = hc.seg_compress(raw, bool(diff), bool(adapt), side, seg)
    assert st == 0, st
    st, info = hc.seg_info(enc)
    n = info.n_segments
    lens = struct.unpack_from(f"<{n}Q", enc, 48)
    offs, o = [], align16(48 + 8 * n)
    for m in lens:
        offs.append(o)
        o = align16(o + m)
    src = ctypes.cast(ctypes.c_char_p(enc), ctypes.c_void_p)
    whole = ctypes.create_string_buffer(len(raw))
    k = ctypes.c_uint64(0)

    def full_then_slice(o, m):
        rc = L.hc_seg_decompress(src, len(enc), ctypes.cast(whole, ctypes.c_void_p), len(raw), ctypes.byref(k), None)
        assert rc == 0, rc
        return whole[o:o + m]

    full_work = int(L.hc_seg_decompress_work_bound(ctypes.byref(info), len(enc)))
    res = {"bytes": len(enc), "segments": n,
           "whole": {"uploaded": len(enc), "device_bytes": len(enc) + 16 + len(raw) + 16 + full_work + 32}, "ranges": {}}
    mid = (len(raw) // 2) & ~65535
    ranges = {"4KiB": (mid + 8192, 4096), "1MiB": (mid + 4096, 1 << 20), "1MiB+1": (mid + 4097, 1 << 20)}
    for name, (o, m) in ranges.items():
        st, first, count = hc.seg_range_segments(info, len(enc), o, m)
        assert st == 0 and count
        span = offs[first + count - 1] + lens[first + count - 1] - offs[first]
        work = int(L.hc_seg_decompress_range_work_bound(ctypes.byref(info), len(enc), o, m))
        if adapt:  # the host call sizes the adaptive workspace by the span, not by the container
            assert first + count < n  # (no range here reaches the last segment)
            covered_raw = count * full_bytes(seg, adapt, side)
            work += int(L.hc_adapt_decompress_work_bound(span, covered_raw, count)) - int(
                L.hc_adapt_decompress_work_bound(len(enc), covered_raw, count))
        out = ctypes.create_string_buffer(m)

        def ranged():
            rc = L.hc_seg_decompress_range(src, len(enc), o, m, ctypes.cast(out, ctypes.c_void_p), m, ctypes.byref(k), None)
            assert rc == 0 and k.value == m, rc

        r = {"offset": o, "length": m, "covered": count, "range_ms": timed(ranged, 2, reps),
             "whole_and_slice_ms": timed(lambda: full_then_slice(o, m), 2, reps),
             "uploaded": align16(48 + 8 * n) + span,
             "device_bytes": align16(48 + 8 * n) + span + 16 + m + 16 + work + 32}
        assert out.raw == raw[o:o + m] and full_then_slice(o, m) == raw[o:o + m]
        r["speedup"] = round(r["whole_and_slice_ms"][0] / r["range_ms"][0], 2)
        res["ranges"][name] = r
    if device:
        import numpy as np
        host = np.zeros(align16(len(enc)), dtype=np.uint8)
        host[:len(enc)] = np.frombuffer(enc, dtype=np.uint8)
        inp = torch.from_numpy(host).cuda()
        dout = torch.empty(len(raw), dtype=torch.uint8, device="cuda")
        olen = torch.zeros(1, dtype=torch.int64, device="cuda")
        stt = torch.zeros(1, dtype=torch.int32, device="cuda")

        def events(fn):
            ts = []
            for i in range(2 + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                assert int(stt.item()) == 0
                if i >= 2:
                    ts.append(e0.elapsed_time(e1))
            return round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)

        work = hc.seg_decompress_dev(inp, dout, olen, stt, info=info, in_len=len(enc))
        res["whole"]["device_ms"] = events(lambda: hc.seg_decompress_dev(inp, dout, olen, stt, info=info, in_len=len(enc),
                                                                         work=work))
        for name, (o, m) in ranges.items():
            w = hc.seg_decompress_range_dev(inp, dout, olen, stt, o, m, info=info, in_len=len(enc), out_cap=m)
            res["ranges"][name]["device_ms"] = events(lambda: hc.seg_decompress_range_dev(
                inp, dout, olen, stt, o, m, info=info, in_len=len(enc), out_cap=m, work=w))
            assert dout[:m].cpu().numpy().tobytes() == raw[o:o + m]
    return res


def update_bench(raw, side, reps, trace=False):
    """one -m container at 64 KiB segments: the two patch lists through hc_seg_update and
    hc_seg_update_dev, and through decode + patch + encode of the whole"""
    import numpy as np
    import torch
    L = hc.lib()
    seg, flags = 65536, hc.HC_FLAG_DIFF
    st, enc = hc.seg_compress(raw, True, False, side, seg)
    assert st == 0, st
    st, info = hc.seg_info(enc)
    rng = np.random.default_rng(5)
    mid = (len(raw) // 2) & ~65535
    y0, x0 = side // 2 + 3, side // 2 + 40
    lists = {"4KiB": [(mid + 8192, 4096)], "tile256": [((y0 + r) * side + x0, 256) for r in range(256)]}
    src = ctypes.cast(ctypes.c_char_p(enc), ctypes.c_void_p)
    cap = 2 * len(enc) + (1 << 20)  # (room for every result here; the bound is about 6x the raw bytes)
    out = ctypes.create_string_buffer(cap)
    alt_raw = ctypes.create_string_buffer(len(raw))
    alt_enc = ctypes.create_string_buffer(cap)
    k = ctypes.c_uint64(0)
    whole_work = int(L.hc_seg_decompress_work_bound(ctypes.byref(info), len(enc))) + int(
        L.hc_seg_compress_work_bound2(len(raw), seg, flags, side))
    res = {"bytes": len(enc), "segments": info.n_segments, "whole_work_bound": whole_work, "lists": {}}

    host = np.zeros(align16(len(enc)), dtype=np.uint8)
    host[:len(enc)] = np.frombuffer(enc, dtype=np.uint8)
    inp = torch.from_numpy(host).cuda()
    dout = torch.empty(align16(cap), dtype=torch.uint8, device="cuda")
    draw = torch.empty(len(raw), dtype=torch.uint8, device="cuda")
    olen = torch.zeros(1, dtype=torch.int64, device="cuda")
    stt = torch.zeros(1, dtype=torch.int32, device="cuda")

    def events(fn):
        ts = []
        for i in range(2 + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            assert int(stt.item()) == 0
            if i >= 2:
                ts.append(e0.elapsed_time(e1))
        return round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)

    dec_work = hc.seg_decompress_dev(inp, draw, olen, stt, info=info, in_len=len(enc))
    enc_work = hc.seg_compress_dev(draw, dout, olen, stt, True, False, side, seg)
    for name, spans in lists.items():
        tri, at = [], 0
        for o, m in spans:
            tri.append((o, m, at))
            at += m
        data = rng.integers(0, 256, at, dtype=np.uint8).tobytes()
        arr, pd = hc.seg_patches(tri), ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p)
        st, covered, decoded = hc.seg_update_segments(info, len(enc), tri)
        assert st == 0
        if trace:  # the device call alone, for a kernel trace
            dpd = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
            w = hc.seg_update_dev(inp, tri, dpd, dout, olen, stt, info=info, in_len=len(enc))
            for _ in range(3):
                hc.seg_update_dev(inp, tri, dpd, dout, olen, stt, info=info, in_len=len(enc), work=w)
            torch.cuda.synchronize()
            continue
        new_raw = bytearray(raw)
        for o, m, s in tri:
            new_raw[o:o + m] = data[s:s + m]
        new_raw = bytes(new_raw)

        def update():
            rc = L.hc_seg_update(src, len(enc), arr, len(tri), pd, len(data), ctypes.cast(out, ctypes.c_void_p), cap,
                                 ctypes.byref(k), None)
            assert rc == 0, rc

        def alternative():
            rc = L.hc_seg_decompress(src, len(enc), ctypes.cast(alt_raw, ctypes.c_void_p), len(raw), ctypes.byref(k), None)
            assert rc == 0, rc
            for o, m, s in tri:
                ctypes.memmove(ctypes.addressof(alt_raw) + o, data[s:s + m], m)
            rc = L.hc_seg_compress2(ctypes.cast(alt_raw, ctypes.c_void_p), len(raw), flags, side, seg,
                                    ctypes.cast(alt_enc, ctypes.c_void_p), cap, ctypes.byref(k))
            assert rc == 0, rc

        r = {"patches": len(tri), "covered": covered, "decoded": decoded,
             "work_bound": hc.seg_update_work_bound(info, len(enc), tri),
             "update_ms": timed(update, 2, reps)}
        n_upd = k.value
        r["decode_patch_encode_ms"] = timed(alternative, 1, reps)
        assert out.raw[:n_upd] == alt_enc.raw[:k.value]  # the same container, byte for byte
        st, want = hc.seg_compress(new_raw, True, False, side, seg)
        assert st == 0 and out.raw[:n_upd] == want
        r["speedup"] = round(r["decode_patch_encode_ms"][0] / r["update_ms"][0], 2)

        dpd = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
        p_src = torch.tensor([s for _, _, s in tri], dtype=torch.int64, device="cuda")
        p_len = torch.tensor([m for _, m, _ in tri], dtype=torch.int64, device="cuda")
        p_dst = torch.tensor([o for o, _, _ in tri], dtype=torch.int64, device="cuda")
        w = hc.seg_update_dev(inp, tri, dpd, dout, olen, stt, info=info, in_len=len(enc))
        r["device_ms"] = events(lambda: hc.seg_update_dev(inp, tri, dpd, dout, olen, stt, info=info, in_len=len(enc), work=w))
        assert dout[:n_upd].cpu().numpy().tobytes() == want and int(olen.item()) == n_upd

        def dev_alternative():
            hc.seg_decompress_dev(inp, draw, olen, stt, info=info, in_len=len(enc), work=dec_work)
            hc.pack_batch(dpd, p_src, p_len, draw, p_dst)
            hc.seg_compress_dev(draw, dout, olen, stt, True, False, side, seg, work=enc_work)

        r["device_decode_patch_encode_ms"] = events(dev_alternative)
        assert dout[:n_upd].cpu().numpy().tobytes() == want
        r["device_speedup"] = round(r["device_decode_patch_encode_ms"][0] / r["device_ms"][0], 2)
        # faster by more than the run's own spread: the slowest update under the fastest alternative
        r["device_faster_beyond_spread"] = r["device_ms"][2] < r["device_decode_patch_encode_ms"][1]
        r["host_faster_beyond_spread"] = r["update_ms"][2] < r["decode_patch_encode_ms"][1]
        res["lists"][name] = r
    # the splice alone: no patch, so the call is the index scan, the seal and one copy of the container
    empty = torch.empty(16, dtype=torch.uint8, device="cuda")
    w = hc.seg_update_dev(inp, [], empty, dout, olen, stt, info=info, in_len=len(enc), patch_data_len=0)
    if trace:
        for _ in range(3):
            hc.seg_update_dev(inp, [], empty, dout, olen, stt, info=info, in_len=len(enc), patch_data_len=0, work=w)
        torch.cuda.synchronize()
        return None
    t = events(lambda: hc.seg_update_dev(inp, [], empty, dout, olen, stt, info=info, in_len=len(enc), patch_data_len=0,
                                         work=w))
    assert dout[:len(enc)].cpu().numpy().tobytes() == enc
    c = events(lambda: dout[:len(enc)].copy_(inp[:len(enc)]))
    res["splice"] = {"identity_ms": t, "bytes_per_s": round(2 * len(enc) / (t[0] * 1e-3)),
                     "device_copy_ms": c, "device_copy_bytes_per_s": round(2 * len(enc) / (c[0] * 1e-3)),
                     "note": "bytes read plus bytes written per second; identity_ms also holds the open and seal launches"}
    return res


def _ptrs(bufs):
    return (ctypes.c_void_p * len(bufs))(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])


def _u64s(vals):
    return (ctypes.c_uint64 * len(vals))(*vals)


def batch_containers(raw, diff, adapt, n, reps, trace):
    """n inputs of BATCH_ITEM bytes through one hc_seg_*_host_batch call and through n single calls"""
    L = hc.lib()
    seg = 65536
    flags = (hc.HC_FLAG_DIFF if diff else 0) | (hc.HC_FLAG_ADAPT if adapt else 0)
    pieces = [raw[k * BATCH_ITEM:(k + 1) * BATCH_ITEM] for k in range(n)]
    cap = int(L.hc_seg_compress_bound2(BATCH_ITEM, seg, flags, BATCH_SIDE))
    ins = [ctypes.c_char_p(p) for p in pieces]
    encs = [ctypes.create_string_buffer(cap) for _ in range(n)]
    decs = [ctypes.create_string_buffer(BATCH_ITEM) for _ in range(n)]
    in_p, enc_p, dec_p = _ptrs(ins), _ptrs(encs), _ptrs(decs)
    in_lens, widths, caps, raw_caps = (_u64s([v] * n) for v in (BATCH_ITEM, BATCH_SIDE, cap, BATCH_ITEM))
    enc_lens, dec_lens = _u64s([0] * n), _u64s([0] * n)
    st = (ctypes.c_int32 * n)()
    k = ctypes.c_uint64(0)

    def enc_batch():
        rc = L.hc_seg_compress_host_batch(in_p, in_lens, widths, n, flags, seg, enc_p, caps, enc_lens, st)
        assert rc == 0 and not any(st), (rc, list(st))

    def dec_batch():
        rc = L.hc_seg_decompress_host_batch(enc_p, enc_lens, None, None, n, dec_p, raw_caps, dec_lens, st, None)
        assert rc == 0 and not any(st), (rc, list(st))

    def enc_loop():
        for i in range(n):
            rc = L.hc_seg_compress2(in_p[i], BATCH_ITEM, flags, BATCH_SIDE, seg, enc_p[i], cap, ctypes.byref(k))
            assert rc == 0 and k.value == enc_lens[i], rc

    def dec_loop():
        for i in range(n):
            rc = L.hc_seg_decompress(enc_p[i], enc_lens[i], dec_p[i], BATCH_ITEM, ctypes.byref(k), None)
            assert rc == 0 and k.value == BATCH_ITEM, rc

    if trace:
        for _ in range(2):
            enc_batch()
            dec_batch()
        return None
    enc_batch()
    batch_enc = [e.raw[:m] for e, m in zip(encs, enc_lens)]
    r = {"items": n, "bytes": sum(enc_lens), "segments_per_item": hc.seg_count(BATCH_ITEM, seg, adapt, BATCH_SIDE)}
    r["encode_batch_ms"] = timed(enc_batch, 2, reps)
    r["encode_loop_ms"] = timed(enc_loop, 1, reps)
    assert [e.raw[:m] for e, m in zip(encs, enc_lens)] == batch_enc  # the loop wrote the same containers
    for d in decs:
        ctypes.memset(d, 0, BATCH_ITEM)
    r["decode_batch_ms"] = timed(dec_batch, 2, reps)
    assert all(d.raw == p for d, p in zip(decs, pieces))
    r["decode_loop_ms"] = timed(dec_loop, 1, reps)
    r["encode_speedup"] = round(r["encode_loop_ms"][0] / r["encode_batch_ms"][0], 2)
    r["decode_speedup"] = round(r["decode_loop_ms"][0] / r["decode_batch_ms"][0], 2)
    return r


def batch_ranges(raw, reps, trace, reads=64, length=4096):
    """`reads` ranged reads of one 4096x4096 -m container at 64 KiB segments: one call against a loop"""
    L = hc.lib()
    st, enc = hc.seg_compress(raw, True, False, SIDE, 65536)
    assert st == 0, st
    ranges = [(k * (len(raw) // reads) + 8192, length) for k in range(reads)]  # each inside one segment
    src = ctypes.c_char_p(enc)
    outs = [ctypes.create_string_buffer(length) for _ in range(reads)]
    in_p, out_p = _ptrs([src] * reads), _ptrs(outs)
    in_lens, caps = _u64s([len(enc)] * reads), _u64s([length] * reads)
    offs, lens, out_lens = _u64s([o for o, _ in ranges]), _u64s([m for _, m in ranges]), _u64s([0] * reads)
    stt = (ctypes.c_int32 * reads)()
    k = ctypes.c_uint64(0)

    def batch():
        rc = L.hc_seg_decompress_host_batch(in_p, in_lens, offs, lens, reads, out_p, caps, out_lens, stt, None)
        assert rc == 0 and not any(stt), (rc, list(stt))

    def loop():
        for i, (o, m) in enumerate(ranges):
            rc = L.hc_seg_decompress_range(in_p[i], len(enc), o, m, out_p[i], m, ctypes.byref(k), None)
            assert rc == 0 and k.value == m, rc

    if trace:
        batch()
        batch()
        return None
    r = {"reads": reads, "length": length, "container_bytes": len(enc), "batch_ms": timed(batch, 2, reps)}
    assert all(b.raw == raw[o:o + m] for b, (o, m) in zip(outs, ranges))
    r["loop_ms"] = timed(loop, 1, reps)
    r["speedup"] = round(r["loop_ms"][0] / r["batch_ms"][0], 2)
    return r


def batch_bench(reps, trace):
    big = photo(BATCH_SIDE)
    res = {"input": f"{BATCH_ITEM}-byte pieces ({BATCH_ITEM // BATCH_SIDE} rows) of a synthetic photo {BATCH_SIDE}x{BATCH_SIDE}, "
                    "64 KiB segments", "timing": "host clock around each synchronous host-buffer call or loop of calls "
                    "(copies included), median [min, max] ms of %d" % reps, "containers": {}}
    for name, (diff, adapt) in (("-m", (1, 0)), ("-a -m", (1, 1))):
        for n in BATCH_NS:
            res["containers"][f"{name} x{n}"] = batch_containers(big, diff, adapt, n, reps, trace)
    res["ranges"] = batch_ranges(photo(), reps, trace)
    return res


def full_bytes(seg, adapt, width):
    """raw bytes of every segment but the last (the cut rule of include/hcodec.h)"""
    return max(8, (seg // width) & ~3) * width if adapt else seg


def glue_share(path):
    glue = total = 0
    per = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            ns = int(float(row["TotalDurationNs"]))
            total += ns
            for g in GLUE:
                if g in row["Name"]:
                    glue += ns
                    per[g] = per.get(g, 0) + ns
    return {"device_ms": round(total / 1e6, 3), "glue_ms": round(glue / 1e6, 3),
            "glue_share": round(glue / total, 5) if total else None,
            "glue_kernels_ms": {k: round(v / 1e6, 4) for k, v in per.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--glue-from")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--whole-reps", type=int, default=2)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--no-whole", action="store_true")
    ap.add_argument("--sizes", type=int, nargs="+", default=list(SIZES))
    ap.add_argument("--range", action="store_true")
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--batch", action="store_true")
    ap.add_argument("--update", action="store_true")
    a = ap.parse_args()
    if not hc.device_ok():
        sys.exit("seg_bench.py needs a gfx950 device: " + hc.device_info())
    if a.update:
        side = 4 * SIDE if a.big else SIDE
        raw = photo(side)
        res = {"input": f"synthetic photo {side}x{side} ({len(raw)} bytes), -m, 64 KiB segments", "timing":
               "update_ms, decode_patch_encode_ms: host clock around the synchronous host-buffer calls (copies included); "
               "device_*: HIP events around the device calls; median [min, max] ms of %d" % a.reps}
        if a.trace_run:
            update_bench(raw, side, a.reps, True)
            return
        res.update(update_bench(raw, side, a.reps))
        print(json.dumps(res))
        return
    if a.batch:
        res = batch_bench(a.reps, a.trace_run)
        if a.trace_run:
            return
        if a.glue_from:
            res["glue"] = glue_share(a.glue_from)
        print(json.dumps(res))
        return
    if a.range:
        raw = photo()
        if a.trace_run:
            for diff, adapt in ((1, 0), (1, 1)):
                range_bench(raw, SIDE, diff, adapt, 65536, 3, False)
            return
        res = {"input": f"synthetic photo {SIDE}x{SIDE} ({len(raw)} bytes)", "timing":
               "range_ms, whole_and_slice_ms: host clock around each synchronous host-buffer call (copies included); "
               "device_ms: HIP events around the device call; median [min, max] ms of %d" % a.reps, "cases": {}}
        for name, (diff, adapt) in (("-m", (1, 0)), ("-a -m", (1, 1))):
            for seg in (16384, 65536):
                res["cases"][f"{name} {seg}"] = range_bench(raw, SIDE, diff, adapt, seg, a.reps, True)
        if a.big:
            raw = photo(4 * SIDE)
            res["big_input"] = f"synthetic photo {4 * SIDE}x{4 * SIDE} ({len(raw)} bytes)"
            res["cases"]["big -m 65536"] = range_bench(raw, 4 * SIDE, 1, 0, 65536, a.reps, True)
        if a.glue_from:
            res["glue"] = glue_share(a.glue_from)
        print(json.dumps(res))
        return
    b = Buffers(photo())
    if a.trace_run:
        for diff, adapt in MODES.values():
            for _ in range(3):
                b.seg_decode(b.seg_encode(diff, adapt, 65536, a.check))
            assert b.exact()
        return
    res = {"input": f"synthetic photo {SIDE}x{SIDE} ({len(b.raw)} bytes)", "timing":
           "host clock around each synchronous host-buffer call (copies included), median [min, max] ms",
           "modes": {}}
    for name, (diff, adapt) in MODES.items():
        m = {"segmented": {}}
        if not a.no_whole:
            n = b.whole_encode(diff, adapt)
            enc = timed(lambda: b.whole_encode(diff, adapt), 0, a.whole_reps)
            dec = timed(lambda: b.whole_decode(n), 1, a.whole_reps)
            assert b.exact()
            m["whole"] = {"bytes": n, "encode_ms": enc, "decode_ms": dec}
        for seg in a.sizes:
            k = b.seg_encode(diff, adapt, seg)
            e = timed(lambda: b.seg_encode(diff, adapt, seg), 2, a.reps)
            b.dec = ctypes.create_string_buffer(len(b.raw))
            d = timed(lambda: b.seg_decode(k), 2, a.reps)
            assert b.exact()
            r = {"bytes": k, "segments": hc.seg_count(len(b.raw), seg, adapt, SIDE), "encode_ms": e, "decode_ms": d}
            if not a.no_whole:
                r.update({"size_ratio": round(k / n, 5), "encode_speedup": round(enc[0] / e[0], 1),
                          "decode_speedup": round(dec[0] / d[0], 1)})
            if a.check:
                kc = b.seg_encode(diff, adapt, seg, True)
                ec = timed(lambda: b.seg_encode(diff, adapt, seg, True), 2, a.reps)
                b.dec = ctypes.create_string_buffer(len(b.raw))
                dc = timed(lambda: b.seg_decode(kc), 2, a.reps)
                assert b.exact()
                r["check"] = {"bytes": kc, "encode_ms": ec, "decode_ms": dc}
            m["segmented"][str(seg)] = r
        res["modes"][name] = m
    if a.glue_from:
        res["glue"] = glue_share(a.glue_from)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

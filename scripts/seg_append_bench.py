#!/usr/bin/env python3
"""Append to a segmented container against coding the whole again.

The container is the synthetic SIDE x SIDE photo (hc.synth_batch; default 16384: 256 MiB) in -m at
64 KiB segments, the workload of the range write's figures. Two appends, 64 KiB and 16 MiB of the
same kind of data (rows of a second photo), each through

  hc_seg_append          host buffers: host clock around the synchronous call, copies included
  hc_seg_append_dev      device buffers: HIP events around the call on the current stream

and each against what the other calls offer for the job, in the same process: hc_seg_decompress,
the concatenation, hc_seg_compress2 of the whole (host), and hc_seg_decompress_dev, a device copy of
the added bytes behind the decoded ones, hc_seg_compress_dev (device). Every figure is the median
(min, max) of the repeats after warm-up, and the results are compared byte for byte.

Beside the times: the device bytes the host call allocates and the bytes it moves over PCIe, both
counted from the container's index and the library's bounds (what hc_seg_append uploads: header
and index, the decoded segment's stream, the added bytes; what it downloads: 32 bytes of verdict,
the coded segments' index words, their streams), and the same for the whole-container path.
The photo's raw bytes are a multiple of the segment size, so these two appends decode nothing
(K == n); --open adds the 64 KiB append to the container of the photo less its last 32 KiB, whose
half-filled last segment is decoded first. --small adds the host append to the SIDE/4 x SIDE/4
container (1/16 of the kept bytes), to see what of the host call's time follows the kept bytes.
Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "huffman-codec_amd", "python"))

import hcodec as hc  # noqa: E402

SEG = 65536
ADDS = {"64KiB": 65536, "16MiB": 16 << 20}


def align16(x):
    return (x + 15) & ~15


def photo(side, k0, rows=None):
    import torch
    rows = side if rows is None else rows
    raw = torch.empty(side * rows, dtype=torch.uint8, device="cuda")
    hc.synth_batch("photo", k0, 1, side, rows, raw, side * rows)
    torch.cuda.synchronize()
    return raw.cpu().numpy().tobytes()


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)


def host_counts(enc, info, add_len, new_len):
    """the host call's device bytes and PCIe bytes, from the index and the bounds"""
    L = hc.lib()
    n = info.n_segments
    st, ninfo, k, dec = hc.seg_append_plan(info, len(enc), add_len)
    coded = ninfo.n_segments - k
    first = align16(48 + 8 * n)
    off, kept_end, last_len = first, first, 0  # the index walk: where the kept block ends, the decoded stream's length
    for j, m in enumerate(struct.unpack_from(f"<{n}Q", enc, 48)):
        if j + 1 == k:
            kept_end = off + m
        if j == n - 1 and dec:
            last_len = m
        off = align16(off + m)
    slots = hc.seg_append_bound(info, len(enc), add_len) - len(enc) - align16(8 * (ninfo.n_segments - n)) - 16
    work = hc.seg_append_work_bound(info, len(enc), add_len)
    new_first = align16(48 + 8 * ninfo.n_segments)
    gathered = new_len - (new_first + align16(kept_end - first))
    up = first + last_len + add_len
    down = 32 + 8 * coded + gathered
    return {"coded_segments": coded, "decoded_segments": dec, "device_bytes": first + last_len + add_len + slots + work + 32,
            "pcie_up": up, "pcie_down": down, "work_bound": work}


def bench(raw, side, reps, whole_reps, adds):
    import numpy as np
    import torch
    L = hc.lib()
    flags = hc.HC_FLAG_DIFF
    st, enc = hc.seg_compress(raw, True, False, side, SEG)
    assert st == 0, st
    st, info = hc.seg_info(enc)
    tail_src = photo(side, 1, max(adds.values()) // side)
    res = {"side": side, "raw_bytes": len(raw), "container_bytes": len(enc), "segments": info.n_segments, "appends": {}}
    src = ctypes.cast(ctypes.c_char_p(enc), ctypes.c_void_p)
    cap = 2 * len(enc) + 8 * max(adds.values()) + (1 << 20)  # (room for every result here; the bound is about 6x the raw bytes)
    out = ctypes.create_string_buffer(cap)
    alt_raw = ctypes.create_string_buffer(len(raw) + max(adds.values()))
    alt_enc = ctypes.create_string_buffer(cap)
    k = ctypes.c_uint64(0)

    host = np.zeros(align16(len(enc)), dtype=np.uint8)
    host[:len(enc)] = np.frombuffer(enc, dtype=np.uint8)
    inp = torch.from_numpy(host).cuda()
    dout = torch.empty(align16(cap), dtype=torch.uint8, device="cuda")
    draw = torch.empty(len(raw) + max(adds.values()), dtype=torch.uint8, device="cuda")
    olen = torch.zeros(1, dtype=torch.int64, device="cuda")
    stt = torch.zeros(1, dtype=torch.int32, device="cuda")

    def events(fn, n):
        ts = []
        for i in range(2 + n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            assert int(stt.item()) == 0
            if i >= 2:
                ts.append(e0.elapsed_time(e1))
        return round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)

    dec_work = hc.seg_decompress_dev(inp, draw, olen, stt, info=info, in_len=len(enc), out_cap=len(raw))
    for name, add_len in adds.items():
        tail = tail_src[:add_len]
        tp = ctypes.cast(ctypes.c_char_p(tail), ctypes.c_void_p)

        def append():
            rc = L.hc_seg_append(src, len(enc), tp, add_len, ctypes.cast(out, ctypes.c_void_p), cap, ctypes.byref(k), None)
            assert rc == 0, rc

        def alternative():
            rc = L.hc_seg_decompress(src, len(enc), ctypes.cast(alt_raw, ctypes.c_void_p), len(raw), ctypes.byref(k), None)
            assert rc == 0, rc
            ctypes.memmove(ctypes.addressof(alt_raw) + len(raw), tail, add_len)
            rc = L.hc_seg_compress2(ctypes.cast(alt_raw, ctypes.c_void_p), len(raw) + add_len, flags, side, SEG,
                                    ctypes.cast(alt_enc, ctypes.c_void_p), cap, ctypes.byref(k))
            assert rc == 0, rc

        r = {"add_bytes": add_len, "append_ms": timed(append, 2, reps)}
        n_app = k.value
        r["decode_concat_encode_ms"] = timed(alternative, 1, whole_reps)
        assert out.raw[:n_app] == alt_enc.raw[:k.value]  # the same container, byte for byte
        r["speedup"] = round(r["decode_concat_encode_ms"][0] / r["append_ms"][0], 2)
        r["host_faster_beyond_spread"] = r["append_ms"][2] < r["decode_concat_encode_ms"][1]
        r.update(host_counts(enc, info, add_len, n_app))
        whole_work = int(L.hc_seg_decompress_work_bound(ctypes.byref(info), len(enc))) + int(
            L.hc_seg_compress_work_bound2(len(raw) + add_len, SEG, flags, side))
        dec_work_b = int(L.hc_seg_decompress_work_bound(ctypes.byref(info), len(enc)))
        r["whole_device_bytes"] = max(len(enc) + len(raw) + dec_work_b,  # the two calls one after the other: the larger
                                      len(raw) + add_len + (whole_work - dec_work_b)
                                      + hc.seg_compress_bound(len(raw) + add_len, SEG, False, side))
        r["whole_pcie_up"] = len(enc) + len(raw) + add_len
        r["whole_pcie_down"] = len(raw) + n_app
        want = out.raw[:n_app]

        dadd = torch.from_numpy(np.frombuffer(tail, dtype=np.uint8).copy()).cuda()
        w = hc.seg_append_dev(inp, dadd, dout, olen, stt, info=info, in_len=len(enc))
        r["device_ms"] = events(lambda: hc.seg_append_dev(inp, dadd, dout, olen, stt, info=info, in_len=len(enc), work=w), reps)
        assert int(olen.item()) == n_app and dout[:n_app].cpu().numpy().tobytes() == want
        whole = draw[:len(raw) + add_len]
        enc_work = hc.seg_compress_dev(whole, dout, olen, stt, True, False, side, SEG)

        def dev_alternative():
            hc.seg_decompress_dev(inp, draw, olen, stt, info=info, in_len=len(enc), work=dec_work, out_cap=len(raw))
            draw[len(raw):len(raw) + add_len].copy_(dadd)
            hc.seg_compress_dev(whole, dout, olen, stt, True, False, side, SEG, work=enc_work)

        r["device_decode_concat_encode_ms"] = events(dev_alternative, whole_reps)
        assert dout[:n_app].cpu().numpy().tobytes() == want
        r["device_speedup"] = round(r["device_decode_concat_encode_ms"][0] / r["device_ms"][0], 2)
        r["device_faster_beyond_spread"] = r["device_ms"][2] < r["device_decode_concat_encode_ms"][1]
        res["appends"][name] = r
        del dadd, w, enc_work
    # the kept block's copy alone, beside the 64 KiB append's device time
    c = events(lambda: dout[:len(enc)].copy_(inp[:len(enc)]), reps)
    res["device_copy_of_the_container_ms"] = c
    return res


def small_host(side, reps):
    """the host append of 64 KiB to the container of a photo 1/16 the size"""
    raw = photo(side, 0)
    st, enc = hc.seg_compress(raw, True, False, side, SEG)
    assert st == 0
    tail = photo(side, 1, 65536 // side)
    L = hc.lib()
    cap = hc.seg_compress_bound(len(raw) + len(tail), SEG, False, side)
    out = ctypes.create_string_buffer(cap)
    k = ctypes.c_uint64(0)
    src, tp = ctypes.cast(ctypes.c_char_p(enc), ctypes.c_void_p), ctypes.cast(ctypes.c_char_p(tail), ctypes.c_void_p)

    def append():
        rc = L.hc_seg_append(src, len(enc), tp, len(tail), ctypes.cast(out, ctypes.c_void_p), cap, ctypes.byref(k), None)
        assert rc == 0, rc

    t = timed(append, 2, reps)
    assert out.raw[:k.value] == hc.seg_compress(raw + tail, True, False, side, SEG)[1]
    return {"side": side, "container_bytes": len(enc), "append_64KiB_ms": t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--whole-reps", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--open", action="store_true")
    a = ap.parse_args()
    if not hc.device_ok():
        sys.exit("seg_append_bench: no usable gfx950 device")
    raw = photo(a.side, 0)
    res = bench(raw, a.side, a.reps, a.whole_reps, ADDS)
    if a.open:  # the last segment half full: it is decoded, and two segments are coded
        res["open"] = bench(raw[:-SEG // 2], a.side, a.reps, a.whole_reps, {"64KiB": 65536})
    if a.small:
        res["small"] = small_host(a.side // 4, a.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

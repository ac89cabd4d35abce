#!/usr/bin/env python3
"""List read of a segmented container against what the other calls offer for a tile.

The input is the synthetic 16384x16384 photo (256 MiB) in -m at 64 KiB segments, four image rows a
segment. A W x W tile (256 and 512) in the middle is read three ways with device buffers, under
HIP events, and three ways with host buffers, under the host clock (copies included):

  list    hc_seg_decompress_ranges_dev / hc_seg_decompress_ranges: one read per row
  batch   hc_seg_decompress_batch_dev / hc_seg_decompress_host_batch: one ranged item per row, all
          naming the same container
  whole   hc_seg_decompress_dev / hc_seg_decompress, then the slices

The three are run in turn, repeat by repeat, so that what else the machine does falls on all of
them; median [min, max] ms. Beside the times: the work bounds (exact, from the formulas), the
device memory the batch call's output takes, and the bytes each host call uploads. --side and
--tiles shrink the case. Prints one JSON line.
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


def align16(x):
    return (x + 15) & ~15


def photo(side):
    import torch
    n = side * side
    raw = torch.empty(n, dtype=torch.uint8, device="cuda")
    hc.synth_batch("photo", 0, 1, side, side, raw, n)
    torch.cuda.synchronize()
    return raw.cpu().numpy().tobytes()


def stats(ts):
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]


def in_turn(fns, warmup, reps):
    """{name: [median, min, max] ms}: every fn once per repeat, in turn; each returns its own ms"""
    ts = {k: [] for k in fns}
    for i in range(warmup + reps):
        for k, fn in fns.items():
            t = fn()
            if i >= warmup:
                ts[k].append(t)
    return {k: stats(v) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=16384)
    ap.add_argument("--tiles", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    if not hc.device_ok():
        sys.exit("seg_reads_bench.py needs a gfx950 device: " + hc.device_info())
    import numpy as np
    import torch
    L = hc.lib()
    side = a.side
    raw = photo(side)
    st, enc = hc.seg_compress(raw, True, False, side, SEG)
    assert st == 0, st
    st, info = hc.seg_info(enc)
    n = info.n_segments
    lens = struct.unpack_from(f"<{n}Q", enc, 48)
    idx = align16(48 + 8 * n)
    offs, o = [], idx
    for m in lens:
        offs.append(o)
        o = align16(o + m)
    img = np.frombuffer(raw, dtype=np.uint8).reshape(side, side)
    res = {"input": f"synthetic photo {side}x{side} ({len(raw)} bytes), -m, 64 KiB segments ({n}), container {len(enc)} bytes",
           "timing": "device: HIP events around the device call; host: host clock around the synchronous host-buffer call "
                     "(copies included); list, batch and whole in turn each repeat; median [min, max] ms of %d" % a.reps,
           "whole_work_bound": int(L.hc_seg_decompress_work_bound(ctypes.byref(info), len(enc))), "tiles": {}}

    host = np.zeros(align16(len(enc)), dtype=np.uint8)
    host[:len(enc)] = np.frombuffer(enc, dtype=np.uint8)
    inp = torch.from_numpy(host).cuda()
    draw = torch.empty(len(raw), dtype=torch.uint8, device="cuda")
    olen = torch.zeros(1, dtype=torch.int64, device="cuda")
    stt = torch.zeros(1, dtype=torch.int32, device="cuda")
    src = ctypes.cast(ctypes.c_char_p(enc), ctypes.c_void_p)
    whole_buf = ctypes.create_string_buffer(len(raw))
    k = ctypes.c_uint64(0)
    whole_work = hc.seg_decompress_dev(inp, draw, olen, stt, info=info, in_len=len(enc))

    def events(fn, ok):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        assert ok()
        return e0.elapsed_time(e1)

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    for W in a.tiles:
        x0, y0 = side // 2 + 40, side // 2 + 3
        st, reads = hc.seg_rect_reads(len(raw), side, x0, y0, W, W)
        assert st == 0
        tile = img[y0:y0 + W, x0:x0 + W].tobytes()
        st, covered, need = hc.seg_reads_segments(info, len(enc), reads)
        assert st == 0 and need == W * W
        ks = sorted({o // SEG for o, m, d in reads} | {(o + m - 1) // SEG for o, m, d in reads})
        assert len(ks) == covered
        r = {"reads": len(reads), "covered": covered, "rows_per_segment": round(len(reads) / covered, 2)}

        # device buffers
        items = [(0, len(enc), info, o, m, align16(d), m) for o, m, d in reads]  # (every out_off a multiple of 16: W is)
        assert all(d % 16 == 0 for o, m, d in reads)
        r["list_work_bound"] = hc.seg_decompress_ranges_work_bound(info, len(enc), reads)
        r["batch_work_bound"] = hc.seg_decompress_batch_work_bound(items)
        dlist = torch.zeros(W * W, dtype=torch.uint8, device="cuda")
        dbatch = torch.zeros(W * W, dtype=torch.uint8, device="cuda")
        lens_b = torch.zeros(len(reads), dtype=torch.int64, device="cuda")
        st_b = torch.full((len(reads),), -1, dtype=torch.int32, device="cuda")
        wl = hc.seg_decompress_ranges_dev(inp, reads, dlist, olen, stt, info=info, in_len=len(enc))
        wb = hc.seg_decompress_batch_dev(inp, dbatch, items, lens_b, st_b)
        torch.cuda.synchronize()
        assert dlist.cpu().numpy().tobytes() == tile == dbatch.cpu().numpy().tobytes()
        rows = torch.arange(W, device="cuda").unsqueeze(1) * side + torch.arange(W, device="cuda").unsqueeze(0) \
            + (y0 * side + x0)

        def dev_whole():
            hc.seg_decompress_dev(inp, draw, olen, stt, info=info, in_len=len(enc), work=whole_work)
            dlist.copy_(draw[rows.reshape(-1)])

        # the library calls themselves, on lists built once: no wrapper's work inside the timed window
        c_reads, c_items = hc.seg_reads(reads), hc.seg_dec_items(items)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda t: ctypes.c_void_p(t.data_ptr())

        def dev_list():
            rc = L.hc_seg_decompress_ranges_dev(p(inp), len(enc), ctypes.byref(info), c_reads, len(reads), p(dlist), W * W,
                                                p(olen), p(stt), None, p(wl), wl.numel(), stream)
            assert rc == 0, rc

        def dev_batch():
            rc = L.hc_seg_decompress_batch_dev(p(inp), p(dbatch), c_items, len(items), p(lens_b), p(st_b), None, p(wb),
                                               wb.numel(), stream)
            assert rc == 0, rc

        r["device_ms"] = in_turn({
            "list": lambda: events(dev_list, lambda: int(stt.item()) == 0),
            "batch": lambda: events(dev_batch, lambda: not bool(st_b.any().item())),
            "whole": lambda: events(dev_whole, lambda: int(stt.item()) == 0),
        }, 2, a.reps)
        assert dlist.cpu().numpy().tobytes() == tile

        # host buffers
        arr = hc.seg_reads(reads)
        out = ctypes.create_string_buffer(W * W)
        P = len(reads)
        outs = [ctypes.create_string_buffer(W) for _ in range(P)]
        in_p = (ctypes.c_void_p * P)(*[src] * P)
        out_p = (ctypes.c_void_p * P)(*[ctypes.cast(b, ctypes.c_void_p) for b in outs])
        u64s = lambda v: (ctypes.c_uint64 * P)(*v)
        in_lens, caps, out_lens = u64s([len(enc)] * P), u64s([W] * P), u64s([0] * P)
        r_offs, r_lens = u64s([o for o, m, d in reads]), u64s([m for o, m, d in reads])
        st_h = (ctypes.c_int32 * P)()

        def host_list():
            rc = L.hc_seg_decompress_ranges(src, len(enc), arr, P, ctypes.cast(out, ctypes.c_void_p), W * W, ctypes.byref(k), None)
            assert rc == 0 and k.value == W * W, rc

        def host_batch():
            rc = L.hc_seg_decompress_host_batch(in_p, in_lens, r_offs, r_lens, P, out_p, caps, out_lens, st_h, None)
            assert rc == 0 and not any(st_h), (rc, list(st_h))

        def host_whole():
            rc = L.hc_seg_decompress(src, len(enc), ctypes.cast(whole_buf, ctypes.c_void_p), len(raw), ctypes.byref(k), None)
            assert rc == 0, rc
            return b"".join(whole_buf[o:o + m] for o, m, d in reads)

        r["host_ms"] = in_turn({"list": lambda: clock(host_list), "batch": lambda: clock(host_batch),
                                "whole": lambda: clock(host_whole)}, 1, a.reps)
        assert out.raw == tile == b"".join(b.raw for b in outs) == host_whole()
        span = lambda a_, b_: offs[b_] + lens[b_] - offs[a_]
        r["uploaded"] = {"list": idx + span(ks[0], ks[-1]),
                         "batch": sum(idx + span(o // SEG, (o + m - 1) // SEG) for o, m, d in reads),
                         "whole": len(enc)}
        d, h = r["device_ms"], r["host_ms"]
        # not slower beyond the run's own spread: the list call's median under the batch call's slowest repeat
        r["device_list_within_spread_of_batch"] = d["list"][0] <= d["batch"][2]
        r["host_list_within_spread_of_batch"] = h["list"][0] <= h["batch"][2]
        res["tiles"][f"{W}x{W}"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()

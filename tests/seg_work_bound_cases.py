"""The argument table of tests/test_seg_work_bounds.py: every public work bound of the segmented
container (hc_seg_*_work_bound*, and the write calls' output bounds hc_seg_update_bound and
hc_seg_append_bound beside theirs) over small arguments, as `key -> thunk` pairs. The bounds are host
arithmetic: no call here needs a device. tests/golden/make_seg_work_bounds.py records the values."""
import ctypes

DIFF, ADAPT, CHECK = 0x80, 0x40, 0x100
WIDTH = 512
# the last three are whole matrices of WIDTH columns: 8 rows (one band at any size), 133 rows (the
# last band takes leftover rows) and 200 rows
IN_LENS = (0, 1, 17, 64, 32789, 2**20 + 3, 8 * WIDTH, 133 * WIDTH, 200 * WIDTH)
SEG_BYTES = (0, 16, 65536)
FLAGS = (0, CHECK, DIFF, DIFF | CHECK, ADAPT, ADAPT | CHECK)


def align16(x):
    return (x + 15) & ~15


def _containers(hc, seg):
    """(name, info, container length) of every table entry the encoder takes, at one segment size.
    The length is a made-up one that passes the header rules; no bound reads more than that."""
    L = hc.lib()
    out = []
    for n in IN_LENS:
        for fl in FLAGS:
            adapt = bool(fl & ADAPT)
            k = int(L.hc_seg_count(n, seg, int(adapt), WIDTH))
            if k == 0:
                continue
            info = hc.SegInfo(n, seg or hc.HC_SEG_DEFAULT_BYTES, WIDTH if adapt else 0, k, fl)
            out.append((f"in={n} seg={seg} flags={fl:#x}", info, align16(48 + 12 * k) + 2 * n + 64 * k))
    return out


def _ranges(info):
    """whole as a range, aligned, one byte further on, empty, and whole segments alone"""
    raw = info.raw_len
    full = max(8, (info.seg_bytes // WIDTH) & ~3) * WIDTH if info.flags & ADAPT else info.seg_bytes
    a, m = (raw // 3) & ~3, raw // 2
    r = [("all", 0, raw), ("aligned", a, m), ("aligned+1", a + 1, m), ("empty", a, 0)]
    if raw > full:
        r.append(("segments", full, min(full, raw - full)))
    return r


def _copy(info, **changes):
    c = type(info)(info.raw_len, info.seg_bytes, info.width, info.n_segments, info.flags)
    for k, v in changes.items():
        setattr(c, k, v)
    return c


def _full(info):
    """the cut of every segment but the last"""
    return max(8, (info.seg_bytes // WIDTH) & ~3) * WIDTH if info.flags & ADAPT else info.seg_bytes


def _patch_lists(info):
    """{name: [(offset, length, src_off)]} for a range write: no segment, one in part, one whole,
    several with the last one among them (an adaptive container's last cut may be longer than
    `full`: there "tail" covers the last segment in part)"""
    raw, full = info.raw_len, _full(info)
    p = {"none": [], "empty": [(raw // 2, 0, 0)]}
    if raw:
        p["partial"] = [(raw // 3, 1, 0)]
        p["whole"] = [(0, min(full, raw), 0)]
    if raw > 2:
        spans = [(0, 1)]
        if raw > 2 * full + 2:  # across a cut, behind the first patch's segment
            spans.append((2 * full - 1, 2))
        spans.append((raw - 1, 1))
        at, p["several"] = 0, []
        for o, m in spans:
            p["several"].append((o, m, at))
            at += m
    if raw > full:  # the last segment whole and the one before it in part
        last = (raw - 1) // full * full
        p["tail"] = [(last - 1, raw - last + 1, 0)]
    return p


def _add_lens(info):
    """0, 1, 16 (in an adaptive container, whose rows are whole: one that the call refuses, 1 row
    and 16 rows), one that closes the last cut exactly, and one that leaves an open tail behind it"""
    full, unit = _full(info), WIDTH if info.flags & ADAPT else 1
    close = -info.raw_len % full or full
    return [0, 1, unit, 16 * unit, close, close + full + unit]


def _write_cases(hc, out, name, info, clen):
    """the four bounds of the write calls (range write, append) over one container"""
    L = hc.lib()
    for pname, tri in _patch_lists(info).items():
        arr = hc.seg_patches(tri)
        out[f"update_bound {name} {pname}"] = (
            lambda info=info, arr=arr, k=len(tri): L.hc_seg_update_bound(ctypes.byref(info), clen, arr, k))
        out[f"update_work {name} {pname}"] = (
            lambda info=info, arr=arr, k=len(tri): L.hc_seg_update_work_bound(ctypes.byref(info), clen, arr, k))
    for add in _add_lens(info):
        out[f"append_bound {name} add={add}"] = (
            lambda info=info, add=add: L.hc_seg_append_bound(ctypes.byref(info), clen, add))
        out[f"append_work {name} add={add}"] = (
            lambda info=info, add=add: L.hc_seg_append_work_bound(ctypes.byref(info), clen, add))
    if info.raw_len != 17:
        return
    # arguments that the calls refuse (0), and an info that fails the rules (16: no workspace; no bound)
    refused = {"unsorted": [(8, 2, 0), (0, 2, 2)], "overlap": [(0, 4, 0), (3, 2, 4)],
               "outside": [(info.raw_len, 1, 0)], "length wraps": [(1, 2**64 - 1, 0)]}
    for pname, tri in refused.items():
        arr = hc.seg_patches(tri)
        out[f"update_bound {name} {pname}"] = (
            lambda info=info, arr=arr, k=len(tri): L.hc_seg_update_bound(ctypes.byref(info), clen, arr, k))
        out[f"update_work {name} {pname}"] = (
            lambda info=info, arr=arr, k=len(tri): L.hc_seg_update_work_bound(ctypes.byref(info), clen, arr, k))
    out[f"append_bound {name} add wraps"] = lambda info=info: L.hc_seg_append_bound(ctypes.byref(info), clen, 2**64 - 1)
    out[f"append_work {name} add wraps"] = lambda info=info: L.hc_seg_append_work_bound(ctypes.byref(info), clen, 2**64 - 1)
    bad = _copy(info, n_segments=info.n_segments + 1)
    one = hc.seg_patches([(0, 1, 0)])
    out[f"update_bound {name} bad info"] = lambda bad=bad: L.hc_seg_update_bound(ctypes.byref(bad), clen, one, 1)
    out[f"update_work {name} bad info"] = lambda bad=bad: L.hc_seg_update_work_bound(ctypes.byref(bad), clen, one, 1)
    out[f"append_bound {name} bad info"] = lambda bad=bad: L.hc_seg_append_bound(ctypes.byref(bad), clen, 1)
    out[f"append_work {name} bad info"] = lambda bad=bad: L.hc_seg_append_work_bound(ctypes.byref(bad), clen, 1)


def cases(hc):
    """{key: thunk}: each thunk calls one bound"""
    L = hc.lib()
    out = {}
    for n in IN_LENS:
        for seg in SEG_BYTES:
            for fl in FLAGS:
                out[f"compress2 in={n} seg={seg} flags={fl:#x}"] = (
                    lambda n=n, seg=seg, fl=fl: L.hc_seg_compress_work_bound2(n, seg, fl, WIDTH))
            for adapt in (0, 1):
                out[f"compress in={n} seg={seg} adapt={adapt}"] = (
                    lambda n=n, seg=seg, adapt=adapt: L.hc_seg_compress_work_bound(n, seg, adapt, WIDTH))

    for seg in SEG_BYTES:
        pool = _containers(hc, seg) if seg else []  # (0 is 65536: the same containers)
        dec_items = []  # (name, info, length, offset, length of the range)
        for name, info, clen in pool:
            _write_cases(hc, out, name, info, clen)
            out[f"decompress {name}"] = (
                lambda info=info, clen=clen: L.hc_seg_decompress_work_bound(ctypes.byref(info), clen))
            if info.raw_len == 17:  # an info that fails the rules: no workspace
                bad = _copy(info, n_segments=info.n_segments + 1)
                out[f"decompress {name} bad info"] = (
                    lambda bad=bad, clen=clen: L.hc_seg_decompress_work_bound(ctypes.byref(bad), clen))
                out[f"range {name} bad info"] = (
                    lambda bad=bad, clen=clen: L.hc_seg_decompress_range_work_bound(ctypes.byref(bad), clen, 0, 0))
            dec_items.append((name + " whole", info, clen, 0, hc.HC_SEG_WHOLE))
            for rname, o, m in _ranges(info):
                out[f"range {name} {rname}"] = (
                    lambda info=info, clen=clen, o=o, m=m:
                    L.hc_seg_decompress_range_work_bound(ctypes.byref(info), clen, o, m))
                if rname != "all":
                    dec_items.append((f"{name} {rname}", info, clen, o, m))

        # decode batches of 1, 2 and 17: every ninth item alone, the next beside one the host rejects
        # for its segment count, the next beside one rejected for a range past the end, and windows
        # over the list (which mix plain and adaptive, checked and unchecked items) with a rejected
        # one inside
        def dec_batch(sel, reject_at=None):
            rows, in_off, out_off = [], 0, 0
            for j, (_, info, clen, o, m) in enumerate(sel):
                if j == reject_at:
                    info = _copy(info, n_segments=info.n_segments + 1)
                rows.append(hc.SegDecItem(in_off, clen, info, o, m, out_off, info.raw_len))
                in_off += align16(clen) + 16
                out_off += align16(info.raw_len) + 16
            arr = (hc.SegDecItem * len(rows))(*rows)
            return lambda: L.hc_seg_decompress_batch_work_bound(arr, len(rows))

        for j, it in enumerate(dec_items):
            if j % 9 == 0:
                out[f"decompress_batch x1 {it[0]}"] = dec_batch([it])
            elif j % 9 == 1:
                out[f"decompress_batch x2 {it[0]} + bad info"] = dec_batch([it, it], reject_at=1)
            elif j % 9 == 2:
                past = (it[0], it[1], it[2], it[1].raw_len + 1, 1)
                out[f"decompress_batch x2 bad range + {it[0]}"] = dec_batch([past, it])
        for a in range(0, len(dec_items), 31):
            sel = [dec_items[(a + 7 * j) % len(dec_items)] for j in range(17)]
            out[f"decompress_batch x17 seg={seg} from {a}"] = dec_batch(sel, reject_at=3)

        # encode batches: one call codes all its items with the same flags
        for fl in FLAGS:
            lens = [n for n in IN_LENS if not (fl & ADAPT) or L.hc_seg_count(n, seg, 1, WIDTH)]

            def enc_batch(sel, reject_at=None, fl=fl, seg=seg):
                rows, in_off, out_off = [], 0, 0
                for j, n in enumerate(sel):
                    cap = int(L.hc_seg_compress_bound2(n, seg, fl, WIDTH))
                    rows.append(hc.SegEncItem(in_off, n, 0 if j == reject_at else WIDTH, out_off, cap))
                    in_off += align16(n) + 16
                    out_off += align16(cap)
                arr = (hc.SegEncItem * len(rows))(*rows)
                return lambda: L.hc_seg_compress_batch_work_bound(arr, len(rows), fl, seg)

            for j, n in enumerate(lens):
                if j % 2 == 0:
                    out[f"compress_batch x1 in={n} seg={seg} flags={fl:#x}"] = enc_batch([n])
                else:
                    out[f"compress_batch x2 in={n} seg={seg} flags={fl:#x} + width 0"] = enc_batch([n, n], reject_at=1)
            for a in range(0, len(lens), 3):
                sel = [lens[(a + 2 * j) % len(lens)] for j in range(17)]
                out[f"compress_batch x17 seg={seg} flags={fl:#x} from {a}"] = enc_batch(sel, reject_at=3)
            if fl & ADAPT:  # an input that is no matrix, which the host rejects by its length
                out[f"compress_batch x2 seg={seg} flags={fl:#x} + in=17"] = enc_batch([lens[0], 17])
    # calls that take no items, and arguments no call takes
    out["compress_batch x0"] = lambda: L.hc_seg_compress_batch_work_bound(None, 0, 0, 16)
    out["decompress_batch x0"] = lambda: L.hc_seg_decompress_batch_work_bound(None, 0)
    out["compress2 seg=24"] = lambda: L.hc_seg_compress_work_bound2(100, 24, 0, WIDTH)
    out["compress2 flags=0x1"] = lambda: L.hc_seg_compress_work_bound2(100, 16, 1, WIDTH)
    out["decompress no info"] = lambda: L.hc_seg_decompress_work_bound(None, 100)
    return out

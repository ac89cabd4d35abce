"""Placement helper for GPU tests of the device batch API (include/hcodec.h): streams at starts
that are only 4-byte aligned, slots of exactly the stated size, and poison in every byte around
them, so that a store past a capacity, an input byte read past its length or a result that depends
on a base address mod 16 shows. (gpu_batch.pack, which the other GPU tests use, puts every slot on a
16-byte boundary, rounds it up to 16 and zero-fills the gaps.)

Plain Python and numpy; torch only uploads. With torch=None the buffers stay numpy arrays, which is
what the CPU model test (test_place_model.py) runs on.
"""
import numpy as np

MARGIN = 64        # poison bytes before the first slot and after the last, at least
WORK_FRONT = 16    # guarded workspace: poison bytes in front of the view (keeps it 16-byte aligned)
WORK_BEHIND = 4096  # and behind it
WORK_POISON = 0xA5


TRUNC_SET = (("grad", 64, 48), ("photo", 41, 33), ("noise", 37, 29))  # each without and with the diff model
TRUNC_CUTS = tuple(range(1, 9))   # bytes cut from the end: status 9
TRUNC_PREFIXES = (0, 1, 8, 9)     # whole-prefix lengths: 8, 8, 8, 9
_trunc = {}


def trunc_streams(oracle_mod):
    """[(name, raw, oracle encoding)] of the truncation set, computed once"""
    if not _trunc:
        out = []
        for kind, w, h in TRUNC_SET:
            raw = oracle_mod.synth(kind, 0, w, h).tobytes()
            for use_diff in (False, True):
                st, enc = oracle_mod.compress(raw, use_diff, False, 512)
                assert st == 0
                out.append((f"{kind} {w}x{h}{' -m' if use_diff else ''}", raw, enc))
        _trunc["v"] = out
    return _trunc["v"]


def _layout(sizes, residues, gap=0):
    """slot i at the first offset >= max(previous end + gap, MARGIN) that is residues[i] mod 16"""
    offs, o = [], MARGIN
    for n, r in zip(sizes, residues):
        o += (r - o) % 16
        offs.append(o)
        o += int(n) + gap
    total = (o + MARGIN + 15) // 16 * 16
    check_disjoint(offs, sizes)
    assert not offs or (min(offs) >= MARGIN and max(o + n for o, n in zip(offs, sizes)) + MARGIN <= total)
    return offs, total


def check_disjoint(offs, sizes):
    order = sorted(range(len(offs)), key=lambda i: (offs[i], sizes[i]))
    for a, b in zip(order, order[1:]):
        assert offs[a] + sizes[a] <= offs[b], "slots overlap"


def layout(sizes, rot, base_res):
    """-> (offs, total): offsets from a view that starts base_res bytes into its allocation, and the
    view's length. Slot i is exactly sizes[i] bytes at an offset that is 4 * ((i + rot) % 4) mod 16;
    each slot begins at the first such offset at or behind the end of the one before, so gaps are
    0..15 bytes. The addresses the library sees are these offsets plus base_res (the allocation is
    16-byte aligned): every one 4-aligned, every residue 0, 4, 8, 12 taken."""
    assert base_res in (0, 4, 8, 12) and rot in (0, 1, 2, 3)
    offs, total = _layout(sizes, [4 * ((i + rot) % 4) for i in range(len(sizes))])
    assert all(o % 4 == 0 for o in offs)
    return offs, total


def layout_bytes(sizes, residues, gap=0):
    """the same for any byte alignment (hc_pack_batch): slot i at residues[i] mod 16, residues
    0..15, at least `gap` bytes between two slots"""
    assert all(0 <= r < 16 for r in residues) and len(residues) == len(sizes)
    return _layout(sizes, residues, gap)


def _poison(poison, n):
    """n bytes of the poison: one byte value, or an array repeated to the length"""
    if isinstance(poison, (int, np.integer)):
        return np.full(n, int(poison), dtype=np.uint8)
    return np.resize(np.asarray(poison, dtype=np.uint8), n).copy()  # (owns its bytes: _whole finds it)


def fill(torch, blobs, offs, total, base_res, poison):
    """the buffer of place() for offsets already laid out -> the view"""
    host = _poison(poison, base_res + total)
    for off, b in zip(offs, blobs):
        assert len(b) == 0 or off + len(b) <= total
        if len(b):
            host[base_res + off:base_res + off + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    if torch is None:
        return host[base_res:]
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 16 == 0
    view = dev[base_res:]
    assert view.data_ptr() % 16 == base_res and view.is_contiguous()
    return view


def place(torch, blobs, sizes, rot, base_res, poison):
    """-> (view, offs, lens): an allocation of poison with blobs[i] copied to slot i of
    layout(sizes, rot, base_res) (len(blobs[i]) <= sizes[i]; b"" leaves the slot poisoned), uploaded;
    the view starts base_res bytes into it, so its own address is only 4-aligned. offs and lens
    (the blobs' lengths) are int64 device tensors (lists with torch=None)."""
    assert len(blobs) == len(sizes) and all(len(b) <= n for b, n in zip(blobs, sizes))
    offs, total = layout(sizes, rot, base_res)
    view = fill(torch, blobs, offs, total, base_res, poison)
    lens = [len(b) for b in blobs]
    if torch is None:
        return view, offs, lens
    return view, dev_i64(torch, offs), dev_i64(torch, lens)


def dev_i64(torch, v):
    return torch.tensor(list(v), dtype=torch.int64, device="cuda")


def _whole(buf):
    """(host copy of the whole allocation behind a view, the view's start in it)"""
    if isinstance(buf, np.ndarray):
        base = buf.base if buf.base is not None else buf
        return np.asarray(base), buf.ctypes.data - base.ctypes.data
    base = buf._base if buf._base is not None else buf
    return base.cpu().numpy(), buf.storage_offset()


def _as_list(v):
    return [int(x) for x in (v if isinstance(v, (list, tuple)) else v.cpu().tolist())]


def outside_untouched(buf, offs, sizes, poison):
    """every byte of the whole allocation outside the slots (those before the view included)
    still equals the poison"""
    return not touched(buf, offs, sizes, poison)


def touched(buf, offs, sizes, poison):
    """the allocation offsets (at most 16) of the bytes outside the slots that differ from the poison"""
    host, start = _whole(buf)
    outside = np.ones(host.size, dtype=bool)
    for o, n in zip(_as_list(offs), _as_list(sizes)):
        outside[start + o:start + o + n] = False
    bad = np.flatnonzero(outside & (host != _poison(poison, host.size)))
    return [int(x) for x in bad[:16]]


def slots(buf, offs, lens):
    """the first lens[i] bytes of every slot, as bytes"""
    host = buf if isinstance(buf, np.ndarray) else buf.cpu().numpy()
    return [host[o:o + n].tobytes() for o, n in zip(_as_list(offs), _as_list(lens))]


def guarded_work(torch, need):
    """-> (allocation, view): WORK_FRONT + need + WORK_BEHIND bytes of 0xA5; the view
    [WORK_FRONT : WORK_FRONT + need] is the `work` to pass, so work_bytes == need exactly"""
    need = int(need)
    if torch is None:
        whole = np.full(WORK_FRONT + need + WORK_BEHIND, WORK_POISON, dtype=np.uint8)
    else:
        whole = torch.full((WORK_FRONT + need + WORK_BEHIND,), WORK_POISON, dtype=torch.uint8, device="cuda")
        assert whole.data_ptr() % 16 == 0
    return whole, whole[WORK_FRONT:WORK_FRONT + need]


def work_guard_untouched(whole, need):
    """the bytes in front of and behind the workspace view are still 0xA5"""
    host = whole if isinstance(whole, np.ndarray) else whole.cpu().numpy()
    need = int(need)
    assert host.size == WORK_FRONT + need + WORK_BEHIND
    return bool((host[:WORK_FRONT] == WORK_POISON).all() and (host[WORK_FRONT + need:] == WORK_POISON).all())

"""Model of the decoder's lane-parallel RLE + diff revert (hc_fgk.hip: revert_block).

The serial revert of transform.cpp:137-159 (then the diff revert of transform.cpp:231-239) is a
4-state machine on r = run counter: a symbol read in state 3 is a count (it emits `count`
copies of the previous symbol, r -> 0); otherwise it is a literal, r -> r + 1 when it equals
the previous symbol and r is 1 or 2, else r -> 1. Each symbol's transition is one of two
functions on {0,1,2,3}, stored as a 4-byte table (byte x = f(x)), so g o f is one byte
permute of g by f (v_perm_b32); functions compose, so a wave-wide inclusive scan of the
compositions gives every symbol's state. Output lengths (1 or count) and diff sums (symbol, or
count x previous symbol, mod 256) are plain scans. Bytes are emitted in two passes: every
literal writes its byte; a lane holds at most one count (a count follows three equal literals,
so counts are >= 4 symbols apart), whose run is an arithmetic sequence mod 256 with the diff
model, a constant without.

The run store (`run_stores`): the lanes that hold a non-empty run are numbered in lane order
(row[]) and taken 16 at a time, four lanes q = 0..3 per run. A run of gn bytes whose first byte
lies at absolute address A is split into hb = min(-A mod 16, gn) head bytes, nu = (gn - hb) / 16
units of 16 bytes at aligned addresses, and eb = gn - 16 nu edge bytes (the head, then what is
left behind the units). Lane q stores units q, q + 4, ...: 16 bytes built from a splat of the
unit's first byte plus P = (0, s, 2s, 3s) for the first dword and + S4 = splat(4s) for each next
one, all with `add8`, a bytewise add without carries between bytes; the next unit of the lane
is 64 s further. Then lane q stores edge bytes q, q + 4, ... one by one. All 16 runs of a group
step together, so a store is masked where a run has no unit or byte left.

A block one of whose runs reaches past the capacity takes the other path (`fallback_stores`):
run by run, the whole wave writes 64 single bytes per step, and the buffer's range check drops
those past the end.

`revert_blocked(symbols, diff, base, cap)` mirrors the kernel: blocks of 256 symbols, 64 lanes
x 4, a carry of (state, last symbol, last output byte) between blocks; `base` is the output's
address mod 16, `cap` its capacity (None: enough).
"""

import numpy as np

F_EQ = 1 | 2 << 8 | 3 << 16 | 0 << 24   # r: 0->1, 1->2, 2->3, 3->0 (count)
F_NE = 1 | 1 << 8 | 1 << 16 | 0 << 24   # r: 0->1, 1->1, 2->1, 3->0
F_ID = 0 | 1 << 8 | 2 << 16 | 3 << 24   # past the block's end


def perm(s1, sel):
    """v_perm_b32(0, s1, sel) for selector bytes 0..3: byte i = byte sel[i] of s1"""
    return sum(((s1 >> (8 * ((sel >> (8 * i)) & 255))) & 255) << (8 * i) for i in range(4))


def compose(g, f):
    """x -> g(f(x))"""
    return perm(g, f)


def apply(f, r):
    return (f >> (8 * r)) & 255


K_L7, K_H = 0x7F7F7F7F, 0x80808080


def add8(a, b):
    """four byte sums in one word, no carry from a byte into the next (ints or uint32 arrays)"""
    return ((a & K_L7) + (b & K_L7)) ^ ((a ^ b) & K_H)


def splat(x):
    """v_perm_b32(0, x, 0): byte 0 of x in all four bytes"""
    return (x & 255) * 0x01010101


def run_stores(base, go, gn, gst, gv):
    """The stores of one group of runs (arrays of R <= 16 entries, or any R for a test): run r is
    gn[r] bytes at output offset go[r] (the output starts at an address that is `base` mod 16),
    byte j = gv[r] + gst[r] * j mod 256. -> [(off, data, on)] in the kernel's order: off[r, q] the
    byte offset lane q of run r stores to, data[r, q, :] the 16 bytes or the 1 byte it stores,
    on[r, q] whether the store happens (the others go to kDrop)."""
    go, gn, gst, gv = (np.asarray(a, dtype=np.int64)[:, None] for a in (go, gn, gst, gv))
    q = np.arange(4, dtype=np.int64)[None, :]
    hb = np.minimum((0 - (base + go)) & 15, gn)
    nu = (gn - hb) >> 4
    eb = gn - 16 * nu
    P = ((gst & 255) << 8 | ((2 * gst) & 255) << 16 | ((3 * gst) & 255) << 24)
    S4 = splat(4 * gst)
    stores = []
    u = q + 0 * nu
    x = gv + gst * (hb + 16 * q)
    o = go + hb + 16 * q
    while (u < nu).any():
        w = [add8(splat(x), P)]
        for _ in range(3):
            w.append(add8(w[-1], S4))
        data = np.stack(w, axis=-1).astype("<u4").view(np.uint8)
        stores.append((o.copy(), data, u < nu))
        u = u + 4
        x = (x + 64 * gst) & 0xFFFFFFFF
        o = o + 64
    e = q + 0 * eb
    while (e < eb).any():
        j = np.where(e < hb, e, e + 16 * nu)
        data = ((gv + gst * j) & 255).astype(np.uint8)[..., None]
        stores.append((go + j, data, e < eb))
        e = e + 4
    return stores


def fallback_stores(go, gn, gst, gv):
    """the capacity path for one run: 64 lanes, one byte each, per step"""
    stores = []
    lane = np.arange(64, dtype=np.int64)[None, :]
    for j0 in range(0, gn, 64):
        j = j0 + lane
        stores.append((go + j, ((gv + gst * j) & 255).astype(np.uint8)[..., None], j < gn))
    return stores


def apply_stores(stores, out, shift=0, hits=None, cap=None):
    """write stores into the byte array `out` at off - shift; hits[i] counts the writes of byte i;
    a byte at or past `cap` (an offset like off) is dropped, as the buffer's range check does for
    single bytes"""
    for off, data, on in stores:
        idx = (off[on] - shift)[:, None] + np.arange(data.shape[-1])
        val = data[on]
        if cap is not None:
            keep = idx + shift < cap
            idx, val = idx[keep], val[keep]
        out[idx] = val
        if hits is not None:
            np.add.at(hits, idx, 1)


def store_runs(runs, base, pos, blk_out, cap=None):
    """a block's runs [(offset in the block, length > 0, first byte, step)] in row[] order, into
    blk_out (the block starts at output offset pos): groups of 16, or run by run when one of them
    reaches past cap"""
    if not runs:
        return
    if cap is not None and any(pos + p + n > cap for p, n, _, _ in runs):
        for p, n, v, s in runs:
            apply_stores(fallback_stores(pos + p, n, s, v), blk_out, pos, cap=cap)
        return
    for g in range(0, len(runs), 16):
        p, n, v, s = (np.array(a, dtype=np.int64) for a in zip(*runs[g:g + 16]))
        stores = run_stores(base, pos + p, n, s, v)
        for off, data, on in stores:  # a 16-byte store lies at an aligned address
            assert data.shape[-1] == 1 or not ((base + off[on]) & 15).any()
        apply_stores(stores, blk_out, pos)


def revert_blocked(symbols, diff, base=0, cap=None):
    sym = list(symbols)
    out = bytearray()
    r_c, last_c, prev_c = 0, 0, 0
    for base_i in range(0, len(sym), 256):
        blk = sym[base_i:base_i + 256]
        m = len(blk)
        blk = blk + [0] * (256 - m)
        prevsym = [last_c] + blk[:-1]
        f = [(F_EQ if blk[i] == prevsym[i] else F_NE) if i < m else F_ID for i in range(256)]
        # per lane: F = f3 o f2 o f1 o f0
        lanes = []
        for l in range(64):
            F = F_ID
            for b in range(4):
                F = compose(f[4 * l + b], F)
            lanes.append(F)
        # inclusive scan (Hillis-Steele, as the kernel does it with shuffles)
        inc = lanes[:]
        off = 1
        while off < 64:
            inc = [compose(inc[l], inc[l - off]) if l >= off else inc[l] for l in range(64)]
            off *= 2
        exc = [F_ID] + inc[:-1]
        # state before each symbol, output lengths and diff sums
        r_before = [0] * 256
        for l in range(64):
            r = apply(exc[l], r_c)
            for b in range(4):
                i = 4 * l + b
                r_before[i] = r
                r = apply(f[i], r)
        count = [i < m and r_before[i] == 3 for i in range(256)]
        length = [(blk[i] if count[i] else 1) if i < m else 0 for i in range(256)]
        dsum = [((blk[i] * prevsym[i]) if count[i] else blk[i]) & 255 if i < m else 0 for i in range(256)]
        lane_len = [sum(length[4 * l:4 * l + 4]) for l in range(64)]
        lane_d = [sum(dsum[4 * l:4 * l + 4]) & 255 for l in range(64)]
        start = [sum(lane_len[:l]) for l in range(64)]
        dstart = [(prev_c + sum(lane_d[:l])) & 255 for l in range(64)]
        blk_out = np.zeros(sum(lane_len), dtype=np.uint8)
        runs = []
        for l in range(64):
            p, prev = start[l], dstart[l]
            assert sum(count[4 * l:4 * l + 4]) <= 1
            for b in range(4):
                i = 4 * l + b
                if count[i]:  # the run: its offset, length, first byte and step
                    c, n_ = prevsym[i], length[i]
                    if n_:
                        runs.append((p, n_, (prev + c) & 255 if diff else c, c if diff else 0))
                    prev = (prev + n_ * c) & 255 if diff else (c if n_ else prev)
                    p += n_
                elif i < m:  # a literal
                    prev = ((prev if diff else 0) + blk[i]) & 255
                    blk_out[p] = prev
                    p += 1
        store_runs(runs, base, len(out), blk_out, cap)  # (runs: in lane order, as row[] holds them)
        out += blk_out.tobytes()
        r_c = apply(inc[63], r_c)
        last_c = blk[m - 1]
        prev_c = (prev_c + sum(lane_d)) & 255 if diff else (int(blk_out[-1]) if len(blk_out) else prev_c)
    return bytes(out if cap is None else out[:cap])

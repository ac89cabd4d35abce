"""Inputs on which the adaptive encoder's block sizes 256, 512 and 1024 win (the sizes costed
from the tile pieces by big_cost_kernel and coded by emit_big_kernel), shared by
tests/test_adapt_big_cases.py (the table checks itself against the oracle alone),
tests/test_adapt_model.py and tests/test_gpu_adapt_big.py. Seeded generators, the case table
with the oracle's winner and the runner-up's distance, and candidate_totals(), which restates
the choice of transform.cpp:294-328 from oracle.rle only. Test infrastructure only.

A case's *pattern* is the matrix the cost and emit kernels see. Without the diff model it is the
raw input; with the diff model the raw input is oracle.undiff(pattern).
"""
import numpy as np


def stripes(W, H, vert, seed, maxh=5, vals=4):
    """rows (vert=0) or columns (vert=1) constant, 1 .. maxh-1 lines per stripe"""
    r = np.random.default_rng(seed)
    n = W if vert else H
    a = []
    while len(a) < n:
        a += [int(r.integers(0, vals))] * int(r.integers(1, maxh))
    a = np.array(a[:n], np.uint8)
    return np.ascontiguousarray(np.repeat(a[None, :], H, 0) if vert else np.repeat(a[:, None], W, 1))


def quilt(W, H, Q, seed, noise=0):
    """Q x Q patches of stripes, their direction alternating like a chessboard"""
    m = np.zeros((H, W), np.uint8)
    for by in range(0, H, Q):
        for bx in range(0, W, Q):
            v = (bx // Q + by // Q + seed) & 1
            m[by:by + Q, bx:bx + Q] = stripes(min(Q, W - bx), min(Q, H - by), v, bx * 7 + by + seed)
    if noise:  # one foreign byte per `noise` elements
        r = np.random.default_rng(seed)
        f = m.reshape(-1)
        idx = r.integers(0, f.size, size=f.size // noise)
        f[idx] = r.integers(0, 256, size=idx.size).astype(np.uint8)
    return m


def longruns(W, H, seed, lo=100, hi=900, vert=False, vals=3):
    """runs in scan order (row-major, or column-major with vert) around the multiples of 258"""
    r = np.random.default_rng(seed)
    n = W * H
    out = np.empty(n, np.uint8)
    p = 0
    prev = -1
    lens = [255, 256, 257, 258, 259, 260, 513, 514, 515, 516, 517, 518, 771, 774, 775]
    while p < n:
        L = int(r.choice(lens)) if r.random() < 0.5 else int(r.integers(lo, hi))
        v = int(r.integers(0, vals))
        v = (v + 1) % vals if v == prev else v
        prev = v
        out[p:p + L] = v
        p += L
    return out.reshape(H, W) if not vert else np.ascontiguousarray(out.reshape(W, H).T)


def pinned(m, pins, value=200):
    """m with the elements (y, x) of pins set to a foreign value. A pin on the last element of a
    block's scan costs the tilings that do not end a block there one byte (a run's last element
    becomes a literal) and the tilings that do end a block there nothing (it was a literal)."""
    m = m.copy()
    for y, x in pins:
        m[y, x] = value
    return m


def candidates(W, H):
    """transform.cpp:309: B = 8, doubling at most 7 times while B <= W and B <= H"""
    out, B = [], 8
    while len(out) <= 7 and B <= W and B <= H:
        out.append(B)
        B *= 2
    return out


_totals = {}


def candidate_totals(m, key=None):
    """{B: (total, blocks, horizontal blocks)} for every candidate B, from oracle.rle alone:
    total = 24 + ceil(blocks / 8) + sum of min(h, v) over the blocks, h / v the lengths of
    oracle.rle of a block's row-major / column-major scan; a block is horizontal when h <= v.
    The encoder keeps the first minimum of total. key: cache the result under this name."""
    import oracle
    if key is not None and key in _totals:
        return _totals[key]
    m = np.ascontiguousarray(m, np.uint8)
    H, W = m.shape
    out = {}
    for B in candidates(W, H):
        data = nb = nh = 0
        for y0 in range(0, H, B):
            for x0 in range(0, W, B):
                blk = m[y0:y0 + B, x0:x0 + B]
                h = len(oracle.rle(np.ascontiguousarray(blk).reshape(-1)))
                v = len(oracle.rle(np.ascontiguousarray(blk.T).reshape(-1)))
                data += min(h, v)
                nb += 1
                nh += h <= v
        out[B] = (24 + (nb + 7) // 8 + data, nb, nh)
    if key is not None:
        _totals[key] = out
    return out


def winner(totals):
    """(first minimum, runner-up, bytes the runner-up is behind); among equal runners-up the
    smaller B"""
    best = min(totals, key=lambda B: (totals[B][0], B))
    rest = [B for B in totals if B != best]
    ru = min(rest, key=lambda B: (totals[B][0], B))
    return best, ru, totals[ru][0] - totals[best][0]


# ------------------------------------------------------------------------------- cases ---
# name -> (builder, winner, runner-up, bytes behind, horizontal blocks, blocks), as the oracle
# measured them; tests/test_adapt_big_cases.py asserts every figure but the longruns' distance.

def _pin_base():
    return quilt(1024, 1024, 1024, 3)  # one patch: vertical stripes throughout


def _pin_base_512():
    return quilt(512, 512, 512, 3)  # vertical stripes throughout


def _diff_of(m):
    import oracle
    return np.frombuffer(oracle.diff(m.reshape(-1)), np.uint8).reshape(m.shape)


TABLE = {
    "quilt-513x257-q256": (lambda: quilt(513, 257, 256, 3), 256, 128, 369, 5, 6),
    "quilt-520x300-q256": (lambda: quilt(520, 300, 256, 3), 256, 128, 394, 3, 6),
    "quilt-520x300-q256-n2000": (lambda: quilt(520, 300, 256, 3, 2000), 256, 128, 349, 3, 6),
    "quilt-1025x513-q512": (lambda: quilt(1025, 513, 512, 3), 512, 256, 9, 5, 6),
    "quilt-1100x1030-q512": (lambda: quilt(1100, 1030, 512, 3), 512, 256, 22, 4, 9),
    "quilt-1100x1030-q512-n3000": (lambda: quilt(1100, 1030, 512, 3, 3000), 512, 256, 154, 4, 9),
    "quilt-1032x1025-q1024": (lambda: quilt(1032, 1025, 1024, 3), 1024, 512, 10, 3, 4),
    "quilt-2049x1025-q1024": (lambda: quilt(2049, 1025, 1024, 3), 1024, 512, 8, 5, 6),
    "quilt-2100x1030-q1024-n5000": (lambda: quilt(2100, 1030, 1024, 3, 5000), 1024, 512, 220, 3, 6),
    "quilt-1290x1026-q1024": (lambda: quilt(1290, 1026, 1024, 3), 1024, 512, 10, 2, 4),
    "quilt-1024x1024-q1024": (lambda: quilt(1024, 1024, 1024, 3), 1024, 512, 3, 0, 1),
    "longruns-520x300-h": (lambda: longruns(520, 300, 820), 256, 128, 1410, 6, 6),
    "longruns-520x300-v": (lambda: longruns(520, 300, 820, vert=True), 256, 128, 680, 0, 6),
    "longruns-1025x513-h": (lambda: longruns(1025, 513, 1538), 512, 256, 693, 6, 6),
    "longruns-1025x513-v": (lambda: longruns(1025, 513, 1538, vert=True), 512, 256, 1995, 4, 6),
    "longruns-1100x1030-h": (lambda: longruns(1100, 1030, 2130), 1024, 512, 3559, 4, 4),
    "longruns-1100x1030-v": (lambda: longruns(1100, 1030, 2130, vert=True), 1024, 512, 4232, 0, 4),
    "longruns-1032x1025-h": (lambda: longruns(1032, 1025, 2057), 1024, 512, 4009, 4, 4),
    "longruns-1032x1025-v": (lambda: longruns(1032, 1025, 2057, vert=True), 1024, 512, 4274, 2, 4),
    # the diff model's view of the quilt: with the diff model on, the raw input is the quilt itself
    "diff-of-quilt-1100x1030-q512": (lambda: _diff_of(quilt(1100, 1030, 512, 3)), 512, 256, 12, 3, 9),
}
LONGRUNS = [k for k in TABLE if k.startswith("longruns")]

# name -> (builder, the two sizes compared, total[second] - total[first], winner)
PINS = {
    "pin-1024-leads-512-by-1": (lambda: pinned(_pin_base(), [(511, 511), (511, 1023)]), (1024, 512), 1, 1024),
    "pin-1024-ties-512": (lambda: pinned(_pin_base(), [(511, 511), (511, 1023), (1023, 511)]), (1024, 512), 0, 512),
    # one level down: the 512 x 512 base leads its 256-blocks by 3 bytes as well
    "pin-512-leads-256-by-1": (lambda: pinned(_pin_base_512(), [(255, 255), (255, 511)]), (512, 256), 1, 512),
    "pin-512-ties-256": (lambda: pinned(_pin_base_512(), [(255, 255), (255, 511), (511, 255)]), (512, 256), 0, 256),
}



def _photo(W, H):
    import oracle
    return oracle.synth("photo", 5, W, H).reshape(H, W)


# six matrices of one shape with different winners (every stream of the batch then has the same
# item counts): name -> builder for those that are not in TABLE. The oracle's winners, in the order
# of UNIFORM: 512, 256, 512, 512, 32 (no block of 256 or more to code) and 512.
UNIFORM_EXTRA = {
    "quilt-1025x513-q256": lambda: quilt(1025, 513, 256, 3),
    "photo-1025x513": lambda: _photo(1025, 513),
    "flat-1025x513": lambda: np.full((513, 1025), 7, np.uint8),
}
UNIFORM = ["quilt-1025x513-q512", "quilt-1025x513-q256", "longruns-1025x513-h", "longruns-1025x513-v",
           "photo-1025x513", "flat-1025x513"]

_patterns = {}


def pattern(name):
    """the case's matrix (H x W uint8, read-only), built once"""
    if name not in _patterns:
        build = UNIFORM_EXTRA[name] if name in UNIFORM_EXTRA else (TABLE.get(name) or PINS[name])[0]
        m = np.ascontiguousarray(build(), np.uint8)
        m.setflags(write=False)
        _patterns[name] = m
    return _patterns[name]


def totals(name):
    return candidate_totals(pattern(name), key=name)


def raw_input(name, use_diff):
    """(raw bytes, width) whose adaptive encode sees the case's pattern"""
    import oracle
    m = pattern(name)
    b = m.tobytes()
    return (bytes(oracle.undiff(b)) if use_diff else b), m.shape[1]

"""Lane-level model of the FGK kernels' walk (hc_fgk.hip: Fgk::walk with HC_WALK_LEAN), on the slot
form tree of tests/fgk_cache_model.py.

The walk finishes an update from position s when the lane-parallel part (update_fast / update_from)
reported a level, or from the leaf of a path too deep for the encoder's cache:

* one exact level at s: the block leader (a far leader when more than 64 positions weigh the same),
  a swap when the leader is neither s nor its parent, the increment. After a swap at a position
  lighter than WALK_LIGHT the parent's level is walked the same way at once;
* the climb back ("chase-back") from the parent to the known path pv (lane k: level k, ROOT lanes
  above): the j-th position passed goes to lane j of td, selected by a running lane mask that
  starts at 1 and is shifted once a level; the mask running out (64 levels) is the bound, a bug.
  The number of levels n is read off the mask once after the loop;
* n == 0 (the parent is on pv): pv stays as it is and update_from(pv, m) runs on the levels from
  the meeting lane m up. n > 0: lanes 0..n-1 take td, lane j >= n takes pv's lane j - n + m (ROOT
  past lane 63), and update_from(pv, 0) runs on all of it;
* a level that reports there is walked again, the path in hand taking pv's role (a further round).

WALK_COST: VALU + SALU instructions, counted in the ISA of encode_kernel<0, 1, false, false> and
decode_kernel<0, 0, false>: per climbed level 12 before, 7 with HC_WALK_LEAN; the path rebuild a
meeting at once no longer does (src, ds_bpermute, two compares and selects, the mask's ctz): 9, of
which the test for it (s_cmp, s_cbranch) costs every chase-back 2.
"""
from fgk_cache_model import ROOT

WALK_LIGHT = 64    # HC_WALK_LIGHT
INSERT_DEPTH = 9   # HC_INSERT_DEPTH: deeper paths are walked from the leaf
WALK_COST = dict(level_old=12, level=7, rebuild=9, meet_test=2)


class WalkBug(Exception):
    pass


def _word(t, p):
    return (t.w[p] << 10) | (t.up[p] if p < ROOT else 0) if p <= ROOT else (1 << 62)


def update_from(t, pv, m):
    """update_from(pv, m) on 64 lanes: -> first reported lane >= m or None (then the root was
    incremented, once: its lanes store the same word)"""
    k = None
    for j in range(m, 64):
        p = pv[j]
        if p != ROOT and not _word(t, p + 1) >= _word(t, p) + 1024:
            k = j
            break
    done = set()
    for j in range(m, 64 if k is None else k):
        if pv[j] not in done:  # (path positions are distinct; the root lanes are one position)
            done.add(pv[j])
            t.w[pv[j]] += 1
    return k


def lanes(path):
    """a bottom-up path without ROOT -> the 64 lanes"""
    assert len(path) < 64
    return list(path) + [ROOT] * (64 - len(path))


def walk(t, s, pv, st):
    """walk(s, pv). st: statistics, updated: chase[n] = chase-backs of n levels, exact = exact
    levels, swaps, far = leaders beyond the 64 positions read, again = parents walked at once,
    rounds[r] = walks with r chase-backs, meet_top = meetings in the lane just below pv's root
    lanes, meet_root = meetings at the root, rebuilds_saved = meetings at once."""
    assert len(pv) == 64 and pv[63] == ROOT
    rounds = 0
    while True:
        f = t.w[s]
        st["exact"] += 1
        again = False
        if t.w[s + 1] == f:
            lead = s
            while t.w[lead + 1] == f:
                lead += 1
            st["far"] += lead - s >= 63  # the 64 positions read (s .. s + 63) all weigh the same or less
            if lead != t.up[s]:
                again = f < WALK_LIGHT
                a, c = t.body[s], t.body[lead]
                t.body[s], t.body[lead] = c, a
                t.relink(c, s)
                t.relink(a, lead)
                t.swaps.append((s, lead))
                st["swaps"] += 1
                s = lead
        t.w[s] += 1
        p = t.up[s] if s != ROOT else 0
        if again and p != ROOT:
            st["again"] += 1
            s = p
            continue
        # the chase-back: a running lane mask, the level count read off it afterwards
        c, td, lm = p, [ROOT] * 64, 1
        while c not in pv:
            td[lm.bit_length() - 1] = c
            lm = (lm << 1) & ((1 << 64) - 1)
            if lm == 0:
                raise WalkBug("64 levels climbed without meeting the path")
            c = t.up[c]
        m = pv.index(c)  # the lowest meeting lane
        n = lm.bit_length() - 1
        rounds += 1
        st["chase"][n] = st["chase"].get(n, 0) + 1
        top = pv.index(ROOT)
        st["meet_root"] += c == ROOT
        st["meet_top"] += m == top - 1
        if n == 0:
            st["rebuilds_saved"] += 1
            k = update_from(t, pv, m)
        else:
            pv = [td[j] if j < n else (pv[j - n + m] if j - n + m < 64 else ROOT) for j in range(64)]
            k = update_from(t, pv, 0)
        if k is None:
            st["rounds"][rounds] = st["rounds"].get(rounds, 0) + 1
            return
        s = pv[k]


def new_stats():
    return dict(n=0, walks=0, deep=0, exact=0, swaps=0, far=0, again=0, chase={}, rounds={}, meet_top=0, meet_root=0,
                rebuilds_saved=0)


def update(t, x, st):
    """the kernels' update of the leaf at x: a path deeper than INSERT_DEPTH is walked from the
    leaf (the encoder's deep miss), any other goes through update_fast first"""
    t.swaps = []
    pv = lanes(t.path(x))
    st["n"] += 1
    if pv.index(ROOT) > INSERT_DEPTH:
        st["walks"] += 1
        st["deep"] += 1
        walk(t, x, pv, st)
        return
    k = update_from(t, pv, 0)
    if k is not None:
        st["walks"] += 1
        walk(t, pv[k], pv, st)


def cost(st):
    """(before, with HC_WALK_LEAN) modelled instructions of the chase-backs' levels and rebuilds"""
    c = WALK_COST
    levels = sum(n * v for n, v in st["chase"].items())
    backs = sum(st["chase"].values())
    return (levels * c["level_old"] + backs * c["rebuild"],
            levels * c["level"] + backs * c["meet_test"] + (backs - st["rebuilds_saved"]) * c["rebuild"])


# ---- the GPU test's vectors (tests/test_gpu_walk.py; their coverage is asserted on the CPU in
# tests/test_walk_model.py). At most 64 streams of at most 4096 symbols, none with a run.

def vectors():
    from fgk_climb_model import draw, fib
    out = []
    # Fibonacci counts in random order: deep trees, long chase-backs, several rounds a walk
    out.append(("fib17", draw(fib(17), 4, cap=4096)))
    out.append(("fib16", draw(fib(16), 1, cap=2584)))
    # a deep chain above many rare symbols: deep leaves swap far across the tree, and the climb
    # back meets the known path only eight levels up
    out.append(("fibrare", draw(fib(14) + [1] * 100, 3, cap=4096)))
    out.append(("georare", draw([int(1.5 ** i) + 1 for i in range(18)] + [3] * 60, 5, cap=4096)))
    # a Fibonacci chain below a flat top of common symbols
    out.append(("flatfib", draw(fib(14) + [100] * 24, 5, first=1, cap=4096)))
    out.append(("flatfib2", draw(fib(12) + [60] * 40, 6, first=2, cap=4096)))
    # 70, 130 and 256 distinct symbols once each (a block of more than 64 equal weights: the far
    # leader), then again in another order, then a skewed tail
    for name, k, seed in (("once70", 70, 7), ("once130", 130, 8), ("once256", 256, 9)):
        syms = [(5 + 3 * i) & 255 for i in range(k)]
        out.append((name, syms + syms[::-1][1:] + draw(fib(13), seed, first=syms[1], cap=1500)))
    # flat alphabets: every update ties and swaps
    out.append(("flat40", draw([90] * 40, 11, cap=3600)))
    out.append(("flat200", draw([20] * 200, 12, cap=4000)))
    # a perfect Fibonacci chain, 15 levels deep, a filler between any two symbols
    chain = []
    f = fib(17)
    for k in range(15):
        chain.append(k)
        for j in range(k - 1):
            chain += [j] * f[k - j - 2]
    out.append(("chain15", [v for s in chain for v in ((1 + s * 7) & 255, 0)][:4096]))
    out.append(("two", [65, 66] * 350))
    out.append(("single", [7]))
    return out

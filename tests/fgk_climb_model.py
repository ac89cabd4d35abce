"""Lane-level model of the FGK kernels' grouped climb and grouped descent (hc_fgk.hip:
Fgk::chase_grouped, HC_CHASE_GROUP; Dec::finish_symbol, HC_DESC_GROUP), on the slot-form tree of
tests/fgk_cache_model.py.

* climb (encoder, path-cache mode): a miss climbs from the leaf with no root test per level. Level
  k's position goes into lane k; the lanes not written yet hold ROOT. Levels 0..PROBE are one group
  (the path cache is probed on the position of level PROBE, as before), the groups after a failed
  probe are GROUP levels each, and the root is looked for once per group: the depth is the first
  lane holding ROOT. A climb that passes the root goes on through the root's parent field, 0, and
  from position 0 (whose word is 0, or a real node's once all 256 symbols have leaves) back up the
  tree: every position read stays <= ROOT, and the lanes from the depth on are set to ROOT.
* descent (decoder): a code longer than the level tables reach walks down from where they stop.
  The first SCHED[-1] levels run in groups when the window holds that many bits: the bits come
  from a copy of the window at fixed offsets, and each level is the bit, the child index (recorded
  at the lane of its depth) and the body read; the inner bits of the group's bodies are tested
  once at each level of SCHED. The first level whose body is not inner ends the code; the levels
  below it read in-range garbage ((body & 255) * 2 + bit <= 511) and are dropped, and only the
  bits up to it are consumed. A group of one level tests the body it read and ends in place.
  Anything longer, or a window short of bits, takes the per-level loop.

Instruction counts (VALU + SALU, from the ISA of encode_kernel<0, 1, false, false> and
decode_kernel<0, 0, false>): see CLIMB_COST and DESC_COST.
"""
from fgk_cache_model import INNER, ROOT, SLOTS, _word

PROBE = 7   # HC_PROBE
GROUP = 4   # HC_CHASE_GROUP
INSERT_DEPTH = 9  # HC_INSERT_DEPTH: the deepest path the encoder caches
SCHED = (1, 4, 5, 6, 8)  # HC_DESC_SCHED: the levels after which the inner test happens

# per level / per root test: the per-level climb (parent commit: 7 in the unrolled part, 3 of them
# the test; 11 in the tail, 7 of them the test) against the grouped one (lshl_add, and, cndmask +
# the mask's s_mov / s_lshl; a test is v_cmp, s_ff1, s_cmp, s_cbranch, in the tail also s_min, s_add)
CLIMB_COST = dict(old_probe=7, old_tail=11, old_turn=3, level=4, test_probe=4, test_tail=6, end=4)
# per level / per inner test: the per-level descent (round 5's count in DESIGN.md: ~16 with its test) against the
# grouped one: bfe, lshl, and_or, lshl_add, 2 cndmask, s_lshr a level; its test is v_and, v_cmp,
# s_mov, s_cbranch. schedule_cost, which chooses SCHED, is levels * level + tests * test. descend()
# counts finer: a code that ends in a group of several levels also pays s_cmp, s_cselect, s_and,
# s_cbranch, s_flbit, xor, sub, 2 readlane, 2 v_mov to pick the level (end); a group of one level
# needs no second cndmask, tests with bfe, v_cmp, s_cbranch and ends in place.
DESC_COST = dict(old_level=16, level=7, test=4, end=11, one_level=6, one_test=3)


def parent_field(t, p):
    """what the kernel reads at position p: the narrow word's parent field (wide / huge: up[p])"""
    assert 0 <= p <= ROOT, p  # the climb never leaves the stream's own arrays
    return _word(t, p) & 1023


def climb(t, s, pc=None):
    """chase_grouped(s): -> (path bottom-up without ROOT, stats). pc: a fgk_cache_model.PathCache
    to probe at level PROBE. stats: levels = parent reads, tests = root tests, probe = None (root
    within PROBE levels) / True / False, over = levels read past the root."""
    tv = [ROOT] * 64
    st = dict(levels=0, tests=0, tail_tests=0, probe=None, over=0)
    for i in range(PROBE):
        tv[i] = s
        s = parent_field(t, s)
        st["levels"] += 1
    tv[PROBE] = s
    st["tests"] += 1
    d = tv.index(ROOT)  # the lanes above PROBE hold it
    if d > PROBE:
        if pc is not None:
            for e in range(SLOTS):  # the first hit: lowest entry, then lowest level
                if pc.ent[e] is not None and s in pc.ent[e][1]:
                    row = pc.ent[e][1]
                    st["probe"] = True
                    return tv[:PROBE] + row[row.index(s):], st
        st["probe"] = False
        nx = PROBE + 1
        while True:  # fixed trip bound: nx ends at 64
            for _ in range(GROUP):
                s = parent_field(t, s)
                tv[nx] = s
                nx += 1
                st["levels"] += 1
            st["tests"] += 1
            st["tail_tests"] += 1
            d = tv.index(ROOT) if ROOT in tv else None
            if not min(63 if d is None else d, 63) >= nx:
                break
        assert nx <= 64
    assert d is not None, "no root within 63 levels"
    st["over"] = st["levels"] - d
    return tv[:d], st


def climb_cost(st, depth):
    """(parent commit's, grouped) instructions of one miss's climb"""
    c = CLIMB_COST
    if st["probe"]:
        return PROBE * c["old_probe"], PROBE * c["level"] + c["test_probe"]
    old = min(depth, PROBE) * c["old_probe"] + max(depth - PROBE, 0) * c["old_tail"] + c["old_turn"]
    new = st["levels"] * c["level"] + c["test_probe"] + st["tail_tests"] * c["test_tail"] + c["end"]
    return old, new


def descend(t, bits, i, x, d, nwin, sched=SCHED):
    """The decoder's long-code descent from position x at depth d (the code starts at bit i; the
    window stands d bits into it with nwin bits). -> (position, depth, levels top-down from d + 1,
    stats). stats: blind = levels run unrolled (sched: in groups), tests, single = levels in the
    per-level loop, refills, cost = modelled instructions."""
    st = dict(blind=0, tests=0, single=0, refills=0, grouped=False, cost=0)
    c = DESC_COST
    base = i + d       # the window's first bit
    if nwin <= 32:
        nwin += 32     # refill
    have = nwin        # bits the window holds, from base

    def bit(k):        # bit k of the window
        assert k < have, "a level took a bit the window does not hold"
        return bits[base + k] if base + k < len(bits) else 0

    depth, d0, lim = d, d, min(d + nwin, 63)
    xv, pt = x, {}
    ended = False
    if depth + sched[-1] <= lim:
        st["grouped"] = True
        bq, k = {}, 0
        for g in sched:
            one = g == k + 1  # a one-level group tests the body it read and ends in place
            while k < g:
                xv = (t.body[xv] & 255) * 2 + bit(k)
                assert xv <= 511
                pt[depth + k + 1] = xv
                if not one:
                    bq[depth + k + 1] = t.body[xv]
                k += 1
                st["blind"] += 1
                st["cost"] += c["one_level"] if one else c["level"]
            st["tests"] += 1
            st["cost"] += c["one_test"] if one else c["test"]
            ends = [depth + k] if one and not t.body[xv] & INNER else [j for j in sorted(bq) if not bq[j] & INNER]
            if ends:
                ended = True
                st["cost"] += 0 if one else c["end"]
                break
        de = depth + sched[-1]
        if ended:
            de = ends[0]
            xv = pt[de]
            pt = {j: p for j, p in pt.items() if j <= de}
        depth = de
    while not ended:
        while True:
            xv = (t.body[xv] & 255) * 2 + bit(depth - d)
            depth += 1
            pt[depth] = xv
            st["single"] += 1
            st["cost"] += c["old_level"]
            if not (t.body[xv] & INNER and depth < lim):
                break
        if not t.body[xv] & INNER or depth >= 63:
            break
        nwin -= depth - d0
        assert nwin == 0
        nwin += 32
        have += 32
        st["refills"] += 1
        d0 = depth
        lim = min(depth + nwin, 63)
    assert depth - d <= have
    return xv, depth, [pt[j] for j in range(d + 1, depth + 1)], st


def schedule_cost(hist, sched):
    """levels run * instructions per level + tests * instructions per test of the grouped descent
    over a histogram {levels below the tables: codes}; a code longer than the schedule goes on in
    the per-level loop"""
    c = DESC_COST
    total = 0
    for n, cnt in hist.items():
        g = next((j for j, e in enumerate(sched) if e >= n), None)
        if g is None:
            total += cnt * (sched[-1] * c["level"] + len(sched) * c["test"] + (n - sched[-1]) * c["old_level"])
        else:
            total += cnt * (sched[g] * c["level"] + (g + 1) * c["test"])
    return total


def per_level_cost(hist):
    return sum(n * cnt * DESC_COST["old_level"] for n, cnt in hist.items())


# ---- the GPU test's vectors (tests/test_gpu_climb.py; their coverage is asserted on the CPU in
# tests/test_climb_model.py)

def draw(counts, seed, first=0, cap=50000):
    """a stream without runs (no two neighbours equal, so tests/fgk_handoff_model.raw_of gives raw
    bytes whose coded symbols are these) in which symbol s occurs counts[s] times, drawn in a
    fixed-seed random order"""
    import random
    left = list(counts)
    rng = random.Random(seed)
    out, prev = [], -1
    while len(out) < cap:
        n = sum(left) - (left[prev] if prev >= 0 else 0)
        if n == 0:
            break
        r = rng.randrange(n)
        for s, c in enumerate(left):
            if s == prev:
                continue
            if r < c:
                break
            r -= c
        left[s] -= 1
        out.append((first + s * 7) & 255)
        prev = s
    return out


def fib(n):
    out, a, b = [], 1, 1
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


def vectors():
    """(name, symbols) of the test's streams, each at most 50 k symbols"""
    out = []
    # a perfect Fibonacci chain, 21 levels deep: stage k brings symbol k in and every older symbol
    # j up to weight fib(k - j); a filler symbol between any two keeps the stream free of runs
    chain = []
    f = fib(22)
    for k in range(20):
        chain.append(k)
        for j in range(k - 1):
            chain += [j] * f[k - j - 2]
    out.append(("chain20", [v for s in chain for v in ((1 + s * 7) & 255, 0)]))
    # Fibonacci counts in random order: symbol s occurs fib(s) times
    out.append(("fib22", draw(fib(22), 4)))
    out.append(("fib19", draw(fib(19), 2, first=3)))
    # a Fibonacci chain of rare symbols below a flat top of 32 common ones (more than the path
    # cache holds: probes of the chain's climbs miss as well as hit)
    out.append(("flatfib", draw(fib(17) + [900] * 32, 5, first=1)))
    out.append(("flatfib2", draw(fib(15) + [300] * 20, 6, first=2)))
    # the same stream behind 1..40 common symbols: moves every long code across the decoder's
    # window words (all bit offsets, together with the streams above)
    short = draw(fib(16), 1)[:1500]
    common = short[0]
    for pre in range(1, 41):
        out.append(("pre%d" % pre, [(common + 1) & 255 if (pre - j) & 1 else common for j in range(pre)] + short))
    # all 256 symbols (position 0 in use: the NYT at 0 once the last one has split), then a skewed tail
    out.append(("ramp", list(range(256)) + draw(fib(19), 7, first=9) + list(range(255, -1, -1))))
    out.append(("one", [65] * 700))
    out.append(("two", [65, 66] * 350 + [66] * 9))
    out.append(("single", [7]))
    return out

"""CPU checks of the grouped climb and the grouped descent (tests/fgk_climb_model.py, the model of
hc_fgk.hip's Fgk::chase_grouped and the grouped part of Dec::finish_symbol): in lockstep with the
plain slot-form tree (fgk_cache_model.Tree.path / descend) the path, the depth and the bits
consumed are equal at every miss of the path cache and at every code longer than the level tables
reach -- on the photo, gradient and noise streams and on the vectors of tests/test_gpu_climb.py,
whose coverage is asserted here, on the CPU. The modelled instruction counts per stream go to
profiles/r11_climb_model.txt."""
import os

import pytest

import fgk_cache_model as M
import fgk_climb_model as C

HERE = os.path.dirname(os.path.abspath(__file__))
REPORT = os.path.join(os.path.dirname(HERE), "profiles", "r11_climb_model.txt")


def lockstep(symbols, nwins=None):
    """Code `symbols` as fgk_cache_model.run does; every miss climbs by the model, every long code
    descends by the model (from every window fill in `nwins`; default: one that cycles 1..64).
    -> statistics"""
    t = M.Tree()
    pc = M.PathCache()
    bits, starts = [], []
    s = dict(n=len(symbols), misses=0, probe_hit=0, probe_miss=0, chase={}, over=0, climb_old=0, climb_new=0,
             after_split=0, past_root_pos0=0, levels_probe=0, levels_tail=0)
    split_last = False
    for sym in symbols:
        fresh = t.where[sym] == 0
        if fresh:
            t.split(sym)
        x = t.where[sym]
        true = t.path(x)
        pv = pc.lookup(sym)
        if pv is None:
            probed = pc.probe(t, x)
            got, st = C.climb(t, x, pc)
            assert got == true, (sym, got, true)
            assert (probed is not None) == (st["probe"] is True)
            assert st["probe"] is not None or len(true) <= C.PROBE
            d = len(true)
            s["misses"] += 1
            s["probe_hit"] += st["probe"] is True
            s["probe_miss"] += st["probe"] is False
            if st["probe"] is not True:
                s["chase"][d] = s["chase"].get(d, 0) + 1
                s["over"] += st["over"]
                # the climb went through position 0 while it holds a real node
                s["past_root_pos0"] += st["over"] > 1 and t.nyt == 0
            s["levels_probe"] += min(st["levels"], C.PROBE)
            s["levels_tail"] += max(st["levels"] - C.PROBE, 0)
            s["after_split"] += split_last and not fresh
            old, new = C.climb_cost(st, d)
            s["climb_old"] += old
            s["climb_new"] += new
            pv = true
            if d <= C.INSERT_DEPTH:  # (the kernel caches no deeper path; the rows could hold 12 levels)
                pc.insert(sym, pv)
        assert pv == true
        code = [p & 1 for p in reversed(pv)]
        starts.append(len(bits))
        bits += code[:-1] + [(sym >> k) & 1 for k in range(7, -1, -1)] if fresh else code
        t.update(x)
        for a, b in t.swaps:
            pc.on_swap(a, b)
        split_last = fresh

    t = M.Tree()
    lt = M.LevelTables()
    s.update(long=0, below={}, offsets=set(), nyt_end=0, refills=0, ungrouped=0, desc_old=0, desc_new=0, desc_levels=0)
    i = 0
    for n, sym in enumerate(symbols):
        assert i == starts[n]
        x, d, pv = lt.lookup(t, bits, i)
        v = 0
        for k in range(8):
            v = (v << 1) | (bits[i + k] if i + k < len(bits) else 0)
        x0, d0 = lt.L[8][v]
        if t.body[x0] & M.INNER:  # the tables stop at an inner position: the descent
            want = list(reversed(t.path(x)))[d0:]
            for nw in (nwins if nwins is not None else (1 + (s["long"] * 7) % 64,)):
                gx, gd, levels, st = C.descend(t, bits, i, x0, d0, nw)
                assert (gx, gd) == (x, d) and levels == want, (n, nw, gx, gd, x, d)
                s["refills"] += st["refills"]
                s["ungrouped"] += not st["grouped"]
            s["desc_old"] += (d - d0) * C.DESC_COST["old_level"]
            s["desc_new"] += st["cost"]
            s["desc_levels"] += d - d0
            s["long"] += 1
            s["below"][d - d0] = s["below"].get(d - d0, 0) + 1
            s["offsets"].add((72 + i) % 64)  # the payload starts at bit 72 of the stream
            s["nyt_end"] += bool(t.body[x] & M.NYT)
        i += d
        if t.body[x] & M.NYT:
            i += 8
            t.split(sym)
            x = t.where[sym]
        else:
            assert t.body[x] == sym
        t.update(x)
        for a, b in t.swaps:
            lt.on_swap(a, b)
    assert i == len(bits)
    return s


def _line(name, s):
    n = max(1, s["n"])
    return ("%-10s n %6d  misses %5d probe hits %5d  climb levels %6d + %6d tail, %5d past the root  "
            "climb instr/symbol %.3f -> %.3f   long codes %5d levels %6d  descent instr/symbol %.3f -> %.3f"
            % (name, s["n"], s["misses"], s["probe_hit"], s["levels_probe"], s["levels_tail"], s["over"],
               s["climb_old"] / n, s["climb_new"] / n, s["long"], s["desc_levels"], s["desc_old"] / n, s["desc_new"] / n))


@pytest.fixture(scope="module")
def report():
    lines = {}
    yield lines
    if len(lines) < 6:
        return  # a partial run leaves the recorded file alone
    head = ("Modelled instructions (VALU + SALU, counted from the ISA: fgk_climb_model.CLIMB_COST / DESC_COST) of the\n"
            "encoder's miss climb and the decoder's long-code descent, per-level form -> grouped form\n"
            "(HC_CHASE_GROUP %d after the probe at level %d; HC_DESC_SCHED %s). First 60 k symbols of each stream.\n"
            "Written by tests/test_climb_model.py.\n\n" % (C.GROUP, C.PROBE, list(C.SCHED)))
    try:
        with open(REPORT, "w") as f:
            f.write(head + "\n".join(lines[k] for k in sorted(lines)) + "\n")
    except OSError:
        pass  # a read-only checkout


def _symbols(oracle_mod, kind, k, w, h):
    return list(oracle_mod.rle(oracle_mod.diff(oracle_mod.synth(kind, k, w, h).tobytes())))[:60000]


@pytest.mark.parametrize("kind,k", [("photo", 0), ("photo", 1), ("photo", 2), ("photo", 3), ("grad", 0), ("noise", 0)])
def test_streams_lockstep(oracle_mod, report, kind, k):
    s = lockstep(_symbols(oracle_mod, kind, k, 512, 512))
    report["%s%d" % (kind, k)] = _line("%s %d" % (kind, k), s)
    assert s["misses"] and s["long"]
    # the grouped descent never costs more in the model, on any kind. The grouped climb always runs
    # its first PROBE levels, so a miss shallower than five levels costs more than before: few
    # enough on every kind (the gradient's dozen misses are all of them) to stay under 0.05
    # instructions per symbol, and on the photo streams the climb as a whole is cheaper
    assert s["desc_new"] <= s["desc_old"]
    assert s["climb_new"] - s["climb_old"] <= 0.05 * s["n"]
    if kind == "photo":
        assert s["climb_new"] < 0.8 * s["climb_old"]


def test_schedule_choice(oracle_mod):
    """HC_DESC_SCHED is the cheapest (levels run * 7 + tests * 4, fgk_climb_model.schedule_cost) of the
    schedules over eight levels that test after the first one -- a one-level descent, nearly all of
    noise's, must not cost more than in the per-level loop -- on the photo histogram, well below the
    per-level loop there, and not above it on noise."""
    import itertools
    photo = lockstep(_symbols(oracle_mod, "photo", 0, 512, 512))["below"]
    noise = lockstep(_symbols(oracle_mod, "noise", 0, 512, 512))["below"]
    best = min((C.schedule_cost(photo, (1,) + mid + (8,)), (1,) + mid + (8,))
               for r in range(0, 7) for mid in itertools.combinations(range(2, 8), r))
    # (schedules within 1 % of each other are one to the model; of those the shortest list is kept)
    assert C.schedule_cost(photo, C.SCHED) <= 1.01 * best[0], best
    assert all(len(sc) >= len(C.SCHED) for r in range(0, 7) for mid in itertools.combinations(range(2, 8), r)
               for sc in [(1,) + mid + (8,)] if C.schedule_cost(photo, sc) <= 1.01 * best[0])
    assert C.schedule_cost(photo, C.SCHED) < 0.7 * C.per_level_cost(photo)
    assert C.schedule_cost(noise, C.SCHED) <= C.per_level_cost(noise)


@pytest.fixture(scope="module")
def vector_stats(oracle_mod):
    """the model on what the kernels code for each vector: the MNP-5 symbols of its diffed raw bytes
    (the designed symbols themselves where they have no runs)"""
    from fgk_handoff_model import raw_of
    out = {}
    for name, sym in C.vectors():
        coded = list(oracle_mod.rle(oracle_mod.diff(raw_of(sym))))
        assert coded == sym or name in ("one", "two"), name
        out[name] = lockstep(coded, nwins=range(1, 65) if len(sym) <= 2000 else None)
    return out


def test_vectors_lockstep_and_coverage(vector_stats):
    vs = vector_stats
    assert all(len(sym) <= 50000 for _, sym in C.vectors())
    tot = lambda key: sum(s[key] for s in vs.values())
    chase = {}
    below = {}
    for s in vs.values():
        for d, c in s["chase"].items():
            chase[d] = chase.get(d, 0) + c
        for d, c in s["below"].items():
            below[d] = below.get(d, 0) + c
    # chase depths 1..>= 20: the probe edge (6 / 7 / 8), beyond a cache row (12 / 13), and every
    # residue of the group schedule after the probe
    assert all(chase.get(d) for d in range(1, 20)) and any(d >= 20 for d in chase), sorted(chase)
    assert {(d - C.PROBE - 1) % C.GROUP for d in chase if d > C.PROBE} == set(range(C.GROUP))
    assert tot("probe_hit") and tot("probe_miss")  # both probe outcomes
    assert tot("after_split")                      # a miss right after a split
    assert vs["ramp"]["past_root_pos0"]            # position 0 in use when a climb passes the root
    assert tot("over")
    # descents of every length 1 .. two groups + 1 (the schedule's levels + 1: into the per-level loop)
    assert all(below.get(n) for n in range(1, C.SCHED[-1] + 2)), sorted(below)
    # long codes at every bit offset of a 64-bit word, one ending at the NYT, refills mid-descent
    offs = set()
    for s in vs.values():
        offs |= s["offsets"]
    assert offs == set(range(64))
    assert tot("nyt_end")
    # (with a window refilled to more than 32 bits at the start, the grouped levels always have
    # their bits: no descent of a valid stream meets the window limit or refills midway)
    assert tot("ungrouped") == 0 and tot("refills") == 0
    # one- and two-symbol streams
    assert vs["one"]["n"] and vs["two"]["n"] and vs["single"]["n"] == 1

"""CPU checks of the walk model (tests/fgk_walk_model.py, the model of hc_fgk.hip's Fgk::walk with
HC_WALK_LEAN: the chase-back by a running lane mask, bounded by the mask running out, and the
meeting at once that keeps the known path): in lockstep with the plain slot-form update
(fgk_cache_model.Tree.update) the tree is the same after every symbol -- on the photo, gradient and
noise streams and on the vectors of tests/test_gpu_walk.py, whose coverage is asserted here, on the
CPU. The chase-backs by length and the modelled instruction counts go to
profiles/r12_walk_model.txt."""
import os

import pytest

import fgk_cache_model as M
import fgk_walk_model as W

HERE = os.path.dirname(os.path.abspath(__file__))
REPORT = os.path.join(os.path.dirname(HERE), "profiles", "r12_walk_model.txt")


def lockstep(symbols):
    """every symbol's update by the model on one tree and by Tree.update on another: equal trees
    after each. -> the model's statistics"""
    t, ref = M.Tree(), M.Tree()
    st = W.new_stats()
    for i, sym in enumerate(symbols):
        if t.where[sym] == 0:
            t.split(sym)
            ref.split(sym)
        x = t.where[sym]
        W.update(t, x, st)
        ref.update(x)
        assert t.swaps == ref.swaps, (i, sym)
        assert t.w == ref.w and t.up == ref.up and t.body == ref.body and t.where == ref.where, (i, sym)
    return st


def _line(name, s):
    n = max(1, s["n"])
    old, new = W.cost(s)
    backs = sum(s["chase"].values())
    levels = sum(k * v for k, v in s["chase"].items())
    hist = " ".join("%d:%d" % (k, s["chase"][k]) for k in sorted(s["chase"]))
    return ("%-8s n %6d  walks %5d (%4d from a deep leaf)  exact levels %.3f swaps %.3f chase-backs %.3f chased levels %.3f "
            "per symbol, %2d %% met at once  instr/symbol %.3f -> %.3f\n         chase-backs by length  %s"
            % (name, s["n"], s["walks"], s["deep"], s["exact"] / n, s["swaps"] / n, backs / n, levels / n,
               round(100 * s["rebuilds_saved"] / max(1, backs)), old / n, new / n, hist))


@pytest.fixture(scope="module")
def report():
    lines = {}
    yield lines
    if len(lines) < 7:
        return  # a partial run leaves the recorded file alone
    c = W.WALK_COST
    head = ("Chase-backs of the walk (Fgk::walk) by length and their modelled instructions (VALU + SALU, counted from\n"
            "the ISA: fgk_walk_model.WALK_COST; %d -> %d a climbed level, %d for the path rebuild a meeting at once skips,\n"
            "%d for its test), the loop before -> HC_WALK_LEAN. First 60 k symbols of each stream; `vectors`: all streams\n"
            "of tests/test_gpu_walk.py. Written by tests/test_walk_model.py.\n\n"
            % (c["level_old"], c["level"], c["rebuild"], c["meet_test"]))
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
    assert s["walks"] and s["chase"]
    old, new = W.cost(s)
    assert new < old
    if kind == "photo":
        # about a third of the chase-backs meet the known path at once
        backs = sum(s["chase"].values())
        assert 0.2 * backs < s["rebuilds_saved"] < 0.5 * backs


@pytest.fixture(scope="module")
def vector_stats(oracle_mod):
    """the model on what the kernels code for each vector: the MNP-5 symbols of its diffed raw bytes"""
    from fgk_handoff_model import raw_of
    out = {}
    for name, sym in W.vectors():
        coded = list(oracle_mod.rle(oracle_mod.diff(raw_of(sym))))
        assert coded == sym, name
        out[name] = lockstep(coded)
    return out


def test_vectors_lockstep_and_coverage(vector_stats, report):
    vs = vector_stats
    vec = W.vectors()
    assert len(vec) <= 64 and all(len(sym) <= 4096 for _, sym in vec)
    tot = lambda key: sum(s[key] for s in vs.values())
    chase, rounds = {}, {}
    for s in vs.values():
        for d, c in s["chase"].items():
            chase[d] = chase.get(d, 0) + c
        for d, c in s["rounds"].items():
            rounds[d] = rounds.get(d, 0) + c
    all_ = W.new_stats()
    for key in all_:
        all_[key] = chase if key == "chase" else rounds if key == "rounds" else tot(key)
    report["vectors"] = _line("vectors", all_)
    # chase-backs of 0, 1, 2 and >= 8 levels
    assert chase.get(0) and chase.get(1) and chase.get(2) and any(d >= 8 for d in chase), sorted(chase)
    # a meeting in the lane just below pv's root lanes, and at the root itself
    assert tot("meet_top") and tot("meet_root")
    # two rounds of chase-back in one walk
    assert any(r >= 2 for r in rounds), sorted(rounds)
    # a block of more than 64 equal weights: the far leader
    assert vs["once70"]["far"] and vs["once256"]["far"]
    # walks from a deep leaf, parents walked at once after a light swap
    assert tot("deep") and tot("again")


def test_bound_ends_a_cycle():
    """a wrong tree never spins: a parent cycle off the known path runs the mask out"""
    t = M.Tree()
    for sym in range(8):
        t.split(sym)
        t.update(t.where[sym])
    x = M.ROOT - 1  # a child of the root: lighter than the root, so its level neither ties nor swaps
    assert t.w[x] < t.w[x + 1] and t.up[x] == M.ROOT
    t.up[x] = x  # (a bug: the position its own parent)
    with pytest.raises(W.WalkBug):
        W.walk(t, x, W.lanes([]), W.new_stats())

"""GPU parity on forged MNP-5 symbol streams (tests/rle_forge_model.py): the decoders' run revert.

revert_block (hc_fgk.hip) turns a block of 256 symbols into bytes with a lane-parallel state scan,
packed scans of offsets and diff sums, and a run store that takes the runs 16 at a time, four
lanes each, split by the absolute address of the run's first byte into head bytes, aligned
16-byte units and edge bytes, with the diff model's arithmetic sequences built by bytewise adds
without carries. The encoder reaches that code only with maximal counts at the places its input
puts them. Here the symbol streams are hand-built (the FGK payload is the oracle encoder's, so the
streams are ordinary to the FGK layer): every run start residue with every length around the
16-byte units and every step; 1..64 runs a block with empty ones between them and the count at
each byte of its lane; runs, states and a count across block boundaries; seeded random streams
(tests/test_rle_forge_model.py asserts on the CPU that the vectors reach these cases). They go
through the shipping library and the debug build's layouts, launches and 4 KiB windows, at
4-byte-aligned starts with exact capacities and poison around them, against capacities cut inside
a run, and through the single-buffer call. The expected status and bytes are always the oracle's,
compared exactly.
"""
import pytest

import gpu_place as gp
import rle_forge_model as rf
from gpu_batch import decompress_batch
from test_gpu_forge import MODES, _restore
from test_gpu_place import _check, _launch

pytestmark = pytest.mark.gpu

RUN_MODES = ("narrow-regular", "narrow-small", "wide", "huge", "window-regular", "window-small")
_cache = {}


def _sets(oracle_mod):
    """{family: ([(name, container)], [the oracle's bytes])}, computed once"""
    if "sets" not in _cache:
        out = {f: ([], []) for f in rf.FAMILIES}
        for name, data in rf.containers(oracle_mod):
            st, want = oracle_mod.decompress(data)
            assert st == 0, name
            out[rf.family(name)][0].append((name, data))
            out[rf.family(name)][1].append(want)
        _cache["sets"] = out
    return _cache["sets"]


def _by_name(oracle_mod):
    if "by_name" not in _cache:
        _cache["by_name"] = {name: (data, want) for cases, wants in _sets(oracle_mod).values()
                             for (name, data), want in zip(cases, wants)}
    return _cache["by_name"]


def _set_mode(hc, mode):
    tree, small, pack, window = MODES[mode]
    hc.debug_set_min_tree(tree)
    hc.debug_set_dec_small(small)
    hc.debug_set_dec_pack(pack)
    hc.debug_set_window(window)


@pytest.mark.parametrize("mode", ("ship",) + RUN_MODES)
def test_rle_forged_every_configuration(gpu, hc, oracle_mod, mode):
    """every vector, one launch a family, capacities exactly the oracle's lengths"""
    torch = gpu
    sets = _sets(oracle_mod)
    if mode != "ship":
        hc.use_debug_build(True)
    try:
        if mode != "ship":
            _set_mode(hc, mode)
        got = {f: decompress_batch(hc, torch, [d for _, d in cases], [len(w) for w in wants])
               for f, (cases, wants) in sets.items()}
    finally:
        if mode != "ship":
            _restore(hc)
    for f, (cases, wants) in sets.items():
        st, back, olens = got[f]
        assert [n for (n, _), s in zip(cases, st) if s != 0] == []
        assert [n for (n, _), b, w, m in zip(cases, back, wants, olens) if b != w or m != len(w)] == []


@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_rle_forged_placement(gpu, hc, oracle_mod, rot):
    """the align and density families at 4-byte-aligned starts of every residue mod 16 (with the
    align family's 0..15 literals in front of the run: every absolute start residue of the run at
    every base residue), exact capacities, 0xA5 around every slot"""
    torch = gpu
    base_res = 4 * ((rot + 1) % 4)
    sets = _sets(oracle_mod)
    cases = sets["align"][0] + sets["density"][0]
    want = sets["align"][1] + sets["density"][1]
    caps = [len(w) for w in want]
    res = _launch(torch, hc.decompress_batch, [d for _, d in cases], caps, rot, base_res)
    st, olens, dout, ooffs = res
    got = gp.slots(dout, ooffs, caps)
    assert [n for (n, _), s, g, w in zip(cases, st, got, want) if s != 0 or g != w] == []
    _check(res, caps, [0] * len(cases), want)


def capacity_cuts(sym):
    """capacities short of the need, from the stream's blocks: inside a run of the last block, in
    the literals behind that block's last run, inside a run a whole block earlier, and 0"""
    blk = rf.blocks(sym)
    start = [sum(b["out"] for b in blk[:i]) for i in range(len(blk))]
    need = start[-1] + blk[-1]["out"]

    def inside(i):
        off, n, _ = max(blk[i]["runs"], key=lambda r: r[1])  # the block's longest run: >= 40 bytes
        assert n >= 40
        return start[i] + off + n // 2
    off, n, _ = [r for r in blk[-1]["runs"] if r[1]][-1]
    behind = start[-1] + off + n + 1
    assert behind < need  # a literal is cut off
    cuts = [inside(len(blk) - 1), behind, 0]
    if len(blk) > 1:
        cuts.append(inside(len(blk) - 2))
    assert all(0 <= c < need for c in cuts) and len(set(cuts)) == len(cuts)
    return need, cuts


CAPACITY_VECTORS = ("align/p5-c255-v%d" % rf.STEPS[(5 * len(rf.ALIGN_COUNTS) + 23) % len(rf.STEPS)],
                    "density/all255-k1", "density/r64-k2")


@pytest.mark.parametrize("where", ["rot0", "rot1", "rot2", "rot3", "window-regular"])
def test_rle_forged_capacity(gpu, hc, oracle_mod, where):
    """out_caps short of the need, the cut inside a run (the block goes byte by byte), behind the
    last run, a block earlier, at 0: HC_ERR_CAPACITY, out_lens = need, the good stream directly
    behind each short slot exact, no byte outside any slot written. What is inside the short slot
    is open, as in test_gpu_place.test_decode_capacity_short_by_d."""
    torch = gpu
    rot = 1 if where == "window-regular" else int(where[3])
    base_res = 4 * ((rot + 1) % 4)
    by_name = _by_name(oracle_mod)
    align = _sets(oracle_mod)["align"]
    blobs, caps, want_st, want, open_slots = [], [], [], [], []
    for name in CAPACITY_VECTORS:
        for flags in ("/00", "/80"):
            data, out = by_name[name + flags]
            need, cuts = capacity_cuts(rf.symbols_of(name))
            assert need == len(out)
            for cap in cuts:
                k = (37 * len(blobs) + 11) % len(align[0])  # the neighbour: some align vector
                open_slots.append(len(blobs))
                blobs += [data, align[0][k][1]]
                caps += [cap, len(align[1][k])]
                want_st += [hc.HC_ERR_CAPACITY, 0]
                want += [need, align[1][k]]
    if where == "window-regular":
        hc.use_debug_build(True)
    try:
        if where == "window-regular":
            _set_mode(hc, where)
        res = _launch(torch, hc.decompress_batch, blobs, caps, rot, base_res)
    finally:
        if where == "window-regular":
            _restore(hc)
    _check(res, caps, want_st, want, set(open_slots))


def test_rle_forged_single_buffer(gpu, hc, oracle_mod):
    """hc.decompress of the all-255 density vector and three carry vectors"""
    by_name = _by_name(oracle_mod)
    for name in ("density/all255-k0", "carry/edge256-s3-c255", "carry/edge512-s3-c1", "carry/nines259"):
        for flags in ("/00", "/80"):
            data, want = by_name[name + flags]
            assert hc.decompress(data) == (0, want), name + flags

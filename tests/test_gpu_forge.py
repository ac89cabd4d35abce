"""GPU parity on forged streams: NYT escapes that name a known symbol (tests/fgk_forge_model.py).

No encoder writes the NYT leaf's code followed by 8 raw bits that name a symbol which already has a
leaf, but the reference accepts it and updates the symbol's own leaf without a split
(huffman.cpp:95-128). The decoder has code for this case alone -- Fgk::find_leaf and the
`chase(known)` branch of Dec::finish_symbol -- which every fast path must reach in a consistent
state: the batch step's hand-off at an NYT entry, decode_small's marks and counts, the level
tables' generations under the escape's swaps, the parents of the wide and huge layouts, the NYT at
position 0 once all 256 symbols are seen.

Before these tests only tests/test_fuzz.py came here, by chance: of its 480 seeded mutants 28 hold
at least one known-symbol escape (31 escapes in all, counted by fgk_forge_model.count_known_escapes;
tests/test_forge_model.py::test_fuzz_census prints the figure), all of them decoded in the shipping
configuration with 64 bytes of slack. Here every vector holds such escapes by construction
(tests/test_forge_model.py asserts it on the CPU, and that the reference binary accepts them), and
they go through the shipping library and, in the debug build, the narrow, wide and huge layouts,
the small-alphabet launch, 1 / 7 codes a batch step and 4 KiB windows; at 4-byte-aligned starts
with exact capacities and poison around them; cut inside an escape; as the symbol stream of the
adaptive path; as one segment of a segmented container. The expected status and bytes are always
the oracle's, compared exactly.
"""
import random

import numpy as np
import pytest

import fgk_forge_model as fm
import seg_check_model
from gpu_batch import compress_batch, decompress_adapt_batch, decompress_batch
from test_gpu_adaptive_bounds import adaptive_stream
from test_gpu_place import _check, _launch, _raws

pytestmark = pytest.mark.gpu

_cache = {}


def _expected(oracle_mod, key, cases):
    """[(status, bytes)] of the oracle for a list of (name, container), computed once"""
    if key not in _cache:
        _cache[key] = [oracle_mod.decompress(data) for _, data in cases]
    return _cache[key]


def _sets(oracle_mod):
    """the forged containers in two batches (the phase set: 64 streams; the rest, flags 0x00 and
    0x80) with the oracle's results"""
    if "sets" not in _cache:
        cases = fm.forged_containers()
        phase = [c for c in cases if c[0].startswith("phase")]
        rest = [c for c in cases if not c[0].startswith("phase")]
        assert len(phase) == fm.PHASES and len(rest) <= 64
        out = []
        for part in (rest, phase):
            want = [oracle_mod.decompress(data) for _, data in part]
            assert all(st == 0 for st, _ in want)
            out.append((part, want))
        _cache["sets"] = out
    return _cache["sets"]


def _restore(hc):
    hc.debug_set_dec_pack(16)
    hc.debug_set_dec_small(0)
    hc.debug_set_min_tree(0)
    hc.debug_set_window(1 << 30)
    hc.debug_set_par_min(1 << 20)
    hc.use_debug_build(False)


# mode: (smallest tree layout, decoder launch hook, codes a batch step, window) -- the layouts and
# launches of tests/test_gpu_climb.py's table, then the pack caps and the 4 KiB window
MODES = {
    "narrow-regular": (0, 2, 16, 1 << 30), "narrow-small": (0, 1, 16, 1 << 30),
    "wide": (1, 0, 16, 1 << 30), "huge": (2, 0, 16, 1 << 30),
    "pack1": (0, 2, 1, 1 << 30), "pack7": (0, 2, 7, 1 << 30), "pack1-small": (0, 1, 1, 1 << 30),
    "pack7-wide": (1, 0, 7, 1 << 30),
    "window-regular": (0, 2, 16, 4096), "window-small": (0, 1, 16, 4096),
}


@pytest.mark.parametrize("mode", ["ship"] + list(MODES))
def test_forged_batch_every_configuration(gpu, hc, oracle_mod, mode):
    torch = gpu
    if mode != "ship":
        tree, small, pack, window = MODES[mode]
        hc.use_debug_build(True)
    try:
        if mode != "ship":
            hc.debug_set_min_tree(tree)
            hc.debug_set_dec_small(small)
            hc.debug_set_dec_pack(pack)
            hc.debug_set_window(window)
        got = [decompress_batch(hc, torch, [d for _, d in part], [len(w) for _, w in want])
               for part, want in _sets(oracle_mod)]
    finally:
        if mode != "ship":
            _restore(hc)
    for (part, want), (st, back, _) in zip(_sets(oracle_mod), got):
        assert [n for (n, _), s in zip(part, st) if s != 0] == []
        assert [n for (n, _), b, (_, w) in zip(part, back, want) if b != w] == []


@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_forged_exact_capacities_and_poison(gpu, hc, oracle_mod, rot):
    """4-byte-aligned starts, out_caps exactly the oracle's lengths, poison around every slot, a
    good stream after every third forged one"""
    torch = gpu
    base_res = 4 * ((rot + 1) % 4)
    raws = _raws(oracle_mod)
    blobs, want = [], []
    for part, exp in _sets(oracle_mod):
        for k, ((_, data), (_, out)) in enumerate(zip(part, exp)):
            blobs.append(data)
            want.append(out)
            if k % 3 == 2:
                r = raws[(len(blobs) + rot) % len(raws)]
                st, e = oracle_mod.compress(r, bool(k & 1), False, 512)
                assert st == 0
                blobs.append(e)
                want.append(r)
    caps = [len(w) for w in want]
    _check(_launch(torch, hc.decompress_batch, blobs, caps, rot, base_res), caps, [0] * len(blobs), want)


@pytest.mark.parametrize("mode", ["ship", "wide"])
def test_forged_truncations(gpu, hc, oracle_mod, mode):
    """every vector cut inside an escape (after the NYT code, after 1..7 raw bits, on the byte that
    ends it): status 9, or status 0 with the oracle's bytes, whichever the oracle says. Capacities:
    the oracle's length where it accepts the stream, else the vector's decoded length + 64"""
    torch = gpu
    cuts = fm.truncated_containers()
    want = _expected(oracle_mod, "cuts", cuts)
    assert {st for st, _ in want} == {0, 9}
    whole = {name.split("/")[0]: len(out) for part, exp in _sets(oracle_mod) for (name, d), (_, out) in zip(part, exp)
             if d[8] == 0}
    caps = [len(out) if st == 0 else whole[name.split(":")[0]] + 64 for (name, _), (st, out) in zip(cuts, want)]
    if mode != "ship":
        hc.use_debug_build(True)
    try:
        if mode != "ship":
            hc.debug_set_min_tree(1)
        st, back, _ = decompress_batch(hc, torch, [d for _, d in cuts], caps)
    finally:
        if mode != "ship":
            _restore(hc)
    assert [n for (n, _), s, (w, _) in zip(cuts, st, want) if s != w] == []
    assert [n for (n, _), b, (w, out) in zip(cuts, back, want) if w == 0 and b != out] == []


ADAPT = [(8, 8, 8), (17, 23, 8), (40, 33, 16), (64, 64, 32), (90, 90, 16)]


def _adapt_cases(oracle_mod):
    """forged FGK payloads around valid adaptive symbol streams, flags 0x40"""
    if "adapt" not in _cache:
        rng = np.random.default_rng(314)
        cases = []
        for k, (w, h, b) in enumerate(ADAPT):
            hdr, body = adaptive_stream(rng, w, h, b)
            sym = hdr + body
            assert len(sym) <= fm.MAX_SYMBOLS
            r = random.Random(400 + k)
            seen, esc = set(), []
            for s in sym:
                esc.append(s in seen and r.random() < 0.08)
                seen.add(s)
            data = fm.container(sym, esc, 0x40)
            assert fm.count_known_escapes(data[9:], len(sym)) > 0
            cases.append(("adapt%dx%d" % (w, h), data))
        want = [oracle_mod.decompress(d) for _, d in cases]
        assert all(st == 0 and len(out) == w * h for (st, out), (w, h, _) in zip(want, ADAPT))
        _cache["adapt"] = (cases, want)
    return _cache["adapt"]


@pytest.mark.parametrize("par", [False, True])
def test_forged_symbol_destination(gpu, hc, oracle_mod, par):
    """the decoder's symbol destination (the adaptive path): batched and single-buffer calls, in the
    shipping configuration and with every stream's block boundaries found by the parallel pass"""
    torch = gpu
    cases, want = _adapt_cases(oracle_mod)
    if par:
        hc.use_debug_build(True)
    try:
        if par:
            hc.debug_set_par_min(0)
        st, back, _ = decompress_adapt_batch(hc, torch, [d for _, d in cases], [len(w) for _, w in want])
        single = [hc.decompress(d) for _, d in cases]
    finally:
        if par:
            _restore(hc)
    assert st == [0] * len(cases)
    assert [n for (n, _), b, (_, w) in zip(cases, back, want) if b != w] == []
    assert [n for (n, _), got, w in zip(cases, single, want) if got != w] == []


@pytest.mark.parametrize("check", [False, True])
@pytest.mark.parametrize("use_diff", [False, True])
def test_forged_container_segment(gpu, hc, oracle_mod, use_diff, check):
    """one segment of a four-segment HCSEG1 container replaced by a forged stream of the same
    decoded bytes (longer: the container is laid out again): HC_OK and the original bytes; the
    CRC-32 of a checked container still verifies, since the bytes are equal"""
    raw = oracle_mod.synth("grad", 3, 128, 128).tobytes()
    st, cont = hc.seg_compress(raw, use_diff=use_diff, seg_bytes=4096, check=check)
    assert st == 0 and cont == seg_check_model.build(raw, use_diff, False, 512, 4096, check)
    streams = seg_check_model.segments(cont)
    assert len(streams) == 4
    k = 2
    seg = raw[k * 4096:(k + 1) * 4096]
    sym = list(oracle_mod.rle(oracle_mod.diff(seg) if use_diff else seg))
    assert len(sym) <= fm.MAX_SYMBOLS
    r = random.Random(500)
    seen, esc = set(), []
    for s in sym:
        esc.append(s in seen and r.random() < 0.05)
        seen.add(s)
    forged = fm.container(sym, esc, 0x80 if use_diff else 0x00)
    assert fm.count_known_escapes(forged[9:], len(sym)) > 0 and len(forged) > len(streams[k])
    assert oracle_mod.decompress(forged) == (0, seg)
    streams[k] = forged
    mine = seg_check_model.repack(cont, streams)
    assert mine != cont and seg_check_model.decode(mine) == (0, seg_check_model.NO_SEGMENT, raw)
    assert hc.seg_decompress(mine, full=True) == (0, raw, len(raw), hc.NO_SEGMENT)


def test_forged_round_trip_is_canonical(gpu, hc, oracle_mod):
    """the decoded bytes of three forged containers, encoded again on the GPU, give the oracle's
    stream, which differs from the forged one: the vectors are not encoder-shaped"""
    torch = gpu
    (rest, want), _ = _sets(oracle_mod)
    pick = [i for i, (name, _) in enumerate(rest) if name in ("skewed/00", "full/00", "mnp5-both/00")]
    assert len(pick) == 3
    forged = [rest[i][1] for i in pick]
    st, back, _ = decompress_batch(hc, torch, forged, [len(want[i][1]) for i in pick])
    assert st == [0, 0, 0] and back == [want[i][1] for i in pick]
    st, encs, _ = compress_batch(hc, torch, back, False)
    assert st == [0, 0, 0]
    for raw, enc, f in zip(back, encs, forged):
        assert (0, enc) == oracle_mod.compress(raw, False, False, 512)
        assert enc != f and oracle_mod.decompress(enc) == (0, raw)

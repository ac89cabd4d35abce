"""The strided chains of code starts (hc_fgk.hip Dec::decode_batch, HC_DEC_CHAIN 2 and 4; model:
tests/fgk_chain_model.py) give the packed step what the chain of single codes gives it: the starts
sv[0..16] wherever one lies inside the window, nval, jmax, se, the start mask and every lane's code
start (fgk_chain_model.same_step states what may differ and why nothing reads it) -- on every depth
map the benchmark's streams produce, on random ones, and on ones built around bit 63. The streams of
tests/test_gpu_chain.py reach every edge the change was specified with."""
import random

import pytest

from fgk_chain_model import EDGES, compose, decode_chain, same_step, stream_bits
from fgk_pack_model import decode_packed
from fgk_topup_model import bench_streams, decode_topup

_cache = {}
PREFIX = 4000  # symbols of each GPU stream the model decodes


def gpu_streams(oracle_mod):
    """(raw, with the diff model): the streams of tests/test_gpu_chain.py -- those of
    tests/test_gpu_pack.py and the ones added for the chain's edges: 6-bit codes (64 symbols, evenly
    spread: a start passes bit 62 inside a group of four), and a stream of three symbols, one of them
    seven times in ten (1- and 2-bit codes: all sixteen links, the cap binds at odd and even starts; the
    RLE in front of the coder caps runs of equal symbols, so sixteen 1-bit codes in a row are rare in
    any stream: the model finds them where a window is parsed past a symbol that changes the tree)"""
    from test_topup_model import gpu_streams as base
    rng = random.Random(41)
    six = bytes(rng.randrange(64) * 4 for _ in range(6000))
    ones = bytes(rng.choice((9, 9, 9, 9, 9, 9, 9, 200, 200, 31)) for _ in range(6000))
    b = base(oracle_mod)
    h = len(b) // 2
    return b[:h] + [(six, True), (ones, True)] + b[h:] + [(six, False), (ones, False)]


def _bench_runs(oracle_mod):
    """per benchmark stream (photo 0-3, grad, noise; 60000 symbols): the symbols, their bits, the run
    at stride 1 and the distinct (dep, lim, left) of its steps with and without the full window"""
    if "b" not in _cache:
        out = []
        for name, syms in bench_streams(oracle_mod):
            bits = stream_bits(syms)
            vec = set()
            runs = {}
            for topup in (True, False):
                runs[topup] = decode_chain(bits, len(syms), 1, topup=topup, on_step=lambda d, l, left: vec.add((tuple(d), l, left)))
            out.append((name, syms, bits, runs, vec))
        _cache["b"] = out
    return _cache["b"]


def _same_tree(t1, t2):
    return t1.w == t2.w and t1.body == t2.body and t1.up == t2.up


def test_bit_level_decoder_beside_the_symbol_level_models(oracle_mod):
    """the model that parses the window's bits restores every symbol and leaves the tree of
    decode_packed / decode_topup; its steps are within 2 % of decode_topup's, whose window it keeps (why
    not equal: the model's docstring)"""
    for name, syms, _, runs, _ in _bench_runs(oracle_mod):
        for topup in (True, False):
            out, st, _, t = runs[topup]
            assert out == syms, name
            t0, ref = decode_topup(syms, topup=topup)[:2]
            assert _same_tree(t, t0) and (topup or _same_tree(t, decode_packed(syms)[0])), name
            print(name, topup, st["steps"], ref["steps"], st["links"])
            assert abs(st["steps"] - ref["steps"]) <= 0.02 * ref["steps"] + 32, name


def test_strides_agree_on_every_step_of_the_benchmark_streams(oracle_mod):
    n = 0
    for _, _, _, _, vec in _bench_runs(oracle_mod):
        for dep, lim, left in vec:
            for cap in (16, 7, 1) if n % 8 == 0 else (16,):
                same_step(list(dep), lim, cap, left)
            n += 1
    assert n > 50000


@pytest.mark.parametrize("stride", [2, 4])
def test_strided_decoders_decode_the_benchmark_streams(oracle_mod, stride):
    """photo 0, grad and noise decoded with the strided chain in the loop, 64 true bits and the
    window's own: every symbol, the tree, and the steps of stride 1"""
    for k in (0, 4, 5):
        name, syms, bits, runs, _ = _bench_runs(oracle_mod)[k]
        for topup in (True, False):
            out, st, ed, t = decode_chain(bits, len(syms), stride, topup=topup)
            assert out == syms and _same_tree(t, runs[topup][3]), name
            assert (st["steps"], st["alone"], st["sent"], ed) == tuple(runs[topup][1][k] for k in ("steps", "alone", "sent")) + (runs[topup][2],)
            assert {stride * k: v for k, v in st["links"].items()} == runs[topup][1]["links"]


def _built(rng):
    """a depth map whose chain puts starts on 61..66: a run of equal depths up to a chosen start,
    then depths that step over bit 63 one way or another"""
    target = rng.randrange(56, 64)
    d = [rng.randrange(1, 9) for _ in range(64)]
    w = rng.choice((4, 5, 6, 7, 8)) if rng.random() < 0.6 else rng.randrange(3, 9)
    s = 0
    while s < target:
        d[s] = min(w, target - s) if target - s < w or rng.random() < 0.9 else rng.randrange(1, min(8, target - s) + 1)
        s += d[s]
    while s < 64:
        d[s] = rng.randrange(1, 9)
        s += d[s]
    return d


def test_strides_agree_on_random_and_built_depth_maps():
    """about 10^5 windows: constant depths 1..8 (all ones, all eights), a tail of another depth, random
    depths up to 2, 3, 4, 6 and 8, and maps built to put starts on 61..66; each at lim 63 and at one
    of 32..62 (32 behind a first 8-bit code: the only way to the exit after four links), every cap
    the debug hook sets and block ends of 1..16 symbols"""
    rng = random.Random(7)
    seen = {k: 0 for k in (61, 62, 63, 64, 65, 66)}
    exits = {4: 0, 8: 0, 12: 0, 16: 0}
    vecs = [[1] * 64, [8] * 64, [6] * 64, [4] * 64, [2] * 64, [1] * 63 + [8], [8] * 63 + [1]]
    for k in range(1, 9):
        vecs += [[k] * 56 + [j] * 8 for j in range(1, 9)]
    for _ in range(25000):
        hi = rng.choice((2, 3, 4, 6, 8, 8))
        vecs.append([rng.randrange(1, hi + 1) for _ in range(64)])
    for _ in range(25000):
        vecs.append(_built(rng))
    for d in vecs:
        for lim in (63, 32 if d[0] == 8 else rng.randrange(32, 63)):
            left = rng.choice((1 << 30, 1 << 30, rng.randrange(1, 17)))
            sv1, _, _, _ = same_step(d, lim, rng.choice((16, 16, 7, 1)), left)
            exits[sum(v != 255 for v in sv1[1:17])] += 1
            if lim == 63:
                for v in sv1[1:17]:
                    if v in seen:
                        seen[v] += 1
    print(seen, exits)
    assert all(v > 100 for v in seen.values()) and all(v > (0 if k == 4 else 100) for k, v in exits.items())


def test_composition_never_wraps():
    """dep2 / dep4 of an offset whose two / four codes end past bit 63 is 64 more than a start can be:
    the chain's next start from there is above every lim, whatever lies at the wrapped offset"""
    rng = random.Random(3)
    for _ in range(2000):
        d = [rng.randrange(1, 9) for _ in range(64)]
        d2 = compose(d)
        d4 = compose(d2)
        for o in range(64):
            for one, two in ((d, d2), (d2, d4)):
                if o + one[o] < 64:
                    assert two[o] == one[o] + one[o + one[o]]
                else:
                    assert two[o] == one[o] + 64 and o + two[o] >= 128


def test_gpu_streams_reach_every_chain_edge(oracle_mod):
    """every stream of tests/test_gpu_chain.py through the model, its bits the payload of the oracle's
    encoding, at caps 16, 7 and 1 (the model's level tables are the kernel's: an entry may be stale), the
    strided chain checked against the single one at every step. Among the steps: a next start at
    exactly bit 62, 63, 64 and later; a composed jump from inside the window to past bit 63; an
    odd-indexed start as the last one taken (at cap 16, and at the caps 7 and 1, which are odd); sixteen
    1-bit codes (starts 0..16); a 6-bit code that carries the start past bit 62 inside a group of four; a
    code that is no leaf in the middle of a step; a stale table entry; a step that the stream's or a
    block's end cuts short; a step that uses bits of the peeked word; an exit after four, eight and
    twelve links -- the exit after eight in the window's own bits only (the small-alphabet launch): behind
    a first code of at most 6 bits (the gate) eight codes end by bit 62 and four by bit 30, below every
    lim, so the exit after four links is never taken. The model reads the first PREFIX symbols of
    every stream. (Truncated streams, whose peeked bits read as zeros, are decoded on the GPU only.)"""
    seen = {cap: {e: 0 for e in EDGES} for cap in (16, 7, 1, "own")}
    for k, (raw, diff) in enumerate(gpu_streams(oracle_mod)):
        syms = list(oracle_mod.rle(oracle_mod.diff(raw)) if diff else oracle_mod.rle(raw))[:PREFIX]
        st, enc = oracle_mod.compress(raw, diff, False, 512)
        assert st == 0
        bits = [(byte >> (7 - j)) & 1 for byte in enc[9:] for j in range(8)]
        for cap in (16, 7, 1, "own"):
            if cap != 16 and k % 5:
                continue
            c = 16 if cap == "own" else cap
            out, _, ed, _ = decode_chain(bits, len(syms), 2 if k % 2 else 4, cap=c, topup=cap != "own",
                                         on_step=lambda d, l, left: same_step(d, l, c, left))
            assert out == syms, (k, cap)
            for e in EDGES:
                seen[cap][e] += ed[e]
    print(seen)
    assert all(v > 0 for e, v in seen[16].items() if e not in ("exit_4", "exit_8")), seen[16]
    assert seen[7]["odd_last"] > 0 and seen[1]["odd_last"] > 0 and seen["own"]["exit_8"] > 0
    assert all(seen[c]["exit_4"] == 0 for c in seen) and seen[16]["exit_8"] == 0

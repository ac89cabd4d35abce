"""GPU parity of the grouped climb and the grouped descent (hc_fgk.hip: Fgk::chase_grouped, the
path-cache encoder's miss chase with one root test per group of levels; Dec::finish_symbol, the
long-code descent with one inner test per group; model: tests/fgk_climb_model.py).

The vectors (fgk_climb_model.vectors, at most 50 k symbols each; tests/test_climb_model.py asserts
on the CPU what they hold): skewed streams with Fibonacci-like symbol counts, whose rare symbols
have codes of up to 20 and more bits; the same behind 1..40 common symbols, which moves every long
code across the decoder's window words; a ramp over all 256 symbols (position 0 in use when a climb
passes the root) with a skewed tail; one- and two-symbol streams. One batch goes through the
shipping library and, in the debug build, through the narrow, wide and huge layouts and the cache,
table and small-alphabet modes, from raw bytes, raw bytes with the diff model and (the adaptive
path) symbols: the encoded bytes equal the oracle's byte for byte and decode to the input. Every
stream cut at each of its last 64 bytes gives the oracle's status and output."""
import pytest

from fgk_climb_model import vectors
from fgk_handoff_model import raw_of
from gpu_batch import compress_adapt_batch, compress_batch, decompress_adapt_batch, decompress_batch

pytestmark = pytest.mark.gpu

_cache = {}


def _batch(oracle_mod, use_diff):
    """(raws, the oracle's encodings), computed once per source"""
    if use_diff not in _cache:
        raws = [raw_of(sym) if use_diff else bytes(sym) for _, sym in vectors()]
        wants = []
        for r in raws:
            st, enc = oracle_mod.compress(r, use_diff, False, 512)
            assert st == 0
            wants.append(enc)
        _cache[use_diff] = (raws, wants)
    return _cache[use_diff]


def _restore(hc):
    hc.debug_set_min_tree(0)
    hc.debug_set_enc_tab(0)
    hc.debug_set_dec_small(0)
    hc.use_debug_build(False)


# mode: (encoder mode hook, smallest tree layout, decoder launch hook)
MODES = {"cache": (1, 0, 2), "wide": (1, 1, 0), "huge": (1, 2, 0), "table": (2, 0, 2), "table-wide": (2, 1, 0),
         "small": (3, 0, 1)}


@pytest.mark.parametrize("mode,use_diff", [("ship", True), ("ship", False), ("cache", True), ("cache", False),
                                           ("wide", True), ("huge", True), ("huge", False), ("table", True),
                                           ("table-wide", True), ("small", True)])
def test_climb_batch_vs_oracle(gpu, hc, oracle_mod, mode, use_diff):
    torch = gpu
    raws, wants = _batch(oracle_mod, use_diff)
    if mode != "ship":
        tab, tree, small = MODES[mode]
        hc.use_debug_build(True)
    try:
        if mode != "ship":
            hc.debug_set_enc_tab(tab)
            hc.debug_set_min_tree(tree)
            hc.debug_set_dec_small(small)
        st, encs, _ = compress_batch(hc, torch, raws, use_diff)
        assert st == [0] * len(raws)
        assert [i for i, (e, w) in enumerate(zip(encs, wants)) if e != w] == []
        st, back, _ = decompress_batch(hc, torch, encs, [len(r) for r in raws])
        assert st == [0] * len(raws)
        assert [i for i, (r, b) in enumerate(zip(raws, back)) if r != b] == []
    finally:
        if mode != "ship":
            _restore(hc)


@pytest.mark.parametrize("use_diff", [True, False])
def test_climb_symbol_source(gpu, hc, oracle_mod, use_diff):
    """the adaptive path hands the FGK kernels symbols: the same vectors as 64-byte-wide matrices"""
    torch = gpu
    raws = [r[:len(r) // 64 * 64] for r in _batch(oracle_mod, True)[0] if len(r) >= 512]
    assert len(raws) >= 40
    st, encs, _ = compress_adapt_batch(hc, torch, raws, [64] * len(raws), use_diff)
    for i, r in enumerate(raws):
        want_st, want = oracle_mod.compress(r, use_diff, True, 64)
        assert want_st == 0 and st[i] == 0 and encs[i] == want, i
    st, back, _ = decompress_adapt_batch(hc, torch, encs, [len(r) for r in raws])
    assert st == [0] * len(raws)
    assert [i for i, (r, b) in enumerate(zip(raws, back)) if r != b] == []


@pytest.mark.parametrize("mode", ["ship", "wide"])
def test_climb_truncated_streams(gpu, hc, oracle_mod, mode):
    """every stream cut at each of its last 64 bytes (a long code cut mid-descent among them): the
    oracle's status (transform.cpp:394-398 ends a stream whose count exceeds its payload with 9)
    and, where it accepts the stream, its output; capacities leave no room to run past a buffer"""
    torch = gpu
    raws, wants = _batch(oracle_mod, True)
    bad, size = [], []
    for r, e in zip(raws, wants):
        for cut in range(1, min(64, len(e)) + 1):
            bad.append(e[:len(e) - cut])
            size.append(len(r))
    expect = [oracle_mod.decompress(b) for b in bad]
    caps = [len(w[1]) if w[0] == 0 else n + 64 for w, n in zip(expect, size)]
    if mode != "ship":
        hc.use_debug_build(True)
    try:
        if mode != "ship":
            hc.debug_set_min_tree(1)
        st, back, _ = decompress_batch(hc, torch, bad, caps)
    finally:
        if mode != "ship":
            _restore(hc)
    assert [j for j, w in enumerate(expect) if st[j] != w[0]] == []
    assert [j for j, w in enumerate(expect) if w[0] == 0 and back[j] != w[1]] == []

"""GPU parity of the walk's lean climb back to the known path (hc_fgk.hip: Fgk::walk, HC_WALK_LEAN:
the chase-back by a running lane mask, bounded by the mask running out, and the meeting at once
that keeps the known path; model: tests/fgk_walk_model.py).

The vectors (fgk_walk_model.vectors: a dozen streams of at most 4096 symbols; tests/
test_walk_model.py asserts on the CPU what their walks hold): chase-backs of 0, 1, 2 and 8 levels,
meetings in the lane just below the known path's root lanes and at the root itself, walks of two
and more rounds of chase-back, blocks of more than 64 equal weights (the far leader: 70, 130 and
256 distinct symbols once each), walks from a deep leaf. One batch goes through the shipping
library and, in the debug build, through the encoder in cache mode and in table mode, the decoder,
and the narrow, wide and huge layouts: the encoded bytes equal the oracle's byte for byte and
decode to the input."""
import pytest

from fgk_handoff_model import raw_of
from fgk_walk_model import vectors
from gpu_batch import compress_batch, decompress_batch

pytestmark = pytest.mark.gpu

_cache = {}


def _batch(oracle_mod, use_diff):
    """(raws, the oracle's encodings), computed once per source"""
    if use_diff not in _cache:
        raws = [raw_of(sym) if use_diff else bytes(sym) for _, sym in vectors()]
        assert len(raws) <= 64 and max(map(len, raws)) <= 4096
        wants = []
        for r in raws:
            st, enc = oracle_mod.compress(r, use_diff, False, 512)
            assert st == 0
            wants.append(enc)
        _cache[use_diff] = (raws, wants)
    return _cache[use_diff]


# mode: (encoder mode hook, smallest tree layout, decoder launch hook)
MODES = {"cache": (1, 0, 2), "wide": (1, 1, 0), "huge": (1, 2, 0), "table": (2, 0, 2), "table-wide": (2, 1, 0),
         "small": (3, 0, 1)}


@pytest.mark.parametrize("mode,use_diff", [("ship", True), ("ship", False), ("cache", True), ("cache", False),
                                           ("wide", True), ("huge", True), ("table", True), ("table", False),
                                           ("table-wide", True), ("small", True)])
def test_walk_batch_vs_oracle(gpu, hc, oracle_mod, mode, use_diff):
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
            hc.debug_set_min_tree(0)
            hc.debug_set_enc_tab(0)
            hc.debug_set_dec_small(0)
            hc.use_debug_build(False)

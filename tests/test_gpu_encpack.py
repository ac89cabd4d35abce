"""GPU parity of the encoder's batch step packed by path depth (hc_fgk.hip code_all_batch,
HC_ENC_PACK: up to 16 cached symbols a step, each on as many lanes as its path has positions;
model: tests/fgk_encpack_model.py, checked in tests/test_encpack_model.py).

One batch of a few hundred short streams (at most 16 KB each) through hc_compress_batch, byte for
byte against the oracle, then decoded back. The streams come from the model's fixed-seed search,
run when this file is collected: streams without runs (their MNP-5 symbols are their diffed bytes,
coded one 256-byte chunk per pass) that together hold
  * a step that takes all 16 symbols, and steps whose lanes end at exactly 63;
  * steps where the next symbol would cross lane 63, with depth sums 62 + 2, 63 + 1 and 55 + 9;
  * a depth-9 symbol first in a step, and one last in a step;
  * a miss, and a fresh symbol (a split), as step symbol j for every j = 0..15;
  * a reported level at some level of symbol j for every j = 0..15, falsely reported ones for
    every j too (the exact test passes them);
  * the ending symbol's record in lane 63 (pack follows);
  * the last step of a pass with fewer than 16 symbols left, ending at a miss, a split and a level
(tests/test_encpack_model.py asserts exactly this coverage). Every candidate of the search also
runs cut to three shorter lengths, which moves the pass ends. The same batch runs in the shipping
library (the vote sends these skewed alphabets to the path cache), with the path cache forced, in
the wide layout, and through the small-alphabet launch, whose copy of the regular step takes over
once a stream has seen more than 16 symbols; in the debug build also with the step capped at 1 and
at 7 symbols (debug_set_enc_pack)."""
import pytest

from fgk_encpack_model import CROSS, PACK, candidates, search
from fgk_handoff_model import raw_of
from gpu_batch import compress_batch, decompress_batch

pytestmark = pytest.mark.gpu

CHOSEN, STATES = search()
CUTS = (1.0, 0.77, 0.52, 0.1)


def _raws():
    names = {name for name, _ in CHOSEN}
    cands = list(candidates())
    assert names <= {name for name, _ in cands}
    raws = []
    for _, syms in cands:
        for cut in CUTS:
            raws.append(raw_of(syms[:int(len(syms) * cut) + (0 if cut == 1.0 else 5)]))
    return raws, [len(set(syms)) for _, syms in cands]


@pytest.fixture(scope="module")
def batch(oracle_mod):
    raws, alphabets = _raws()
    assert 200 <= len(raws) <= 400 and max(map(len, raws)) <= 16384
    assert sum(a > 16 for a in alphabets) >= 8  # streams that outgrow the small-alphabet steps
    wants = []
    for r in raws:
        st, enc = oracle_mod.compress(r, True, False, 512)
        assert st == 0
        wants.append(enc)
    return raws, wants


def test_search_reaches_the_states():
    """(the full coverage is asserted on the CPU: tests/test_encpack_model.py)"""
    assert all(STATES["miss", j] and STATES["fresh", j] for j in range(PACK))
    assert all(any(STATES["level", j, l] for l in range(9)) for j in range(PACK))
    assert STATES["full",] and STATES["end63",] and STATES["fill64",]
    assert all(STATES["cross", s, d] for s, d in CROSS)
    assert STATES["deep_first",] and STATES["deep_last",]
    assert any(k[0] == "false" for k in STATES)


@pytest.mark.parametrize("mode,cap", [("ship", 16), ("cache", 16), ("wide", 16), ("small", 16),
                                      ("cache", 1), ("cache", 7), ("wide", 7), ("small", 7), ("small", 1)])
def test_encpack_batch_vs_oracle(gpu, hc, batch, mode, cap):
    torch = gpu
    raws, wants = batch
    if mode == "ship":
        st, encs, _ = compress_batch(hc, torch, raws, True)
    else:
        hc.use_debug_build(True)
        try:
            hc.debug_set_enc_pack(cap)
            hc.debug_set_enc_tab(3 if mode == "small" else 1)
            hc.debug_set_min_tree(1 if mode == "wide" else 0)
            st, encs, _ = compress_batch(hc, torch, raws, True)
        finally:
            hc.debug_set_min_tree(0)
            hc.debug_set_enc_tab(0)
            hc.debug_set_enc_pack(16)
            hc.use_debug_build(False)
    assert st == [0] * len(raws)
    assert [i for i, (e, w) in enumerate(zip(encs, wants)) if e != w] == []
    st, back, _ = decompress_batch(hc, torch, encs, [len(r) for r in raws])
    assert st == [0] * len(raws)
    assert [i for i, (r, b) in enumerate(zip(raws, back)) if r != b] == []

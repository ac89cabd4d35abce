"""GPU parity of the encoder's batch-step hand-offs (hc_fgk.hip code_all_batch: the symbol that
ends a regular step is finished from what the step's lanes hold, HC_ENC_HANDOFF_MISS /
HC_ENC_HANDOFF_LEVEL; model: tests/fgk_handoff_model.py, checked in tests/test_handoff_model.py).
The bytes are the oracle's whichever of the two parts the library was built with; the states below
are what the step's lanes hold when it hands over.

One batch of a few hundred short streams (at most 6 KB each) through hc_compress_batch, byte for
byte against the oracle, then decoded back. The streams come from the model's fixed-seed search,
run when this file is collected: streams without runs (their MNP-5 symbols are their diffed bytes,
coded one 256-byte chunk per pass) that together end a step
  * at a miss of step symbol j = 0..6, and at a fresh symbol (a split) for j = 0..6;
  * at a reported level l of a cached symbol j for every pair (j, l), j = 0..6, l = 0..8, except
    (0, 6), (0, 7), (0, 8), (2, 8), (3, 8), (4, 7), (4, 8), (5, 7), (5, 8), (6, 7), (6, 8), which
    no searched input reaches (tests/test_handoff_model.py asserts exactly this coverage);
  * at falsely reported levels (the walk's exact test passes them) of every depth 0..7;
  * with the hand-off's record in lane 63 (sink.n + jf + 1 == 64: pack follows);
  * in the last step of a pass with fewer than seven symbols left, at a miss, a split and a level.
Every candidate of the search also runs cut to three shorter lengths, which moves the pass ends.
The same batch runs in the shipping library (the vote sends these skewed alphabets to the path
cache), with the path cache forced, in the wide layout, and through the small-alphabet launch,
whose copy of the regular step takes over once a stream has seen more than 16 symbols."""
import pytest

from fgk_handoff_model import candidates, raw_of, search
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
    """(the full coverage is asserted on the CPU: tests/test_handoff_model.py)"""
    assert all(STATES["miss", j] and STATES["fresh", j] and STATES["level", j, 0] for j in range(7))
    assert STATES["fill64",] and any(k[0] == "false" for k in STATES)


@pytest.mark.parametrize("mode", ["ship", "cache", "wide", "small"])
def test_handoff_batch_vs_oracle(gpu, hc, batch, mode):
    torch = gpu
    raws, wants = batch
    if mode == "ship":
        st, encs, _ = compress_batch(hc, torch, raws, True)
    else:
        hc.use_debug_build(True)
        try:
            hc.debug_set_enc_tab(3 if mode == "small" else 1)
            hc.debug_set_min_tree(1 if mode == "wide" else 0)
            st, encs, _ = compress_batch(hc, torch, raws, True)
        finally:
            hc.debug_set_min_tree(0)
            hc.debug_set_enc_tab(0)
            hc.use_debug_build(False)
    assert st == [0] * len(raws)
    assert [i for i, (e, w) in enumerate(zip(encs, wants)) if e != w] == []
    st, back, _ = decompress_batch(hc, torch, encs, [len(r) for r in raws])
    assert st == [0] * len(raws)
    assert [i for i, (r, b) in enumerate(zip(raws, back)) if r != b] == []

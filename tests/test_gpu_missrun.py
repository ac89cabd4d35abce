"""GPU parity of the encoder's miss run (hc_fgk.hip code_all_batch, HC_ENC_MISS_RUN: behind the
symbol that ended a regular step and was coded alone, the symbols the step read as uncached are
coded alone too instead of starting a step that takes nothing; model: tests/fgk_missrun_model.py).
The bytes are the oracle's whether the library was built with the rule or without it (the shipping
build leaves it off: it measured slower); the states below are what the
encoder's steps meet either way.

The vectors (fgk_missrun_model.search: six streams of about 1500 symbols; tests/
test_missrun_model.py asserts on the CPU what their steps hold): runs of 2 and 3 uncached symbols
behind steps that took 0 and 1 symbols, a run of 15 (behind a step that took nothing: more lanes
than that a step does not read), runs behind steps that took 13 and 14, runs that reach the step's
last read lane, runs cut by the end of the pass, runs with symbols not seen before (splits), runs
with a repeat that is cached by the time it is coded (A A, a two-byte run that MNP-5 codes as two
symbols, and A B A), runs during which the record lanes fill, runs behind a cached symbol whose
level was reported. Every vector also runs cut short, which moves the pass ends. One batch goes
through the shipping library and, in the debug build, with the step capped at 1, 7 and 16 symbols
(debug_set_enc_pack) in cache mode, in the wide layout and through the small-alphabet launch: the
encoded bytes equal the oracle's byte for byte and decode to the input."""
import pytest

from fgk_handoff_model import raw_of
from fgk_missrun_model import search
from gpu_batch import compress_batch, decompress_batch

pytestmark = pytest.mark.gpu

CUTS = (1.0, 0.83, 0.41)


@pytest.fixture(scope="module")
def batch(oracle_mod):
    chosen, _ = search()
    raws = [raw_of(syms[:int(len(syms) * cut)]) for _, syms in chosen for cut in CUTS]
    assert len(raws) <= 64 and max(map(len, raws)) <= 4096
    wants = []
    for r in raws:
        st, enc = oracle_mod.compress(r, True, False, 512)
        assert st == 0
        wants.append(enc)
    return raws, wants


@pytest.mark.parametrize("mode,cap", [("ship", 16), ("cache", 1), ("cache", 7), ("cache", 16),
                                      ("wide", 1), ("wide", 7), ("wide", 16), ("small", 7), ("small", 16)])
def test_missrun_batch_vs_oracle(gpu, hc, batch, mode, cap):
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

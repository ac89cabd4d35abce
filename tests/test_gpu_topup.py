"""GPU parity of the decoder's batch steps on a window of 64 true bits (hc_fgk.hip HC_DEC_TOPUP 1:
BitSource::peek ORs the next unread word below the window's valid bits before a step, and
BitSource::take_peeked refills once when the step used bits of it; model: tests/fgk_topup_model.py).
The streams are those of tests/test_gpu_pack.py, with and without the diff model; the model passes
through every edge of the window's bookkeeping on them (a step that takes exactly the valid bits,
one bit more, nearly the whole peeked word; a refill at negative nwin that rolls the chunk over;
the payload's last word peeked and used: tests/test_topup_model.py
test_gpu_streams_reach_every_window_edge), so no further stream is added. The oracle's encodings
are decoded with the cap forced to 1, 7 and 16 codes (16: the build's HC_DEC_PACK, the most a step
takes) in the regular, wide, small-alphabet and rate-chosen launches and across window edges;
damaged streams end with the oracle's status. (The small-alphabet launch keeps the window's own bits,
HC_DEC_TOPUP_SMALL 0: forcing it for every narrow stream checks that path on the same streams.)
The streams, caps and launches are those of tests/test_gpu_pack.py, which this file repeats under
the names the window change was specified with; test_streams_are_the_models ties them to the model."""
import pytest

from gpu_batch import decompress_batch
from test_gpu_pack import _inputs, _restore
from test_topup_model import gpu_streams

CAPS = (1, 7, 16)


def test_streams_are_the_models(oracle_mod):
    """(no GPU needed) the streams decoded below are the ones the model was run on"""
    raws, _ = _inputs(oracle_mod)
    want = gpu_streams(oracle_mod)
    assert raws == [r for r, _ in want]
    assert [k < len(raws) // 2 for k in range(len(raws))] == [d for _, d in want]
    assert max(len(r) for r in raws) <= 65536


@pytest.mark.gpu
@pytest.mark.parametrize("launch", ["rate", "wide", "small", "regular"])
def test_full_window_decoder_vs_oracle(gpu, hc, oracle_mod, launch):
    torch = gpu
    raws, encs = _inputs(oracle_mod)
    hc.use_debug_build(True)
    try:
        if launch == "wide":
            hc.debug_set_min_tree(1)
        elif launch != "rate":
            hc.debug_set_dec_small(1 if launch == "small" else 2)
        for cap in CAPS:
            hc.debug_set_dec_pack(cap)
            st, back, _ = decompress_batch(hc, torch, encs, [len(r) for r in raws])
            assert st == [0] * len(raws), cap
            assert [i for i, (r, b) in enumerate(zip(raws, back)) if r != b] == [], cap
    finally:
        _restore(hc)


@pytest.mark.gpu
def test_full_window_decoder_window_edges(gpu, hc, oracle_mod):
    torch = gpu
    raws, encs = _inputs(oracle_mod)
    hc.use_debug_build(True)
    try:
        hc.debug_set_window(4096)
        st, back, _ = decompress_batch(hc, torch, encs, [len(r) for r in raws])
        assert st == [0] * len(raws)
        assert [i for i, (r, b) in enumerate(zip(raws, back)) if r != b] == []
    finally:
        _restore(hc)


@pytest.mark.gpu
def test_full_window_decoder_damaged_streams(gpu, hc, oracle_mod):
    """the eight truncated and eight byte-flipped streams of
    test_gpu_pack.test_packed_decoder_damaged_streams at every cap: every status the oracle's
    (transform.cpp:394-398; a truncated stream's peeked words past its end read as zeros, like
    its refills), status-0 outputs the oracle's; capacities leave no room to run past a buffer"""
    torch = gpu
    raws, encs = _inputs(oracle_mod)
    raws, encs = raws[:8], encs[:8]
    bad = []
    for k, e in enumerate(encs):
        bad.append(e[: len(e) // 2])
        b = bytearray(e)
        b[9 + (k * 131) % (len(e) - 9)] ^= 0x5A
        bad.append(bytes(b))
    wants = [oracle_mod.decompress(blob) for blob in bad]
    caps = [len(w[1]) if w[0] == 0 else 2 * len(raws[j // 2]) + 1024 for j, w in enumerate(wants)]
    res = {}
    hc.use_debug_build(True)
    try:
        for cap in CAPS:
            hc.debug_set_dec_pack(cap)
            res[cap] = decompress_batch(hc, torch, bad, caps)
    finally:
        _restore(hc)
    for cap, (st, back, _) in res.items():
        for j, want in enumerate(wants):
            assert st[j] == want[0], (cap, j)
            if want[0] == 0:
                assert back[j] == want[1], (cap, j)

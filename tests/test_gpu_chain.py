"""GPU parity of the packed batch step with the strided chain of code starts (hc_fgk.hip
Dec::decode_batch, HC_DEC_CHAIN: the depth map composed with itself, the serial chain over every
second or fourth start, the starts in between filled in lane-parallel; model:
tests/fgk_chain_model.py). The streams are those of tests/test_gpu_pack.py and two more for the
chain's edges (tests/test_chain_model.py gpu_streams: 6-bit codes, and 1-bit codes with longer ones
among them), with and without the diff model; test_chain_model.test_gpu_streams_reach_every_chain_edge
runs the model over them and finds every edge the change was specified with. The oracle's encodings
are decoded by the shipped step with the cap forced to 1, 7 and 16 codes in the regular, wide,
small-alphabet and rate-chosen launches and across window edges; truncated and byte-flipped streams
end with the oracle's status."""
import pytest

from gpu_batch import decompress_batch
from test_chain_model import gpu_streams
from test_gpu_pack import _inputs, _restore

CAPS = (1, 7, 16)
_cache = {}


def _streams(oracle_mod):
    """(raws, encodings by the oracle), computed once; the encodings test_gpu_pack has made are taken
    from it"""
    if not _cache:
        have = {}
        praws, pencs = _inputs(oracle_mod)
        for k, (r, e) in enumerate(zip(praws, pencs)):
            have[(r, k < len(praws) // 2)] = e
        raws, encs = [], []
        for r, diff in gpu_streams(oracle_mod):
            e = have.get((r, diff))
            if e is None:
                st, e = oracle_mod.compress(r, diff, False, 512)
                assert st == 0
            raws.append(r)
            encs.append(e)
        assert max(len(r) for r in raws) <= 65536 and len(raws) <= 64
        _cache["v"] = (raws, encs)
    return _cache["v"]


def test_streams_are_the_models(oracle_mod):
    """(no GPU needed) the streams decoded below are the ones the model was run on, test_gpu_pack's
    among them"""
    raws, encs = _streams(oracle_mod)
    assert raws == [r for r, _ in gpu_streams(oracle_mod)]
    praws, pencs = _inputs(oracle_mod)
    assert set(praws) <= set(raws) and set(pencs) <= set(encs)
    assert len(raws) == len(praws) + 4


@pytest.mark.gpu
@pytest.mark.parametrize("launch", ["rate", "wide", "small", "regular"])
def test_strided_chain_decoder_vs_oracle(gpu, hc, oracle_mod, launch):
    torch = gpu
    raws, encs = _streams(oracle_mod)
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
def test_strided_chain_decoder_shipped_build(gpu, hc, oracle_mod):
    """the shipping library (no debug hooks: its own instantiations of the step)"""
    torch = gpu
    raws, encs = _streams(oracle_mod)
    st, back, _ = decompress_batch(hc, torch, encs, [len(r) for r in raws])
    assert st == [0] * len(raws)
    assert [i for i, (r, b) in enumerate(zip(raws, back)) if r != b] == []


@pytest.mark.gpu
def test_strided_chain_decoder_window_edges(gpu, hc, oracle_mod):
    torch = gpu
    raws, encs = _streams(oracle_mod)
    hc.use_debug_build(True)
    try:
        hc.debug_set_window(4096)
        for cap in CAPS:
            hc.debug_set_dec_pack(cap)
            st, back, _ = decompress_batch(hc, torch, encs, [len(r) for r in raws])
            assert st == [0] * len(raws), cap
            assert [i for i, (r, b) in enumerate(zip(raws, back)) if r != b] == [], cap
    finally:
        _restore(hc)


@pytest.mark.gpu
def test_strided_chain_decoder_damaged_streams(gpu, hc, oracle_mod):
    """every third stream truncated to half (its peeked bits past the end read as zeros) and with one
    flipped payload byte, at every cap: every status the oracle's (transform.cpp:394-398), status-0
    outputs the oracle's; capacities leave no room to run past a buffer"""
    torch = gpu
    raws, encs = _streams(oracle_mod)
    raws, encs = raws[::3], encs[::3]
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

"""GPU parity of the decoder's packed batch step (hc_fgk.hip Dec::decode_batch: one lane per code
bit, up to 16 codes per step; model: tests/fgk_pack_model.py, checked against the one-symbol loop
in tests/test_pack_model.py). The oracle's encodings (transform.cpp:363-384, huffman.cpp:95-217) of
streams whose codes are short (the 16-code cap binds), deep (codes cross the tables' 8 bits),
tied, or end inside a step are decoded with the cap forced to 1, 7 and 16 codes, in the narrow and
wide layouts, by the regular and the small-alphabet launch and across window edges; damaged
streams end with the oracle's status."""
import numpy as np
import pytest

from gpu_batch import decompress_batch
from test_batch_model import _small_streams, _streams
from test_pack_model import extra_streams

pytestmark = pytest.mark.gpu

_cache = {}


def _inputs(oracle_mod):
    """(raws, encodings by the oracle), computed once: every stream with and without the diff model"""
    if not _cache:
        raws = _streams(oracle_mod) + _small_streams() + extra_streams()
        raws.append(oracle_mod.synth("photo", 3, 256, 256).tobytes())
        raws.append(bytes((7 * k * k + k // 3) & 255 for k in range(300)))  # a block of 256 symbols ends inside a step
        assert max(len(r) for r in raws) <= 65536
        raws = raws + raws
        encs = []
        for k, r in enumerate(raws):
            st, e = oracle_mod.compress(r, k < len(raws) // 2, False, 512)
            assert st == 0
            encs.append(e)
        _cache["v"] = (raws, encs)
    return _cache["v"]


def _restore(hc):
    hc.debug_set_dec_pack(16)
    hc.debug_set_dec_small(0)
    hc.debug_set_min_tree(0)
    hc.debug_set_window(1 << 30)
    hc.use_debug_build(False)


@pytest.mark.parametrize("launch", ["rate", "wide", "small", "regular"])
def test_packed_decoder_vs_oracle(gpu, hc, oracle_mod, launch):
    torch = gpu
    raws, encs = _inputs(oracle_mod)
    hc.use_debug_build(True)
    try:
        if launch == "wide":
            hc.debug_set_min_tree(1)
        elif launch != "rate":
            hc.debug_set_dec_small(1 if launch == "small" else 2)
        for cap in (1, 7, 16):
            hc.debug_set_dec_pack(cap)
            st, back, _ = decompress_batch(hc, torch, encs, [len(r) for r in raws])
            assert st == [0] * len(raws), cap
            assert [i for i, (r, b) in enumerate(zip(raws, back)) if r != b] == [], cap
    finally:
        _restore(hc)


def test_packed_decoder_window_edges(gpu, hc, oracle_mod):
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


def test_packed_decoder_damaged_streams(gpu, hc, oracle_mod):
    """the first eight streams truncated to half and with one flipped payload byte: every status the
    oracle's (transform.cpp:394-398), status-0 outputs the oracle's; capacities leave no room to
    run past a buffer"""
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
        for cap in (1, 7, 16):
            hc.debug_set_dec_pack(cap)
            res[cap] = decompress_batch(hc, torch, bad, caps)
    finally:
        _restore(hc)
    for cap, (st, back, _) in res.items():
        for j, want in enumerate(wants):
            assert st[j] == want[0], (cap, j)
            if want[0] == 0:
                assert back[j] == want[1], (cap, j)

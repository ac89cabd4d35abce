"""The packed decoder step and the encoder's two layouts chosen by hysteresis
(tests/fgk_pack_model.py; hc_fgk.hip Dec::decode_batch, code_all_batch) leave the tree of the
one-symbol loop -- the encoder its codes too -- and never pass a symbol that the exact leader test
(fgk_batch_model.batch_len) fails: the model asserts that at every step."""
import numpy as np
import pytest

from fgk_batch_model import decode, encode
from fgk_pack_model import PACK_MAX, decode_packed, encode_hyst
from test_batch_model import _small_streams, _streams


def extra_streams():
    """a 0.9 / 0.1 two-symbol stream (1-bit codes: the 16-code cap binds) and a 1.1-Zipf stream
    over 256 symbols (depths cross 6, and 8, often)"""
    rng = np.random.default_rng(29)
    two = rng.choice(np.array([17, 200], np.uint8), 8000, p=[0.9, 0.1]).tobytes()
    zipf = 1.0 / np.arange(1, 257) ** 1.1
    z = rng.choice(rng.permutation(256), 12000, p=zipf / zipf.sum()).astype(np.uint8).tobytes()
    return [two, z]


_ref = {}


def _cases(oracle_mod):
    """(symbols, the one-symbol loop's codes and tree) per stream, computed once"""
    if not _ref:
        out = []
        for syms in _streams(oracle_mod) + _small_streams() + extra_streams():
            syms = list(syms)
            c, t, _ = encode(syms, batched=False)
            out.append((syms, c, t))
        _ref["v"] = out
    return _ref["v"]


def _same_tree(t1, t2):
    return t1.w == t2.w and t1.body == t2.body and t1.up == t2.up


@pytest.mark.parametrize("cap,window", [(PACK_MAX, True), (12, True), (7, True), (1, True), (PACK_MAX, False)])
def test_packed_decoder_equals_one_symbol_loop(oracle_mod, cap, window):
    total = {"steps": 0, "n": 0}
    for k, (syms, _, t1) in enumerate(_cases(oracle_mod)):
        t2, st = decode_packed(syms, cap=cap, window=window)
        assert _same_tree(t1, t2), k
        assert st["alone"] + st["sent"] <= len(syms) and st["steps"] <= len(syms)
        total["steps"] += st["steps"]
        total["n"] += len(syms)
    assert cap == 1 or total["steps"] < total["n"]


@pytest.mark.parametrize("bits", [8, 5])
def test_packed_decoder_exit_gate_leaves_the_tree_alone(oracle_mod, bits):
    """the first-code gate (the kernel's HC_DEC_EXIT_BITS, 7 by default) only chooses which path
    decodes a symbol: the nine-lane layout's 8 and a low 5 leave the same tree"""
    for k, (syms, _, t1) in enumerate(_cases(oracle_mod)):
        t2, _ = decode_packed(syms, exit_bits=bits)
        assert _same_tree(t1, t2), k


def test_cap_binds_on_one_bit_codes(oracle_mod):
    """the two-symbol stream: steps end at the 16-code cap (the others at a tie of its few
    positions, which fails the tentative test), none takes more"""
    syms = list(extra_streams()[0])
    _, st = decode_packed(syms)
    assert st["capped"] > 0
    assert len(syms) <= PACK_MAX * st["steps"] + st["alone"] + st["sent"]


def test_packed_decoder_takes_fewer_steps_on_a_photo(oracle_mod):
    """photo -c -m, where the nine-lane layout stopped at its seven-symbol cap in most steps: at
    least a fifth fewer steps (the bar the kernel work was started on)"""
    raw = oracle_mod.synth("photo", 0, 256, 256).tobytes()
    syms = list(oracle_mod.rle(oracle_mod.diff(raw)))
    t0, s0 = decode(syms, batched=True)
    t1, s1 = decode_packed(syms, cap=7, window=False, exit8=False)
    t2, s2 = decode_packed(syms)
    assert _same_tree(t0, t1) and _same_tree(t0, t2)
    assert s2["steps"] + s2["sent"] <= 0.8 * (s1["steps"] + s1["sent"])


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_encoder_hysteresis_equals_one_symbol_loop(oracle_mod, layout):
    shallow = 0
    for k, (syms, c1, t1) in enumerate(_cases(oracle_mod)):
        c2, t2, st = encode_hyst(syms, layout)
        assert c1 == c2, k
        assert _same_tree(t1, t2), k
        shallow += st["shallow"]
    assert (shallow == 0) == (layout == 1)

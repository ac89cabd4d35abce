"""The case table of tests/adapt_big_cases.py checks itself against the oracle alone, so the
GPU test built on it (tests/test_gpu_adapt_big.py) cannot quietly lose its sensitivity: every
case's winner is the declared one of 256 / 512 / 1024, the runner-up is as close as declared (a
cost off by that many bytes flips the winner), both scan directions occur among the winner's
blocks, and the pinned matrices sit exactly 1 byte and exactly 0 bytes apart (first minimum).
Reference: transform.cpp:294-328 (applyAdaptRLE), restated by candidate_totals from oracle.rle.
"""
import pytest

import adapt_big_cases as C


def _oracle_winner(oracle_mod, name):
    m = C.pattern(name)
    st, stream, B = oracle_mod.adapt(m.tobytes(), m.shape[1], m.shape[0])
    assert st == 0 and int.from_bytes(stream[16:24], "big") == B
    return B, len(stream)


@pytest.mark.parametrize("name", list(C.TABLE))
def test_table_row(oracle_mod, name):
    """the oracle's winner, the runner-up's distance and the h / all block counts are the
    table's (the longruns' distance is background: it is printed, not asserted)"""
    _, win, ru, behind, nh, nb = C.TABLE[name]
    t = C.totals(name)
    got_win, got_ru, got_behind = C.winner(t)
    B, n = _oracle_winner(oracle_mod, name)
    print(f"{name}: winner {got_win}, runner-up {got_ru} {got_behind} bytes behind, "
          f"blocks h/all {t[got_win][2]}/{t[got_win][1]}")
    assert B == win == got_win and n == t[win][0]
    assert (t[win][2], t[win][1]) == (nh, nb)
    assert got_ru == ru
    if name not in C.LONGRUNS:
        assert got_behind == behind


def test_table_keeps_its_sensitivity(oracle_mod):
    assert {v[1] for v in C.TABLE.values()} == {256, 512, 1024}  # (test_table_row: the oracle's)
    rows = {k: (v[1], C.winner(C.totals(k))[2], C.totals(k)[v[1]]) for k, v in C.TABLE.items()
            if k not in C.LONGRUNS}  # the close calls and mixed directions are the quilts' part
    for B in (512, 1024):  # a runner-up at most 64 bytes behind, twice
        assert sum(1 for w, d, _ in rows.values() if w == B and d <= 64) >= 2, B
    for B in (256, 512, 1024):  # both directions among the winner's blocks
        assert any(w == B and 0 < t[2] < t[1] for w, _, t in rows.values()), B


@pytest.mark.parametrize("name", list(C.PINS))
def test_pins(oracle_mod, name):
    _, (a, b), gap, win = C.PINS[name]
    t = C.totals(name)
    assert t[b][0] - t[a][0] == gap
    assert all(t[B][0] > t[a][0] for B in t if B not in (a, b))
    assert C.winner(t)[0] == win
    assert _oracle_winner(oracle_mod, name) == (win, t[win][0])


def test_pin_pairs():
    """each pair: exactly 1 byte, then exactly 0 bytes, between the same two sizes"""
    for big, small in ((1024, 512), (512, 256)):
        pair = sorted((v[2], v[3]) for v in C.PINS.values() if v[1] == (big, small))
        assert pair == [(0, small), (1, big)]


def test_uniform_batch_winners(oracle_mod):
    """the six 1025 x 513 matrices of the uniform batch have different winners, 256 and 512 and
    one below 256 among them (emit_big_kernel codes some and skips the others)"""
    wins = [_oracle_winner(oracle_mod, k)[0] for k in C.UNIFORM]
    assert all(C.pattern(k).shape == (513, 1025) for k in C.UNIFORM)
    assert {256, 512} <= set(wins) and min(wins) < 256, wins

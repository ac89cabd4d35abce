"""The packed decoder step on a window of 64 true bits (tests/fgk_topup_model.py; hc_fgk.hip
Dec::decode_batch with HC_DEC_TOPUP 1) leaves the one-symbol loop's tree after every step, reads
exactly the code lengths' sum of bits through the kernel's window bookkeeping (nwin negative after
a step that used the peeked word, one refill, the chunk rollover inside it), and takes the step
counts the change was started on. The streams of tests/test_gpu_topup.py reach every edge of the
bookkeeping in the model, so the GPU test runs them."""
import pytest

from fgk_topup_model import EVENTS, bench_streams, decode_topup
from test_batch_model import _small_streams, _streams
from test_pack_model import extra_streams

# photo streams 0-3, first 60000 symbols, cap 16: (steps, symbols alone) with 63 bits at every step,
# and the steps of the window's own bits they are measured against (at least 8 % fewer)
PHOTO_STEPS = [(5994, 3475), (6157, 3776), (5551, 2897), (5572, 3036)]
PHOTO_STEPS_20 = [(5667, 3696), (5814, 4016), (5189, 3093), (5267, 3250)]

_cache = {}


def gpu_streams(oracle_mod):
    """(raw, diff model) of tests/test_gpu_topup.py: the streams of tests/test_gpu_pack.py, every
    one with and without the diff model. No further stream is needed: the search (every stream
    below, through decode_topup at cap 16) finds each event of EVENTS, see
    test_gpu_streams_reach_every_window_edge."""
    raws = _streams(oracle_mod) + _small_streams() + extra_streams()
    raws.append(oracle_mod.synth("photo", 3, 256, 256).tobytes())
    raws.append(bytes((7 * k * k + k // 3) & 255 for k in range(300)))
    return [(r, True) for r in raws] + [(r, False) for r in raws]


def _bench(oracle_mod):
    if "b" not in _cache:
        _cache["b"] = bench_streams(oracle_mod)
    return _cache["b"]


@pytest.mark.parametrize("cap", [16, 20])
def test_full_window_in_lockstep_with_one_symbol_update(oracle_mod, cap):
    """photo 0-3, grad and noise: the same tree as the one-symbol update after every step and
    every symbol decoded alone, and the bits read are the code lengths' sum (both asserted inside
    the model); photo takes the step counts of the estimate, grad and noise the shipped window's"""
    want = PHOTO_STEPS if cap == 16 else PHOTO_STEPS_20
    for k, (name, syms) in enumerate(_bench(oracle_mod)):
        _, st, _ = decode_topup(syms, cap=cap, lockstep=True)
        print(name, cap, st)
        if k < 4:
            assert (st["steps"], st["alone"]) == want[k], name
        elif cap == 16:
            _, st0, _ = decode_topup(syms, cap=cap, topup=False)
            assert (st["steps"], st["alone"]) == (st0["steps"], st0["alone"]), name


def test_full_window_takes_fewer_steps_than_the_windows_own_bits(oracle_mod):
    for k, (name, syms) in enumerate(_bench(oracle_mod)[:4]):
        t0, st0, _ = decode_topup(syms, topup=False, lockstep=True)
        t1, st1, _ = decode_topup(syms)
        assert t0.w == t1.w and t0.body == t1.body and t0.up == t1.up
        assert st0["sj_eq_n0"] == st0["neg_refill_rolls_chunk"] == 0
        assert st1["steps"] <= 0.92 * st0["steps"], name
        assert st1["capped"] > st0["capped"] and st1["ended_window"] < st0["ended_window"], name


def test_gpu_streams_reach_every_window_edge(oracle_mod):
    """every stream of the GPU test through the model, its length from the oracle's encoding: the
    bits read fill the payload to its last byte, and among them the steps take sj = n0, sj = n0 + 1
    and sj >= n0 + 24 bits, refill at negative nwin from word 63 of a chunk, and peek -- and use --
    the payload's last word"""
    seen = {e: 0 for e in EVENTS}
    for k, (raw, diff) in enumerate(gpu_streams(oracle_mod)):
        syms = list(oracle_mod.rle(oracle_mod.diff(raw)) if diff else oracle_mod.rle(raw))
        st, enc = oracle_mod.compress(raw, diff, False, 512)
        assert st == 0
        _, ev, win = decode_topup(syms, last_word=(len(enc) - 1) // 4)
        assert 9 + (win.consumed() + 7) // 8 == len(enc), k
        for e in EVENTS:
            seen[e] += ev[e]
    print(seen)
    assert all(seen[e] > 0 for e in EVENTS), seen

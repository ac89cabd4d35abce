"""GPU parity of the adaptive encoder where the block sizes 256, 512 and 1024 win: the sizes
whose costs big_cost_kernel joins from tile_cost_kernel's pieces and whose blocks
emit_big_kernel codes one wave per block, and whose streams unblock_kernel scatters on decode.

The inputs are the self-checking table of tests/adapt_big_cases.py (tests/test_adapt_big_cases.py
holds it to the oracle): winners 256 / 512 / 1024 with the runner-up 3 .. 22 bytes behind, pinned
matrices 1 byte and 0 bytes apart (first minimum), edge blocks and tile pieces 1 element wide or
high, widths that are no multiple of 8 or 128, runs around the multiples of 258 in both scans.
Byte equality with the oracle's stream is the bar, and every stream decodes back to its input.
Reference: transform.cpp:294-361, main.cpp:39-128.
"""
import pytest

import adapt_big_cases as C
from gpu_batch import compress_adapt_batch, decompress_adapt_batch

pytestmark = pytest.mark.gpu

_want = {}


def _oracle_stream(oracle_mod, name, use_diff):
    """(raw, width, the oracle's -c -a [-m] stream), computed once per case"""
    key = (name, use_diff)
    if key not in _want:
        raw, W = C.raw_input(name, use_diff)
        st, want = oracle_mod.compress(raw, use_diff, True, W)
        assert st == 0
        _want[key] = (raw, W, want)
    return _want[key]


def _block_size(oracle_mod, name):
    m = C.pattern(name)
    st, stream, B = oracle_mod.adapt(m.tobytes(), m.shape[1], m.shape[0])
    assert st == 0 and int.from_bytes(stream[16:24], "big") == B
    return B


def _run(hc, torch, oracle_mod, names, use_diff, extra=()):
    """one encode call and one decode call over the named cases, `extra` (raw, width, want
    status) inputs interleaved one after every case until they run out"""
    items, extra = [], list(extra)
    for name in names:
        raw, W, want = _oracle_stream(oracle_mod, name, use_diff)
        items.append((name, raw, W, 0, want))
        if extra:
            raw, W, st = extra.pop(0)
            want = oracle_mod.compress(raw, use_diff, True, W)[1] if st == 0 else b""
            items.append((f"extra {len(raw)} bytes, width {W}", raw, W, st, want))
    assert not extra
    st, enc, _ = compress_adapt_batch(hc, torch, [it[1] for it in items], [it[2] for it in items], use_diff)
    for i, (name, raw, W, want_st, want) in enumerate(items):
        assert st[i] == want_st, (name, st[i], want_st)
        if want_st == 0:
            assert enc[i] == want, f"{name} (stream {i}): GPU adaptive stream differs from the oracle"
    ok = [i for i, it in enumerate(items) if it[3] == 0]
    dst, dec, _ = decompress_adapt_batch(hc, torch, [enc[i] for i in ok], [len(items[i][1]) for i in ok])
    assert dst == [0] * len(ok)
    for j, i in enumerate(ok):
        assert dec[j] == items[i][1], f"{items[i][0]} (stream {i}): round trip differs"


@pytest.mark.parametrize("use_diff", [False, True])
def test_adapt_big_mixed_batch(gpu, hc, oracle_mod, use_diff):
    """every table and pin case in one call, interleaved with matrices that have no candidate
    >= 256 (64 x 200 noise, 8 x 8) and the reference's error inputs (width 0 -> 4, size not a
    multiple of the width -> 6, a side < 8 -> 12): the streams' item counts differ and repeat,
    so find_item takes its binary search"""
    names = list(C.TABLE) + list(C.PINS)
    won = {_block_size(oracle_mod, k) for k in names}
    assert {256, 512, 1024} <= won
    extra = [(oracle_mod.synth("noise", 2, 64, 200).tobytes(), 64, 0),
             (b"\x01" * 64, 0, 4),
             (oracle_mod.synth("photo", 6, 8, 8).tobytes(), 8, 0),
             (b"\x02" * 70, 8, 6),
             (b"\x03" * 80, 16, 12)]
    assert [oracle_mod.compress(r, use_diff, True, w)[0] for r, w, st in extra if w] == [0, 0, 6, 12]
    _run(hc, gpu, oracle_mod, names, use_diff, extra)


@pytest.mark.parametrize("use_diff", [False, True])
def test_adapt_big_uniform_batch(gpu, hc, oracle_mod, use_diff):
    """six 1025 x 513 matrices with different winners in one call: every stream has the same
    item counts, so find_item divides; emit_big_kernel codes the winner's blocks, skips the
    other candidates' items and skips the photo (winner < 256) entirely"""
    wins = [_block_size(oracle_mod, k) for k in C.UNIFORM]
    assert {256, 512} <= set(wins) and min(wins) < 256, wins
    _run(hc, gpu, oracle_mod, C.UNIFORM, use_diff)


@pytest.mark.parametrize("use_diff", [False, True])
@pytest.mark.parametrize("name", ["quilt-1032x1025-q1024", "pin-1024-ties-512"])
def test_adapt_big_single_buffer(gpu, hc, oracle_mod, name, use_diff):
    """hc_compress / hc_decompress (a batch of one: the n = 1 launch geometry) on a 1024 winner
    with edge blocks 8 wide and 1 high, and on the exact 512 / 1024 tie"""
    raw, W, want = _oracle_stream(oracle_mod, name, use_diff)
    st, enc = hc.compress(raw, use_diff, True, W)
    assert st == 0 and enc == want, f"{name}: GPU adaptive stream differs from the oracle"
    st, back = hc.decompress(enc)
    assert st == 0 and back == raw

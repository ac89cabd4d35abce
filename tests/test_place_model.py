"""The placement helper of the GPU placement tests (tests/gpu_place.py), checked on the CPU: the
layout takes every residue 0, 4, 8, 12 with exact slot sizes and gaps of 0..15 bytes, and
outside_untouched sees one flipped byte anywhere outside the slots. The oracle pins the truncation
cases test_gpu_place.py decodes with a live tail: a stream cut by 1..8 bytes ends with status 9
(transform.cpp:394-398), a prefix under 9 bytes with 8 (main.cpp:99-104)."""
import numpy as np
import pytest

import gpu_place as gp

SIZES = [0, 1, 3, 4, 5, 15, 16, 17, 63, 1353, 16, 0, 12, 64]


@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_layout_residues_and_gaps(rot):
    base_res = 4 * ((rot + 1) % 4)
    offs, total = gp.layout(SIZES, rot, base_res)
    assert [o % 16 for o in offs] == [4 * ((i + rot) % 4) for i in range(len(SIZES))]
    assert {o % 16 for o in offs} == {0, 4, 8, 12}
    assert {(o + base_res) % 16 for o in offs} == {0, 4, 8, 12}  # the addresses the library sees
    assert all(o % 4 == 0 for o in offs)
    ends = [o + n for o, n in zip(offs, SIZES)]
    gaps = [b - a for a, b in zip(ends, offs[1:])]
    assert all(0 <= g <= 15 for g in gaps)  # in order, disjoint, never further than the next residue
    assert min(gaps) == 0 and max(gaps) >= 8
    assert offs[0] >= gp.MARGIN and ends[-1] + gp.MARGIN <= total


def test_layout_bytes_any_residue():
    sizes = list(range(40))
    res = [(7 * i + 3) % 16 for i in range(40)]
    offs, total = gp.layout_bytes(sizes, res)
    assert [o % 16 for o in offs] == res and set(res) == set(range(16))
    assert all(a + n <= b for a, n, b in zip(offs, sizes, offs[1:]))


def test_overlap_is_refused():
    gp.check_disjoint([64, 72, 72, 80], [8, 0, 8, 1])
    with pytest.raises(AssertionError):
        gp.check_disjoint([64, 71], [8, 8])
    with pytest.raises(AssertionError):
        gp.check_disjoint([80, 64], [4, 17])


@pytest.mark.parametrize("poison", [0xA5, "random"])
@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_outside_untouched_sees_one_byte(rot, poison):
    if poison == "random":
        poison = np.random.default_rng(7).integers(0, 256, size=1 << 14, dtype=np.uint8)
    base_res = 4 * ((rot + 1) % 4)
    blobs = [bytes([i + 1]) * n for i, n in enumerate(SIZES)]
    buf, offs, lens = gp.place(None, blobs, SIZES, rot, base_res, poison)
    assert lens == SIZES and gp.slots(buf, offs, lens) == blobs
    assert gp.outside_untouched(buf, offs, SIZES, poison)
    ends = [o + n for o, n in zip(offs, SIZES)]
    gaps = [(e, o) for e, o in zip(ends, offs[1:]) if o > e]
    # in gaps (right behind a slot, right before one), before the first slot (also before the
    # view), after the last slot (also the allocation's last byte)
    spots = [gaps[0][0], gaps[-1][1] - 1, gaps[len(gaps) // 2][0], offs[0] - 1, 0, -base_res, ends[-1], buf.size - 1]
    for at in spots:
        whole, start = gp._whole(buf)
        whole[start + at] ^= 0x40
        assert not gp.outside_untouched(buf, offs, SIZES, poison), at
        assert gp.touched(buf, offs, SIZES, poison) == [start + at]
        whole[start + at] ^= 0x40
    assert gp.outside_untouched(buf, offs, SIZES, poison)
    # a byte inside a slot is the slot's own business
    buf[offs[9] + 5] ^= 0x40
    assert gp.outside_untouched(buf, offs, SIZES, poison)


def test_guarded_work():
    whole, view = gp.guarded_work(None, 1000)
    assert whole.size == 16 + 1000 + 4096 and view.size == 1000
    assert view.ctypes.data - whole.ctypes.data == 16
    view[:] = 0
    assert gp.work_guard_untouched(whole, 1000)
    for at in (15, 1016, whole.size - 1):
        whole[at] = 0
        assert not gp.work_guard_untouched(whole, 1000)
        whole[at] = 0xA5


def test_oracle_pins_truncation(oracle_mod):
    streams = gp.trunc_streams(oracle_mod)
    assert len(streams) == 6
    assert [len(e) for name, _, e in streams if name == "grad 64x48 -m"] == [63]
    for name, raw, enc in streams:
        assert oracle_mod.decompress(enc) == (0, raw), name
        for k in gp.TRUNC_CUTS:
            assert oracle_mod.decompress(enc[:-k]) == (9, b""), (name, k)
        assert [oracle_mod.decompress(enc[:n]) for n in gp.TRUNC_PREFIXES] == [(8, b"")] * 3 + [(9, b"")], name

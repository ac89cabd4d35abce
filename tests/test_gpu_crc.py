"""hc_crc32_batch on the GPU against zlib.crc32: every length class of the kernel (one lane per
range up to 64 bytes, one wavefront above: head bytes, aligned 16-byte pieces in tiles of 64,
tail bytes) at every start alignment, and more ranges than one launch has lanes or wavefronts."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = list(range(18)) + [63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537, 2**20 + 3]
# one tile of a wavefront is 1024 bytes: a full one, one piece more and less, with and without head and tail
LENGTHS += [1023, 1024, 1025, 1040, 2047, 2048, 2049]
GUARD = 0x5A5A5A5A


def _run(hc, torch, data, offs, lens, guard=8):
    """-> the crc words of the ranges, with `guard` words on either side checked untouched"""
    n = len(offs)
    d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda() if len(data) else \
        torch.zeros(16, dtype=torch.uint8, device="cuda")
    o = torch.tensor(offs, dtype=torch.int64, device="cuda")
    m = torch.tensor(lens, dtype=torch.int64, device="cuda")
    crc = torch.full((n + 2 * guard,), GUARD, dtype=torch.int32, device="cuda")
    hc.crc32_batch(d, o, m, crc[guard:guard + n])
    torch.cuda.synchronize()
    got = crc.cpu().numpy().view(np.uint32)
    assert (got[:guard] == GUARD).all() and (got[guard + n:] == GUARD).all()
    return got[guard:guard + n].tolist()


def _want(data, offs, lens):
    view = memoryview(data)
    return [zlib.crc32(view[o:o + m]) for o, m in zip(offs, lens)]


@pytest.mark.parametrize("fill", ["random", "zeros", "ones"])
def test_lengths_and_alignments(hc, gpu, fill):
    size = 16 + max(LENGTHS) + 16
    if fill == "random":
        data = np.random.default_rng(7).integers(0, 256, size, dtype=np.uint8).tobytes()
    else:
        # equal bytes: only the init term tells zeros of different lengths apart
        data = (b"\x00" if fill == "zeros" else b"\xff") * size
    offs = [a for n in LENGTHS for a in range(16)]
    lens = [n for n in LENGTHS for a in range(16)]
    got = _run(hc, gpu, data, offs, lens)
    want = _want(data, offs, lens)
    bad = [(o, m) for o, m, g, w in zip(offs, lens, got, want) if g != w]
    assert not bad, bad[:8]
    if fill == "zeros":
        assert len(set(want)) == len(LENGTHS)  # the lengths are told apart


def test_many_short_ranges(hc, gpu):
    """70000 ranges of 0 to 40 bytes, anywhere in the buffer, in one call"""
    rng = np.random.default_rng(8)
    data = rng.integers(0, 256, 1 << 16, dtype=np.uint8).tobytes()
    lens = rng.integers(0, 41, 70000).tolist()
    offs = rng.integers(0, (1 << 16) - 40, 70000).tolist()
    assert _run(hc, gpu, data, offs, lens) == _want(data, offs, lens)


def test_more_ranges_than_lanes(hc, gpu):
    """300000 ranges of 0 to 200 bytes: both kinds of range, each more than one launch takes at once"""
    rng = np.random.default_rng(9)
    data = rng.integers(0, 256, 1 << 16, dtype=np.uint8).tobytes()
    lens = rng.integers(0, 201, 300000).tolist()
    offs = rng.integers(0, (1 << 16) - 200, 300000).tolist()
    assert sum(m > 64 for m in lens) > 100000 and sum(m <= 64 for m in lens) > 80000
    assert _run(hc, gpu, data, offs, lens) == _want(data, offs, lens)


def test_no_ranges(hc, gpu):
    assert _run(hc, gpu, b"abc" * 16, [], []) == []
    assert hc.lib().hc_crc32_batch(None, None, None, 0, None, None) == 0


def test_ranges_may_overlap_and_repeat(hc, gpu):
    data = b"123456789" * 20
    assert _run(hc, gpu, data, [0, 0, 9, 0, 3], [9, 9, 9, 180, 100]) == [0xCBF43926] * 3 + [
        zlib.crc32(data), zlib.crc32(data[3:103])]

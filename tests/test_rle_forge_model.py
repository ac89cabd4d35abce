"""CPU checks of the forged MNP-5 symbol streams of tests/rle_forge_model.py: the oracle decodes
every container to the RLE (and diff) revert of its symbols, every family reaches the cases it
was built for (a census by the serial machine of rle_forge_model.blocks, so a vector set that
misses its case fails here and not silently on the GPU), and the reference binary, when built,
agrees exit code for exit code and byte for byte. The GPU side is tests/test_gpu_rle_forge.py.
"""
import pytest

import rle_forge_model as rf


def _family(name):
    return [(n, s) for n, s in rf.vectors() if rf.family(n) == name]


def test_vectors_vs_oracle(oracle_mod, capsys):
    cases = rf.containers(oracle_mod)
    assert len(cases) == 2 * len(rf.vectors())
    for name, data in cases:
        sym = rf.symbols_of(name)
        assert data[:9] == len(sym).to_bytes(8, "little") + bytes([int(name[-2:], 16)])
        st, got = oracle_mod.decompress(data)
        want = oracle_mod.unrle(sym)
        if data[8] & 0x80:
            want = oracle_mod.undiff(want)
        assert st == 0 and got == want, name
        assert got == rf.expand(sym, bool(data[8] & 0x80)), name
    with capsys.disabled():
        per = {f: len(_family(f)) for f in rf.FAMILIES}
        print(f"\n[rle forge] symbol streams per family {per}, {len(cases)} containers, "
              f"{sum(len(d) for _, d in cases)} bytes in, "
              f"{sum(len(rf.expand(s, False)) for _, s in rf.vectors()) * 2} bytes out")


def test_align_census():
    """one non-trivial run per stream; every (run start mod 16, count) pair, and all 256 run bytes
    at the three cross points"""
    seen, cross = set(), {pc: set() for pc in rf.ALIGN_CROSS}
    steps = set()
    for name, sym in _family("align"):
        blk = rf.blocks(sym)
        assert len(blk) == 1 and blk[0]["state"] == 0 and len(blk[0]["runs"]) == 1, name
        off, n, v = blk[0]["runs"][0]
        assert blk[0]["out"] == len(sym) - 1 + n and rf.final_state(sym) in (1, 2), name
        seen.add((off % 16, n))
        if "cross" in name:
            cross[(off - 3, n)].add(v)
        else:
            steps.add(v)
    assert seen >= {(r, c) for r in range(16) for c in rf.ALIGN_COUNTS}
    assert all(vs == set(range(256)) for vs in cross.values())
    assert steps == set(rf.STEPS)


def test_density_census():
    """every listed number of non-empty runs in one block, with zero counts between them wherever
    there are fewer than the block's count symbols; the count at each byte of its lane; short and
    long runs in one group of 16; a block of 16512 bytes"""
    reached, at_byte, biggest = {}, set(), 0
    mixed_group = False
    for name, sym in _family("density"):
        blk = rf.blocks(sym)
        assert 2 <= len(blk) <= 3, name
        for b in blk:
            assert len(set(b["lanes"])) == len(b["lanes"])  # one count a lane at most
            live = [r for r in b["runs"] if r[1]]
            reached.setdefault(len(live), set()).add(len(b["runs"]) - len(live))
            at_byte |= {i % 4 for i in b["counts"]}
            biggest = max(biggest, b["out"])
            for g in range(0, len(live), 16):
                lens = [n for _, n, _ in live[g:g + 16]]
                mixed_group |= min(lens) == 1 and max(lens) == 255
    for runs in rf.DENSITY_RUNS:
        assert runs in reached, runs
        assert runs == 64 or max(reached[runs]) >= 63 - runs, (runs, reached[runs])  # skipped lanes
    assert at_byte == {0, 1, 2, 3}
    assert mixed_group
    assert biggest == 64 * (3 + 255) == 16512
    # 64 runs in one block with the count at every byte of the lane
    full = {b["counts"][0] % 4 for _, sym in _family("density") for b in rf.blocks(sym)
            if sum(1 for r in b["runs"] if r[1]) == 64}
    assert full == {0, 1, 2, 3}


def test_carry_census():
    """each state 0..3 crosses a block boundary (the first and the second), a count is the first
    symbol of a block, streams end in state 3 at a block end and mid-block, the exact lengths"""
    carried = {1: set(), 2: set()}
    first_count, end3, lengths = set(), set(), set()
    for name, sym in _family("carry"):
        blk = rf.blocks(sym)
        lengths.add(len(sym))
        for k in (1, 2):
            if len(blk) > k:
                carried[k].add(blk[k]["state"])
                if blk[k]["counts"][:1] == [0]:
                    first_count.add((k, blk[k]["runs"][0][1]))
        if rf.final_state(sym) == 3:
            end3.add(len(sym) % 256 == 0)
    assert carried[1] == {0, 1, 2, 3} and carried[2] == {0, 1, 2, 3}
    assert first_count >= {(k, c) for k in (1, 2) for c in rf.CARRY_COUNTS}
    assert end3 == {False, True}
    assert lengths >= set(rf.EXACT_LENGTHS) | set(range(250, 266))
    # the second boundary lies behind a block that ends in a run
    for name, sym in _family("carry"):
        if name.startswith("carry/edge512"):
            off, n, v = rf.blocks(sym)[0]["runs"][-1]
            assert (n, v) == (200, 7) and off + n == rf.blocks(sym)[0]["out"], name
    # all nines: the count's value, the run byte and the literal behind it are equal
    sym = dict(_family("carry"))["carry/nines260"]
    assert [r[1:] for b in rf.blocks(sym) for r in b["runs"]] == [(9, 9)] * (260 // 4)


def test_random_census():
    fam = _family("random")
    assert 190 <= len(fam) <= 210
    assert {len(set(s)) for _, s in fam if len(s) > 900} >= {2, 3, 5, 256}
    assert sum(len(s) > 4900 for _, s in fam) == 6 and min(len(s) for _, s in fam) < 20
    assert any(set(s) == {0, 255} for _, s in fam) and any(set(s) == {0, 1, 255} for _, s in fam)
    assert max(len(b["runs"]) for _, s in fam for b in rf.blocks(s)) >= 30


def reference_subset(oracle_mod):
    """the carry family and 16 containers of each other family, spread over it"""
    cases = rf.containers(oracle_mod)
    pick = [c for c in cases if rf.family(c[0]) == "carry"]
    for f in ("align", "density", "random"):
        fam = [c for c in cases if rf.family(c[0]) == f]
        pick += [fam[(2 * i * len(fam)) // 32 + (i & 1)] for i in range(16)]  # both flags
    return pick


def test_vectors_vs_reference(oracle_mod, tmp_path):
    """the reference binary decodes the hand-built containers as the oracle does"""
    if not oracle_mod.ref_available():
        pytest.skip("reference binary not built (oracle/_ref)")
    o2 = oracle_mod.ref_available(o2=True)
    cases = reference_subset(oracle_mod)
    assert len({n for n, _ in cases}) == len(cases)
    for name, data in cases:
        rc, out, _ = oracle_mod.run_ref(["-d"], data, str(tmp_path), o2=o2, timeout=120)
        st, mine = oracle_mod.decompress(data)
        assert rc == st == 0, (name, rc, st)
        assert out == mine, name

"""CPU checks of the forged streams of tests/fgk_forge_model.py (NYT escapes that name a known
symbol): every vector holds what it was built for, the oracle's two tree forms decode each one to
its symbols (huffman.cpp:95-128: no split for a symbol that has a leaf), the reference binary, when
built, agrees byte for byte and exit code for exit code, and the cuts inside an escape end with
status 9 or decode, as the oracle says. The GPU side is tests/test_gpu_forge.py.
"""
import pytest

import fgk_forge_model as fm
from fgk_cache_model import ROOT


def _info(sym, esc):
    info = []
    bits = fm.forge(sym, esc, info)
    return bits, info


def _by_name():
    return {name: (sym, esc) for name, sym, esc in fm.vectors()}


def test_every_vector_reaches_the_path():
    for name, sym, esc in fm.vectors():
        assert len(sym) <= fm.MAX_SYMBOLS
        bits, info = _info(sym, esc)
        payload = fm.pack_bits(bits)
        got, known, whole = fm.decode(payload, len(sym))
        assert whole and got == list(sym), name
        assert known == len(info) == fm.count_known_escapes(payload, len(sym)), name
        assert (known > 0) == (name != "second-control"), name
        assert fm.container(sym, esc, 0x80) == fm.wrap(len(sym), 0x80, bits)


def test_second_symbol_vectors():
    v = _by_name()
    bits, info = _info(*v["second"])
    assert bits == [0, 1, 0, 0, 0, 0, 0, 1] + [0] + [0, 1, 0, 0, 0, 0, 0, 1]  # 8 raw bits, then 0 + 8 bits
    assert info == [(1, ROOT - 2, 1, 1)]
    assert _info(*v["second-control"])[0] == [0, 1, 0, 0, 0, 0, 0, 1] + [1]
    for k in fm.SECOND_AT:
        sym, esc = v["first@%d" % k]
        _, info = _info(sym, esc)
        # the first known escape is symbol k, behind k - 1 new ones: the NYT stands 2 (k - 1) below
        # the root and stays there (17: at kSmallNyt exactly)
        assert info[0][:2] == (k - 1, ROOT - 2 * (k - 1))
        assert len(set(sym[:k - 1])) == k - 1 and sym[k - 1] in sym[:k - 1]
        assert len(set(sym)) > k - 1 and len(info) > 3  # new symbols and more escapes behind it
    assert ROOT - 2 * (17 - 1) == fm.SMALL_NYT


def test_small_alphabet_vectors():
    v = _by_name()
    for name in ("small4", "small-grow"):
        sym, esc = v[name]
        bits, info = _info(sym, esc)
        assert len(sym) == 3000
        assert len(bits) * 2 < len(sym) * 5, name  # the rate rule picks the small-alphabet launch
        assert 0.03 * len(sym) < len(info) < 0.07 * len(sym), name
    assert len(set(v["small4"][0])) == 4
    sym, esc = v["small-grow"]
    assert len(set(sym)) > 16 and len(set(sym[:1500])) == 4
    _, info = _info(sym, esc)
    # escapes while the NYT is above kSmallNyt (the small decoder's range) and after it left it
    assert sum(nyt >= fm.SMALL_NYT for _, nyt, _, _ in info) > 50
    assert sum(nyt < fm.SMALL_NYT for _, nyt, _, _ in info) > 5


def test_noise_skewed_and_full_vectors():
    v = _by_name()
    sym, esc = v["noise"]
    _, info = _info(sym, esc)
    assert len(sym) == 3000 and len(set(sym)) == 256 and 100 < len(info) < 200
    assert sum(d > 8 for _, _, d, _ in info) > 20  # deep codes
    for name in ("skewed", "skewed15"):
        sym, esc = v[name]
        _, info = _info(sym, esc)
        hot = sorted(set(sym), key=sym.count)[-3:]
        assert sum(sym[i] in hot and d <= 3 for i, _, d, _ in info) > 40, name   # the cached, shallow part
        assert sum(d > 8 for _, _, d, _ in info) >= 3, name                       # deep -> walk after chase(known)
    sym, esc = v["full"]
    _, info = _info(sym, esc)
    assert sorted(sym[:256]) == list(range(256)) and len(sym) == 256 + 1500
    assert len(info) > 100 and all(nyt == 0 for _, nyt, _, _ in info)  # find_leaf runs with p > 0


def test_run_and_phase_vectors():
    v = _by_name()
    for name, syms in (("run-same", 1), ("run-alt", 2), ("run-rare", 1)):
        sym, esc = v[name]
        _, info = _info(sym, esc)
        at = [i for i, _, _, _ in info]
        assert len(at) == 64 and at == list(range(at[0], at[0] + 64)), name
        assert len({sym[i] for i in at}) == syms, name
    # the escapes of the phase set start at every bit offset mod 64, and so do their raw bits
    starts, raws = set(), set()
    base = None
    for pre in range(fm.PHASES):
        sym, esc = v["phase%d" % pre]
        assert len(set(sym[:pre])) <= 1 and (base is None or sym[pre:] == base)
        base = sym[pre:]
        for i, _, _, nyt_len in _info(sym, esc)[1]:
            start = len(fm.forge(sym[:i], esc[:i])) if pre in (0, 63) else None
            if start is not None:
                starts.add((72 + start) % 64)
                raws.add((72 + start + nyt_len) % 64)
    assert len(starts) > 48 and len(raws) > 48
    # each phase shifts the tail by one bit more (the first common symbol costs 8 bits, the rest 1)
    lens = [len(_info(*v["phase%d" % pre])[0]) for pre in range(fm.PHASES)]
    assert len({(n - lens[0]) % 64 for n in lens}) > 32


def test_mnp5_vectors():
    v = _by_name()
    for name, roles in (("mnp5-third", {"third"}), ("mnp5-count", {"count"}), ("mnp5-both", {"third", "count", "lit"})):
        sym, esc = v[name]
        role = fm.mnp5_roles(sym)
        _, info = _info(sym, esc)
        seen = {role[i] for i, _, _, _ in info}
        assert seen == roles, (name, seen)
        assert len(info) > 50
        if "third" in roles:  # a count follows the escaped symbol
            assert all(role[i + 1] == "count" for i, _, _, _ in info if role[i] == "third" and i + 1 < len(sym))


def test_forged_streams_vs_oracle(oracle_mod):
    for name, sym, esc in fm.vectors():
        payload = fm.pack_bits(fm.forge(sym, esc))
        for slot in (False, True):
            st, got = oracle_mod.fgk_decode(payload, len(sym), slot_form=slot)
            assert st == 0 and got == bytes(sym), (name, slot)
    for name, data in fm.forged_containers():
        sym = _by_name()[name.split("/")[0]][0]
        st, got = oracle_mod.decompress(data)
        want = oracle_mod.unrle(bytes(sym))
        assert st == 0 and got == (oracle_mod.undiff(want) if data[8] & 0x80 else want), name


def test_truncations_vs_oracle(oracle_mod):
    seen = {0: 0, 9: 0}
    cuts = fm.truncated_containers()
    assert len(cuts) == 10 * (len(fm.vectors()) - 1)  # (the control has no escape to cut)
    for name, data in cuts:
        count = int.from_bytes(data[:8], "little")
        st, got = oracle_mod.decompress(data)
        assert st in (0, 9), name
        seen[st] += 1
        sym, _, whole = fm.decode(data[9:], count)
        assert whole == (st == 0), name
        for slot in (False, True):
            st2, got2 = oracle_mod.fgk_decode(data[9:], count, slot_form=slot)
            assert st2 == st and (st or got2 == bytes(sym)), (name, slot)
        if st == 0:
            assert got == oracle_mod.unrle(bytes(sym)), name
    assert seen[0] > 50 and seen[9] > 300, seen


def test_forged_streams_vs_reference(oracle_mod, tmp_path):
    """the reference binary accepts the forged streams: its exit code and bytes are the oracle's"""
    if not oracle_mod.ref_available():
        pytest.skip("reference binary not built (oracle/_ref)")
    o2 = oracle_mod.ref_available(o2=True)
    cases = fm.forged_containers() + [c for c in fm.truncated_containers() if not c[0].startswith("phase") or
                                      c[0].split(":")[0] in ("phase0", "phase21", "phase42", "phase63")]
    for name, data in cases:
        rc, out, _ = oracle_mod.run_ref(["-d"], data, str(tmp_path), o2=o2, timeout=120)
        st, mine = oracle_mod.decompress(data)
        assert rc == st, (name, rc, st)
        if rc == 0:
            assert out == mine, name


def fuzz_census(oracle_mod):
    """(mutants of tests/test_fuzz.py with at least one known-symbol escape, mutants, escapes in all)"""
    from test_fuzz import _mutants
    hit = total = 0
    cases = _mutants(oracle_mod)
    for _, data in cases:
        if len(data) < 9:
            continue
        n = fm.count_known_escapes(data[9:], int.from_bytes(data[:8], "little"))
        hit += n > 0
        total += n
    return hit, len(cases), total


def test_fuzz_census(oracle_mod, capsys):
    """a measurement, not a bound: how often the seeded fuzz set reaches the known-symbol escape
    (the figure in tests/test_gpu_forge.py's docstring)"""
    hit, cases, total = fuzz_census(oracle_mod)
    with capsys.disabled():
        print(f"\n[fuzz census] {hit} of {cases} mutants hold a known-symbol escape ({total} escapes in all)")
    assert cases == 480

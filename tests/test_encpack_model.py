"""The encoder's batch step packed by path depth (tests/fgk_encpack_model.py; hc_fgk.hip
code_all_batch, HC_ENC_PACK): up to 16 cached symbols a step, each on as many lanes as its path has
positions, while the depths sum to at most 63. Codes and the final tree are the one-symbol loop's
-- on photo streams 0-3 (the first 60000 MNP-5 symbols of each 512x512 -c -m stream), a grad and a
noise stream and every candidate stream of fgk_handoff_model.candidates() -- the step count on the
photo streams is at most 0.70 of the 7 x 9 layout's, and the streams the GPU test encodes
(tests/test_gpu_encpack.py) end a step in every state it lists."""
import pytest

from fgk_batch_model import encode as encode_loop
from fgk_encpack_model import CROSS, PACK, encode_packed, search
from fgk_handoff_model import candidates as handoff_candidates
from fgk_handoff_model import raw_of, same_tree
from fgk_pack_model import encode_hyst

# States of the list in tests/test_gpu_encpack.py that no searched stream ends a step in: none.
# (The issue asks for a reported level at some level of every step symbol j = 0..15, not at every
# level: the (j, l) pairs reached are those of test_handoff_model.py for j <= 6 and thin out behind
# them, as a report at a deep level needs every level below it to pass by the step's counts.)
UNREACHED = set()


@pytest.fixture(scope="module")
def found():
    return search()


def _mnp5(oracle_mod, kind, k, w=512, h=512):
    raw = oracle_mod.synth(kind, k, w, h).tobytes()
    return list(oracle_mod.rle(oracle_mod.diff(raw)))


@pytest.mark.parametrize("kind,k", [("photo", 0), ("photo", 1), ("photo", 2), ("photo", 3), ("grad", 0), ("noise", 0)])
def test_packed_equals_one_symbol_loop(oracle_mod, kind, k):
    syms = _mnp5(oracle_mod, kind, k, *((512, 512) if kind == "photo" else (256, 128)))[:60000]
    codes, tree, st = encode_packed(syms, lockstep=True)  # asserts the code and the tree at every symbol
    c0, t0, _ = encode_loop(syms, batched=False)
    assert codes == c0 and same_tree(tree, t0)
    assert st["taken",] + st["alone",] == len(syms)
    if kind == "photo":
        # the 7 x 9 layout's steps on the same symbols (fgk_pack_model.encode_hyst, deep layout only)
        c7, t7, s7 = encode_hyst(syms, 1)
        assert c7 == codes and same_tree(t7, tree)
        ratio = st["steps",] / s7["steps"]
        print(f"photo {k}: 7 x 9 {s7['steps']} steps, packed {st['steps',]} ({ratio:.3f}), "
              f"alone {s7['alone']} -> {st['alone',]}")
        assert ratio <= 0.70
        for cap in (1, 7, 12):  # the debug hook's caps and the A/B's
            cc, tc, sc = encode_packed(syms[:20000], cap=cap)
            assert cc == codes[:20000] and sc["steps",] >= st["steps",] * 20000 // len(syms)


def test_handoff_candidates_in_lockstep():
    for name, syms in handoff_candidates():
        codes, tree, st = encode_packed(syms, lockstep=True)
        assert len(codes) == len(syms), name


def test_packed_whatever_the_pass_length(oracle_mod):
    syms = _mnp5(oracle_mod, "photo", 5, 160, 120)
    c0, t0, _ = encode_loop(syms, batched=False)
    for chunk in (256, 61, 7, 1 << 20):
        c1, t1, _ = encode_packed(syms, chunk=chunk)
        assert c1 == c0 and same_tree(t1, t0), chunk


def test_searched_streams_in_lockstep(oracle_mod, found):
    chosen, _ = found
    for name, syms in chosen:
        if name.startswith("cross"):  # (the other families: test_handoff_candidates_in_lockstep)
            encode_packed(syms, lockstep=True)
        # no runs: the symbols the kernel codes are the stream's, a 256-byte chunk per pass
        assert oracle_mod.rle(oracle_mod.diff(raw_of(syms))) == bytes(syms), name


def test_searched_streams_cover_every_step_end(found):
    chosen, st = found
    assert len(chosen) <= 64
    assert all(len(syms) <= 16384 for _, syms in chosen)
    want = {("full",), ("end63",), ("deep_first",), ("deep_last",), ("fill64",)}
    want |= {("cross", s, d) for s, d in CROSS}
    want |= {(kind, j) for kind in ("miss", "fresh") for j in range(PACK)}
    want |= {("short", kind) for kind in ("miss", "fresh", "level")}
    missing = {k for k in want if st[k] == 0}
    # a reported level at some level of step symbol j, a falsely reported one among them
    missing |= {("level", j) for j in range(PACK) if not any(st["level", j, l] for l in range(9))}
    assert missing == UNREACHED
    false = sum(v for key, v in st.items() if key[0] == "false")
    assert 0 < false < sum(v for key, v in st.items() if key[0] == "level")
    assert {key[1] for key in st if key[0] == "false"} == set(range(PACK))

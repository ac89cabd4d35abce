"""The encoder's batch step with its hand-offs (tests/fgk_handoff_model.py; hc_fgk.hip
code_all_batch, HC_ENC_HANDOFF_MISS / HC_ENC_HANDOFF_LEVEL): a cached symbol whose level reported
keeps the increments of its levels below the report and walks from the reported level with the
step's row as the known path (built behind HC_ENC_HANDOFF_LEVEL, off in the shipped kernel, whose
step is the model's handoff=False). In lockstep with the plain Tree.update the code about to be sent and
the whole tree are identical at every symbol -- on photo streams 0-3 (the first 60000 MNP-5
symbols of each 512x512 -c -m stream), a grad and a noise stream, falsely reported levels among
them -- and the streams the GPU test encodes end a step in every state it lists."""
import pytest

from fgk_handoff_model import encode, raw_of, same_tree, search

# (step symbol j, level l) pairs no candidate stream of fgk_handoff_model.candidates() ends a step
# at: a report at a level that deep needs the eight or nine levels below it to pass by the step's
# counts while the level itself comes within them of its next position, which the searched families
# produce only behind a heavier symbol of the same step (so never at j = 0), and ever more rarely
# the later the symbol stands in its step
UNREACHED = {(0, 6), (0, 7), (0, 8), (2, 8), (3, 8), (4, 7), (4, 8), (5, 7), (5, 8), (6, 7), (6, 8)}


@pytest.fixture(scope="module")
def found():
    return search()


def _mnp5(oracle_mod, kind, k, w=512, h=512):
    raw = oracle_mod.synth(kind, k, w, h).tobytes()
    return list(oracle_mod.rle(oracle_mod.diff(raw)))


@pytest.mark.parametrize("kind,k", [("photo", 0), ("photo", 1), ("photo", 2), ("photo", 3), ("grad", 0), ("noise", 0)])
def test_handoff_in_lockstep_with_plain_update(oracle_mod, kind, k):
    syms = _mnp5(oracle_mod, kind, k, *((512, 512) if kind == "photo" else (256, 128)))[:60000]
    codes, tree, st = encode(syms)  # asserts the code and the tree at every symbol
    assert len(codes) == len(syms) and st["alone",] > 0
    if k == 0:  # ... and so does the shipped step (the level hand-off off)
        assert encode(syms, handoff=False)[0] == codes
    if kind == "photo":
        # steps end at reported levels, some of them false: the walk's exact test decides
        levels = sum(v for key, v in st.items() if key[0] == "level")
        false = sum(v for key, v in st.items() if key[0] == "false")
        assert 0 < false < levels
        assert all(st["miss", j] > 0 for j in range(7))


def test_handoff_equals_parent_step(oracle_mod):
    """the same codes and the same tree as the step that takes every increment of the failing
    symbol back and tests all its levels again, whatever the pass length"""
    syms = _mnp5(oracle_mod, "photo", 5, 160, 120)
    for chunk in (256, 61, 7, 1 << 20):
        c1, t1, _ = encode(syms, chunk=chunk, lockstep=False)
        c0, t0, _ = encode(syms, chunk=chunk, handoff=False, lockstep=False)
        assert c1 == c0 and same_tree(t1, t0), chunk


def test_searched_streams_in_lockstep(oracle_mod, found):
    chosen, _ = found
    for name, syms in chosen:
        encode(syms)
        # no runs: the symbols the kernel codes are the stream's, a 256-byte chunk per pass
        assert oracle_mod.rle(oracle_mod.diff(raw_of(syms))) == bytes(syms), name


def test_searched_streams_cover_every_step_end(found):
    chosen, st = found
    assert len(chosen) <= 64
    assert all(len(syms) <= 16384 for _, syms in chosen)
    for j in range(7):
        assert st["miss", j] > 0 and st["fresh", j] > 0, j
    missing = {(j, l) for j in range(7) for l in range(9) if st["level", j, l] == 0}
    assert missing == UNREACHED
    assert any(key[0] == "false" for key in st)
    # a falsely reported level at every depth reached, and true reports too
    assert {key[2] for key in st if key[0] == "false"} >= set(range(8))
    assert sum(v for key, v in st.items() if key[0] == "false") < sum(v for key, v in st.items() if key[0] == "level")
    assert st["fill64",] > 0  # the hand-off's record in lane 63: pack follows
    assert all(st["short", kind] > 0 for kind in ("miss", "fresh", "level"))

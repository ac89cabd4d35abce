"""CPU checks of the miss-run model (tests/fgk_missrun_model.py, the model of HC_ENC_MISS_RUN in
hc_fgk.hip's code_all_batch): with the rule off it is fgk_encpack_model.encode_packed step for step;
with runs capped at 1 and uncapped, in lockstep with the plain Tree.update, every code and the tree
after every symbol are the one-symbol loop's -- on the photo streams and on the vectors of
tests/test_gpu_missrun.py, whose coverage is asserted here. Steps, empty steps and the symbols coded
in runs go to profiles/r12_missrun_model.txt."""
import os

import pytest

import fgk_missrun_model as R
from fgk_encpack_model import encode_packed

HERE = os.path.dirname(os.path.abspath(__file__))
REPORT = os.path.join(os.path.dirname(HERE), "profiles", "r12_missrun_model.txt")


def _symbols(oracle_mod, kind, k):
    return list(oracle_mod.rle(oracle_mod.diff(oracle_mod.synth(kind, k, 512, 512).tobytes())))[:60000]


@pytest.fixture(scope="module")
def report():
    lines = {}
    yield lines
    if len(lines) < 4:
        return  # a partial run leaves the recorded file alone
    head = ("Batch steps of the path-cache encoder (fgk_missrun_model.encode_missrun) without the miss run, with runs of at\n"
            "most one symbol and with runs of up to 15 (HC_ENC_MISS_RUN_MAX as shipped): steps / steps that took nothing /\n"
            "symbols coded alone (of them in a run). First 60 k symbols of each stream. Written by tests/test_missrun_model.py.\n\n")
    try:
        with open(REPORT, "w") as f:
            f.write(head + "\n".join(lines[k] for k in sorted(lines)) + "\n")
    except OSError:
        pass  # a read-only checkout


@pytest.mark.parametrize("kind,k", [("photo", 0), ("photo", 1), ("photo", 2), ("photo", 3)])
def test_streams_lockstep(oracle_mod, report, kind, k):
    syms = _symbols(oracle_mod, kind, k)
    codes0, _, base = encode_packed(syms)
    res = {}
    for rc in (0, 1, R.RUN_MAX):
        codes, _, st = R.encode_missrun(syms, run_cap=rc, lockstep=(rc != 0))
        assert codes == codes0
        res[rc] = st
    off, one, full = res[0], res[1], res[R.RUN_MAX]
    # off: the packed step as it was
    assert [off[key,] for key in ("steps", "empty", "alone", "taken")] == [base[key,] for key in ("steps", "empty", "alone", "taken")]
    assert off["direct",] == 0
    report["%s%d" % (kind, k)] = "%-8s" % ("%s %d" % (kind, k)) + "   ".join(
        "%s %5d / %4d / %5d (%4d)" % (name, st["steps",], st["empty",], st["alone",], st["direct",])
        for name, st in (("off", off), ("run <= 1", one), ("run <= 15", full)))
    # every run symbol saves the step that would have taken nothing, or (cached by then: a repeat)
    # leaves a step one symbol shorter: steps fall by at least the fall of the empty ones
    for st in (one, full):
        assert off["steps",] - st["steps",] >= off["empty",] - st["empty",] > 0
        repeats = sum(v for key, v in st.items() if key[0] == "run_repeat")
        assert st["alone",] - off["alone",] <= repeats
    assert full["steps",] <= one["steps",] and full["empty",] <= one["empty",]
    # the issue's figure: runs of one symbol take away more than a third of the empty steps
    assert one["empty",] < 0.67 * off["empty",]


def test_vectors_lockstep_and_coverage(oracle_mod):
    from fgk_handoff_model import raw_of
    chosen, states = R.search()
    assert 1 <= len(chosen) <= 64 and all(len(s) <= 4096 for _, s in chosen)
    for name, syms in chosen:
        assert list(oracle_mod.rle(oracle_mod.diff(raw_of(syms)))) == syms, name
        want = encode_packed(syms)[0]
        for cap in (1, 7, 16):
            for rc in (1, R.RUN_MAX):
                assert R.encode_missrun(syms, run_cap=rc, cap=cap, lockstep=True)[0] == want, (name, cap, rc)
    s16, s7, s1 = states[16], states[7], states[1]
    runs = lambda s: {(k[1], k[2]) for k in s if k[0] == "run"}
    # runs of 2 and 3 behind steps that took 0 and 1 symbols, a run of 15 (behind a step that took
    # nothing: its 16 lanes hold the symbol coded alone and the run), and the longest runs there
    # are lanes for behind steps that took 13 and 14
    assert {(2, 0), (2, 1), (3, 0), (3, 1), (15, 0), (2, 13), (1, 14)} <= runs(s16)
    assert {(2, 0), (3, 1), (6, 0), (1, 5)} <= runs(s7)  # a step of at most 7: runs end at its cap
    assert not runs(s1)                                  # a step of one symbol reads no further lane
    assert s16["run_last",] and s16["run_pass",] and s7["run_pass",]
    assert s16["run_fresh",] and s7["run_fresh",]
    assert s16["run_repeat", 1] and s16["run_repeat", 2]  # A A and A B A, the repeat cached by then
    assert s16["run_fill",]
    assert s16["run_level",]  # a run behind a cached symbol whose level was reported

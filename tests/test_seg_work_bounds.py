"""Every public work bound of the segmented container (hc_seg_compress_work_bound{,2},
hc_seg_decompress_work_bound, hc_seg_decompress_range_work_bound, hc_seg_*_batch_work_bound,
hc_seg_update_work_bound, hc_seg_append_work_bound, and the output bounds of the last two) returns
what it returned at the commit named in tests/golden/seg_work_bounds.json: callers size their
workspaces by these, and the single and batch calls carve theirs with shared code. Host arithmetic,
no device."""
import json
import os

import seg_work_bound_cases


def test_work_bounds_are_the_recorded_ones(hc):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_work_bounds.json")) as f:
        want = json.load(f)["bounds"]
    table = seg_work_bound_cases.cases(hc)
    assert sorted(table) == sorted(want)
    got = {k: int(f()) for k, f in table.items()}
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} of {len(want)} bounds differ (got, recorded): {sorted(wrong.items())[:8]}"
    # the table reaches every kind of answer: workspaces, the rejected info's 16, invalid arguments' 0
    assert {0, 16} < set(want.values()) and sum(1 for v in want.values() if v > 16) > len(want) // 2

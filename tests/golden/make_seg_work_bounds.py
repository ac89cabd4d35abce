"""Record every public work bound of the segmented container over the table of
tests/seg_work_bound_cases.py into tests/golden/seg_work_bounds.json, from the library as built:

    python tests/golden/make_seg_work_bounds.py COMMIT

COMMIT names the commit the library was built from; it is stored beside the values. The bounds are
part of the API (callers size their workspaces by them), so a change of the glue must leave every
value as it is; tests/test_seg_work_bounds.py compares. Host arithmetic only: no device needed.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "huffman-codec_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hcodec  # noqa: E402
import seg_work_bound_cases  # noqa: E402


def main():
    bounds = {k: int(f()) for k, f in seg_work_bound_cases.cases(hcodec).items()}
    # as many entries to a line as fit into 118 columns
    lines, line = [], ""
    for k, v in bounds.items():
        e = f"{json.dumps(k)}: {v}, "
        if line and len(line) + len(e) > 118:
            lines.append(line.rstrip())
            line = ""
        line += e
    lines.append(line.rstrip(", "))
    with open(os.path.join(HERE, "seg_work_bounds.json"), "w") as f:
        f.write('{"commit": "%s", "bounds": {\n%s\n}}\n' % (sys.argv[1], "\n".join(lines)))
    print(len(bounds), "bounds,", sum(1 for v in bounds.values() if v > 16), "of them of a workspace")


if __name__ == "__main__":
    main()

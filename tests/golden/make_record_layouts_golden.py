"""Writes record_layouts.json: what tests/test_record_layout_host.py::recorded returns on ONE checkout of the package, the one
given on the command line — the commit before the packed records got their one description.  The record is the reference of
that test; it is made once and regenerated only when a layout or a message is changed on purpose.

    python tests/golden/make_record_layouts_golden.py path/to/checkout [out.json]      (no GPU, no built library needed)"""
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main(checkout, out=os.path.join(HERE, "record_layouts.json")):
    # the package comes from the checkout given, the cases from the test module beside this file
    sys.path[:0] = [os.path.abspath(checkout), os.path.dirname(HERE)]
    inference = importlib.import_module("esa_pose_estimation_amd.inference")
    pipeline = importlib.import_module("esa_pose_estimation_amd.pipeline")
    assert os.path.abspath(inference.__file__).startswith(os.path.abspath(checkout) + os.sep), inference.__file__
    import test_record_layout_host as T
    rec = T.recorded(inference, pipeline)
    missing = sorted(set(T.REFUSALS) - set(rec["refusals"]))
    if missing:
        raise SystemExit(f"not refused with a ValueError by this checkout: {missing}")
    with open(out, "w") as f:                 # one line per entry: a changed layout or message shows as one changed line
        parts = [f' "{part}": {{\n' + ",\n".join(f"  {json.dumps(key)}: {json.dumps(v)}" for key, v in entries.items()) + "\n }"
                 for part, entries in rec.items()]
        f.write("{\n" + ",\n".join(parts) + "\n}\n")
    print(f"{sum(len(v) for v in rec.values())} entries -> {out}")


if __name__ == "__main__":
    main(*sys.argv[1:3])

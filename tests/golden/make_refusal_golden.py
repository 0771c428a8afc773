"""Writes refusal_messages.json: the message each case of tests/test_refusal_ladder_host.py is refused with by ONE build of the
library, the one given on the command line — a build of the commit before the entries' bodies were shared.  The record is the
reference of that test; it is made once and regenerated only when a message is changed on purpose.

    python tests/golden/make_refusal_golden.py path/to/libesahrnet.so [out.json]      (needs a GPU: the cases behind the
                                                                                       commit check run on a committed handle)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import test_refusal_ladder_host as T  # noqa: E402


def main(lib_path, out=os.path.join(HERE, "refusal_messages.json")):
    from esa_pose_estimation_amd import _lib as L
    lib = L.load_other(lib_path)
    rec = {}
    h = T.uncommitted_handle(lib, L)
    for entry, case in T._cases(T.FRAMES_HOST, T.FRAMES):
        rec[f"{entry}/{case}"] = T.refuse_frames(lib, entry, T.host_base(h), T.FRAMES_HOST[case][0])
    lib.esahrnet_destroy(h)
    for entry, case in T._cases(T.ALONE_HOST, T.ALONE):
        rec[f"{entry}/{case}"] = T.refuse_alone(lib, entry, T.ALONE_HOST[case][0])
    import torch
    if torch.cuda.is_available():
        clib, base, need, _keep = T.committed_setup(lib_path)
        for entry, case in T._cases(T.FRAMES_COMMITTED, T.FRAMES):
            rec[f"{entry}/{case}"] = T.refuse_frames(clib, entry, dict(base, wsb=need[entry]), T.FRAMES_COMMITTED[case][0], need[entry])
    else:
        print("no GPU: the cases behind the commit check are left out, the record is INCOMPLETE")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} messages -> {out}")


if __name__ == "__main__":
    main(*sys.argv[1:3])

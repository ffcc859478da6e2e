"""The library entries of two TrainStep iterations on every host route of a training render of the shipped tri-plane geometry, as one table:
per entry its name, every scalar argument, "ptr" / "null" per pointer argument and the stream as an ordinal by first appearance
(tests/ray_grad_ref.py: _entry_record, TRAINING_CASES); per case the sha256 of the parameters afterwards where the route is reproducible, and
the number of torch.zeros / zeros_like calls train_utils and ops made during the backward.

    python tools/training_entry_table.py            # needs the GPU; writes tests/training_entry_table.json from THIS tree

tests/test_ray_grad.py replays the cases and compares them with the committed file.  The file is regenerated only by a change that means to
move a launch; a refactor of the host route must leave it as it is (it is recorded at the PARENT of such a change and committed unchanged)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "training_entry_table.json")


def table(pkg):
    import ray_grad_ref as R
    return {name: R.training_case(pkg, name) for name in R.TRAINING_CASES}


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import nvsr_amd

    nvsr_amd.capi.lib()                             # (raises if the library is not built)
    t = table(nvsr_amd)
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as fh:
        json.dump(t, fh, separators=(",", ":"))
        fh.write("\n")
    for name, case in t.items():
        print("%-40s %4d entries, streams %s, zeros %d, sha256 %s" % (name, len(case["entries"]), sorted({e[2] for e in case["entries"] if e[2] is not None}),
                                                                   case["zeros"], case["sha256"]))

"""What the executor does for a fixed list of small trees, one JSON line per tree: to compare two builds of the library.

    python tools/plan_fingerprint.py > new.jsonl;  SIGOPS_LIB=/path/to/other/libsigops.so python tools/plan_fingerprint.py > old.jsonl

Every tree is planned once and executed THREE times into the same result, so that where the plan is eligible the direct
launches, the graph capture and a replay all run.  A line holds the SHA-256 of the result's bytes after each execute, the
plan's steps as (name, algorithmic bytes, launches) and the launch / stage / scratch / byte counts of `stats()`.  Every
kernel's summation order is fixed by the frame index, so two builds that launch the same kernels with the same arguments
print the same lines.  The trees: every entry of tests/cases.py's CASES, then one per launch routine of csrc/executor.cpp
that those do not reach, built as the tests named beside them build theirs (tests/forms_corpus.py, which
tests/test_gpu_forms.py runs too and holds to the oracle).  Inputs are seeded.

`--ladders`: after those, one line in the same format per (case, rung) of that test's four ladders -- every form of the
resampler and of the IIR that csrc/stages.cpp chooses between -- sunk into a planar host result as the test sinks them.
"""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sigops_amd as so  # noqa: E402,F401
from forms_corpus import ResultView, corpus, ladders, rung_env  # noqa: E402  (the trees and the result views: shared with tests/test_gpu_forms.py)


def fingerprint(tree, **view):
    v = ResultView(tree, **view)
    plan = v.plan()
    try:
        hashes = []
        for _ in range(3):
            plan.execute(v.ptr, torch.cuda.current_stream().cuda_stream)
            plan.check(torch.cuda.current_stream().cuda_stream)
            hashes.append(hashlib.sha256(v.bytes()).hexdigest())
        st = plan.stats()
        return {"sha256": hashes, "steps": [(s["name"], s["algorithmic_bytes"], s["launches"]) for s in plan.steps()],
                "stats": {k: st[k] for k in ("n_launches", "n_stages", "scratch_bytes", "algorithmic_bytes")}, "executes": plan.counters()}
    finally:
        plan.close()


def main():
    for name, build, result, env in corpus():
        old = {k: os.environ.get(k) for k in env}
        os.environ.update({k: str(v) for k, v in env.items()})
        try:
            line = fingerprint(build(), **result)
        except Exception as e:  # (a tree the engine refuses is refused by both builds, in the same words)
            line = {"error": "%s: %s" % (type(e).__name__, e)}
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        print(json.dumps({"tree": name, **line}), flush=True)
    if "--ladders" in sys.argv[1:]:  # then every (case, rung) of test_gpu_forms.py's four ladders, the rung's switches set for the plan's creation
        for name, build, switches, kv in ladders():
            with rung_env(switches, kv):
                try:
                    line = fingerprint(build(), where="host")
                except Exception as e:
                    line = {"error": "%s: %s" % (type(e).__name__, e)}
            print(json.dumps({"tree": name, **line}), flush=True)


if __name__ == "__main__":
    main()

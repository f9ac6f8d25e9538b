#!/usr/bin/env python3
"""Record what the launcher and the runner do with every case of tests/launcher_cases.py:
    python tests/golden/make_launcher_matrix.py [path of the tree whose marl_amd is recorded; default: this one]
The tree needs its library built (the shape checks call its *_supported functions, which are host code).  The committed
tests/golden/launcher_matrix.json was written from the commit before main.py and runner.py were put on marl_amd/algorithms.py's table:
a worktree of that commit, built, and this script run on it give the same file.  Data only."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import launcher_cases as lc  # noqa: E402


def main():
    build = {lc.build_id(c): lc.eval_build(c) for c in lc.BUILD_CASES}
    with tempfile.TemporaryDirectory() as tmp:
        runner = {lc.runner_id(c): lc.eval_runner(c, tmp) for c in lc.RUNNER_CASES}
    data = {"build": lc.pack_build(build), "runner": lc.pack_runner(runner)}
    assert lc.unpack_build(data["build"]) == build and lc.unpack_runner(data["runner"]) == runner
    with open(lc.PATH, "w") as f:
        json.dump(data, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    raised = sum("raises" in o for o in build.values())
    print("%d build cases (%d raise), %d runner cases (%d distinct outcomes), %d bytes" % (
        len(build), raised, len(runner), len(data["runner"]["outcomes"]), os.path.getsize(lc.PATH)))


if __name__ == "__main__":
    main()

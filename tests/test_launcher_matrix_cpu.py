"""The launcher and the runner do with every case of tests/launcher_cases.py what tests/golden/launcher_matrix.json recorded (written by
tests/golden/make_launcher_matrix.py before main.py and runner.py were put on marl_amd/algorithms.py's table): the namespace field for
field, absent fields included; an exception's type and text; whether it came before or after the environment, the controller, the worker
and the buffer were made; which classes were built and in which order.  No GPU: the environments are stubs and every class the runner
builds records its name."""
import json

import pytest

import launcher_cases as lc


@pytest.fixture(scope="module")
def recorded():
    return lc.load()


def _text(x):
    return json.dumps(x, sort_keys=True)        # (as text: 1, 1.0 and True are three values)


def _differences(want, got):
    """per differing case the fields that moved: {id: {field: (recorded, now)}}"""
    bad = {}
    for k in want:
        if _text(want[k]) != _text(got[k]):
            w, g = ({f: _text(v) for f, v in dict(o, **o.get("args", {})).items() if f != "args"} for o in (want[k], got[k]))
            bad[k] = {f: (w.get(f, "<absent>"), g.get(f, "<absent>")) for f in sorted(set(w) | set(g)) if w.get(f) != g.get(f)}
    return bad


@pytest.mark.parametrize("name", lc.NAMES)
def test_build_does_what_it_did(name, recorded):
    cases = [c for c in lc.BUILD_CASES if c[0] == name]
    want = {lc.build_id(c): recorded[0][lc.build_id(c)] for c in cases}
    assert len(want) == len(lc.ENVS) * len(lc.MAPS) * len(lc.EXTRAS)
    bad = _differences(want, {lc.build_id(c): lc.eval_build(c) for c in cases})
    assert not bad, (len(bad), dict(list(bad.items())[:5]))


@pytest.mark.parametrize("name", lc.NAMES)
def test_runner_builds_what_it_built(name, recorded, tmp_path):
    cases = [c for c in lc.RUNNER_CASES if c[0] == name]
    want = {lc.runner_id(c): recorded[1][lc.runner_id(c)] for c in cases}
    assert len(want) == 2 * 2 ** len(lc.FLAGS)
    bad = _differences(want, {lc.runner_id(c): lc.eval_runner(c, str(tmp_path)) for c in cases})
    assert not bad, (len(bad), dict(list(bad.items())[:5]))

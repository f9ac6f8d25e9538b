"""TD(lambda) returns without a GPU: the numpy oracle against the fixture of the reference's build_td_lambda_targets
(tests/golden/make_td_lambda_golden.py), the closed forms at lambda 0 and 1, why the terminal flag is masked, the argument
parser and the C ABI's declaration of the kernel."""
import os
import re
import types

import numpy as np
import pytest

import td_lambda_oracle as tl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(golden_dir):
    return tl.load_cases(golden_dir)


def test_fixture_holds_every_case(cases):
    assert len(cases) == len(tl.SHAPES) * len(tl.LAMBDAS)
    for key, lam, (q, r, term, padded), G, G_lit in cases:
        B, T = q.shape
        assert key == tl.case_key(B, T) and G.shape == G_lit.shape == (B, T) and G.dtype == np.float64
        m = 1.0 - padded
        assert padded[0].sum() == 0 and term[0, T - 1] == 1 and (m * term)[0].sum() == 1      # full length, ends on the last step
        assert m[1].sum() == 1 and term[1, 0] == 1                                          # length 1
        assert padded[2].sum() == 0 and term[2].sum() == 0                                    # never terminates
        assert np.all(term[padded == 1] == 1)                                                 # padded steps carry term = 1
        if T > 1:
            assert np.abs(q[padded == 1]).min() >= tl.JUNK                                    # junk behind the episodes
            assert len({int(x) for x in m.sum(axis=1)}) >= min(3, T)                              # ragged


def test_oracle_reproduces_the_reference(cases):
    for key, lam, (q, r, term, padded), G, _ in cases:
        got = tl.returns(q, r, term, padded, tl.GAMMA, lam)
        assert np.abs(got - G).max() <= 1e-12 * max(1.0, np.abs(G).max()), (key, lam)


def test_lambda_zero_is_the_one_step_target(cases):
    for key, lam, (q, r, term, padded), G, _ in cases:
        if lam != 0.0:
            continue
        q, r, term, padded = (x.astype(np.float64) for x in (q, r, term, padded))
        ref = (1.0 - padded) * (r + tl.GAMMA * q * (1.0 - term))
        np.testing.assert_array_equal(tl.returns(q, r, term, padded, tl.GAMMA, 0.0), ref)
        assert np.abs(G - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def test_lambda_one_is_the_monte_carlo_return():
    """gamma = 1, integer rewards: plain suffix sums over the real steps, plus q[T-1] for the episode that never terminates"""
    for B, T in tl.SHAPES:
        q, r, term, padded = tl.make_case(B, T, seed=7)
        rng = np.random.default_rng(T)
        r = rng.integers(-3, 4, size=(B, T)).astype(np.float64)
        G = tl.returns(q, r, term, padded, 1.0, 1.0)
        m = 1.0 - padded
        suffix = np.cumsum((m * r)[:, ::-1], axis=1)[:, ::-1]
        boot = np.zeros((B, 1))
        boot[2, 0] = q[2, T - 1]
        np.testing.assert_array_equal(G, suffix + boot)


def test_one_step_window_is_the_one_step_target():
    q, r, term, padded = tl.make_case(7, 1, seed=3)
    for lam in tl.LAMBDAS:
        G = tl.returns(q, r, term, padded, tl.GAMMA, lam)
        ref = (1.0 - padded) * (r + tl.GAMMA * q.astype(np.float64) * (1.0 - term))
        assert np.abs(G - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def test_episodes_are_independent(cases):
    for key, lam, (q, r, term, padded), G, _ in cases:
        a = tl.returns(q[:3], r[:3], term[:3], padded[:3], tl.GAMMA, lam)
        b = tl.returns(q[3:], r[3:], term[3:], padded[3:], tl.GAMMA, lam)
        np.testing.assert_array_equal(np.concatenate([a, b]), tl.returns(q, r, term, padded, tl.GAMMA, lam))


def test_unmasked_terminal_flags_let_the_padding_in(cases):
    """why the flag is masked: with the batches' raw flags (1 on every padded step) the reference's 1 - sum(terminated) goes
    negative and the padded rows' values run back through the episode"""
    seen = 0
    for key, lam, (q, r, term, padded), G, G_lit in cases:
        if lam == 0.0 or q.shape[1] < 2:
            continue
        assert np.abs(G_lit - G).max() > np.abs(G).max(), (key, lam)
        seen += 1
    assert seen == 10


def test_arguments():
    from marl_amd.common.arguments import get_common_args, get_mixer_args
    assert get_common_args(["--td_lambda", "0.8"]).td_lambda == 0.8
    a = get_common_args([])
    assert a.td_lambda is None
    assert get_mixer_args(a).td_lambda is None
    b = get_common_args(["--td_lambda", "0.25"])
    assert get_mixer_args(b).td_lambda == 0.25
    ns = types.SimpleNamespace(map="2s3z")            # a reference-style namespace: no such field, and none appears
    assert not hasattr(get_mixer_args(ns), "td_lambda")
    from marl_amd.dropin.common.arguments import get_common_args as dropin_args
    assert dropin_args(["--td_lambda", "1"]).td_lambda == 1.0


def test_td_lambda_validation():
    from marl_amd.algorithm.common import td_lambda_of, GraphedUpdate
    ns = types.SimpleNamespace
    assert td_lambda_of(ns()) is None and td_lambda_of(ns(td_lambda=None)) is None
    assert td_lambda_of(ns(td_lambda=0)) == 0.0 and td_lambda_of(ns(td_lambda=1)) == 1.0
    assert td_lambda_of(ns(td_lambda=np.float32(0.5))) == 0.5
    for bad in (1.5, -0.1, float("nan"), "0.8", True):
        with pytest.raises(ValueError):
            td_lambda_of(ns(td_lambda=bad))
    assert "td_lambda" in GraphedUpdate.SCHEDULE_ARGS


def test_kernel_is_declared():
    from marl_amd import _lib
    txt = open(os.path.join(ROOT, "include", "marl_hip.h")).read()
    assert re.search(r"\bint\s+marl_td_lambda_returns\s*\(", txt)
    res, argtypes = _lib.SIGNATURES["marl_td_lambda_returns"]
    assert res is _lib.I and argtypes == [_lib.P] * 4 + [_lib.F, _lib.F, _lib.P, _lib.I, _lib.I, _lib.P]
    mk = open(os.path.join(ROOT, "marl_amd", "csrc", "Makefile")).read()
    assert "td_lambda.hip" in mk and os.path.exists(os.path.join(ROOT, "marl_amd", "csrc", "td_lambda.hip"))

"""MAIC training without a GPU: the float64 oracle (tests/maic_train_oracle.py) against the reference's own autograd, the
distance of every GPU test case from its discontinuities, the float32 yardstick of the oracle, and the --MAIC_train switch.

The LeakyReLU margin counts the pre-activations whose derivative reaches a gradient (maic_train_oracle.head_margins): a case
holds up to bs * N * (N + 1) * 64 of them and about 3.6e-5 of a smooth density fall under 1e-5 of the maximum, so the head
cases with bs = 37 give most environments no gradient, as the TD loss's mask does, and the MMM2 update has short episodes."""
import os
import types

import numpy as np
import pytest
import torch

import maic_oracle as mo
import maic_train_oracle as mt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEL_MARGIN, CLAMP_MARGIN, LEAKY_MARGIN = 1e-3, 1e-3, 1e-5
_HEAD, _UPD = {}, {}


def head_pair(case):
    if case not in _HEAD:
        args, state, h, q, eps, u_act, dq_val = mt.head_case_inputs(case)
        a = (state, h, q, eps, u_act, dq_val, case[1], args.n_agents, case[2], case[3])
        _HEAD[case] = (mt.head_grads(*a), mt.head_grads(*a, dtype=torch.float32))
    return _HEAD[case]


def update_pair(case):
    if case[0] not in _UPD:
        _UPD[case[0]] = mt.reference_update(case)
    return _UPD[case[0]]


@pytest.mark.parametrize("shape", ["2s3z", "MMM2"])
def test_oracle_matches_the_reference_autograd(shape):
    """gradients of sum(return_q * G) through the reference MAICAgent (training-mode BatchNorm, sampled latents): 1e-10"""
    fx = np.load(os.path.join(GOLDEN, "maic_%s_train_grad.npz" % shape))
    args = mo.maic_args(shape)
    N = args.n_agents
    state = mo.maic_state(args, seed=int(fx["seed"]))
    bs = fx["h"].shape[0] // N
    fc2 = state["fc2.weight"].astype(np.float64)
    q = fx["h"] @ fc2.T + state["fc2.bias"].astype(np.float64)
    r = mt.head_grads(state, fx["h"], q, fx["eps"], None, None, bs, N, False, True, G=fx["G"])
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    assert rel(r["out"]["return_q"], fx["return_q"]) < 1e-10
    assert rel(r["dh"] + fx["G"].astype(np.float64) @ fc2, fx["dh"]) < 1e-10          # the fixture's dh includes the fc2 path
    names = [k[5:] for k in fx.files if k.startswith("grad/")]
    assert sorted(names) == sorted(r["grads"]) and len(names) == 14
    for k in names:
        ref = fx["grad/" + k]
        assert np.abs(r["grads"][k] - ref).max() <= 1e-10 * max(np.abs(ref).max(), np.abs(fx["grad/" + mt.layer_of(k) + ".weight"]).max()), k


@pytest.mark.parametrize("case", mt.HEAD_CASES, ids=[mt.head_case_id(c) for c in mt.HEAD_CASES])
def test_head_case_margins(case):
    r64, _ = head_pair(case)
    print(mt.head_case_id(case), "clamp %.2e leaky %.2e" % (r64["clamp_margin"], r64["leaky_margin"]))
    assert r64["clamp_margin"] > CLAMP_MARGIN
    assert r64["leaky_margin"] > LEAKY_MARGIN


@pytest.mark.parametrize("case", mt.UPDATE_CASES, ids=[c[0] for c in mt.UPDATE_CASES])
def test_update_case_margins(case):
    o64, _ = update_pair(case)
    print(case[0], "selection %.2e clamp %.2e leaky %.2e" % (o64["selection_margin"], o64["clamp_margin"], o64["leaky_margin"]))
    assert o64["selection_margin"] > SEL_MARGIN
    assert o64["clamp_margin"] > CLAMP_MARGIN
    assert o64["leaky_margin"] > LEAKY_MARGIN


def _yardstick(name, a32, a64):
    """float32 oracle within 1e-4 * max|ref| of the float64 one"""
    a32, a64 = np.asarray(a32, dtype=np.float64), np.asarray(a64, dtype=np.float64)
    err, top = np.abs(a32 - a64).max(), np.abs(a64).max()
    print("%-44s max|ref| %.3e  float32 error %.3e" % (name, top, err))
    return err <= mt.TOL * top


def _grad_yardstick(name, bn_batch, g32, grads64):
    """every gradient within 1e-4 * max|ref|.  The two that are zero analytically (maic_train_oracle.is_zero_gradient) have the
    float64 rounding for max|ref|, which bounds nothing: they must BE zero - below 1e-9 of their layer's largest gradient - and
    their float32 error is held against that largest gradient; the GPU tests bound them by 4 x this error."""
    g = grads64[name]
    ok = _yardstick("grad " + name, g32, g)
    if not mt.is_zero_gradient(name, bn_batch):
        return ok
    top = max(np.abs(x).max() for n, x in grads64.items() if mt.layer_of(n) == mt.layer_of(name))
    return np.abs(g).max() <= 1e-9 * top and np.abs(np.asarray(g32, dtype=np.float64) - g).max() <= mt.TOL * top


@pytest.mark.parametrize("case", mt.HEAD_CASES, ids=[mt.head_case_id(c) for c in mt.HEAD_CASES])
def test_head_float32_yardstick(case):
    r64, r32 = head_pair(case)
    assert _yardstick("dh", r32["dh"], r64["dh"])
    for k in r64["grads"]:
        assert _grad_yardstick(k, case[3], r32["grads"][k], r64["grads"]), k


@pytest.mark.parametrize("case", mt.UPDATE_CASES, ids=[c[0] for c in mt.UPDATE_CASES])
def test_update_float32_yardstick(case):
    o64, o32 = update_pair(case)
    assert abs(o32["loss"] - o64["loss"]) <= mt.TOL * abs(o64["loss"])
    assert abs(o32["grad_norm"] - o64["grad_norm"]) <= mt.TOL * o64["grad_norm"]
    for n, g in o64["grads"].items():
        if n.startswith("agent.inference_net."):
            assert not g.any() and not o32["grads"][n].any(), n
            continue
        assert _grad_yardstick(n, case[6], o32["grads"][n], o64["grads"]), n
        keep = mt.step_is_decided(n, o64["grads"])
        if keep.any():
            assert _yardstick("param " + n, o32["params"][n][keep], o64["params"][n][keep]), n
    for tag in ("bn_eval", "bn_target"):
        for k in (mo.BN + "running_mean", mo.BN + "running_var"):
            assert _yardstick(tag + " " + k, o32[tag][k], o64[tag][k]), k


# ---------------------------------------------------------------------------------------------------- the switch
def test_argument_defaults():
    from marl_amd.common.arguments import get_common_args
    a = get_common_args([])
    assert a.MAIC is False and a.MAIC_train is False
    a = get_common_args(["--MAIC", "True", "--MAIC_train", "True"])
    assert a.MAIC is True and a.MAIC_train is True
    assert get_common_args(["--MAIC_train", "False"]).MAIC_train is False


def _runner_args(**over):
    a = mo.maic_args("2s3z")
    a.env, a.result_dir, a.model_dir, a.load_model = "synthetic", "/nonexistent", "/nonexistent", False
    a.MAIC = False
    a.__dict__.update(over)
    return a


def _patched_runner(monkeypatch, tmp_path, **over):
    """Runner with every builder replaced by a recorder: what it would have built"""
    from marl_amd import runner
    built = []
    for name in ("MAICMAC", "RTWMAC", "SharedMACWithState", "SharedMAC", "RolloutWorker", "ReplayBuffer", "MAICQLearner",
                 "MAICTDLearner", "QLearner"):
        monkeypatch.setattr(runner, name, lambda *a, _n=name, **k: built.append(_n) or types.SimpleNamespace(record_sink=None))
    logger = types.SimpleNamespace(setup_tb=lambda *a, **k: None)
    args = _runner_args(result_dir=str(tmp_path), **over)
    return built, lambda: runner.Runner(types.SimpleNamespace(), logger, args)


def test_maic_train_needs_maic(monkeypatch, tmp_path):
    built, make = _patched_runner(monkeypatch, tmp_path, MAIC_train=True)
    with pytest.raises(ValueError):
        make()
    assert built == []


@pytest.mark.parametrize("over,exc", [(dict(RTW=True), ValueError), (dict(world_model=True), ValueError),
                                      (dict(alg="qtran_base"), NotImplementedError), (dict(overlap_rollout=True), NotImplementedError)])
def test_trained_variant_keeps_the_refusals(over, exc, monkeypatch, tmp_path):
    built, make = _patched_runner(monkeypatch, tmp_path, MAIC=True, MAIC_train=True, **over)
    with pytest.raises(exc):
        make()
    assert built == []


def test_switch_picks_the_learner(monkeypatch, tmp_path):
    built, make = _patched_runner(monkeypatch, tmp_path, MAIC=True)
    make()
    assert "MAICQLearner" in built and "MAICTDLearner" not in built
    built2, make2 = _patched_runner(monkeypatch, tmp_path, MAIC=True, MAIC_train=True)
    make2()
    assert "MAICTDLearner" in built2 and "MAICQLearner" not in built2

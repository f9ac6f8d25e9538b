"""The MAIC agent's MI and entropy losses without a GPU: the float64 oracle (tests/maic_aux_oracle.py) against the reference's own
forward(train_mode=True) and autograd, the distance of every GPU test case from its discontinuities, the float32 yardstick of
the oracle, the clamped case's populations, the two new arguments and the refusals.

Analytically zero gradients (maic_aux_oracle.is_zero_gradient): w_query.bias - the d logits of a softmax sum to zero, under the
entropy term as under the TD loss - and, under batch statistics, embed_net.0.bias and inference_net.0.bias, which sit in front of
a BatchNorm that subtracts the column mean.  Their max|ref| is rounding and bounds nothing: they are held to be zero here, and the
GPU tests bound them by 4 x the float32 oracle's own error."""
import os

import numpy as np
import pytest
import torch

import maic_oracle as mo
import maic_train_oracle as mt
import maic_aux_oracle as ma
from test_maic_train_cpu import _patched_runner, _yardstick

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_KER, _UPD = {}, {}


def kernel_pair(case):
    if case[:1] + case[4:] not in _KER:
        args, state, h, q, eps = ma.kernel_case_inputs(case)
        a = (state, h, q, eps, case[2], args.n_agents, False, case[4])
        _KER[case[:1] + case[4:]] = (ma.kernel_reference(*a), ma.kernel_reference(*a, dtype=torch.float32))
    return _KER[case[:1] + case[4:]]


def update_pair(case):
    if case[0] not in _UPD:
        _UPD[case[0]] = ma.reference_updates(case)
    return _UPD[case[0]]


@pytest.mark.parametrize("shape", ["2s3z", "MMM2"])
def test_oracle_matches_the_reference(shape):
    """both losses, d (mi + ent) / d h and / d every head parameter, both BatchNorm modules' buffers: 1e-10"""
    fx = np.load(os.path.join(GOLDEN, "maic_%s_aux.npz" % shape))
    args = mo.maic_args(shape)
    N = args.n_agents
    state = mo.maic_state(args, seed=int(fx["seed"]))
    bs = fx["h"].shape[0] // N
    r = ma.full_grads(state, fx["h"], fx["return_q"], fx["eps"], bs, N, False, True)
    assert abs(r["mi"] - float(fx["mi_loss"])) < 1e-10 * float(fx["mi_loss"])
    assert abs(r["ent"] - float(fx["entropy_loss"])) < 1e-10 * float(fx["entropy_loss"])
    assert np.abs(r["dh"] - fx["dh"]).max() < 1e-10 * np.abs(fx["dh"]).max()
    names = [k[5:] for k in fx.files if k.startswith("grad/")]
    # the reference's backward also reaches fc1 and the GRU through h; msg_net and fc2 receive nothing
    assert sorted(k for k in names if not k.startswith(("fc1.", "rnn."))) == sorted(r["grads"]) and len(r["grads"]) == 16
    for k in r["grads"]:
        ref = fx["grad/" + k]
        assert np.abs(r["grads"][k] - ref).max() <= 1e-10 * max(np.abs(ref).max(), np.abs(fx["grad/" + mt.layer_of(k) + ".weight"]).max()), k
    for k, v in r["buffers"].items():
        assert np.abs(np.asarray(v, dtype=np.float64) - fx["buf/" + k]).max() < 1e-10, k
    # embed_net.1 is not evaluated a second time by the losses: the head's forward moved it once
    assert int(fx["buf/embed_net.1.num_batches_tracked"]) == int(state["embed_net.1.num_batches_tracked"]) + 1


@pytest.mark.parametrize("case", ma.KERNEL_CASES, ids=[ma.kernel_case_id(c) for c in ma.KERNEL_CASES])
def test_kernel_case_margins(case):
    r64, _ = kernel_pair(case)
    print(ma.kernel_case_id(case), " ".join("%s %.2e" % (k, r64[k]) for k in ma.MARGINS))
    for k in ma.MARGINS:
        assert r64[k] > ma.MARGIN, k


@pytest.mark.parametrize("ccase", ma.COMBINED_CASES, ids=[ma.kernel_case_id(c[0]) for c in ma.COMBINED_CASES])
def test_combined_case_margins_and_shares(ccase):
    """the combined backward's case is clear of the discontinuities of both parts, and neither part is lost in the other's bound"""
    r = ma.combined_reference(ccase)
    print(ma.kernel_case_id(ccase[0]), "clamp %.2e leaky %.2e MI share of dh %.2f" % (r["clamp_margin"], r["leaky_margin"], r["aux_share"]))
    assert r["clamp_margin"] > ma.MARGIN and r["leaky_margin"] > ma.MARGIN
    assert all(v > ma.MARGIN for v in r["aux_margins"].values())
    assert 0.1 < r["aux_share"] < 10


def test_clamped_case_populates_both_sides_of_both_clamps():
    for case in ma.KERNEL_CASES:
        if case[3]:
            r64, _ = kernel_pair(case)
            print(ma.kernel_case_id(case), "inference variances under the floor %.3f, alphas under 1e-4 %.3f" % (r64["below2"], r64["below_alpha"]))
            assert 0.05 <= r64["below2"] <= 0.95
            assert 0.05 <= r64["below_alpha"] <= 0.95


@pytest.mark.parametrize("case", ma.UPDATE_CASES, ids=[c[0] for c in ma.UPDATE_CASES])
def test_update_case_margins(case):
    o64, _ = update_pair(case)
    for step in o64:
        m = dict(step["aux_margins"], selection=step["selection_margin"], clamp=step["clamp_margin"], leaky=step["leaky_margin"])
        print(case[0], " ".join("%s %.2e" % kv for kv in m.items()))
        for k, v in m.items():
            assert v > ma.MARGIN, k


def _grad_yardstick(name, bn_batch, g32, grads64):
    """test_maic_train_cpu._grad_yardstick with this file's list of analytically zero gradients"""
    g = grads64[name]
    ok = _yardstick("grad " + name, g32, g)
    if not ma.is_zero_gradient(name, bn_batch):
        return ok
    top = max(np.abs(x).max() for n, x in grads64.items() if mt.layer_of(n) == mt.layer_of(name))
    return np.abs(g).max() <= 1e-9 * top and np.abs(np.asarray(g32, dtype=np.float64) - g).max() <= ma.TOL * top


@pytest.mark.parametrize("case", ma.KERNEL_CASES, ids=[ma.kernel_case_id(c) for c in ma.KERNEL_CASES])
def test_kernel_float32_yardstick(case):
    r64, r32 = kernel_pair(case)
    for k in ("mi", "ent", "dh", "dpar"):
        assert _yardstick(k, r32[k], r64[k]), k
    for k in r64["grads"]:
        assert _grad_yardstick(k, case[4], r32["grads"][k], r64["grads"]), k
    for k in (ma.IBN + "running_mean", ma.IBN + "running_var"):
        assert _yardstick(k, r32["buffers"][k], r64["buffers"][k]), k


@pytest.mark.parametrize("case", ma.UPDATE_CASES, ids=[c[0] for c in ma.UPDATE_CASES])
def test_update_float32_yardstick(case):
    o64, o32 = update_pair(case)
    keep = None
    for ts, (s64, s32) in enumerate(zip(o64, o32)):
        for k in ("loss", "mi_sum", "ent_sum", "grad_norm"):
            assert abs(s32[k] - s64[k]) <= ma.TOL * abs(s64[k]), k
        for n, g in s64["grads"].items():
            assert _grad_yardstick(n, case[2], s32["grads"][n], s64["grads"]), n
        step = {n: mt.step_is_decided(n, s64["grads"]) for n in s64["grads"]}
        keep = step if keep is None else {n: keep[n] & step[n] for n in keep}
        for n in keep:
            if keep[n].any():
                assert _yardstick("param " + n, s32["params"][n][keep[n]], s64["params"][n][keep[n]]), n
        for tag in ("bn_eval", "bn_target"):
            for p in (mo.BN, ma.IBN):
                for k in (p + "running_mean", p + "running_var"):
                    ok = _yardstick(tag + " " + k, s32[tag][k], s64[tag][k])
                    if ma.follows_a_free_bias(k, case[2], ts):
                        # bounded by the walk of the bias in front of it: 10 lr per step, seen through momentum 0.1
                        assert np.abs(s32[tag][k] - s64[tag][k]).max() <= 10 * 5e-4 * ts, k
                    else:
                        assert ok, k
    # inference_net moves, and only because of the MI term
    first = o64[0]
    assert all(np.abs(first["grads"]["agent.inference_net.%s" % k]).max() > 0 for k in ("0.weight", "1.weight", "3.weight", "3.bias"))


def test_update_total_is_td_plus_the_two_means():
    o64, _ = update_pair(ma.UPDATE_CASES[0])
    s = o64[0]
    assert s["T"] == ma.UT and s["mi_sum"] > 0 and s["ent_sum"] > 0
    assert abs(s["loss"] - (s["td"] + (s["mi_sum"] + s["ent_sum"]) / s["T"])) < 1e-12
    # the buffers of inference_net.1 moved once per transition index, the target copy did not
    assert int(s["bn_eval"][ma.IBN + "num_batches_tracked"]) == 3 + ma.UT
    assert int(s["bn_target"][ma.IBN + "num_batches_tracked"]) == 3


# ---------------------------------------------------------------------------------------------------- arguments and refusals
def test_argument_defaults():
    from marl_amd.common.arguments import get_common_args
    a = get_common_args([])
    assert a.mi_loss_weight == 0.0 and a.entropy_loss_weight == 0.0
    a = get_common_args(["--mi_loss_weight", "0.001", "--entropy_loss_weight", "0.01"])
    assert a.mi_loss_weight == 0.001 and a.entropy_loss_weight == 0.01


@pytest.mark.parametrize("over", [dict(mi_loss_weight=0.001), dict(entropy_loss_weight=0.01)])
def test_a_loss_weight_needs_maic_train(over, monkeypatch, tmp_path):
    built, make = _patched_runner(monkeypatch, tmp_path, MAIC=True, **over)
    with pytest.raises(ValueError):
        make()
    assert built == []
    built, make = _patched_runner(monkeypatch, tmp_path, MAIC=True, MAIC_train=True, **over)
    make()
    assert "MAICTDLearner" in built


def test_forward_still_refuses_train_mode_with_a_weight():
    from marl_amd.network.maic import MAICAgent
    args = ma.shape_args("2s3z")
    agent = MAICAgent(args.obs_shape + args.n_actions + args.n_agents, args)
    with pytest.raises(NotImplementedError):
        agent.forward(torch.zeros(5, 96), torch.zeros(5, 64), 1, train_mode=True)

"""MAIC without a GPU: the float64 restatement (tests/maic_oracle.py) against the fixtures recorded from the reference
MAICAgent, the module's state-dict layout, argument defaults, the Runner's refusals, the drop-in names and the shape gate."""
import os
import types

import numpy as np
import pytest
import torch

import maic_oracle as mo

MODES = [("test", "eval"), ("test", "batch"), ("samp", "eval"), ("samp", "batch")]


def _fx(golden_dir, shape, tag=None):
    return np.load(os.path.join(golden_dir, "maic_%s_%s.npz" % (shape, tag or "inputs")))


@pytest.mark.parametrize("shape", ["2s3z", "MMM2"])
def test_state_dict_layout_is_the_references(shape, golden_dir):
    from marl_amd.network.maic import MAICAgent
    fx = _fx(golden_dir, shape)
    args = mo.maic_args(shape)
    agent = MAICAgent(args.obs_shape + args.n_actions + args.n_agents, args)
    got = [(k, ",".join(map(str, v.shape))) for k, v in agent.state_dict().items()]
    assert got == list(zip(fx["keys"].tolist(), fx["shapes"].tolist()))
    assert [(k, ",".join(map(str, s))) for k, s in mo.key_shapes(args)] == got
    agent.load_state_dict({k: torch.tensor(v) for k, v in mo.maic_state(args).items()}, strict=True)
    assert agent.init_hidden().shape == (1, 64) and agent.training


@pytest.mark.parametrize("shape", ["2s3z", "MMM2"])
@pytest.mark.parametrize("mode", MODES, ids=["_".join(m) for m in MODES])
def test_oracle_equals_reference_fixture(shape, mode, golden_dir):
    fi, fx = _fx(golden_dir, shape), _fx(golden_dir, shape, "_".join(mode))
    args = mo.maic_args(shape)
    N = args.n_agents
    bs = fi["inputs"].shape[0] // N
    test_mode, bn_train = mode[0] == "test", mode[1] == "batch"
    eps = None if test_mode else torch.tensor(fx["eps"], dtype=torch.float64)
    p = mo.p64(mo.maic_state(args, seed=int(fi["seed"])))
    o = mo.forward(p, torch.tensor(fi["inputs"], dtype=torch.float64), torch.tensor(fi["h0"], dtype=torch.float64), bs, N,
                   test_mode, bn_train, eps)
    for k in ("return_q", "latent", "alpha", "msg", "running_mean", "running_var"):
        np.testing.assert_allclose(o[k].numpy(), fx[k], rtol=0, atol=1e-10, err_msg=k)
    np.testing.assert_allclose(o["h"].numpy(), fi["h"], rtol=0, atol=1e-10)
    assert o["num_batches_tracked"] == int(fx["num_batches_tracked"]) == 3 + int(bn_train)
    if test_mode:       # the gate is exercised: a good share of the off-diagonal alphas is exactly zero
        off = fx["alpha"][~np.broadcast_to(np.eye(N, dtype=bool), fx["alpha"].shape)]
        assert 0.2 < (off == 0).mean() < 0.9


def test_oracle_serial_rollout_equals_fixture(golden_dir):
    from oracle import rollout as orl
    fx = np.load(os.path.join(golden_dir, "maic_serial.npz"))
    args = mo.maic_args("2s3z", episode_limit=8)
    p = mo.p64(mo.maic_state(args, seed=int(fx["seed"])))

    def fwd(inp, h):
        o = mo.forward(p, inp, h, 1, args.n_agents, True, False)
        return o["return_q"], o["h"]
    ep, rew, wins, steps = mo.serial_rollout(fwd, args, orl.SerialSynthEnv(orl.SynthSMAC(5, 80, 120, 11, 8, seed=5)), 6)
    for k in ("u", "padded", "terminated", "avail_u"):
        np.testing.assert_array_equal(ep[k], fx[k], err_msg=k)
    np.testing.assert_allclose(ep["o"], fx["o"], atol=1e-12)
    np.testing.assert_allclose(rew, fx["rewards"], atol=1e-12)
    assert steps == int(fx["steps"]) and list(wins) == list(fx["wins"])


def test_hash_noise_is_standard_normal():
    z = mo.hash_noise(3, np.arange(64), np.full(64, 17), 10).astype(np.float64)
    assert z.shape == (64, 10, 80) and np.isfinite(z).all()
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    assert not np.array_equal(z[0], z[1])


def test_argument_defaults():
    from marl_amd.common.arguments import get_common_args, get_maic_args
    a = get_common_args([])
    assert a.MAIC is False
    assert get_common_args(["--MAIC", "True"]).MAIC is True
    get_maic_args(a)
    assert (a.latent_dim, a.nn_hidden_size, a.var_floor, a.attention_dim) == (8, 64, 0.002, 32)
    from marl_amd.main import build
    args, env = None, None
    try:
        args, env = build(["--MAIC", "True", "--map", "2s3z"])
    except RuntimeError:        # no GPU for the env: the parser part is what this test is about
        return
    assert args.MAIC and args.latent_dim == 8


def _runner_args(**over):
    a = mo.maic_args("2s3z")
    a.env, a.result_dir, a.model_dir = "synthetic", "/nonexistent/result", "/nonexistent/model"
    a.__dict__.update(over)
    return a


@pytest.mark.parametrize("over,exc", [
    (dict(RTW=True), ValueError),
    (dict(world_model=True), ValueError),
    (dict(alg="qtran_base"), NotImplementedError),
    (dict(alg="qtran_alt"), NotImplementedError),
    (dict(overlap_rollout=True), NotImplementedError),
])
def test_runner_refuses_before_building(over, exc, monkeypatch):
    from marl_amd import runner
    built = []
    for name in ("MAICMAC", "RTWMAC", "SharedMACWithState", "SharedMAC", "RolloutWorker"):
        monkeypatch.setattr(runner, name, lambda *a, _n=name, **k: built.append(_n))
    with pytest.raises(exc):
        runner.Runner(types.SimpleNamespace(), None, _runner_args(**over))
    assert built == []


def test_learner_train_refuses_and_touches_nothing():
    from marl_amd.algorithm.maic_q_learner import MAICQLearner
    learner = MAICQLearner.__new__(MAICQLearner)         # no device needed: train must not look at anything
    with pytest.raises(NotImplementedError):
        learner.train({}, 0)
    assert learner.__dict__ == {}


def test_forward_refuses_training_losses_before_any_launch():
    from marl_amd.network.maic import MAICAgent
    args = mo.maic_args("2s3z")
    args.mi_loss_weight = 0.001
    agent = MAICAgent(96, args)
    before = {k: v.clone() for k, v in agent.state_dict().items()}
    with pytest.raises(NotImplementedError):
        agent(torch.zeros(5, 96), torch.zeros(5, 64), 1, train_mode=True)
    assert all(torch.equal(v, before[k]) for k, v in agent.state_dict().items())


def test_dropin_names_resolve():
    import importlib
    import sys
    from marl_amd import dropin
    root = os.path.dirname(dropin.__file__)
    sys.path.insert(0, root)
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k.split(".")[0] in ("network", "controller", "common")}
    try:
        assert importlib.import_module("network.MAIC").MAICAgent.__module__ == "marl_amd.network.maic"
        assert importlib.import_module("controller.share_params").MAICMAC.__module__ == "marl_amd.controller.share_params"
        assert importlib.import_module("common.arguments").get_maic_args.__module__ == "marl_amd.common.arguments"
    finally:
        sys.path.remove(root)
        for k in list(sys.modules):
            if k.split(".")[0] in ("network", "controller", "common"):
                del sys.modules[k]
        sys.modules.update(saved)


def test_supported_shapes():
    from marl_amd import ops
    for N, O, A in mo.SHAPES.values():
        assert ops.maic_supported(N, O, A)
    assert not ops.maic_supported(17, 80, 11)
    assert not ops.maic_supported(5, 80, 33)
    assert not ops.maic_supported(5, 80, 11, H=32)
    args = mo.maic_args("2s3z")
    args.n_agents = 17
    from marl_amd.network.maic import MAICAgent
    with pytest.raises(ValueError):
        MAICAgent(96, args)

"""The battle environment under the rollout worker, the learners and the launcher: RolloutWorker's per-step path over BattleEnv with a
Q controller and a sampling policy controller, one update of a Q learner and of an actor-critic on such a batch, main.build's shapes
and refusals, and Runner.evaluate's win rate (the first one here that depends on what the agents did)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
E = 8


def build(alg, tmp_path, *more):
    from marl_amd.main import build
    args, env = build(["--env", "battle", "--map", "3m", "--alg", alg, "--n_envs", str(E), "--seed", "5", "--evaluate_epoch", "1",
                       "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "model")] + list(more))
    args.save_cycle = 10 ** 9
    return args, env


def rollout(alg, tmp_path, mac_name, evaluate=False):
    from marl_amd.controller import share_params
    from marl_amd.rollout import RolloutWorker
    args, env = build(alg, tmp_path)
    torch.manual_seed(2)
    mac = getattr(share_params, mac_name)(args)
    w = RolloutWorker(env, mac, args)
    ep, rewards, wins, steps = w.generate_episodes(E, evaluate=evaluate)
    return args, env, mac, w, ep, rewards, wins, steps


def check_record(rec, rewards, wins, steps):
    T, N, A = rec.T, rec.N, rec.A
    assert (T, N, rec.O, rec.S, A) == (60, 3, 30, 48, 9) and rec.E == E
    f = {k: getattr(rec, k).cpu().numpy() for k in ("obs", "state", "avail", "u", "r", "term", "padded", "length", "won")}
    t, L = np.arange(T)[None, :], f["length"][:, None]
    assert (f["length"] >= 1).all() and (f["length"] <= T).all() and set(np.unique(f["won"])) <= {0, 1}
    np.testing.assert_array_equal(f["padded"], (t >= L).astype(np.float32))
    np.testing.assert_array_equal(f["term"], (t >= L - 1).astype(np.float32))
    assert (f["r"] >= 0).all() and (f["r"][t >= L] == 0).all() and np.isfinite(f["obs"]).all() and np.isfinite(f["state"]).all()
    live = np.broadcast_to((t < L)[:, :, None], f["u"].shape)
    assert (f["u"][~live] == -1).all()
    taken = np.take_along_axis(f["avail"][:, :T], np.maximum(f["u"], 0)[..., None], axis=3)[..., 0]
    assert (taken[live] == 1).all()                                          # u is an available action wherever the episode is live
    past = np.arange(T + 1)[None, :] > L
    assert not f["obs"][past].any() and not f["state"][past].any() and not f["avail"][past].any()
    assert f["avail"][~past].reshape(-1, A).sum(axis=1).min() >= 1
    np.testing.assert_allclose(rewards, f["r"].sum(axis=1), rtol=1e-6)
    assert wins == [bool(x) for x in f["won"]] and steps == int(f["length"].sum())
    return f


@pytest.mark.parametrize("alg,mac_name", [("qmix", "SharedMAC"), ("central_v", "PolicyMAC")])
def test_rollout_obeys_the_record_invariants_and_repeats_bit_for_bit(alg, mac_name, tmp_path):
    args, env, mac, w, ep, rewards, wins, steps = rollout(alg, tmp_path, mac_name)
    assert not hasattr(env, "fused_step") and not hasattr(env, "whole_rollout") and env.episode == 0
    assert mac.stochastic == (mac_name == "PolicyMAC")
    a = check_record(ep.record, rewards, wins, steps)
    assert len({tuple(x) for x in a["u"][:, 0]}) > 1 or a["r"].sum() > 0       # the controller's choices reach the environment
    b = rollout(alg, tmp_path, mac_name)[4].record
    for k, v in a.items():
        np.testing.assert_array_equal(v.view(np.uint32) if v.dtype == np.float32 else v,
                                      getattr(b, k).cpu().numpy().view(np.uint32 if v.dtype == np.float32 else v.dtype), err_msg=k)


def _params(learner_or_mac):
    return torch.cat([p.detach().reshape(-1).clone() for p in learner_or_mac.agent.parameters()])


def test_one_qmix_update_on_a_battle_batch(tmp_path):
    from marl_amd.algorithm.q_learner import QLearner
    args, env, mac, w, ep, *_ = rollout("qmix", tmp_path, "SharedMAC")
    learner = QLearner(mac, args)
    before = _params(mac)
    loss = float(learner.train(ep, 0))
    assert np.isfinite(loss) and loss > 0
    after = _params(mac)
    assert torch.isfinite(after).all() and not torch.equal(before, after)


def test_one_central_v_update_on_a_battle_batch(tmp_path):
    from marl_amd.algorithm.central_v import CentralVLearner
    args, env, mac, w, ep, *_ = rollout("central_v", tmp_path, "PolicyMAC")
    learner = CentralVLearner(mac, args)
    before = _params(mac)
    loss = float(learner.train(ep, 0, epsilon=w.epsilon))
    assert np.isfinite(loss) and np.isfinite(float(learner.actor_loss))
    after = _params(mac)
    assert torch.isfinite(after).all() and not torch.equal(before, after)


def test_launcher_reports_the_tables_shapes(tmp_path):
    from marl_amd.main import build as main_build
    from marl_amd.env.battle import BattleEnv
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    out = ["--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "model"), "--n_envs", "4"]
    for name, shapes in (("3m", (3, 30, 48, 9, 60)), ("2s3z", (5, 80, 120, 11, 120)), ("3s5z", (8, 128, 216, 14, 150))):
        for alg in ("qmix", "qatten", "lica"):
            args, env = main_build(["--env", "battle", "--map", name, "--alg", alg] + out)
            assert type(env) is BattleEnv and env.n_envs == 4 and args.env == "battle" and args.map == name
            assert (args.n_agents, args.obs_shape, args.state_shape, args.n_actions, args.episode_limit) == shapes
    args, env = main_build(["--env", "smac", "--map", "2s3z"] + out)               # --env smac keeps meaning synthetic
    assert type(env) is SyntheticSMACEnv and args.env == "synthetic"


def test_launcher_refusals(tmp_path):
    from marl_amd.main import build as main_build, make_runner
    from marl_amd.utils.logging import Logger
    with pytest.raises(ValueError, match="medivac"):
        main_build(["--env", "battle", "--map", "MMM2"])
    with pytest.raises(ValueError, match="no map 'corridor'"):
        main_build(["--env", "battle", "--map", "corridor", "--alg", "qatten"])
    args, env = build("qmix", tmp_path, "--evaluate_epoch", "0")
    args.overlap_rollout = True
    r = make_runner(args, env, Logger())
    with pytest.raises(RuntimeError, match="whole-rollout kernel"):
        r.run(0)


def test_evaluate_returns_the_mean_of_the_records_won(tmp_path):
    from marl_amd.main import make_runner
    from marl_amd.utils.logging import Logger
    args, env = build("qmix", tmp_path)
    torch.manual_seed(2)
    r = make_runner(args, env, Logger())
    seen = []
    inner = r.rolloutWorker.generate_episodes

    def spy(*a, **k):
        out = inner(*a, **k)
        seen.append((k.get("evaluate", False), out[0].record))
        return out
    r.rolloutWorker.generate_episodes = spy
    win_rate, reward = r.evaluate()
    (evaluate, rec), = seen
    assert evaluate and rec.E == E
    assert win_rate == float(rec.won.float().mean().item()) and 0.0 <= win_rate <= 1.0
    assert reward == pytest.approx(float(rec.r.sum(1).mean().item()), rel=1e-6)
    # the launcher's training loop runs to its end on this environment
    r.rolloutWorker.generate_episodes = inner
    r.args.n_steps = 1
    assert np.isfinite(float(r.run(0))) and r.train_steps >= 1 and env.episode >= 2

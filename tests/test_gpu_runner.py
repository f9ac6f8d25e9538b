"""Runner / launcher / matrix-game harness on the GPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_runner_loop_synthetic(tmp_path):
    from marl_amd.main import build
    from marl_amd.runner import Runner
    from marl_amd.utils.logging import Logger
    args, env = build(["--alg", "qmix", "--map", "2s3z", "--n_envs", "16", "--n_steps", "6000",
                       "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "model"),
                       "--evaluate_epoch", "16", "--evaluate_cycle", "3000"])
    args.save_cycle = 2
    log = Logger()
    runner = Runner(env, log, args)
    loss = runner.run(0)
    assert np.isfinite(loss)
    assert len(log.stats["total_loss"]) >= 3 and len(runner.eval_episode_rewards) >= 3
    assert (tmp_path / "model" / "qmix" / "2s3z" / "1_rnn_net_params.pkl").exists()
    steps = [t for t, _ in log.stats["episode_length"]]
    assert steps == sorted(steps) and steps[-1] >= 6000
    # epsilon annealed once per lock-step
    assert runner.rolloutWorker.epsilon < 1.0


@pytest.mark.parametrize("alg,iters", [("qtran_base", 3000), ("qplex", 3000)])
def test_matrix_game_finds_the_optimal_joint_action(alg, iters):
    """payoff [[8,-12,-12],[-12,0,0],[-12,0,0]]: QPLEX / QTRAN-base reach joint action [0,0] (reward 8) as
    in the reference's result/*/MatrixGame/episode_rewards.npy."""
    from marl_amd.matrix_game_test import run
    torch.manual_seed(0)
    q_tot, joint, individual, loss = run(alg, iters, verbose=False)
    assert joint == [0, 0], (q_tot, joint)
    # the learned value is still approaching 8 after 3000 updates; how close it gets by then depends on fp32 summation
    # order (SGD is chaotic), the greedy joint action does not
    assert abs(q_tot[0, 0] - 8.0) < 2.5


def test_matrix_game_qmix_lands_in_the_suboptimal_basin():
    """QMIX's monotonic mixer cannot represent this payoff: the reference's run ends at reward 0
    (result/qmix/MatrixGame/episode_rewards.npy: 2001 evaluations, the last ones all 0), i.e. a greedy joint action in
    the [[0,0],[0,0]] block instead of [0,0] (reward 8) - matrix_game_test.py:101-113."""
    from marl_amd.matrix_game_test import run, PAYOFF1
    torch.manual_seed(0)
    q_tot, joint, individual, loss = run("qmix", 2000, verbose=False)
    assert PAYOFF1[joint[0]][joint[1]] == 0, (q_tot, joint)
    assert PAYOFF1[individual[0]][individual[1]] == 0, individual          # what the decentralised greedy agents play
    assert q_tot[0, 0] < q_tot[joint[0], joint[1]]


def _runner(tmp_path, tag, extra=(), seed=3, **over):
    from marl_amd.main import build
    from marl_amd.runner import Runner
    from marl_amd.utils.logging import Logger
    args, env = build(["--alg", "qmix", "--map", "2s3z", "--n_envs", "16", "--n_steps", "9000",
                       "--result_dir", str(tmp_path / (tag + "_res")), "--model_dir", str(tmp_path / (tag + "_model")),
                       "--evaluate_epoch", "0"] + list(extra))
    args.buffer_size = 48            # 3 rollouts fill the ring: later rollouts overwrite stored episodes
    args.batch_size = 16
    args.save_cycle = 10 ** 9
    for k, v in over.items():
        setattr(args, k, v)
    torch.manual_seed(seed)
    np.random.seed(seed)
    return Runner(env, Logger(), args)


def test_overlapped_rollout_equals_the_same_schedule_on_one_stream(tmp_path):
    """rollout k+1 on a side stream while update k trains.  The rollout reads a snapshot of the agent
    taken before update k and the sampler skips the ring slots in flight, so the two-stream run must give exactly the
    losses of the same lag-1 schedule executed on ONE stream; the reference's lag-0 cadence (default) differs."""
    a = _runner(tmp_path, "ov", overlap_rollout=True)
    a.run(0)
    b = _runner(tmp_path, "ser", overlap_rollout="lag1_serial")
    b.run(0)
    c = _runner(tmp_path, "ref")
    c.run(0)
    assert len(a.losses) == len(b.losses) == len(c.losses) >= 5
    assert a.losses == b.losses                      # bitwise: same kernels, same inputs, only the stream differs
    assert a.losses[:1] == c.losses[:1] and a.losses != c.losses      # lag 1 vs the reference's lag 0
    assert a.rolloutWorker.epsilon < 1.0 and a._side is not None and b._side is None


def test_full_resume_continues_bitwise(tmp_path):
    """optimizer state, targets, epsilon, loop counters, env episode counter and the numpy RNG state
    survive save_resume / load_resume: a resumed Runner repeats the original run's next updates bit for bit.  (The
    replay ring is deliberately not in the file - it refills; the test transplants a snapshot of it.)"""
    def iterate(r, k):           # k iterations of the runner loop (episode lengths vary, so step by step)
        for _ in range(k):
            r.args.n_steps = r.time_steps + 1
            r.run(0)
    a = _runner(tmp_path, "full")
    iterate(a, 3)
    ck = str(tmp_path / "resume.pt")
    a.save_resume(ck)
    ring = (a.buffer.record.clone(), a.buffer.current_idx, a.buffer.current_size)
    at_save = (a.time_steps, a.train_steps, a.evaluate_steps, a.rolloutWorker.epsilon, a.env.episode)
    iterate(a, 2)
    assert len(a.losses) == 5
    b = _runner(tmp_path, "resumed", seed=77, resume=ck)      # a different initialisation: everything comes from the file
    assert (b.time_steps, b.train_steps, b.evaluate_steps, b.rolloutWorker.epsilon, b.env.episode) == at_save
    assert b.train_steps == 3 and b.rolloutWorker.epsilon < 1.0
    b.buffer.record, b.buffer.current_idx, b.buffer.current_size = ring
    iterate(b, 2)
    assert b.losses == a.losses[3:]
    assert torch.equal(b.learner._flat.flat, a.learner._flat.flat)
    assert torch.equal(b.learner.optimizer.s1, a.learner.optimizer.s1)
    assert torch.equal(b.learner.target_net.agent._flat.flat, a.learner.target_net.agent._flat.flat)


def test_reference_style_main_flow_on_dropin(tmp_path):
    """main.py's steps written against the reference's module paths (tests/dropin_main_flow.py) through the launcher:
    `runner`, `smac.env` (synthetic shim), `common.arguments`, `utils.logging` resolve to marl_amd and a short run trains."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-m", "marl_amd.dropin", os.path.join(root, "tests", "dropin_main_flow.py"),
                        "--alg", "qmix", "--map", "2s3z", "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "m")],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=root, MARL_N_ENVS="16", MPLBACKEND="Agg"))
    assert p.returncode == 0 and "MAIN_FLOW_OK" in p.stdout, (p.stdout[-1500:], p.stderr[-3000:])


def test_reference_style_matrix_game_flow_on_dropin(tmp_path):
    """matrix_game_test.py's steps written against the reference's module paths (tests/dropin_matrix_game_flow.py) through the
    launcher: QTRAN-base on the matrix game trains on the MI355X classes and reads its Q tables."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-m", "marl_amd.dropin", os.path.join(root, "tests", "dropin_matrix_game_flow.py")],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=root, MPLBACKEND="Agg"))
    assert p.returncode == 0 and "MATRIX_FLOW_OK" in p.stdout, (p.stdout[-1500:], p.stderr[-3000:])


def test_main_flow_vectorises_a_real_smac_install(tmp_path):
    """A `smac` package that IS importable (here: a stand-in whose StarCraft2Env is a serial host environment with the
    reference's env API) + MARL_N_ENVS > 1: the launcher wraps it in HostVectorEnv, and main.py's flow trains on the lock-step
    rollout over host environments (reference main.py:16-29, rollout.py:42,61-64,86-88)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = tmp_path / "site" / "smac"
    pkg.mkdir(parents=True)
    (pkg / "__init__.py").write_text("")
    (pkg / "env.py").write_text(
        "import itertools\n"
        "from oracle.rollout import SynthSMAC, SerialSynthEnv\n"
        "_ids = itertools.count()\n"
        "class StarCraft2Env(SerialSynthEnv):\n"
        "    def __init__(self, map_name='2s3z', **kw):\n"
        "        assert map_name == '2s3z'\n"
        "        super().__init__(SynthSMAC(5, 80, 120, 11, 24, seed=3), env_id=next(_ids))\n")
    p = subprocess.run([sys.executable, "-m", "marl_amd.dropin", os.path.join(root, "tests", "dropin_main_flow.py"),
                        "--alg", "qmix", "--map", "2s3z", "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "m")],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=root + os.pathsep + str(tmp_path / "site"), MARL_N_ENVS="6",
                                MARL_ENV_THREADS="3", MPLBACKEND="Agg"))
    assert p.returncode == 0 and "MAIN_FLOW_OK" in p.stdout, (p.stdout[-1500:], p.stderr[-3000:])
    assert "marl_amd.env.host_vector" in p.stdout

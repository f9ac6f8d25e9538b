"""One row of marl_amd/algorithms.py is all a new algorithm name needs: the launcher applies its table, keeps its kept fields and runs
its check on both sides of the environment, make_runner builds its controller and learner, and its refusal comes before anything is
built.  No GPU: the environment is a stub and the classes are stubs set on marl_amd.runner."""
import types

import pytest


class _Logger:
    def setup_tb(self, path):
        pass


@pytest.fixture
def toy(monkeypatch, tmp_path):
    from marl_amd import algorithms, main, runner
    seen = types.SimpleNamespace(checks=[], envs=[], built=[])

    def table(args):
        args.toy_width, args.td_lambda = 7, 0.9

    def env(*a, **k):
        seen.envs.append(1)
        return type("E", (), {"get_env_info": lambda self: dict(n_actions=11, n_agents=5, state_shape=120, obs_shape=80, episode_limit=120)})()

    stub = lambda name: lambda *a, **k: seen.built.append(name) or types.SimpleNamespace(kind=name, record_sink=None)
    monkeypatch.setitem(algorithms.ALGORITHMS, "toy", algorithms.Row(
        table=table, keeps=("td_lambda",), check="runner:toy_check", early=dict(n_agents=None, n_actions=4), mac="ToyMAC",
        learner="ToyLearner", launcher_only=True, no_switch="%s is a toy: not with %s"))
    monkeypatch.setattr(runner, "toy_check", lambda args: seen.checks.append((len(seen.envs), args.n_agents, args.n_actions)), raising=False)
    for name in ("ToyMAC", "ToyLearner"):
        monkeypatch.setattr(runner, name, stub(name), raising=False)
    for name in ("RolloutWorker", "ReplayBuffer"):
        monkeypatch.setattr(runner, name, stub(name))
    monkeypatch.setattr(main, "SyntheticSMACEnv", env)
    return main, seen, ["--alg", "toy", "--map", "MMM2", "--result_dir", str(tmp_path)]


def test_build_applies_the_row(toy):
    main, seen, argv = toy
    args, _ = main.build(argv)
    assert (args.toy_width, args.td_lambda) == (7, 0.9)                  # the table, over get_mixer_args
    args, _ = main.build(argv + ["--td_lambda", "0.3"])
    assert (args.toy_width, args.td_lambda) == (7, 0.3)                  # a given value of a kept field survives it
    # the check ran once before each environment was made, on the map's agents and the row's own actions, and once after it
    assert seen.checks == [(0, 10, 4), (1, 5, 11), (1, 10, 4), (2, 5, 11)] and len(seen.envs) == 2


def test_make_runner_builds_the_rows_classes(toy):
    main, seen, argv = toy
    args, env = main.build(argv)
    r = main.make_runner(args, env, _Logger())
    assert (r.mac.kind, r.learner.kind, r.on_policy, r.buffer) == ("ToyMAC", "ToyLearner", True, None)
    assert seen.built == ["ToyMAC", "RolloutWorker", "ToyLearner"]


def test_the_rows_refusal_comes_before_anything_is_built(toy):
    main, seen, argv = toy
    args, env = main.build(argv + ["--RTW", "True"])
    with pytest.raises(ValueError, match="^toy is a toy: not with RTW$"):
        main.make_runner(args, env, _Logger())
    assert seen.built == []

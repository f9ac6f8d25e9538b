"""Host-side logic that needs no GPU: replay ring arithmetic vs the reference fixture, the device
form of get_max_episode_len, argument parsing, drop-in module paths."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import seeded, learners


def test_replay_host_mode_matches_reference(golden_dir):
    from marl_amd.common.replaybuffer import ReplayBuffer
    fix = np.load(os.path.join(golden_dir, "replay.npz"))
    args = seeded.make_args("2s3z", "qmix", episode_limit=3, buffer_size=7)
    buf = ReplayBuffer(args)
    log = []
    for i, n in enumerate([1, 3, 2, 3, 1, 7, 2]):
        before = buf.current_idx
        buf.store_episode(seeded.make_batch(args, n, seed=300 + i))
        log.append([before, buf.current_idx, buf.current_size])
    np.testing.assert_array_equal(np.array(log), fix["state_log"])
    np.testing.assert_array_equal(buf.buffers["r"], fix["final_r"])
    np.random.seed(21)
    s = buf.sample(5)
    np.testing.assert_array_equal(s["r"], fix["sample_r"])
    np.testing.assert_array_equal(s["u"], fix["sample_u"])
    assert set(s) == {"o", "u", "s", "r", "o_next", "s_next", "avail_u", "avail_u_next", "u_onehot", "padded", "terminated"}


def test_first_terminated_len_matches_reference_rule():
    from marl_amd.hostutil import DeviceBatch, onehot_to_index
    rng = np.random.default_rng(0)
    for _ in range(50):
        B, T = int(rng.integers(1, 6)), int(rng.integers(1, 9))
        term = (rng.random((B, T, 1)) < 0.25).astype(np.float64)
        assert DeviceBatch.first_terminated_len(torch.tensor(term), T) == learners.max_episode_len(term, T)
    assert DeviceBatch.first_terminated_len(torch.zeros(3, 5, 1), 5) == 5      # quirk Q2: none terminated
    oh = torch.tensor([[0., 1, 0], [0, 0, 0], [0, 0, 1]])
    assert onehot_to_index(oh).tolist() == [1, -1, 2]


def test_scratch_is_one_class_and_zero_fills_at_allocation_only():
    from marl_amd import hostutil
    from marl_amd.algorithm import common
    assert common.Scratch is hostutil.Scratch                                  # importable from its old place
    buf, cpu = hostutil.Scratch(), torch.device("cpu")
    z = buf.get("z", (3, 2), cpu, torch.int32, zero=True)
    assert z.dtype == torch.int32 and z.shape == (3, 2) and not z.any()
    z.fill_(7)
    assert buf.get("z", (3, 2), cpu, torch.int32, zero=True) is z and (z == 7).all()     # not filled again
    assert buf.get("z", (3, 2), cpu) is not z and buf.get("z", (2, 3), cpu, torch.int32) is not z   # one per (name, shape, dtype)


def test_scratch_row_and_flat_buffers():
    """The one Scratch class behind the learners, the controllers and the mixers: `get` hands back the same tensor for the same
    (name, shape, dtype); `get_rows` pads the row pitch to 16 bytes; `get_flat` is keyed by name alone, only grows, and moves the
    shared workspace generation exactly when it REPLACES a buffer (a captured graph holds the old address)."""
    from marl_amd import hostutil, ops
    buf, cpu = hostutil.Scratch(), torch.device("cpu")
    a = buf.get("a", (3, 5), cpu)
    assert buf.get("a", (3, 5), cpu) is a and buf.get("a", [3, 5], cpu, torch.float32) is a
    r = buf.get_rows("r", 7, 78, cpu)
    assert r.shape == (7, 78) and r.dtype == torch.float32 and r.stride() == (80, 1) and r.stride(0) * r.element_size() % 16 == 0
    assert buf.get_rows("r", 7, 78, cpu).data_ptr() == r.data_ptr()
    assert buf.get_rows("r4", 7, 64, cpu).stride() == (64, 1)                   # already a multiple of 4 floats: no pad
    gen = ops.WS.gen
    f = buf.get_flat("f", 10, cpu)
    assert f.dtype == torch.float32 and f.dim() == 1 and f.numel() >= 10 and ops.WS.gen == gen      # a first allocation replaces nothing
    assert buf.get_flat("f", 4, cpu) is f and buf.get_flat("f", 10, cpu) is f and buf.get_flat("f", 0, cpu) is f and ops.WS.gen == gen
    f2 = buf.get_flat("f", 11, cpu)
    assert f2 is not f and f2.numel() >= 11 and ops.WS.gen == gen + 1
    assert buf.get_flat("f", 10, cpu) is f2 and ops.WS.gen == gen + 1           # grow-only
    assert buf.get_flat("h", 0, cpu).numel() >= 1 and buf.get_flat("h", 1, cpu) is not f2 and ops.WS.gen == gen + 1
    ops.WS.retire()
    assert ops.WS.gen == gen + 2


def test_struct_cache_follows_the_pointers_and_not_the_copies():
    """hostutil.cached_struct: one entry per (owner, name), rebuilt exactly when a tracked pointer has moved; a deep copy of the
    owner (a target mixer) starts without entries, and an owner that goes away takes its entries along."""
    import copy
    import gc
    from marl_amd import hostutil

    class At:          # stands for a device tensor at an address
        is_cuda = True

        def __init__(self, ptr):
            self.ptr = ptr

        def data_ptr(self):
            return self.ptr

    class Owner:
        pass
    owner, built = Owner(), []

    def build():
        built.append(object())
        return built[-1]
    a = hostutil.cached_struct(owner, "w", [At(16), At(32)], build)
    assert hostutil.cached_struct(owner, "w", [At(16), At(32)], build) is a and len(built) == 1      # fresh tensor objects, same storage
    b = hostutil.cached_struct(owner, "w", [At(16), At(48)], build)
    assert b is not a and len(built) == 2 and hostutil.cached_struct(owner, "w", [At(16), At(48)], build) is b
    g = hostutil.cached_struct(owner, ("w", True), [At(64), At(80)], build)                          # e.g. the gradient struct
    assert g is not b and len(built) == 3 and hostutil.cached_struct(owner, "w", [At(16), At(48)], build) is b
    twin = copy.deepcopy(owner)
    assert hostutil.cached_struct(twin, "w", [At(16), At(48)], build) is not b and len(built) == 4
    n = len(hostutil._STRUCTS)
    del owner, twin
    gc.collect()
    assert len(hostutil._STRUCTS) == n - 2


DROPIN_TOP = ("rollout", "runner", "controller", "algorithm", "common", "network", "env", "utils", "smac")


def _forget_dropin_modules():
    for m in list(sys.modules):
        if m.split(".")[0] in DROPIN_TOP:
            sys.modules.pop(m, None)


def test_arguments_match_reference_tables():
    from marl_amd.common.arguments import (get_common_args, get_mixer_args, get_coma_args, get_centralv_args,
                                           get_reinforce_args, get_commnet_args, get_g2anet_args, get_RTW_args)
    a = get_mixer_args(get_common_args(["--cuda", "False", "--alg", "qplex"]))
    assert a.cuda is False and a.alg == "qplex"          # the reference would parse "False" as True
    assert a.rnn_hidden_dim == 64 and a.qmix_hidden_dim == 32 and a.double_q and a.target_update_cycle == 200
    assert abs(a.anneal_epsilon - 0.95 / 50000) < 1e-15
    assert a.RTW is False and a.load_model is False
    assert get_RTW_args(a) is None and a.attn_dim == 64 and a.not_self_model is True     # reference :48-53
    b = get_coma_args(get_common_args([]))
    assert (b.critic_dim, b.lr_actor, b.lr_critic, b.td_lambda, b.epsilon_anneal_scale) == (128, 1e-4, 1e-3, 0.8, 'episode')
    c = get_centralv_args(get_common_args([]))
    assert c.td_lambda == 0.8 and c.target_update_cycle == 200 and c.anneal_epsilon == 0.00064
    d = get_reinforce_args(get_common_args([]))
    assert not hasattr(d, "td_lambda") and d.min_epsilon == 0.02 and d.grad_norm_clip == 10
    assert get_commnet_args(get_common_args(["--map", "3m"])).k == 2 and get_commnet_args(get_common_args([])).k == 3
    g = get_g2anet_args(get_common_args([]))
    assert g.attention_dim == 32 and g.hard is True


def test_reference_import_lines_resolve_to_dropin(golden_dir):
    """The LITERAL import statements of the reference's callers (runner.py:3-11, matrix_game_test.py:3-10,
    main.py:1-5; committed as data in tests/golden/reference_import_lines.json) executed with marl_amd/dropin first on
    sys.path, exactly as `python -m marl_amd.dropin <script>` arranges it: every hot-path name must come from marl_amd.
    `smac` (StarCraft II, not vendored by the reference) resolves to the synthetic-env shim when the real package is
    not installed."""
    import json
    from marl_amd.dropin.__main__ import install
    table = json.load(open(os.path.join(golden_dir, "reference_import_lines.json")))
    saved_path = list(sys.path)
    pkg_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "marl_amd") + os.sep
    _forget_dropin_modules()
    try:
        install()
        for script, ent in table.items():
            ns = {}
            for line in ent["imports"]:
                exec(line, ns)          # raises ImportError if a name is missing
            for name, obj in ns.items():
                mod = getattr(obj, "__module__", None) or getattr(obj, "__name__", "")
                if name in ("plt", "np", "os", "__builtins__"):
                    continue
                f = os.path.abspath(getattr(sys.modules.get(str(mod)), "__file__", "") or "")
                assert f.startswith(pkg_dir), (script, name, mod, f)      # defined inside marl_amd/ (dropin stubs included)
        # what main.py:10-12 and matrix_game_test.py:36-37 call right after the imports
        ns = {}
        exec("from common.arguments import get_common_args, get_mixer_args, get_RTW_args", ns)
        argv, sys.argv = sys.argv, ["x"]
        try:
            args = ns["get_common_args"]()
        finally:
            sys.argv = argv
        ns["get_mixer_args"](args)
        ns["get_RTW_args"](args)
        assert args.RTW is False and args.world_loss_weight == 1
    finally:
        sys.path[:] = saved_path
        _forget_dropin_modules()


def test_reference_matrix_game_script_runs_on_dropin():
    """The steps of the reference's matrix_game_test.py, written against its module paths (tests/dropin_matrix_game_flow.py),
    through the launcher.  Without a GPU the run must get as far as the learner's constructor (every import, get_common_args,
    the env, SharedMAC and RolloutWorker resolved to marl_amd) and stop at "no CPU fallback"; with a GPU the same script
    trains (tests/test_gpu_runner.py::test_reference_style_matrix_game_flow_on_dropin)."""
    import re
    import subprocess
    if torch.cuda.is_available():
        import pytest
        pytest.skip("covered by the GPU harness")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "tests", "dropin_matrix_game_flow.py")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:      # nothing lands in the tree
        p = subprocess.run([sys.executable, "-m", "marl_amd.dropin", script], cwd=tmp, capture_output=True, text=True,
                           env=dict(os.environ, PYTHONPATH=root, MPLBACKEND="Agg"), timeout=300)
    assert p.returncode != 0
    assert "Init RolloutWorker" in p.stdout                              # marl_amd.rollout.RolloutWorker.__init__
    assert "QTRANLearner runs only on the MI355X HIP kernels (no CPU fallback)" in p.stderr, p.stderr[-2000:]
    # every frame of the traceback below the launcher lies in the script or in marl_amd
    frames = re.findall(r'File "([^"]+)"', p.stderr)
    i = frames.index(script)
    pkg = os.path.join(root, "marl_amd") + os.sep
    assert frames[i + 1:] and all(f.startswith(pkg) for f in frames[i + 1:]), frames
    assert any(f.endswith(os.path.join("marl_amd", "algorithm", "qtran_learner.py")) for f in frames)


def test_matrix_game_get_episodes_matches_reference(golden_dir):
    from marl_amd.env.single_state_matrix_game import TwoAgentsMatrixGame
    fix = np.load(os.path.join(golden_dir, "rollout.npz"))
    env = TwoAgentsMatrixGame([[8, -12, -12], [-12, 0, 0], [-12, 0, 0]])
    for k, v in env.get_episodes().items():
        np.testing.assert_allclose(np.asarray(v, dtype=np.float64), fix["matrix_get_episodes/" + k])
    r, term, info = env.step([0, 0])
    assert r == 8 and term is True


def test_state_dicts_match_reference_checkpoints(golden_dir):
    """Checkpoint interop: the key names and tensor shapes of the product modules equal
    those of the .pkl files the reference ships under model/{vdn,qplex,qtran_base}/2s3z (table
    extracted by torch.load in the build container; model/qmix/2s3z/*rnn* are RTW-agent files and
    are skipped).  Modules are constructed on CPU - no compute is called."""
    import json
    from marl_amd.network.q_network import RNNQNet
    from marl_amd.network.mixer import QMixMixer, DMAQer, QtranQBase, QtranV, VDNMixer
    table = json.load(open(os.path.join(golden_dir, "reference_checkpoint_shapes.json")))
    def shapes(m):
        return {k: list(v.shape) for k, v in m.state_dict().items()}
    checked = 0
    for path, ref in table.items():
        alg = path.split("/")[1]
        args = seeded.make_args("2s3z", alg)
        kind = os.path.basename(path)
        if "rnn_net" in kind:
            if alg == "qmix":
                continue                                    # RTW agent checkpoints (16 extra keys)
            got = shapes(RNNQNet(96, args))
        elif "v_net" in kind:
            got = shapes(QtranV(args))
        else:
            got = shapes({"vdn": VDNMixer, "qmix": QMixMixer, "qplex": DMAQer, "qtran_base": QtranQBase}[alg](args))
        assert got == ref, path
        checked += 1
    assert checked >= 20


def test_qplex_state_dict_names_for_every_lambda_net_depth():
    """DMAQer's checkpoint names and shapes (in order) equal seeded.qplex_param_shapes - the table the golden generator
    loads strictly into the reference's modules - for adv_hypernet_layers 1, 2 and 3 (mixer.py:116-139: a bare Linear,
    Linear-ReLU-Linear, three Linears), on a map whose state width is a multiple of 4 and on one whose is not.  Any other
    depth raises in both, as the reference does."""
    import pytest
    from marl_amd.network.mixer import DMAQer
    for shape in ("2s3z", "MMM2"):
        for nl in (1, 2, 3):
            args = seeded.make_args(shape, "qplex", adv_hypernet_layers=nl)
            got = [(k, tuple(v.shape)) for k, v in DMAQer(args).state_dict().items()]
            want = seeded.qplex_param_shapes(args)
            assert got == want, (shape, nl)
            K, N = args.num_kernel, args.n_agents
            assert len(want) == 8 + 3 * K * 2 * nl
            last = "" if nl == 1 else ".%d" % (2 * (nl - 1))
            assert dict(want)["si_weight.key_extractors.0%s.weight" % last] == (1, args.state_shape if nl == 1 else 64)
            assert dict(want)["si_weight.action_extractors.%d%s.bias" % (K - 1, last)] == (N,)
        args = seeded.make_args(shape, "qplex", adv_hypernet_layers=4)
        with pytest.raises(Exception):
            DMAQer(args)
        with pytest.raises(ValueError):
            seeded.qplex_param_shapes(args)


def test_launcher_vectorises_an_importable_smac(tmp_path, monkeypatch):
    """`python -m marl_amd.dropin` with a real `smac` on the path: MARL_N_ENVS > 1 swaps smac.env.StarCraft2Env for a
    factory of HostVectorEnv over that many real environments (not called here - it needs the GPU); <= 1 leaves it alone."""
    pkg = tmp_path / "smac"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "env.py").write_text("class StarCraft2Env:\n    pass\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    _forget_dropin_modules()
    from marl_amd.dropin.__main__ import vectorise_real_smac
    import smac.env as se
    real = se.StarCraft2Env
    assert vectorise_real_smac(1) is False and se.StarCraft2Env is real
    assert vectorise_real_smac(8) is True
    assert se.StarCraft2Env is not real and se.StarCraft2Env._marl_real is real
    assert vectorise_real_smac(8) is True and se.StarCraft2Env._marl_real is real      # idempotent
    _forget_dropin_modules()


_OVERLAP = "overlapped rollouts use the whole-rollout kernel, which has no %s head"
_RUNNER_REFUSALS = [
    (dict(RTW=True, alg="qtran_base"), NotImplementedError,
     "RTW with a QTRAN learner is not supported (the reference's QTRANLearner cannot drive an RTW controller)"),
    (dict(RTW=True, alg="qtran_alt"), NotImplementedError,
     "RTW with a QTRAN learner is not supported (the reference's QTRANLearner cannot drive an RTW controller)"),
    (dict(RTW=True, overlap_rollout=True), NotImplementedError, _OVERLAP % "RTW"),
    (dict(world_model=True, RTW=True), ValueError, "world_model and RTW are two different agents: choose one"),
    (dict(world_model=True, alg="qtran_base"), ValueError, "Mixer qtran_base not recognised."),
    (dict(world_model=True, alg="qtran_alt"), ValueError, "Mixer qtran_alt not recognised."),
    (dict(world_model=True, alg="iql"), ValueError, "Mixer iql not recognised."),
    (dict(world_model=True, overlap_rollout=True), NotImplementedError, _OVERLAP % "world-model"),
    (dict(MAIC=True, RTW=True), ValueError, "MAIC, RTW and world_model are three different agents: choose one"),
    (dict(MAIC=True, world_model=True), ValueError, "MAIC, RTW and world_model are three different agents: choose one"),
    (dict(MAIC=True, alg="qtran_base"), NotImplementedError, "MAIC with a QTRAN learner is not supported"),
    (dict(MAIC=True, alg="qtran_alt"), NotImplementedError, "MAIC with a QTRAN learner is not supported"),
    (dict(MAIC=True, overlap_rollout=True), NotImplementedError, _OVERLAP % "MAIC"),
    # the first check that fires wins: the RTW row runs before the world-model row, world-model's before MAIC's
    (dict(RTW=True, world_model=True, alg="qtran_base"), NotImplementedError,
     "RTW with a QTRAN learner is not supported (the reference's QTRANLearner cannot drive an RTW controller)"),
    (dict(RTW=True, world_model=True, overlap_rollout=True), NotImplementedError, _OVERLAP % "RTW"),
    (dict(world_model=True, MAIC=True, alg="qtran_alt"), ValueError, "Mixer qtran_alt not recognised."),
    (dict(world_model=True, MAIC=True, overlap_rollout=True), NotImplementedError, _OVERLAP % "world-model"),
]


@pytest.mark.parametrize("over,exc,text", _RUNNER_REFUSALS, ids=["+".join("%s=%s" % kv for kv in o.items())
                                                                 for o, _, _ in _RUNNER_REFUSALS])
def test_runner_refusals_keep_type_and_text(over, exc, text, monkeypatch):
    """every refusal of an agent switch (runner.py's module docstring) with its exact exception type and text, raised
    before a controller, a rollout worker or a replay buffer is built"""
    from marl_amd import runner
    built = []
    for name in ("RolloutWorker", "ReplayBuffer"):
        monkeypatch.setattr(runner, name, lambda *a, _n=name, **k: built.append(_n))
    args = seeded.make_args("2s3z", "qmix")
    args.__dict__.update(over)
    with pytest.raises(exc) as info:
        runner.Runner(None, None, args)
    assert type(info.value) is exc and str(info.value) == text
    assert built == []


@pytest.mark.parametrize("cls,head", [("RTWMAC", "RTW"), ("SharedMACWithState", "world-model"), ("MAICMAC", "MAIC")])
def test_launch_episodes_refuses_a_controller_with_a_head(cls, head):
    from marl_amd.controller import share_params
    from marl_amd.rollout import RolloutWorker
    worker = RolloutWorker.__new__(RolloutWorker)
    worker.env, worker.mac = None, None
    mac_cls = getattr(share_params, cls)
    text = "launch_episodes runs the whole-rollout kernel, which has no %s head: use generate_episodes" % head
    for kw in (dict(mac=mac_cls.__new__(mac_cls)), dict()):
        worker.mac = None if kw else mac_cls.__new__(mac_cls)
        with pytest.raises(RuntimeError) as info:
            worker.launch_episodes(**kw)
        assert str(info.value) == text

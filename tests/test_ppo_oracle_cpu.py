"""MAPPO on the CPU: properties of tests/ppo_oracle.py (the float64 restatement the GPU tests hold marl_ppo_loss_bwd,
marl_masked_standardize and PPOLearner to), the conditions every learner run of the GPU file must meet (no ReLU at its kink, no
ratio at a clip edge, clipped rows where the clip is test-sized), the float32 yardstick of every tensor that file compares, and the
launcher's table and refusals."""
import numpy as np
import pytest
import torch

import policy_oracle as po
import ppo_oracle as pp


def _case(shape, eps):
    rows = pp.kernel_case(shape, eps, pp.kernel_seed(shape))
    B, T, N, A = shape
    t = lambda k: torch.tensor(rows[k].astype(np.float64))
    return rows, (t("logits").view(B * T, N, A), t("avail").view(B * T, N, A), torch.tensor(rows["u"].astype(np.int64)).view(B * T, N),
                  t("adv"), t("logp_old").view(B * T, N), t("padded"))


@pytest.mark.parametrize("eps", pp.KERNEL_EPS)
@pytest.mark.parametrize("shape", pp.KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_cases_hold_their_classes_and_their_distance(shape, eps):
    """kernel_case asserts both itself; the shapes with fewer than 16 live rows hold what they can"""
    rows, _ = _case(shape, eps)
    few = {(3, 1, 2, 3): ("unclipped",), (2, 3, 2, 30): ("unclipped", "clipped_high_pos", "below_low_pos")}
    have = tuple(c for c in pp.CLASSES if rows["classes"][c] > 0)
    assert have == few.get(shape, pp.CLASSES), (shape, rows["classes"])
    assert np.isnan(rows["logp_old"][rows["pad_rows"]]).all() and np.isfinite(rows["logp_old"][~rows["pad_rows"]]).all()


@pytest.mark.parametrize("beta", [0.0, 0.01])
@pytest.mark.parametrize("eps", pp.KERNEL_EPS)
def test_gradient_gate_is_autograd_of_the_minimum_clamp_form(eps, beta):
    """- m (clipped ? 0 : adv rho) d log pi(u) / dz - beta m dH / dz against autograd of - sum m min(rho adv, clamp(rho) adv) -
    beta sum m H, in float64: 1e-12 relative"""
    for shape in pp.KERNEL_SHAPES[:5]:
        _, (z, a, u, adv, old, padded) = _case(shape, eps)
        z = z.clone().requires_grad_(True)
        out = pp.numerator(z, a, u, adv, old, padded, eps, beta, pp.KERNEL_CLIP)
        (auto,) = torch.autograd.grad(out["num"], z, retain_graph=True)
        coef = pp.gate_coefficient(out, padded)
        w = (1.0 - padded)[:, None] * out["live"].to(torch.float64)
        (hand,) = torch.autograd.grad((coef * out["logp"]).sum() - beta * (w * out["ent"]).sum(), z)
        assert float((auto - hand).abs().max()) <= 1e-12 * float(auto.abs().max())
        assert bool((auto[~out["live"]] == 0).all())
        if out["clipped"].any() and beta == 0.0:
            assert float(auto[out["clipped"]].abs().max()) == 0.0                 # a clipped row has no surrogate gradient
        assert float(out["nclip"]) == float(out["clipped"].sum()) and int(out["clipped"].sum()) == \
            rowsum(pp.row_classes(out, a, pp.KERNEL_CLIP), ("clipped_high_pos", "clipped_low_neg"))


def rowsum(counts, keys):
    return sum(counts[k] for k in keys)


@pytest.mark.parametrize("eps", pp.KERNEL_EPS)
def test_first_pass_is_the_plain_policy_gradient_of_the_advantage(eps):
    """logp_old None: rho = 1, nothing is clipped, and the gradient is policy_oracle's actor gradient with G = adv and no baseline;
    the numerator's value is the surrogate's, - sum m adv over the rows with a policy (not - sum m adv log pi)"""
    for shape in pp.KERNEL_SHAPES[:5]:
        _, (z, a, u, adv, old, padded) = _case(shape, eps)
        z = z.clone().requires_grad_(True)
        out = pp.numerator(z, a, u, adv, None, padded, eps, 0.0, pp.KERNEL_CLIP)
        (g,) = torch.autograd.grad(out["num"], z)
        num0, logp0, den0 = po.actor_numerator(z, a, u, adv, torch.zeros_like(adv), padded, eps)
        (g0,) = torch.autograd.grad(num0, z)
        assert float((g - g0).abs().max()) <= 1e-12 * float(g0.abs().max())
        assert not out["clipped"].any() and bool((out["rho"] == 1.0).all()) and float(out["den"]) == float(den0)
        value = -((1.0 - padded)[:, None] * adv[:, None] * out["live"]).sum()      # rows with one available action included
        np.testing.assert_allclose(float(out["num"].detach()), float(value), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(out["logp"].detach().numpy(), (logp0 * (1.0 - padded)[:, None]).detach().numpy(), rtol=0, atol=1e-14)


@pytest.mark.parametrize("rows,how", [(1, "rand"), (2, "rand"), (65, "rand"), (4097, "rand"), (4097, "allpad"), (4097, "one"), (4097, "far")])
def test_standardize_against_numpy(rows, how):
    x, padded = pp.standardize_case(rows, how)
    out, mean, var, M = pp.standardize(torch.tensor(x.astype(np.float64)), torch.tensor(padded.astype(np.float64)))
    live = padded == 0
    assert M == live.sum() and bool((out.numpy()[~live] == 0).all())
    if M == 0:
        assert not out.numpy().any() and (mean, var) == (0.0, 0.0)
        return
    xl = x[live].astype(np.float64)
    np.testing.assert_allclose(mean, xl.mean(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(var, xl.var(), rtol=1e-11, atol=1e-13)          # numpy's var is around the mean as well
    np.testing.assert_allclose(out.numpy()[live], (xl - xl.mean()) / (xl.std() + 1e-5), rtol=1e-11, atol=1e-12)


# ---------------------------------------------------------------------------------------------------- the learner runs
@pytest.mark.parametrize("key", list(pp.RUNS))
def test_runs_and_float32_yardstick(key):
    """Every learner run of the GPU file: no ReLU pre-activation that carries a gradient within 1e-5 of zero and no ratio within
    1e-4 of a clip edge in any pass (float64 and float32 then take the same branches, and so does the GPU); clipped rows of both
    signs beside unclipped ones where the clip is test-sized; and the oracle in float32 against float64 stays under a quarter of
    1e-4 * max|ref| on every tensor, except those pp.F32_EXCEPTIONS lists with their float32-oracle error."""
    ref, f32 = pp.run_updates(key, torch.float64), pp.run_updates(key, torch.float32)
    assert ref["near_zero"] == 0, "a ReLU pre-activation within 1e-5 of zero: choose another seed"
    assert ref["clip_margin"] >= 1e-4, ref["clip_margin"]
    assert ref["classes"] == f32["classes"]
    name, clip, epochs = pp.RUNS[key][0], pp.RUNS[key][2], pp.RUNS[key][3]
    print(key, "classes of update 0:", [tuple(c.values()) for c in ref["classes"]], "margin %.2e" % ref["clip_margin"])
    if key in pp.CLIPPED_RUNS:
        assert clip == pp.TEST_CLIP[name] and epochs == 3
        c = ref["classes"][pp.CLIPPED_PASS[name]]
        assert c["unclipped"] > 0 and c["clipped_high_pos"] > 0 and c["clipped_low_neg"] > 0, c
    else:
        assert clip == 0.2
    worst = {}
    for k, r in ref.items():
        if k in ("near_zero", "clip_margin", "classes"):
            continue
        r = np.asarray(r, dtype=np.float64)
        err = float(np.abs(np.asarray(f32[k], dtype=np.float64) - r).max())
        scale = float(np.abs(r).max())
        bound = 0.25 * 1e-4 * scale + 1e-7
        if err > 0.1 * bound:
            print("%-12s %-44s f32 err %.3e  max|ref| %.3e  share of 1e-4 max|ref| %.3f" % (key, k, err, scale, err / (1e-4 * scale + 1e-30)))
        exc = pp.F32_EXCEPTIONS.get((key, k))
        if exc is not None:
            # no more than about the recorded size.  No lower limit: where RMSprop's step hangs on the rounding of a gradient near
            # zero, the float32 error depends on the host's summation order
            assert err <= 1.5 * exc, (k, err, exc)
        elif err > bound:
            worst[k] = (err, bound)
    assert not worst, worst
    assert not [k for k in pp.F32_EXCEPTIONS if k[0] == key and k[1] not in ref]


def test_matrix_last_pass_holds_no_clipped_row():
    """what ppo_oracle.CLIPPED_PASS says of the matrix game: the third pass finds every ratio inside the test-sized clip again"""
    ref = pp.run_updates("matrix")
    assert pp.CLIPPED_PASS["matrix"] == 1 and ref["classes"][2] == dict(zip(pp.CLASSES, (18, 0, 0, 0, 0)))


# ---------------------------------------------------------------------------------------------------- launcher
@pytest.fixture
def fake_env(monkeypatch):
    from marl_amd import main
    made = []

    def env(*a, **k):
        made.append(1)
        return type("E", (), {"get_env_info": lambda s: dict(n_actions=11, n_agents=5, state_shape=120, obs_shape=80, episode_limit=120)})()
    monkeypatch.setattr(main, "SyntheticSMACEnv", env)
    return made


def test_launcher_builds_the_mappo_table(fake_env):
    from marl_amd import main
    args, _ = main.build(["--alg", "mappo"])
    assert (args.lr_actor, args.lr_critic, args.critic_dim, args.epsilon, args.epsilon_anneal_scale) == (1e-4, 1e-3, 128, 0.5, "episode")
    assert (args.td_lambda, args.ppo_clip, args.ppo_epochs, args.ppo_norm_adv, args.optimizer) == (0.95, 0.2, 5, True, "RMS")
    args, _ = main.build(["--alg", "mappo", "--ppo_clip", "0.1", "--ppo_epochs", "3", "--ppo_norm_adv", "False", "--td_lambda", "0.5",
                          "--optimizer", "Adam"])
    assert (args.td_lambda, args.ppo_clip, args.ppo_epochs, args.ppo_norm_adv, args.optimizer) == (0.5, 0.1, 3, False, "Adam")
    args, _ = main.build(["--alg", "mappo", "--ppo_epochs", "1"])
    assert (args.ppo_clip, args.ppo_epochs, args.ppo_norm_adv) == (0.2, 1, True)
    args, _ = main.build(["--alg", "central_v"])                      # the other tables are as they were
    assert args.td_lambda == 0.8 and args.ppo_clip is None and args.ppo_epochs is None and args.ppo_norm_adv is None


def test_launcher_refusals(fake_env, tmp_path):
    from marl_amd import main
    from marl_amd.runner import Runner
    from marl_amd.utils.logging import Logger
    for argv in (["--ppo_clip", "0"], ["--ppo_clip", "1"], ["--ppo_clip", "-0.2"], ["--ppo_clip", "1.5"], ["--ppo_epochs", "0"],
                 ["--ppo_epochs", "-2"]):
        with pytest.raises(ValueError, match="ppo_"):
            main.build(["--alg", "mappo"] + argv)
    for alg in ("mappo+commnet", "mappo+g2anet"):
        with pytest.raises(ValueError, match="central_v, coma or reinforce"):
            main.build(["--alg", alg])
    assert fake_env == []                                               # no environment was made by any of them
    args, env = main.build(["--alg", "mappo", "--MAIC", "True", "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "model")])
    with pytest.raises(ValueError, match="not with MAIC"):
        main.make_runner(args, env, Logger())
    args, env = main.build(["--alg", "mappo", "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "model")])
    for sw in ("RTW", "world_model"):
        setattr(args, sw, True)
        with pytest.raises(ValueError, match="not with " + sw):
            main.make_runner(args, env, Logger())
        setattr(args, sw, False)
    with pytest.raises(ValueError, match="learner mappo cannot find!"):      # the runner's own tables do not hold the name
        Runner(env, Logger(), args)


def test_learner_settings_are_checked_before_anything_is_built():
    from marl_amd.algorithm.ppo import PPOLearner, ppo_settings_of
    from marl_amd.controller.share_params import PolicyMAC
    args, _, _ = pp.run_case("2s3z")
    assert ppo_settings_of(args) == (pp.TEST_CLIP["2s3z"], 3, True)
    mac = PolicyMAC(args)
    for field, bad in (("ppo_clip", 0.0), ("ppo_clip", 1.0), ("ppo_clip", float("nan")), ("ppo_epochs", 0), ("ppo_epochs", 2.5), ("td_lambda", 1.5)):
        keep = getattr(args, field)
        setattr(args, field, bad)
        with pytest.raises(ValueError):
            PPOLearner(mac, args)
        setattr(args, field, keep)
    assert not hasattr(mac.agent, "_flat")                # nothing was built
    for field in ("ppo_clip", "ppo_epochs", "ppo_norm_adv"):
        delattr(args, field)
    assert ppo_settings_of(args) == (0.2, 5, True)

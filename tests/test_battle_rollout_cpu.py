"""The host side of the battle whole-rollout kernel (csrc/battle_rollout.hip): the --battle_fused switch, the launch plan and the
shapes it places.  The plan functions are host code, so the library answers on a machine without a GPU."""
import pytest

from marl_amd import ops
from marl_amd.common.arguments import get_common_args
from marl_amd.env.battle import BATTLE_MAPS, battle_shapes

LDS_CAP = 160 * 1024
ENVS = (1, 3, 65, 257, 1281, 20000)


def test_the_switch_parses_and_defaults_to_off():
    assert get_common_args(["--env", "battle", "--battle_fused", "True"]).battle_fused is True
    assert get_common_args(["--env", "battle", "--battle_fused", "False"]).battle_fused is False
    assert get_common_args(["--env", "battle"]).battle_fused is False


def _lds_of_row_tiles(N, O, A, last_action):
    """the plan's LDS bytes as a function of its row tiles: affine in them, so two plans with different row tiles give the line"""
    seen = {}
    for E in (1, 256 * 16, 256 * 32, 256 * 48, 256 * 64, 256 * 128):
        _, _, rt, lds = ops.battle_rollout_plan(E, N, O, A, last_action, True)
        seen[rt] = lds
    (r0, l0), (r1, l1) = sorted(seen.items())[:2]
    per = (l1 - l0) // (r1 - r0)
    assert (l1 - l0) % (r1 - r0) == 0 and all(l == l0 + per * (r - r0) for r, l in seen.items())
    return lambda rt: l0 + per * (rt - r0)


@pytest.mark.parametrize("last_action", [True, False])
@pytest.mark.parametrize("name", sorted(BATTLE_MAPS))
def test_plan_invariants(name, last_action):
    N, O, S, A, T = battle_shapes(name)
    lds_of = _lds_of_row_tiles(N, O, A, last_action)
    rt_cap = max(rt for rt in range(1, 9) if lds_of(rt) <= LDS_CAP)         # the row tiles 160 KB hold, eight at the most
    epw_cap = 16 * rt_cap // N
    for E in ENVS:
        wgs, epw, rt, lds = ops.battle_rollout_plan(E, N, O, A, last_action, True)
        assert epw >= 1 and epw * N <= 16 * rt and rt <= 8 and lds <= LDS_CAP, (E, wgs, epw, rt, lds)
        assert rt == (epw * N + 15) // 16                                   # no empty row tile
        assert wgs == (E + epw - 1) // epw
        assert epw == min((E + 255) // 256, epw_cap), (E, epw, epw_cap)      # one workgroup per CU until the LDS cap binds
    if name == "3m":
        assert ops.battle_rollout_plan(20000, N, O, A, last_action, True)[1] == epw_cap < (20000 + 255) // 256


def test_supported_shapes():
    for name in BATTLE_MAPS:
        N, O, S, A, T = battle_shapes(name)
        assert ops.battle_rollout_supported(N, O, A)
    assert not ops.battle_rollout_supported(27, 200, 33)       # A = 33: past the two action tiles (and past the sixteen units of a side)
    assert not ops.battle_rollout_supported(0, 10, 6)
    with pytest.raises(Exception):
        ops.battle_rollout_plan(64, 0, 10, 6)

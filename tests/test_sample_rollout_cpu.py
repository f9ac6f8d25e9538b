"""The float64 sampled rollout of every case of tests/sample_rollout_cases.py on its own: the GPU half
(tests/test_gpu_sample_rollout.py) excludes draws that lie within SAMPLER_EXCLUDE of a float64 CDF boundary and, where two fp32
paths are compared, every cell after such a draw of its row.  Both exclusions are capped there; here the oracle alone is held to half
of the first cap and to half of the second (2.5 % against 5 %), so the GPU tests cannot pass by excluding what they should check.

Expected: a draw lies within 1e-5 of one of at most A - 1 inner boundaries with probability about 2e-5 (A - 1) <= 6.2e-4, a cell is
not prefix-clean with about T times that, <= 0.5 % at these T.  Achieved with the seeds of sample_rollout_cases (env 5, draws 77,
agent 11), near draws / unclean cells / live cells of the episodes 0 and 1:
    2s3z-e0 0/0/1100, 0/0/1195;  2s3z-e03 1/8/1100, 0/0/1195;  2s3z-e1 0/0/1100, 1/3/1195;  2s3z-sharp 0/0/1100, 0/0/1195 (logit
    gaps up to 141);  2s3z-700 2/5/12360, 4/7/12120;  2s3z-noact 0/0/1100, 0/0/1195;  a16 3/4/16992, 5/15/16720;
    MMM2 0/0/1750, 0/0/1660;  a32 4/9/4248, 3/6/4180;  n49 1/3/5145, 1/4/5047;  n1 0/0/2472, 1/2/2424
the worst shares: 9.4e-4 of the draws (a32; the cap here is 2.5e-3) and 0.73 % of the cells (2s3z-e03; 2.5 %).
"""
import numpy as np
import pytest

import policy_oracle as po
import sample_rollout_cases as src


@pytest.mark.parametrize("c", src.CASES, ids=src.CASE_IDS)
def test_oracle_rollout_meets_both_caps(c):
    for episode in (0, 1):
        out = src.rollout64(c, episode=episode)
        live3 = np.broadcast_to(out["live"][..., None], out["u"].shape)
        n_live = int(live3.sum())
        assert n_live > 0 and (out["u"][live3] >= 0).all() and (out["u"][~live3] == -1).all()
        near = int(((out["margin"] < po.SAMPLER_EXCLUDE) & live3).sum())
        unclean = int((~src.prefix_clean(out["margin"], out["live"]) & live3).sum())
        print(c["name"], episode, "near", near, "unclean", unclean, "live", n_live, "gap %.1f" % out["gap"])
        if c["name"] == "2s3z-sharp":
            assert out["gap"] > 80.0          # the case is there for the exponent clamp
        assert near < po.SAMPLER_CAP / 2 * n_live
        assert unclean < 0.025 * n_live


def test_prefix_clean_on_a_hand_made_array():
    big = 1.0
    margin = np.full((2, 4, 3), big)
    live = np.array([[True, True, True, True], [True, True, False, False]])
    margin[0, 1, 2] = 1e-7                  # row (0, 2): unclean from step 1 on
    margin[0, 3, 0] = 9.9e-6                # row (0, 0): only the last step
    margin[1, 0, 1] = po.SAMPLER_EXCLUDE    # at the bound: clean
    margin[1, 2, 0] = 0.0                   # a padded step: does not count
    got = src.prefix_clean(margin, live)
    want = np.ones((2, 4, 3), bool)
    want[0, 1:, 2] = False
    want[0, 3, 0] = False
    assert got.shape == (2, 4, 3) and (got == want).all()

"""TEST INFRASTRUCTURE ONLY -- the data-parallel VecNormalize rule on the CPU: oracle/vecnorm_ref.py's
VecNormalizeRef over all R * L lanes, with every statistics update taken through the product's rule
(gym_puzzles_amd.vec_env moments_local_ref per rank, moments_combine_ref in rank order, rms_merge_ref).
tests/test_norm_dist.py holds it to the exact rule of tests/vecnorm_exact.py; tests/test_ddp_norm_gpu.py
replays the device's gathered parts through the same functions.  Never imported by the product.
"""
from __future__ import annotations

import numpy as np

from gym_puzzles_amd.vec_env import moments_combine_ref, moments_local_ref, rms_merge_ref
from oracle.vecnorm_ref import RunningMeanStd, VecNormalizeRef


class DistRunningMeanStd(RunningMeanStd):
    """RunningMeanStd whose batch is the lanes of ``world`` ranks, ``lanes_per_rank`` each, in rank order."""

    def __init__(self, world, lanes_per_rank, shape=()):
        super().__init__(shape)
        self.world, self.lanes_per_rank = world, lanes_per_rank
        self.parts = None            # the gathered parts of the last update, [world, 2 C]

    def update(self, x) -> None:
        L = self.lanes_per_rank
        x = np.asarray(x, np.float64)
        assert x.shape[0] == self.world * L
        self.parts = np.stack([moments_local_ref(x[r * L:(r + 1) * L]) for r in range(self.world)])
        bm, bv, n = moments_combine_ref(self.parts, L)
        if x.ndim == 1:
            bm, bv = bm[0], bv[0]
        self.mean, self.var, self.count = rms_merge_ref(self.mean, self.var, self.count, bm, bv, n)


class DistVecNormalizeRef(VecNormalizeRef):
    """One VecNormalize over ``world * lanes_per_rank`` lanes whose statistics follow the data-parallel rule."""

    def __init__(self, world, lanes_per_rank, obs_dim, **kw):
        super().__init__(world * lanes_per_rank, obs_dim, **kw)
        self.obs_rms = DistRunningMeanStd(world, lanes_per_rank, (obs_dim,))
        self.ret_rms = DistRunningMeanStd(world, lanes_per_rank, ())


def replay_update(stats: dict, parts, L: int, obs: bool, ret: bool) -> dict:
    """The statistics (a DeviceVecNormalize.get_stats() dict) after one call whose gathered ``parts`` are
    given: the obs columns merged when ``obs``, the returns column when ``ret``, by the rule."""
    D = len(stats["obs_mean"])
    out = {k: np.array(v, np.float64) for k, v in stats.items()}
    bm, bv, n = moments_combine_ref(np.asarray(parts, np.float64)[:, :2 * (D + 1)], L)
    if obs:
        out["obs_mean"], out["obs_var"], out["obs_count"] = rms_merge_ref(out["obs_mean"], out["obs_var"], out["obs_count"],
                                                                          bm[:D], bv[:D], n)
    if ret:
        out["ret_mean"], out["ret_var"], out["ret_count"] = rms_merge_ref(out["ret_mean"], out["ret_var"], out["ret_count"],
                                                                          bm[D], bv[D], n)
    return out


def two_rank_nonfinite_inputs():
    """130 lanes for two ranks of 65: clean lanes for rank 0 and vecnorm_exact.nonfinite_inputs() as rank 1's
    (a NaN in column 1 at step 2, +inf in column 2 at step 3, a NaN reward at step 4), so every non-finite
    value enters on rank 1 only."""
    import vecnorm_exact as ve
    bad, clean = ve.nonfinite_inputs(), ve.make_inputs(65, 3, 3003)
    cat = lambda a, b: None if a is None else np.concatenate([a, b])  # noqa: E731
    inputs = {"L": 130, "D": 3, "obs0": cat(clean["obs0"], bad["obs0"]),
              "steps": [{k: cat(c[k], b[k]) for k in c} for c, b in zip(clean["steps"], bad["steps"])]}
    assert not any(np.isnan(s["obs"][:65]).any() or np.isnan(s["reward"][:65]).any() for s in inputs["steps"])
    return inputs


def column0(inputs):
    """The inputs restricted to obs column 0, with NaN rewards replaced by 0 (they do not reach that column)."""
    out = {"L": inputs["L"], "D": 1, "obs0": inputs["obs0"][:, :1].copy(), "steps": []}
    for s in inputs["steps"]:
        out["steps"].append({"obs": s["obs"][:, :1].copy(), "term": s["term"][:, :1].copy(), "done": s["done"],
                             "reward": np.where(np.isnan(s["reward"]), np.float32(0), s["reward"]), "reward64": None})
    return out

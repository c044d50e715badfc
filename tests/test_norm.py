"""On-device VecNormalize + Monitor statistics (mrp_norm.hip) and the numpy
restatement of stable-baselines3's algorithm (oracle/vecnorm_ref.py; SB3 is not installed, so
parity with SB3 itself is unpinned).

The contract (tests/vecnorm_exact.py: the rule over Fractions, bounds derived from the inputs):
statistics within the derived bound of the exact moments, float32 outputs within half a float32
ulp of the exact value plus the propagated bound, counts and Monitor bit-exact, NaN propagated as
numpy does.  Here, on the CPU, the restatement is held to it and deliberately wrong variants of
it are shown to be rejected; tests/test_norm_gpu.py holds the device to it on the same inputs.

The env-driven GPU tests below cover the wiring with Batch at 1024 lanes of v0 and compare the
device with the restatement: batch moments are float64 on both sides but summed in a different
order (a 256-thread tree on the device, row after row in numpy), so statistics agree to rtol 1e-10
and normalised float32 outputs to 2 ulp-scale (rtol 1e-6, atol 1e-6) there.  Monitor episode
returns are sequential float64 sums of the same rewards in the same order: bit-exact.
"""
from __future__ import annotations

import os

import numpy as np
import pytest


def test_running_mean_std_merge_is_batch_invariant():
    from oracle.vecnorm_ref import RunningMeanStd
    rs = np.random.RandomState(0)
    x = rs.normal(3.0, 2.0, size=(600, 5))
    a, b = RunningMeanStd((5,)), RunningMeanStd((5,))
    a.update(x)
    for k in range(0, 600, 150):
        b.update(x[k:k + 150])
    np.testing.assert_allclose(a.mean, b.mean, rtol=1e-12)
    np.testing.assert_allclose(a.var, b.var, rtol=1e-9)
    assert a.count == pytest.approx(600 + 1e-4) and b.count == pytest.approx(600 + 1e-4)
    # the epsilon-count prior barely moves the batch moments
    np.testing.assert_allclose(a.mean, x.mean(0), rtol=1e-6)
    np.testing.assert_allclose(a.var, x.var(0), rtol=1e-5)


def test_vecnormalize_restatement_semantics():
    from oracle.vecnorm_ref import VecNormalizeRef
    n = VecNormalizeRef(4, 2, clip_obs=1.0)
    o = n.reset(np.array([[0, 0], [1, 1], [2, 2], [3, 3]], np.float32))
    assert o.dtype == np.float32 and np.all(np.abs(o) <= 1.0)
    r = np.array([1, 2, 3, 4], np.float32)
    _, rn, _, er, el = n.step(np.zeros((4, 2), np.float32), r, np.array([0, 1, 0, 0], np.uint8))
    np.testing.assert_allclose(n.returns, [1, 0, 3, 4])          # returns[done] = 0 after the update
    assert er[1] == 2.0 and el[1] == 1 and n.ep_len[1] == 0 and n.ep_len[0] == 1
    assert np.all(np.abs(rn) <= 10.0)
    n.training = False
    before = n.obs_rms.mean.copy()
    n.step(np.ones((4, 2), np.float32), r, np.zeros(4, np.uint8))
    np.testing.assert_array_equal(n.obs_rms.mean, before)      # frozen statistics in evaluation


@pytest.mark.gpu
def test_device_vecnormalize_matches_restatement(gpu_lib):
    import torch

    from gym_puzzles_amd import Batch, DeviceVecNormalize
    from oracle.vecnorm_ref import VecNormalizeRef
    lanes, steps = 1024, 120
    dev = torch.device("cuda", 0)
    b = Batch(0, lanes, seed=21)
    b.set_auto_reset(True)
    b.set_time_limit(40)                 # every lane finishes episodes inside the run
    O = b.obs_dim
    norm = DeviceVecNormalize(lanes, O, 0)
    ref = VecNormalizeRef(lanes, O)
    obs0 = torch.from_numpy(b.reset().copy()).to(dev)
    nobs = torch.zeros_like(obs0)
    norm.reset(obs0, nobs)
    np.testing.assert_allclose(nobs.cpu().numpy(), ref.reset(obs0.cpu().numpy()), rtol=1e-6, atol=1e-6)
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    obs, rew, done, trunc, term = z(lanes, O), z(lanes), z(lanes, dt=torch.uint8), z(lanes, dt=torch.uint8), z(lanes, O)
    nrew, nterm, epr, epl = z(lanes), z(lanes, O), z(lanes, dt=torch.float64), z(lanes, dt=torch.int32)
    s = torch.cuda.current_stream(dev)
    b.set_stream(s.cuda_stream)
    n_done = 0
    for t in range(steps):
        b.step_device(0, obs.data_ptr(), rew.data_ptr(), done.data_ptr(), trunc.data_ptr(), 0, term.data_ptr())
        norm.step(obs, rew, done, nobs, nrew, term, nterm, epr, epl)
        ho, hr, hd, ht = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy(), term.cpu().numpy()
        o, r, tt, er, el = ref.step(ho, hr, hd, ht)
        np.testing.assert_allclose(nobs.cpu().numpy(), o, rtol=1e-6, atol=1e-6, err_msg=f"obs @{t}")
        np.testing.assert_allclose(nrew.cpu().numpy(), r, rtol=1e-6, atol=1e-6, err_msg=f"reward @{t}")
        m = hd.astype(bool)
        n_done += int(m.sum())
        if m.any():
            np.testing.assert_allclose(nterm.cpu().numpy()[m], tt[m], rtol=1e-6, atol=1e-6, err_msg=f"terminal obs @{t}")
            np.testing.assert_array_equal(epr.cpu().numpy()[m], er[m], err_msg=f"episode return @{t}")
            np.testing.assert_array_equal(epl.cpu().numpy()[m], el[m], err_msg=f"episode length @{t}")
    assert n_done >= 2 * lanes
    st = norm.get_stats()
    np.testing.assert_allclose(st["obs_mean"], ref.obs_rms.mean, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(st["obs_var"], ref.obs_rms.var, rtol=1e-10)
    np.testing.assert_allclose([st["obs_count"], st["ret_count"]], [ref.obs_rms.count, ref.ret_rms.count], rtol=1e-15)
    np.testing.assert_allclose([st["ret_mean"], st["ret_var"]], [ref.ret_rms.mean, ref.ret_rms.var], rtol=1e-10)
    # evaluation mode freezes the statistics; set/get round-trips them
    norm.training = False
    b.step_device(0, obs.data_ptr(), rew.data_ptr(), done.data_ptr(), trunc.data_ptr(), 0, term.data_ptr())
    norm.step(obs, rew, done, nobs, nrew, term, nterm, epr, epl)
    st2 = norm.get_stats()
    np.testing.assert_array_equal(st2["obs_mean"], st["obs_mean"])
    norm.set_stats(st)
    np.testing.assert_array_equal(norm.get_stats()["obs_var"], st["obs_var"])
    norm.close()
    b.close()


@pytest.mark.gpu
def test_vecnormalize_wrapper_sb3_surface(gpu_lib):
    from gym_puzzles_amd import MultiRobotPuzzleVecEnv, MultiRobotPuzzleVecNormalize
    env = MultiRobotPuzzleVecNormalize(MultiRobotPuzzleVecEnv("MultiRobotPuzzle-v0", 64, seed=5, max_episode_steps=20))
    o = env.reset()
    assert o.shape == (64, 28) and o.dtype == np.float32
    rs = np.random.RandomState(1)
    eps = 0
    for _ in range(45):
        o, r, d, infos = env.step(rs.uniform(-1, 1, size=(64, 6)).astype(np.float32))
        assert np.all(np.abs(o) <= 10.0) and np.all(np.abs(r) <= 10.0)
        for i in np.nonzero(d)[0]:
            eps += 1
            ep = infos[i]["episode"]
            assert 1 <= ep["l"] <= 20 and infos[i]["terminal_observation"].shape == (28,)
    assert eps >= 2 * 64
    env.close()


@pytest.mark.gpu
def test_monitor_sums_the_float64_rewards(gpu_lib):
    """Monitor's episode return sums the env's float64 rewards (SB3's Monitor sums the Python
    floats step() returns), not their float32 roundings: mrp_step_device_ex's reward64 feeds
    mrp_norm_step_device_ex, checked against a sequential float64 sum on the host."""
    import torch

    from gym_puzzles_amd import Batch, DeviceVecNormalize
    lanes, steps = 256, 60
    dev = torch.device("cuda", 0)
    b = Batch(0, lanes, seed=8)
    b.set_auto_reset(True)
    b.set_time_limit(20)
    O = b.obs_dim
    norm = DeviceVecNormalize(lanes, O, 0)
    obs0 = torch.from_numpy(b.reset().copy()).to(dev)
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    nobs = torch.zeros_like(obs0)
    norm.reset(obs0, nobs)
    obs, rew, rew64, done = z(lanes, O), z(lanes), z(lanes, dt=torch.float64), z(lanes, dt=torch.uint8)
    nrew, epr, epl = z(lanes), z(lanes, dt=torch.float64), z(lanes, dt=torch.int32)
    b.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    acc = np.zeros(lanes, np.float64)
    n_done = 0
    for _ in range(steps):
        b.step_device(0, obs.data_ptr(), rew.data_ptr(), done.data_ptr(), 0, 0, 0, d_reward64=rew64.data_ptr())
        norm.step(obs, rew, done, nobs, nrew, ep_return=epr, ep_len=epl, reward64=rew64)
        r64, r32, d = rew64.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy().astype(bool)
        np.testing.assert_array_equal(r64.astype(np.float32), r32)
        acc = acc + r64
        if d.any():
            np.testing.assert_array_equal(epr.cpu().numpy()[d], acc[d])
            acc[d] = 0.0
            n_done += int(d.sum())
    assert n_done >= 2 * lanes
    norm.close()
    b.close()


@pytest.mark.gpu
def test_vecnormalize_save_load_and_eval_flags(gpu_lib, tmp_path):
    """train/test.py:66-68's flow: VecNormalize.load(path, env); env.training = False;
    env.norm_reward = False.  The loaded wrapper carries the saved statistics bit for bit, stops
    updating them once training is off, and returns raw rewards with norm_reward off (raw obs with
    norm_obs off) while the normalised values stay what the statistics give."""
    from gym_puzzles_amd import MultiRobotPuzzleVecEnv, MultiRobotPuzzleVecNormalize
    rs = np.random.RandomState(3)
    act = lambda: rs.uniform(-1, 1, size=(64, 6)).astype(np.float32)  # noqa: E731
    env = MultiRobotPuzzleVecNormalize(MultiRobotPuzzleVecEnv("MultiRobotPuzzle-v0", 64, seed=5, max_episode_steps=20))
    env.reset()
    for _ in range(30):
        env.step(act())
    path = str(tmp_path / "saved_env.pkl")   # train.py:149 / test.py:66 use this exact name
    env.save(path)
    assert os.path.exists(path) and not os.path.exists(path + ".npz")
    st = env.get_stats()
    env.close()

    ev = MultiRobotPuzzleVecNormalize.load(path, MultiRobotPuzzleVecEnv("MultiRobotPuzzle-v0", 64, seed=9,
                                                                        max_episode_steps=20))
    for k, v in st.items():
        np.testing.assert_array_equal(ev.get_stats()[k], v)
    ev.training = False
    ev.norm_reward = False
    ev.reset()
    for _ in range(25):
        o, r, d, infos = ev.step(act())
        np.testing.assert_array_equal(r, ev.get_original_reward())   # raw rewards
        assert np.all(np.abs(o) <= ev.clip_obs)
    for k, v in st.items():   # training off: the statistics did not move
        np.testing.assert_array_equal(ev.get_stats()[k], v)
    ev.norm_obs = False
    o, r, d, infos = ev.step(act())
    np.testing.assert_array_equal(o, ev.get_original_obs())
    ev.close()


def test_restatement_norm_obs_off_freezes_obs_statistics():
    """SB3 VecNormalize updates obs_rms only when training and norm_obs; the returns' statistics
    still move with norm_obs off."""
    from oracle.vecnorm_ref import VecNormalizeRef
    rs = np.random.RandomState(2)
    n = VecNormalizeRef(8, 3, norm_obs=False)
    n.reset(rs.normal(size=(8, 3)))
    for _ in range(5):
        n.step(rs.normal(size=(8, 3)), rs.normal(size=8), np.zeros(8, bool))
    np.testing.assert_array_equal(n.obs_rms.mean, np.zeros(3))
    np.testing.assert_array_equal(n.obs_rms.var, np.ones(3))
    assert n.obs_rms.count == 1e-4 and n.ret_rms.count > 1


@pytest.mark.gpu
def test_device_norm_obs_off_matches_restatement(gpu_lib):
    """norm_obs=False on the device: obs statistics frozen, returns' statistics as SB3's."""
    import torch

    from gym_puzzles_amd import Batch, DeviceVecNormalize
    from oracle.vecnorm_ref import VecNormalizeRef
    lanes, steps = 128, 30
    dev = torch.device("cuda", 0)
    b = Batch(0, lanes, seed=4)
    b.set_auto_reset(True)
    b.set_time_limit(15)
    O = b.obs_dim
    norm = DeviceVecNormalize(lanes, O, 0)
    norm.norm_obs = False
    ref = VecNormalizeRef(lanes, O, norm_obs=False)
    o0 = b.reset().copy()
    nobs = torch.zeros((lanes, O), device=dev)
    norm.reset(torch.from_numpy(o0).to(dev), nobs)
    ref.reset(o0)
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    obs, rew, done, nrew = z(lanes, O), z(lanes), z(lanes, dt=torch.uint8), z(lanes)
    b.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    for _ in range(steps):
        b.step_device(0, obs.data_ptr(), rew.data_ptr(), done.data_ptr())
        norm.step(obs, rew, done, nobs, nrew)
        ref.step(obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy())
    st = norm.get_stats()
    np.testing.assert_array_equal(st["obs_mean"], np.zeros(O))
    np.testing.assert_array_equal(st["obs_var"], np.ones(O))
    assert st["obs_count"] == 1e-4
    np.testing.assert_allclose([st["ret_mean"], st["ret_var"], st["ret_count"]],
                               [ref.ret_rms.mean, ref.ret_rms.var, ref.ret_rms.count], rtol=1e-10)
    norm.close()
    b.close()


@pytest.mark.gpu
def test_device_vecnormalize_refuses_wrong_tensors_before_any_launch(gpu_lib):
    """reset and step check every tensor (a float64 or short one would be an out-of-bounds device
    access): each wrong one raises ValueError and the statistics afterwards are bitwise what they were."""
    import torch

    from gym_puzzles_amd import Batch, DeviceVecNormalize
    n = 4
    dev = torch.device("cuda", 0)
    b = Batch(0, n, seed=2)
    O = b.obs_dim
    norm = DeviceVecNormalize(n, O, 0)
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    obs = torch.from_numpy(b.reset().copy()).to(dev)
    nobs, rew, nrew, done = z(n, O), torch.ones(n, device=dev), z(n), z(n, dt=torch.uint8)
    norm.reset(obs, nobs)
    norm.step(obs, rew, done, nobs, nrew)
    before = norm.get_stats()
    wrong = {
        "reset: float64 obs": lambda: norm.reset(obs.double(), nobs),
        "reset: short obs": lambda: norm.reset(obs[:n - 1].contiguous(), nobs),
        "reset: non-contiguous obs_out": lambda: norm.reset(obs, z(n, 2 * O)[:, ::2]),
        "reset: CPU obs": lambda: norm.reset(obs.cpu(), nobs),
        "step: float64 obs": lambda: norm.step(obs.double(), rew, done, nobs, nrew),
        "step: short reward": lambda: norm.step(obs, rew[:n - 1].contiguous(), done, nobs, nrew),
        "step: bool done": lambda: norm.step(obs, rew, done.bool(), nobs, nrew),
        "step: non-contiguous obs_out": lambda: norm.step(obs, rew, done, z(n, 2 * O)[:, ::2], nrew),
        "step: CPU reward_out": lambda: norm.step(obs, rew, done, nobs, nrew.cpu()),
        "step: float32 ep_return": lambda: norm.step(obs, rew, done, nobs, nrew, ep_return=z(n)),
        "step: int64 ep_len": lambda: norm.step(obs, rew, done, nobs, nrew, ep_len=z(n, dt=torch.int64)),
    }
    for what, call in wrong.items():
        with pytest.raises(ValueError):
            call()
        after = norm.get_stats()
        assert all(np.array_equal(np.asarray(after[k]), np.asarray(before[k])) for k in before), what
    norm.step(obs, rew, done, obs, nrew)                      # element-wise: in place stays legal
    assert norm.get_stats()["ret_count"] > before["ret_count"]
    norm.close()
    b.close()


# ---- the exact rule (tests/vecnorm_exact.py): the restatement passes it, wrong rules do not ---------------

def _exact():
    import vecnorm_exact
    return vecnorm_exact


def _runs():
    """(id, inputs, constructor arguments, script, exact records) of every case and scenario."""
    ve = _exact()
    for i, c in enumerate(ve.CASES):
        yield ve.case_id(c), ve.case_inputs(i), ve.ARGS[c[2]], ve.plain_script(), ve.exact_case(i)
    for name in ve.SCENARIOS:
        inputs, args, script = ve.scenario(name)
        yield name, inputs, args, script, ve.exact_scenario(name)


def test_restatement_is_within_the_exact_bounds():
    """oracle/vecnorm_ref.py, a correct float64 implementation, passes the checkers on every case with
    the statistics below half their bound (the device gets the same room); an output's bound is mostly
    the half ulp of its own float32 rounding, so there the limit is the bound itself."""
    from oracle.vecnorm_ref import VecNormalizeRef
    ve = _exact()
    worst = dict.fromkeys(ve.RATIO_KEYS, 0.0)
    for name, inputs, args, script, exact in _runs():
        got = ve.run_script(ve.RefAdapter(VecNormalizeRef(inputs["L"], inputs["D"], **args)), inputs, script)
        w = ve.judge(got, exact, *ve.clips(args), where=name)
        worst = {k: max(worst[k], w[k]) for k in worst}
    print("restatement, worst error / bound:", {k: float(f"{v:.3g}") for k, v in worst.items()})
    for k in ("obs_mean", "obs_var", "ret_mean", "ret_var", "obs_slack", "reward_slack", "term_slack"):
        assert worst[k] < 0.5, (k, worst[k])


def _wrong_rms(kind):
    from oracle.vecnorm_ref import RunningMeanStd
    f32 = np.float32

    class Wrong(RunningMeanStd):
        def update(self, x):
            x = np.asarray(x, np.float64)
            n = x.shape[0]
            xs = x[:-1] if kind == "last lane dropped" or (kind == "last lane dropped at L % 256 == 1" and n % 256 == 1) else x
            if kind == "float32 sums":
                x32 = x.astype(f32)
                bm32 = x32.sum(axis=0, dtype=f32) / f32(n)
                bm, bv = np.asarray(bm32, np.float64), np.asarray(((x32 - bm32) ** 2).sum(axis=0, dtype=f32) / f32(n), np.float64)
            else:
                bm = xs.sum(axis=0) / n
                if kind == "one-pass variance":
                    bv = (xs * xs).sum(axis=0) / n - bm * bm
                else:
                    bv = ((xs - bm) ** 2).sum(axis=0) / (n - 1 if kind == "sample variance" else n)
            delta = bm - self.mean
            tot = self.count + n
            c = tot if kind == "post-update count in the merge" else self.count
            new_mean = self.mean + delta * n / tot
            m2 = self.var * c + bv * n + delta * delta * c * n / tot
            self.mean, self.var, self.count = new_mean, m2 / tot, tot
    return Wrong


def _wrong_vec(kind):
    from oracle.vecnorm_ref import VecNormalizeRef
    f32 = np.float32

    class Wrong(VecNormalizeRef):
        def normalize_obs(self, obs):
            if kind == "eps outside the square root":
                x = (np.asarray(obs, np.float64) - self.obs_rms.mean) / (np.sqrt(self.obs_rms.var) + self.epsilon)
                return np.clip(x, -self.clip_obs, self.clip_obs).astype(f32)
            if kind == "clip after the float32 cast":
                x = (np.asarray(obs, np.float64) - self.obs_rms.mean) / np.sqrt(self.obs_rms.var + self.epsilon)
                return np.clip(x.astype(f32), -f32(self.clip_obs), f32(self.clip_obs))
            return super().normalize_obs(obs)

        def normalize_reward(self, r):
            if kind == "eps outside the square root":
                x = np.asarray(r, np.float64) / (np.sqrt(self.ret_rms.var) + self.epsilon)
                return np.clip(x, -self.clip_reward, self.clip_reward).astype(f32)
            if kind == "clip after the float32 cast":
                x = np.asarray(r, np.float64) / np.sqrt(self.ret_rms.var + self.epsilon)
                return np.clip(x.astype(f32), -f32(self.clip_reward), f32(self.clip_reward))
            return super().normalize_reward(r)

        def step(self, obs, reward, done, term_obs=None, reward64=None):
            stale_term = self.normalize_obs(term_obs) if term_obs is not None else None
            advanced = self.returns * self.gamma + np.asarray(reward, np.float64)
            if kind == "returns advanced in evaluation mode" and not self.training:
                self.returns = advanced
            o, r, t, er, el = super().step(obs, reward, done, term_obs, reward64)
            if kind == "returns not zeroed on done" and self.training:
                self.returns = advanced
            if kind == "terminal obs with the pre-update statistics":
                t = stale_term
            return o, r, t, er, el
    return Wrong


_WRONG_RMS = ("one-pass variance", "float32 sums", "last lane dropped", "last lane dropped at L % 256 == 1",
              "sample variance", "post-update count in the merge")
_WRONG_VEC = ("eps outside the square root", "returns not zeroed on done", "returns advanced in evaluation mode",
              "terminal obs with the pre-update statistics")


def _make_wrong(kind, L, D, args):
    from oracle.vecnorm_ref import VecNormalizeRef
    if kind in _WRONG_RMS:
        n, rms = VecNormalizeRef(L, D, **args), _wrong_rms(kind)
        n.obs_rms, n.ret_rms = rms((D,)), rms(())
        return n
    return _wrong_vec(kind)(L, D, **args)


@pytest.mark.parametrize("kind", _WRONG_RMS + _WRONG_VEC)
def test_checkers_reject_a_wrong_rule(kind):
    """Each deliberately wrong variant of the restatement is rejected on at least one case: the inputs
    and bounds of tests/vecnorm_exact.py leave none of these mistakes room to hide."""
    ve = _exact()
    rejected = []
    for name, inputs, args, script, exact in _runs():
        got = ve.run_script(ve.RefAdapter(_make_wrong(kind, inputs["L"], inputs["D"], args)), inputs, script)
        w = ve.judge(got, exact, *ve.clips(args), fail=False, where=name)
        if max(w[k] for k in w if not k.endswith("_slack")) > 1.0:
            rejected.append(name)
    print(f"{kind}: rejected on {len(rejected)} runs: {rejected}")
    assert rejected, f"the checkers let '{kind}' through on every case"


def test_clip_after_the_float32_cast_is_the_same_rule():
    """Rounding to float32 is monotonic, so float32(min(max(x, -c), c)) == min(max(float32(x), -float32(c)),
    float32(c)) for every x and c: clipping after the cast with a float32 threshold differs nowhere and is
    not a wrong rule.  Pinned here bit for bit (clip thresholds 10, 2 and 0.5, and 0.1, which float32
    does not hold), so that nobody looks for a rejection that cannot exist."""
    from oracle.vecnorm_ref import VecNormalizeRef
    ve = _exact()
    runs = list(_runs())
    name, inputs, _, script, _ = runs[4]
    runs.append((name + "-clip0.1", inputs, {"clip_obs": 0.1, "clip_reward": 0.1}, script, None))
    for name, inputs, args, script, _ in runs:
        a = ve.run_script(ve.RefAdapter(VecNormalizeRef(inputs["L"], inputs["D"], **args)), inputs, script)
        wrong = _make_wrong("clip after the float32 cast", inputs["L"], inputs["D"], args)
        b = ve.run_script(ve.RefAdapter(wrong), inputs, script)
        for x, y in zip(a, b):
            for k in ("obs_out", "reward_out", "term_out"):
                if x.get(k) is not None:
                    np.testing.assert_array_equal(x[k].view(np.uint32), y[k].view(np.uint32), err_msg=f"{name} {k}")


def test_restatement_propagates_nan_like_numpy():
    """np.clip returns NaN for NaN and saturates +-inf.  A NaN (or an inf, whose variance is inf - inf)
    poisons its column's statistics, so that column is NaN in every lane from that step on and
    nothing else is; a NaN reward does the same to the return statistics and every later reward."""
    from oracle.vecnorm_ref import VecNormalizeRef
    ve = _exact()
    assert np.isnan(np.clip(np.nan, -1, 1)) and np.clip(np.inf, -1, 1) == 1 and np.clip(-np.inf, -1, 1) == -1
    inputs = ve.nonfinite_inputs()
    ref = VecNormalizeRef(65, 3)
    got = ve.run_script(ve.RefAdapter(ref), inputs, ve.plain_script())
    for t, g in enumerate(got):          # call 0 is the reset, call t is step t
        cols = [c for c, first in ((1, 2), (2, 3)) if t >= first]
        want = np.zeros((65, 3), bool)
        want[:, cols] = True
        np.testing.assert_array_equal(np.isnan(g["obs_out"]), want, err_msg=f"obs_out @{t}")
        np.testing.assert_array_equal(np.isnan(g["stats"]["obs_mean"]) | np.isinf(g["stats"]["obs_mean"]), want[0])
        np.testing.assert_array_equal(np.isnan(g["stats"]["obs_var"]), want[0])
        if t:
            np.testing.assert_array_equal(np.isnan(g["term_out"]), want, err_msg=f"term_out @{t}")
            np.testing.assert_array_equal(np.isnan(g["reward_out"]), np.full(65, t >= 4), err_msg=f"reward_out @{t}")
            assert np.isnan(g["stats"]["ret_mean"]) == np.isnan(g["stats"]["ret_var"]) == (t >= 4)
    # Monitor: the lane's episode sum is NaN from the NaN reward until the lane is done
    lane, alive = 64, True
    for t in range(4, 7):
        assert np.isnan(got[t]["ep_return"][lane]) == alive and not np.isnan(np.delete(got[t]["ep_return"], lane)).any()
        alive = alive and not inputs["steps"][t - 1]["done"][lane]

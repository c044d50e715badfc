"""Data-parallel VecNormalize on the device in one process (csrc/mrp_norm.hip: k_moments<true>, k_norm_merge and
k_apply behind mrp_norm_local_device / mrp_norm_apply_device): at world size 1 the local phase, the copy-only
exchange and the apply phase must give the unsharded path's bits; the ABI refuses bad arguments before any
HIP call; DeviceVecNormalize refuses wrong tensors before any launch.  Two ranks run in
tests/test_ddp_norm_gpu.py.
"""
from __future__ import annotations

import numpy as np
import pytest
import vecnorm_exact as ve
from ppo_cases import bits

pytestmark = pytest.mark.gpu

SENT32 = np.uint32(0x7FC12345)
SENT64 = np.uint64(0x7FF80000DEADBEEF)


class _Dev:
    """DeviceVecNormalize behind the interface vecnorm_exact.run_script drives; outputs start as sentinels."""

    def __init__(self, L, D, shard=None, **args):
        import torch

        from gym_puzzles_amd import DeviceVecNormalize
        self.torch, self.dev, self.L, self.D = torch, torch.device("cuda", 0), L, D
        self.norm = DeviceVecNormalize(L, D, 0, shard=shard, **args)

    @property
    def training(self):
        return self.norm.training

    @training.setter
    def training(self, v):
        self.norm.training = v

    def set_stats(self, st):
        self.norm.set_stats(st)

    def _up(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def _sent(self, shape, bits):
        return self._up(np.full(shape, bits).view({4: np.float32, 8: np.float64}[bits.dtype.itemsize]))

    def reset(self, obs):
        out = self._sent(obs.shape, SENT32)
        self.norm.reset(self._up(obs), out)
        return {"obs_out": out.cpu().numpy(), "stats": self.norm.get_stats()}

    def step(self, obs, reward, done, term=None, reward64=None):
        L, D = self.L, self.D
        o, r, t = self._sent((L, D), SENT32), self._sent((L,), SENT32), self._sent((L, D), SENT32)
        epr, epl = self._sent((L,), SENT64), self._up(np.full(L, -12345, np.int32))
        self.norm.step(self._up(obs), self._up(reward), self._up(done), o, r, self._up(term), t, epr, epl, self._up(reward64))
        return {"obs_out": o.cpu().numpy(), "reward_out": r.cpu().numpy(), "term_out": t.cpu().numpy(),
                "ep_return": epr.cpu().numpy(), "ep_len": epl.cpu().numpy(), "stats": self.norm.get_stats()}


def _script(D):
    """A reset and 6 steps with a training toggle and a set_stats in between."""
    rs = np.random.RandomState(77)
    st = {"obs_mean": rs.normal(size=D) * 3.0, "obs_var": rs.uniform(0.5, 2.0, size=D), "obs_count": 1e6,
          "ret_mean": 0.75, "ret_var": 1.5, "ret_count": 1e6}
    return [("reset",), ("step", 0), ("step", 1), ("training", False), ("step", 2), ("training", True), ("step", 3),
            ("set_stats", st), ("step", 4), ("step", 5)]


@pytest.mark.parametrize("shape", [(1, 28), (257, 7), (600, 69)], ids=lambda s: f"L{s[0]}-D{s[1]}")
def test_world_size_one_equals_the_unsharded_path_bit_for_bit(gpu_lib, shape):
    """Every output (sentinels where nothing is written included) and every statistic after every call."""
    from gym_puzzles_amd.dist import Shard
    L, D = shape
    inputs = ve.make_inputs(L, D, 5000 + L, with_reward64=True)
    plain, shard = _Dev(L, D), _Dev(L, D, shard=Shard(0, 1, L))
    assert plain.norm.exchange is None and shard.norm.exchange.parts.shape == (1, 64 * -(-2 * (D + 1) // 64))
    a = ve.run_script(plain, inputs, _script(D))
    b = ve.run_script(shard, inputs, _script(D))
    parts = shard.norm.exchange.parts.cpu().numpy()
    plain.norm.close(), shard.norm.close()
    assert len(a) == len(b) == 7
    for t, (x, y) in enumerate(zip(a, b)):
        for k in x:
            if k != "stats":
                assert np.array_equal(bits(x[k], None), bits(y[k], None)), f"{k} @{t}"
        for k, v in x["stats"].items():
            assert np.array_equal(bits(np.asarray(v), None), bits(np.asarray(y["stats"][k]), None)), f"{k} @{t}"
    assert a[-1]["stats"]["obs_count"] == 1e6 + 2 * L and np.isfinite(parts[0, :2 * (D + 1)]).all()
    assert not parts[0, 2 * (D + 1):].any(), "the local phase wrote past its part"


def test_norm_obs_off_exchanges_the_returns_column_only(gpu_lib):
    """norm_obs off at world size 1: the obs entries of the part are never written, the obs statistics keep
    their initial bits and the return statistics equal the unsharded path's."""
    import torch

    from gym_puzzles_amd.dist import Shard
    L, D = 65, 3
    inputs = ve.make_inputs(L, D, 5100)
    plain, shard = _Dev(L, D), _Dev(L, D, shard=Shard(0, 1, L))
    plain.norm.norm_obs = shard.norm.norm_obs = False
    shard.norm.exchange.mine.copy_(torch.from_numpy(np.full(64, SENT64).view(np.float64)))
    a = ve.run_script(plain, inputs, ve.plain_script(2))
    b = ve.run_script(shard, inputs, ve.plain_script(2))
    mine = bits(shard.norm.exchange.mine.cpu().numpy(), None)
    plain.norm.close(), shard.norm.close()
    assert np.all(mine[:2 * D] == SENT64) and np.all(mine[2 * D:2 * D + 2] != SENT64) and np.all(mine[2 * D + 2:] == SENT64)
    for x, y in zip(a, b):
        for k, v in x["stats"].items():
            assert np.array_equal(bits(np.asarray(v), None), bits(np.asarray(y["stats"][k]), None)), k
    assert b[-1]["stats"]["obs_count"] == 1e-4 and b[-1]["stats"]["ret_count"] == (1e-4 + L) + L


def test_host_wrapper_passes_the_shard_through(gpu_lib, tmp_path):
    """MultiRobotPuzzleVecNormalize(venv, shard=) at world size 1: the same arrays and statistics as the unsharded
    wrapper, and save() / load(..., shard=) carry the statistics bit for bit into a sharded instance."""
    from gym_puzzles_amd import MultiRobotPuzzleVecEnv, MultiRobotPuzzleVecNormalize
    from gym_puzzles_amd.dist import Shard
    N = 64
    make = lambda: MultiRobotPuzzleVecEnv("MultiRobotPuzzle-v0", N, seed=5, max_episode_steps=6)  # noqa: E731
    plain, shard = MultiRobotPuzzleVecNormalize(make()), MultiRobotPuzzleVecNormalize(make(), shard=Shard(0, 1, N))
    assert plain.norm.exchange is None and shard.norm.exchange is not None and shard.norm.shard.global_lanes == N
    rs = np.random.RandomState(1)
    assert np.array_equal(bits(plain.reset(), None), bits(shard.reset(), None))
    for _ in range(8):
        act = rs.uniform(-1, 1, size=(N, 6)).astype(np.float32)
        (o1, r1, d1, i1), (o2, r2, d2, i2) = plain.step(act), shard.step(act)
        assert np.array_equal(bits(o1, None), bits(o2, None)) and np.array_equal(bits(r1, None), bits(r2, None)) and np.array_equal(d1, d2)
        assert [i.get("episode") for i in i1] == [i.get("episode") for i in i2]
    st = shard.get_stats()
    for k, v in plain.get_stats().items():
        assert np.array_equal(bits(np.asarray(v), None), bits(np.asarray(st[k]), None)), k
    count = 1e-4
    for _ in range(9):                       # the reset and 8 steps, one float64 add each
        count = count + N
    assert st["obs_count"] == count
    path = str(tmp_path / "saved_env.pkl")
    shard.save(path)
    plain.close(), shard.close()
    back = MultiRobotPuzzleVecNormalize.load(path, make(), shard=Shard(0, 1, N))
    assert back.norm.exchange is not None
    for k, v in st.items():
        assert np.array_equal(bits(np.asarray(v), None), bits(np.asarray(back.get_stats()[k]), None)), k
    back.close()


def test_abi_refuses_bad_arguments(gpu_lib):
    """Through ctypes: null parts, R = 0, a short stride, parts overlapping obs_out and a part overlapping obs
    are MRP_E_ARG with a message that names the function, and the statistics keep their bits."""
    import torch

    from gym_puzzles_amd import DeviceVecNormalize
    lib, dev = gpu_lib, torch.device("cuda", 0)
    L, D = 8, 3
    n_part = lib.mrp_norm_part_len(D)
    assert n_part == 2 * (D + 1) and lib.mrp_norm_part_len(0) == -1
    norm = DeviceVecNormalize(L, D, 0)
    h = norm._h
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    obs, rew, done, nrew = torch.randn(L, D, device=dev), torch.randn(L, device=dev), z(L, dt=torch.uint8), z(L)
    big = z(2 * L * D + 64, dt=torch.float64)          # room for parts and, inside it, an obs_out
    parts, inside = big[:n_part], big[4:].view(torch.float32)[:L * D]
    nobs = z(L, D)
    before = norm.get_stats()
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def apply(R, d_parts, stride, obs_out, step=1):
        return lib.mrp_norm_apply_device(h, R, p(d_parts), stride, step, p(obs), p(rew), None, p(done), None, p(obs_out), p(nrew),
                                         None, None, None)
    err = lambda: lib.mrp_norm_last_error(h)  # noqa: E731
    assert apply(1, None, n_part, nobs) == -1 and b"mrp_norm_apply_device" in err() and b"null" in err()
    assert apply(0, parts, n_part, nobs) == -1 and b"mrp_norm_apply_device: R < 1" in err()
    assert apply(1, parts, n_part - 1, nobs) == -1 and b"mrp_norm_apply_device: part_stride" in err()
    assert apply(1, parts, n_part, inside) == -1 and b"mrp_norm_apply_device" in err() and b"overlaps" in err()
    assert apply(1, parts, n_part, None) == -1 and apply(1, parts, n_part, nobs, step=0) == 0      # reset needs no reward
    assert lib.mrp_norm_apply_device(None, 1, p(parts), n_part, 1, p(obs), p(rew), None, p(done), None, p(nobs), p(nrew), None,
                                     None, None) == -1
    assert b"mrp_norm_apply_device" in lib.mrp_norm_last_error(None)
    assert lib.mrp_norm_local_device(h, p(obs), p(rew), 1, None) == -1 and b"mrp_norm_local_device" in err()
    assert lib.mrp_norm_local_device(h, None, p(rew), 1, p(parts)) == -1
    assert lib.mrp_norm_local_device(h, p(obs), None, 1, p(parts)) == -1
    assert lib.mrp_norm_local_device(h, p(obs), p(rew), 1, p(obs.view(-1)[2:].view(torch.float64))) == -1 and b"overlaps" in err()
    torch.cuda.synchronize(dev)
    after = norm.get_stats()
    # the one accepted call above was a reset-form apply on zero parts with R = 1: it merged, so compare before it
    assert after["obs_count"] == before["obs_count"] + L and after["ret_count"] == before["ret_count"]
    norm.close()


def test_mismatched_tensors_raise_before_launch(gpu_lib):
    """A sharded instance checks its tensors like the unsharded one, and its exchange at construction."""
    import torch

    from gym_puzzles_amd import DeviceVecNormalize
    from gym_puzzles_amd.dist import GradExchange, Shard
    dev = torch.device("cuda", 0)
    L, D = 4, 5
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    norm = DeviceVecNormalize(L, D, 0, shard=Shard(0, 1, L))
    obs, nobs, rew, nrew, done = torch.randn(L, D, device=dev), z(L, D), torch.ones(L, device=dev), z(L), z(L, dt=torch.uint8)
    norm.reset(obs, nobs)
    norm.step(obs, rew, done, nobs, nrew)
    before = norm.get_stats()
    wrong = {
        "reset: float64 obs": lambda: norm.reset(obs.double(), nobs),
        "reset: short obs": lambda: norm.reset(obs[:L - 1].contiguous(), nobs),
        "reset: CPU obs": lambda: norm.reset(obs.cpu(), nobs),
        "step: short reward": lambda: norm.step(obs, rew[:L - 1].contiguous(), done, nobs, nrew),
        "step: bool done": lambda: norm.step(obs, rew, done.bool(), nobs, nrew),
        "step: non-contiguous obs_out": lambda: norm.step(obs, rew, done, z(L, 2 * D)[:, ::2], nrew),
        "step: float32 ep_return": lambda: norm.step(obs, rew, done, nobs, nrew, ep_return=z(L)),
    }
    for what, call in wrong.items():
        with pytest.raises(ValueError):
            call()
        after = norm.get_stats()
        assert all(np.array_equal(np.asarray(after[k]), np.asarray(before[k])) for k in before), what
    norm.step(obs, rew, done, obs, nrew)                       # element-wise: in place stays legal
    assert norm.get_stats()["ret_count"] == before["ret_count"] + L
    norm.close()
    sh = Shard(0, 1, L)
    for what, make in {
        "float32 exchange": lambda: GradExchange(sh, 2 * (D + 1), dev),
        "short exchange": lambda: GradExchange(sh, 2 * D, dev, dtype=torch.float64),
        "host exchange": lambda: GradExchange(sh, 2 * (D + 1), "cpu", dtype=torch.float64),
    }.items():
        with pytest.raises(ValueError):
            DeviceVecNormalize(L, D, 0, exchange=make())
    with pytest.raises(ValueError):
        DeviceVecNormalize(L, D, 0, shard=Shard(0, 1, L + 1))

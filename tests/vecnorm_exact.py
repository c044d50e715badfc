"""TEST INFRASTRUCTURE ONLY -- the exact rule of VecNormalize + Monitor (oracle/vecnorm_ref.py's
algorithm over ``fractions.Fraction``), error bounds derived from the inputs, the synthetic cases
that tests/test_norm.py (CPU, the float64 restatement) and tests/test_norm_gpu.py (the device,
csrc/mrp_norm.hip) share, and the checkers that judge both.  Never imported by the product.

Exact rule
----------
``ExactVecNormalize`` keeps every statistic as a ``Fraction``.  float32 inputs are dyadic rationals,
so a column's batch mean and population variance come from two integer sums; the Chan merge, the
count (from ``Fraction(1e-4)``) and the discounted returns ``returns * gamma + reward`` (reset on
done) are exact.  Counts and Monitor's sums are *also* kept as the sequential float64 sums every
implementation must reproduce bit for bit.  A normalised value ``(x - mean) / sqrt(var + eps)`` is
evaluated in ``np.longdouble`` (64-bit mantissa) from the statistics split into a float64 head and
tail, so the cancellation ``x - mean`` loses nothing; that evaluation's own error (below
``2**-60 |z|``) is part of the bound.

Bounds (u = 2**-53, a float64 rounding; nothing here comes from the code under test)
------------------------------------------------------------------------------------
gamma(L), the roundings on the longest path of either implementation, with a margin of 2:

* the column sum: the device adds ``ceil(L / 256)`` values per thread and then 8 tree levels;
  numpy's ``x.sum(axis=0)`` of a C-ordered [L, D] array adds the rows one after the other,
  ``L - 1`` adds (pairwise summation only applies along a contiguous axis), so
  ``sum_path(L) = max(ceil(L / 256) + 8, L - 1)``;
* the rest of the path, ``MERGE_OPS = 16``: for the mean ``/ n``, ``bm - mean``, ``* n``, ``/ tot``,
  ``+`` (5) and the count, itself the rounded sum of up to 7 updates and one more add for ``tot``
  (8); for the variance ``x - bm``, the square (which doubles it: 3), ``/ n``, ``* n``, two adds,
  ``/ tot`` (5) and the count (8);
* ``gamma(L) = 2 * (sum_path(L) + MERGE_OPS)``.

One update of a column with old exact statistics (m, v, c), batch x, exact batch moments (bm, bv),
``delta = bm - m``, ``tot = c + L``; dm and dv are the bounds carried from the earlier updates
(the exact rule carries exact statistics, an implementation carries rounded ones):

* mean: ``dm' = dm * c / tot + gamma u (mean|x| + |m|)``;
* variance: ``dv' = dv * c / tot + gamma u (mean((x - bm)^2) L / tot + v c / tot + delta^2 c L / tot^2)``:
  the three summands of the merged variance, each with the weight it enters with.  Unweighted
  (``mean((x - bm)^2) + v + delta^2``) the bound also holds, but it is then ruled by the first update's
  ``delta^2`` (the prior mean is 0, its count 1e-4): on the offset column that is 1.7e7 where the merged
  variance is 6.5, and a one-pass variance passed every case.  The error of the computed ``delta``
  (about ``dm``) enters ``delta^2`` as ``2 |delta| dm c L / tot^2``; that has no term of its own: it is
  second to ``v c / tot`` on every column here and takes its share of gamma's margin (the measured
  ratios below are where it shows, on the one-lane cases).
* returns: an implementation's ``returns`` are rounded twice per step.  Per lane
  ``A = A * gamma + |reward|`` and ``E = E * gamma + 2 u A`` (both reset on done) bound the error of
  a lane's return; mean(A) stands for mean|x| above and the input error ``e = E + mean(E)`` adds
  ``mean(E) L / tot`` to dm' and ``mean(2 |x - bm| e + e^2) L / tot`` to dv'.

A float32 output gets half a float32 ulp of the exact value, plus the propagated
``(dm + |x - mean| dv / (2 (var + eps))) / sd``, plus ``16 u |z|`` for the float64 evaluation of the
implementation (subtract, add, sqrt, divide) and the longdouble evaluation here.  Where the exact
value lies outside ``+-clip`` by more than the propagated part the output must be ``float32(+-clip)``
bit for bit; within it of the threshold it may be either.

Measured worst error / bound (all cases of ``CASES`` and all ``SCENARIOS``)
---------------------------------------------------------------------------
                                        obs_mean  obs_var  ret_mean  ret_var  slack of the outputs
float64 restatement, CPU                0.0218    0.319    0.0139    0.0629   0.00018
device, MI355X (tests/test_norm_gpu.py) 0.0218    0.319    0.0139    0.0629   0.00018

tests/test_norm.py asserts the restatement's below 0.5, so the device has the same room.  The worst
ratios come from the one-lane cases (L1-D28-clipped, L2-D3-gamma1), where gamma(L) is smallest and both
implementations do the same few operations; at 257 lanes and more both stay below 0.011, the device
below 0.007.  An output's ratio comes close to 1.0 by construction: most of its bound is the half ulp of its
own float32 rounding, and some element always lands next to a tie.  The "slack" column is the share of
the rest of the bound that is in use, ``max(0, error - half ulp) / (bound - half ulp)``.
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the exact normalised values need a 64-bit mantissa"
U = 2.0 ** -53
MERGE_OPS = 16
OUT_OPS = 16


def sum_path(L: int) -> int:
    return max(-(-L // 256) + 8, L - 1)


def gamma_u(L: int) -> float:
    return 2 * (sum_path(L) + MERGE_OPS) * U


# ---- exact arithmetic ------------------------------------------------------------------------------

def _split(f: Fraction):
    """Fraction -> (float64 head, float64 tail): head + tail equals f to 2**-106."""
    hi = float(f)
    return hi, float(f - Fraction(hi))


def _ld(f: Fraction):
    hi, lo = _split(f)
    return LD(hi) + LD(lo)


def _moments_of_ints(ints, scale: Fraction):
    """Exact mean and population variance of ``ints[i] * scale``."""
    n = len(ints)
    s1 = sum(ints)
    s2 = sum(i * i for i in ints)
    return Fraction(s1, n) * scale, Fraction(n * s2 - s1 * s1, n * n) * scale * scale


def _column_moments(col: np.ndarray):
    """Exact batch moments of a float32 column: every value is mant * 2**exp with a 24-bit mant."""
    m, e = np.frexp(col.astype(np.float64))
    mant = (m * 2.0 ** 24).astype(np.int64)
    e = e.astype(np.int64) - 24
    nz = mant != 0
    emin = int(e[nz].min()) if nz.any() else 0
    ints = [int(a) << int(b - emin) if a else 0 for a, b in zip(mant.tolist(), e.tolist())]
    return _moments_of_ints(ints, Fraction(2) ** emin)


def _fraction_moments(xs):
    """Exact batch moments of Fractions with power-of-two denominators."""
    den = max(x.denominator for x in xs)
    return _moments_of_ints([x.numerator * (den // x.denominator) for x in xs], Fraction(1, den))


class _Rms:
    """Exact RunningMeanStd of one column, with the bounds an implementation's copy is held to."""

    def __init__(self):
        self.mean, self.var, self.count = Fraction(0), Fraction(1), Fraction(1e-4)
        self.dm = self.dv = 0.0

    def update(self, bm: Fraction, bv: Fraction, n: int, mean_abs: float, in_dm: float = 0.0, in_dv: float = 0.0):
        g = gamma_u(n)
        c, tot = self.count, self.count + n
        delta = bm - self.mean
        w, wn = float(c / tot), float(Fraction(n) / tot)
        step = g * (mean_abs + abs(float(self.mean)))
        self.dv = self.dv * w + g * (float(bv) * wn + float(self.var) * w + float(delta) ** 2 * w * wn) + in_dv * wn
        self.dm = self.dm * w + step + in_dm * wn
        self.var = (self.var * c + bv * n + delta * delta * c * n / tot) / tot
        self.mean = self.mean + delta * n / tot
        self.count = tot


class ExactVecNormalize:
    """The exact rule.  ``reset`` and ``step`` return a record (dict) of exact values and bounds:

    ``obs`` / ``reward`` / ``term``: (exact pre-clip value [longdouble], propagated bound, total bound)
    ``stats`` / ``stat_bounds``: dicts like DeviceVecNormalize.get_stats() (longdouble / float64)
    ``obs_count`` / ``ret_count`` / ``ep_return`` / ``ep_len``: the bit-exact float64 / int values
    """

    def __init__(self, n_lanes, obs_dim, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8, norm_obs=True):
        self.L, self.D = n_lanes, obs_dim
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = clip_obs, clip_reward, gamma, epsilon
        self.training, self.norm_obs = True, norm_obs
        self.obs_rms = [_Rms() for _ in range(obs_dim)]
        self.ret_rms = _Rms()
        self.obs_count64 = self.ret_count64 = 1e-4
        self._restart()

    def _restart(self):
        L = self.L
        self.returns = [Fraction(0)] * L
        self.ret_abs, self.ret_err = np.zeros(L), np.zeros(L)
        self.ep_ret, self.ep_len = np.zeros(L, np.float64), np.zeros(L, np.int64)

    def set_stats(self, st: dict):
        """Load float64 statistics (exact values, so the carried bounds restart at zero)."""
        for j, r in enumerate(self.obs_rms):
            r.mean, r.var, r.count = Fraction(float(st["obs_mean"][j])), Fraction(float(st["obs_var"][j])), \
                Fraction(float(st["obs_count"]))
            r.dm = r.dv = 0.0
        r = self.ret_rms
        r.mean, r.var, r.count = (Fraction(float(st[k])) for k in ("ret_mean", "ret_var", "ret_count"))
        r.dm = r.dv = 0.0
        self.obs_count64, self.ret_count64 = float(st["obs_count"]), float(st["ret_count"])

    # -- statistics
    def _update_obs(self, obs):
        mean_abs = np.abs(obs.astype(np.float64)).mean(axis=0)
        for j, r in enumerate(self.obs_rms):
            bm, bv = _column_moments(obs[:, j])
            r.update(bm, bv, self.L, float(mean_abs[j]))
        self.obs_count64 = self.obs_count64 + float(self.L)

    def _update_returns(self, reward):
        g = Fraction(float(self.gamma))
        self.returns = [x * g + Fraction(float(r)) for x, r in zip(self.returns, reward)]
        self.ret_abs = self.ret_abs * float(self.gamma) + np.abs(reward.astype(np.float64))
        self.ret_err = self.ret_err * float(self.gamma) + 2 * U * self.ret_abs
        bm, bv = _fraction_moments(self.returns)
        e = self.ret_err + self.ret_err.mean()
        dev = np.abs(np.array([float(x - bm) for x in self.returns]))
        self.ret_rms.update(bm, bv, self.L, float(self.ret_abs.mean()), in_dm=float(self.ret_err.mean()),
                            in_dv=float((2 * dev * e + e * e).mean()))
        self.ret_count64 = self.ret_count64 + float(self.L)

    def _stats(self):
        o = self.obs_rms
        st = {"obs_mean": np.array([_ld(r.mean) for r in o]), "obs_var": np.array([_ld(r.var) for r in o]),
              "ret_mean": _ld(self.ret_rms.mean), "ret_var": _ld(self.ret_rms.var)}
        bd = {"obs_mean": np.array([r.dm for r in o]), "obs_var": np.array([r.dv for r in o]),
              "ret_mean": self.ret_rms.dm, "ret_var": self.ret_rms.dv}
        return st, bd

    # -- normalised values
    def _norm_obs(self, x):
        """(exact [L, D] longdouble, propagated bound, total bound) of a float32 [L, D] array."""
        o = self.obs_rms
        eps = Fraction(float(self.epsilon))
        mh, ml = (np.array(v) for v in zip(*[_split(r.mean) for r in o]))
        ve = np.array([_ld(r.var + eps) for r in o])
        dm, dv = np.array([r.dm for r in o]), np.array([r.dv for r in o])
        sd = np.sqrt(ve)
        num = (x.astype(LD) - mh.astype(LD)) - ml.astype(LD)
        z = num / sd
        prop = ((dm + np.abs(num) * dv / (2 * ve)) / sd).astype(np.float64)
        return z, prop, prop + _half_ulp32(z) + OUT_OPS * U * np.abs(z).astype(np.float64)

    def _norm_reward(self, r):
        ve = _ld(self.ret_rms.var + Fraction(float(self.epsilon)))
        sd = np.sqrt(ve)
        z = r.astype(LD) / sd
        prop = (np.abs(r.astype(LD)) * self.ret_rms.dv / (2 * ve) / sd).astype(np.float64)
        return z, prop, prop + _half_ulp32(z) + OUT_OPS * U * np.abs(z).astype(np.float64)

    def _record(self, **kw):
        st, bd = self._stats()
        kw.update(stats=st, stat_bounds=bd, obs_count=self.obs_count64, ret_count=self.ret_count64)
        return kw

    def reset(self, obs):
        if self.training and self.norm_obs:
            self._update_obs(obs)
        self._restart()
        return self._record(obs=self._norm_obs(obs))

    def step(self, obs, reward, done, term_obs=None, reward64=None):
        done = np.asarray(done).astype(bool)
        if self.training and self.norm_obs:
            self._update_obs(obs)
        rec = {"obs": self._norm_obs(obs)}
        if self.training:
            self._update_returns(reward)
        rec["reward"] = self._norm_reward(reward)
        if term_obs is not None:
            rec["term"] = self._norm_obs(term_obs)
        self.ep_ret = self.ep_ret + (reward.astype(np.float64) if reward64 is None else reward64)
        self.ep_len = self.ep_len + 1
        rec["ep_return"], rec["ep_len"], rec["done"] = self.ep_ret.copy(), self.ep_len.copy(), done
        self.ep_ret[done] = 0.0
        self.ep_len[done] = 0
        for l in np.nonzero(done)[0]:
            self.returns[l] = Fraction(0)
        self.ret_abs[done] = 0.0
        self.ret_err[done] = 0.0
        return self._record(**rec)


def _half_ulp32(z):
    """Half the float32 spacing at |z| (the subnormal spacing 2**-149 below 2**-126)."""
    _, e = np.frexp(np.abs(z).astype(np.float64))
    return np.ldexp(1.0, np.maximum(e.astype(np.int64) - 25, -150))


# ---- checkers --------------------------------------------------------------------------------------

def _ratio(err, bound):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)     # a NaN where a number belongs is unbounded error
    return float(r.max()) if r.size else 0.0


def check_stats(got, exact, bounds, what="statistic", fail=True) -> float:
    """Worst |got - exact| / bound of a statistic (scalars or arrays); raises above 1 unless ``fail`` is off."""
    err = np.abs(np.asarray(got, np.float64).astype(LD) - np.asarray(exact, LD))
    worst = _ratio(err, bounds)
    if fail and not worst <= 1.0:
        raise AssertionError(f"{what}: error / bound = {worst:.3g}")
    return worst


def check_outputs(got, exact, bounds, clip, what="output", fail=True, prop=None):
    """Worst error / bound of float32 outputs against ``exact`` pre-clip values.  ``bounds`` is the
    total bound per element; ``prop`` (default: ``bounds``) its propagated part, which decides
    whether an element is saturated.  Returns (worst ratio, worst share of the slack above the half ulp)."""
    got = np.asarray(got)
    assert got.dtype == np.float32, f"{what}: {got.dtype}"
    z, bounds = np.asarray(exact, LD), np.asarray(bounds, np.float64)
    prop = bounds if prop is None else np.asarray(prop, np.float64)
    c = LD(float(clip))
    c32 = np.float32(clip)
    sat = np.where(z > c + prop, 1, 0) - np.where(z < -c - prop, 1, 0)      # surely saturated
    near = (sat == 0) & (np.abs(z) >= c - prop)                             # either is allowed
    at_clip = got.view(np.uint32) == np.where(z > 0, c32, -c32).astype(np.float32).view(np.uint32)
    err = np.abs(got.astype(LD) - z).astype(np.float64)
    err = np.where(np.isnan(got), np.inf, err)
    err = np.where((sat != 0) | near, np.where(at_clip, 0.0, np.where(near, err, np.inf)), err)
    worst = _ratio(err, bounds)
    half = _half_ulp32(z)
    slack = _ratio(np.where(np.isfinite(err), np.maximum(err - half, 0.0), 0.0), np.maximum(bounds - half, 1e-300))
    if fail and not worst <= 1.0:
        i = np.unravel_index(np.argmax(np.where(np.isfinite(err), err / bounds, np.inf)), err.shape) if err.size else ()
        raise AssertionError(f"{what}: error / bound = {worst:.3g} at {i}: got {got[i]!r}, exact {float(z[i])!r}, "
                             f"bound {bounds[i]:.3g}")
    return worst, slack


# ---- synthetic cases -------------------------------------------------------------------------------

DEFAULTS = {}
CLIPPED = {"clip_obs": 2.0, "clip_reward": 0.5, "gamma": 0.9, "epsilon": 1e-3}
UNDISCOUNTED = {"gamma": 1.0}
ARGS = {"default": DEFAULTS, "clipped": CLIPPED, "gamma1": UNDISCOUNTED}
N_STEPS = 6
# (lanes, columns, constructor arguments): every shape with at least one set, every set at small and
# large shapes; the clipped set wherever the N(0, 1) * 50 column exists (D >= 7)
CASES = [(1, 1, "default"), (1, 28, "clipped"), (2, 3, "gamma1"), (63, 5, "default"), (64, 7, "clipped"),
         (64, 7, "default"), (255, 7, "gamma1"), (256, 1, "default"), (257, 1, "clipped"), (257, 1, "gamma1"),
         (257, 28, "default"), (257, 28, "clipped"), (600, 69, "clipped"), (600, 69, "default")]


def case_id(case) -> str:
    return f"L{case[0]}-D{case[1]}-{case[2]}"


def clips(args):
    """(clip_obs, clip_reward) of a set of constructor arguments, as ``judge`` takes them."""
    return args.get("clip_obs", 10.0), args.get("clip_reward", 10.0)


def _columns(rs, L, D):
    """[L, D] float32; column j is of kind j % 7."""
    x = np.zeros((L, D), np.float64)
    for j in range(D):
        k = j % 7
        if k == 0:
            x[:, j] = rs.normal(size=L)
        elif k == 1:
            x[:, j] = 3.25                                            # batch variance exactly 0
        elif k == 2:
            x[:, j] = 4096.0 + rs.randint(-3, 4, size=L) * 2.0 ** -11   # offset 1e9 times the spread
        elif k == 3:
            x[:, j] = rs.normal(size=L) * 1e-20                         # var << eps
        elif k == 4:
            x[:, j] = rs.normal(size=L) * 1e18
        elif k == 5:
            x[:, j] = np.where(rs.rand(L) < 0.4, -0.0, 0.0)
        else:
            x[:, j] = rs.normal(size=L) * 50.0                          # saturates clip_obs = 2 on both sides
    return x.astype(np.float32)


def make_inputs(L, D, seed, n_steps=N_STEPS, with_reward64=False, done_p=None):
    """One reset and ``n_steps`` steps of inputs: {"obs0", "steps": [{obs, reward, reward64, done, term}]}.
    Step 1 has no lane done, step 2 every lane, later steps about 30 %."""
    rs = np.random.RandomState(seed)
    out = {"L": L, "D": D, "obs0": _columns(rs, L, D), "steps": []}
    for t in range(n_steps):
        r64 = rs.normal(size=L) * np.where(rs.rand(L) < 0.2, 1e3, 1.0)     # a fifth reach clip_reward
        r32 = r64.astype(np.float32)
        if with_reward64:
            assert np.all(r32.astype(np.float64) != r64)                   # not float32-representable
        p = (0.0, 1.0)[t] if t < 2 else 0.3
        done = (rs.rand(L) < (p if done_p is None else done_p)).astype(np.uint8)
        out["steps"].append({"obs": _columns(rs, L, D), "reward": r32, "reward64": r64 if with_reward64 else None,
                             "done": done, "term": _columns(rs, L, D)})
    return out


@functools.lru_cache(maxsize=None)
def case_inputs(i: int):
    L, D, _ = CASES[i]
    return make_inputs(L, D, 1000 + i, with_reward64=bool(i % 2))


# A scenario is a script over one set of inputs: ("reset",), ("step", k), ("training", flag),
# ("set_stats", stats).  CASES are the plain script; SCENARIOS add the mode changes.
def plain_script(n_steps=N_STEPS):
    return [("reset",)] + [("step", k) for k in range(n_steps)]


def eval_script():
    """Three training steps, three in evaluation mode, then two in training again."""
    return ([("reset",)] + [("step", k) for k in range(3)] + [("training", False)] + [("step", k) for k in range(3, 6)]
            + [("training", True)] + [("step", k) for k in range(6, 8)])


def reset_script():
    """reset after three steps, then three more."""
    return [("reset",)] + [("step", k) for k in range(3)] + [("reset",)] + [("step", k) for k in range(3, 6)]


@functools.lru_cache(maxsize=None)
def scenario(name: str):
    """(inputs, constructor arguments, script)"""
    if name == "eval":      # no lane is done while frozen unless the pattern says so: 30 % per step
        return make_inputs(257, 7, 2001, n_steps=8, with_reward64=True), DEFAULTS, eval_script()
    if name == "reset":
        return make_inputs(257, 7, 2002, with_reward64=False), DEFAULTS, reset_script()
    if name == "set_stats":   # statistics with counts of 1e9 loaded after the reset, then two steps
        rs = np.random.RandomState(2003)
        st = {"obs_mean": rs.normal(size=7) * 3.0, "obs_var": rs.uniform(0.5, 2.0, size=7), "obs_count": 1e9,
              "ret_mean": 0.75, "ret_var": 1.5, "ret_count": 1e9}
        return make_inputs(257, 7, 2003, n_steps=2), DEFAULTS, [("reset",), ("set_stats", st), ("step", 0), ("step", 1)]
    raise KeyError(name)


SCENARIOS = ("eval", "reset", "set_stats")


def nonfinite_inputs():
    """(65, 3) inputs with a NaN in one lane of column 1 at step 2, +inf in one lane of column 2 at
    step 3 and a NaN reward in the last lane at step 4; a fresh copy on every call."""
    inp = make_inputs(65, 3, 3001)
    inp["steps"][1]["obs"][7, 1] = np.nan
    inp["steps"][2]["obs"][40, 2] = np.inf
    inp["steps"][3]["reward"][64] = np.nan
    return inp


def run_script(impl, inputs, script, use_term=True, use_reward64=True):
    """Drive ``impl`` (reset(obs), step(obs, reward, done, term, reward64), .training, set_stats) and
    collect what each call returned."""
    out = []
    for op in script:
        if op[0] == "reset":
            out.append(impl.reset(inputs["obs0"]))
        elif op[0] == "step":
            s = inputs["steps"][op[1]]
            out.append(impl.step(s["obs"], s["reward"], s["done"], s["term"] if use_term else None,
                                 s["reward64"] if use_reward64 else None))
        elif op[0] == "training":
            impl.training = op[1]
        elif op[0] == "set_stats":
            impl.set_stats(op[1])
    return out


_exact_cache = {}


def exact_records(key, inputs, args, script, **kw):
    """The exact rule's records of a script, computed once per ``key`` and shared (never modified)."""
    if key not in _exact_cache:
        ex = ExactVecNormalize(inputs["L"], inputs["D"], **args, **kw)
        _exact_cache[key] = run_script(ex, inputs, script)
    return _exact_cache[key]


def exact_case(i: int):
    return exact_records(("case", i), case_inputs(i), ARGS[CASES[i][2]], plain_script())


def exact_scenario(name: str):
    inputs, args, script = scenario(name)
    return exact_records(("scenario", name), inputs, args, script)


RATIO_KEYS = ("obs_mean", "obs_var", "ret_mean", "ret_var", "obs_out", "reward_out", "term_out",
              "obs_slack", "reward_slack", "term_slack")


def judge(got, exact, clip_obs=10.0, clip_reward=10.0, fail=True, where="") -> dict:
    """Judge the records ``got`` of an implementation (dicts with ``obs_out``, optional ``reward_out`` /
    ``term_out`` / ``ep_return`` / ``ep_len`` and ``stats``) against the exact records.  Bit-exact parts
    (counts, Monitor) are asserted; returns the worst error / bound per RATIO_KEYS."""
    worst = dict.fromkeys(RATIO_KEYS, 0.0)

    def keep(k, v):
        worst[k] = max(worst[k], v)

    def bad(msg):
        if fail:
            raise AssertionError(msg)
        keep("obs_mean", math.inf)

    assert len(got) == len(exact)
    for t, (g, e) in enumerate(zip(got, exact)):
        w = f"{where} call {t}"
        for k in ("obs_mean", "obs_var", "ret_mean", "ret_var"):
            keep(k, check_stats(g["stats"][k], e["stats"][k], e["stat_bounds"][k], f"{w} {k}", fail))
        for k in ("obs_count", "ret_count"):
            if float(g["stats"][k]) != e[k]:
                bad(f"{w} {k}: {g['stats'][k]!r} != {e[k]!r}")
        z, prop, tot = e["obs"]
        r, s = check_outputs(g["obs_out"], z, tot, clip_obs, f"{w} obs_out", fail, prop)
        keep("obs_out", r), keep("obs_slack", s)
        if "reward" in e:
            z, prop, tot = e["reward"]
            r, s = check_outputs(g["reward_out"], z, tot, clip_reward, f"{w} reward_out", fail, prop)
            keep("reward_out", r), keep("reward_slack", s)
            m = e["done"]
            if g.get("term_out") is not None and m.any():
                z, prop, tot = e["term"]
                r, s = check_outputs(g["term_out"][m], z[m], tot[m], clip_obs, f"{w} term_out", fail, prop[m])
                keep("term_out", r), keep("term_slack", s)
            if g.get("ep_return") is not None and not np.array_equal(np.asarray(g["ep_return"])[m], e["ep_return"][m]):
                bad(f"{w} ep_return")
            if g.get("ep_len") is not None and not np.array_equal(np.asarray(g["ep_len"])[m], e["ep_len"][m]):
                bad(f"{w} ep_len")
    return worst


class RefAdapter:
    """oracle/vecnorm_ref.VecNormalizeRef (or a variant of it) behind the interface run_script drives."""

    def __init__(self, ref):
        self.ref = ref

    @property
    def training(self):
        return self.ref.training

    @training.setter
    def training(self, v):
        self.ref.training = v

    def _stats(self):
        r = self.ref
        return {"obs_mean": r.obs_rms.mean.copy(), "obs_var": r.obs_rms.var.copy(), "obs_count": r.obs_rms.count,
                "ret_mean": r.ret_rms.mean, "ret_var": r.ret_rms.var, "ret_count": r.ret_rms.count}

    def set_stats(self, st):
        r = self.ref
        r.obs_rms.mean, r.obs_rms.var = np.array(st["obs_mean"], np.float64), np.array(st["obs_var"], np.float64)
        r.obs_rms.count = float(st["obs_count"])
        r.ret_rms.mean, r.ret_rms.var, r.ret_rms.count = (float(st[k]) for k in ("ret_mean", "ret_var", "ret_count"))

    def reset(self, obs):
        with np.errstate(all="ignore"):
            return {"obs_out": self.ref.reset(obs), "stats": self._stats()}

    def step(self, obs, reward, done, term=None, reward64=None):
        with np.errstate(all="ignore"):
            o, r, t, er, el = self.ref.step(obs, reward, done, term, reward64=reward64)
        return {"obs_out": o, "reward_out": r, "term_out": t, "ep_return": er, "ep_len": el, "stats": self._stats()}


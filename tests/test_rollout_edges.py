"""Gains, rollouts and fused risk at the shapes where their kernels change path (cilqr_gains_batch*, cilqr_rollout_batch,
cilqr_score_rollouts, cilqr_rollout_risk, cilqr_rollout_risk_sampled; include/cilqr.h).  The neighbouring modules hold these calls to
the oracle at N = 12, 50, 2 and S = 70, 64, 300, 5, 1; every case here is a shape none of them reaches.

Expected values come from the CPU oracle alone, through the suite's helpers: o_gains, o_rollout, o_risk and the scenes of
tests/test_rollout_risk.py, `_expected` of tests/test_candidate_score.py, `_reduce` / `_case` of tests/test_rollout_risk_fused.py, the
reduction and the scene construction of tests/test_risk_sampled.py, scenes.materialise_samples.  Tolerances are the suite's own and no
other: gains and rollout entries |d| <= 1e-9 * max(1, max|oracle value| of that solve) (`_close`); the four row sums rtol 1e-9 as
test_score_rollouts_against_the_oracle; WORST_C / MAX_C 1e-9 absolute; counts, shares, rows, entries, steps and ok exact; bit
comparisons where two device paths must agree.  What makes the exact comparisons meaningful is asserted on the oracle's numbers in
the CPU tests (every finite c more than 1e-6 from 0, worst-row and worst-entry gaps above 1e-6), together with the shape property a
case is there for.  No row, solve or field is masked out of a comparison.

What each case is there to reach:
  horizon N = 1       one step: load_nominal / risk_finish with one live lane, a rollout tile of 2 states and 1 control
          N = 7       ONE exactly full rollout tile: n_st = 8 states, n_u = 7 controls
          N = 8, 16   a last rollout tile of one state and ZERO controls ((N + 1) % 8 == 1, N % 8 == 0)
          N = 9, 15   a last tile of 2 states / 1 control, and of 8 states / 7 controls after a full one
          N = 63      gains phase 0 (t <= N) fills the wavefront exactly, phase L (t < N) leaves one lane idle
          N = 64      phase 0 starts a second trip for one state; phase L, load_nominal, risk_finish fill one trip exactly
          N = 65      the second trip of every stride-64 loop over steps runs for one step
          N = 130     a third trip (t = 128, 129); the cross-trip max / min / first-step merges of risk_finish and of the sampled
                      kernel's (t, o) counters see three values per lane
          every N with S = 65: one full wavefront and a one-row tail.  Obstacle 0 of a solve lies beside the plan's LAST scored state
          and obstacle 1 beside an early one, so that for N > 64 hit steps exist at t >= 64 and below it (N = 64 scores the states
          t <= 63: there the second trip holds X_64 alone, which load_nominal and the gains' phase 0 read).
  rows    S = 1       one row, 63 idle lanes;  63 / 64 / 65  around one wavefront;  128  two full wavefronts and no tail;
          S = 255 / 256 / 257  the G = 1 -> 2 seam of launch_risk_pair: at 257 the second workgroup has ONE row, three of its
          wavefronts skip the loop (the sampled kernel: build and wait only), and the finish kernel merges two partial records
  clamps  all six branches of dyn_step (cilqr_rollout_core.hpp) bind: acc_max, acc_min, yaw_hi, yaw_lo, the speed floor, speed_max
  NaN     a NaN in each offset component, and +inf in the speed, through cilqr_rollout_batch's staging tiles
  LDS     the largest accepted shape of rollout_batch (N = 356), rollout_risk (N = 73, M = 16; M = 0 at N = 384),
          rollout_risk_sampled (N = 12, 2 x 332 samples) and the longest gains chain (N = 384); one more step or sample is refused by
          the host check, before any launch, with CILQR_ERR_UNSUPPORTED

Scenes (every seed below was fixed by a CPU search over the conditions the CPU tests assert):
  horizon  make_static(2, N, 2, O.default_params(N), seed(N)), solved by the oracle.  Its random obstacles lie 10 m and more ahead and
           the plan avoids them, so no short horizon would see a hit: obstacle 0 of solve b is put 1.0 m ahead of the plan's state at
           step N - 1 and (lat0(N) + 0.4 b) m to its LEFT, obstacle 1 beside the state at step min(2, N - 1), (lat1(N) + 0.1 b) m to
           its RIGHT, both standing, heading = that state's, constant over the horizon (the way scene R places its obstacle 0).  The
           feedback draws the rows together along the horizon, so obstacle 0 is hit by all rows or none (it gives the late hit
           steps) and obstacle 1, met while the offsets still spread the rows, gives a share the offsets decide.  The plan is not
           solved again: every call here takes the trajectory as given, and gains beside a close obstacle are the harder case.
           Offsets pose_offsets(65, 0.16, 0.16, 0.017, seed(N)); gains lamb 1 and 1e-3; rollouts k_scale 0 and 1; risk at k_scale 0.
           Sampled form (N >= 63): the two obstacles as nominal tables, PCG64(seed(N) + 1).normal(0, 1, (2, 2, 3, 3)) * POSE_SIGMA.
  rows     scene R's solves 0 and 1 cut to 4 steps by `_case(..., N=4)`.  One draw pose_offsets(257, 0.16, 0.16, 0.017, ROW_SEED); a case
           of S rows takes its first S rows (pose_offsets(S, ...) draws x, y, theta one after the other, so its rows would differ
           with S, and neither "the first rows keep their bits across S" nor "S = 257 is S = 256 merged with row 256" could hold).
           Sampled: the construction of tests/test_risk_sampled.py with (B 2, 2 x 4 samples, S 257, lat0 3.4, oseed 9, ROW_SEED).
  clamps   scene R and scene L, the oracle's gains at lamb 1, k_scale 0, 64 offsets from ONE default_rng(77): x ~ normal(0, 1),
           y ~ normal(0, 1.5), v ~ uniform(-8, 28), theta ~ normal(0, 0.3), drawn in this order.
  NaN      scene R, S = 70, its own offsets as a per-solve set; row 3 of solve 2 changed.
  LDS      make_static(1, 356, 1, seed 356), (1, 73, 16, seed 73) and (1, 384, 1, seed 384), solved by the oracle, pose_offsets of the
           same seed; sampled: the construction of tests/test_risk_sampled.py with (B 1, 2 x 332 samples, S 2, lat0 3.4, oseed 12, 7).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_risk_sampled as TS
from conftest import ROOT
from test_candidate_score import COLLISION, CONTROL, MAX_C, OBSTACLE, TRACK, UNCERTAINTY, _bits, _expected
from test_rollout_risk import SUM_RTOL, _close, _scene_l, _scene_r, o_gains, o_risk, o_rollout
from test_rollout_risk_fused import _case, _check_against, _device, _reduce, _same

gpu = pytest.mark.gpu

ABS_TOL, MARGIN = 1e-9, 1e-6
ERR_UNSUPPORTED = -4
LDS_MAX = 64 * 1024
RR_COLLISION, RR_WORST_C, RR_WORST_ROW, RR_WORST_ENTRY, RR_FIRST_STEP, RR_STEP_SHARE = range(6)
R_COLLISION, R_WORST_C, R_WORST_ROW, R_MEAN_TOTAL = range(4)
SENTINEL, SENTINEL_HITS, BASE = -777.25, -7, 3.25  # no share, count, row, entry, step or c of any case equals the first two

HORIZONS = (1, 7, 8, 9, 15, 16, 63, 64, 65, 130)
SAMPLED_HORIZONS = (63, 64, 65, 130)
HORIZON_SCENES = {1: (101, (3.0, 2.9)), 7: (107, (3.2, 3.1)), 8: (108, (3.2, 3.2)), 9: (109, (3.0, 3.2)), 15: (115, (3.0, 3.15)),
                  16: (116, (3.0, 3.25)), 63: (163, (3.2, 3.0)), 64: (164, (3.2, 3.0)), 65: (165, (3.0, 3.15)),
                  130: (330, (3.2, 3.25))}  # N: (seed, (lat of obstacle 0, lat of obstacle 1)), the first of a CPU search that meets the conditions
ROW_COUNTS = (1, 63, 64, 65, 128, 255, 256, 257)
ROW_SEED = 854  # the first seed whose rows 255 AND 256 both hit in one solve (a CPU search over 1 ... 854)
CLAMP_NAMES = ("acc_max", "acc_min", "yaw_hi", "yaw_lo", "speed floor", "speed_max")
NAN_VARIANTS = ((0, np.nan), (1, np.nan), (2, np.nan), (3, np.nan), (2, np.inf))  # (component of the offset, value)
NAN_SOLVE, NAN_ROW = 2, 3
N_ROLLOUT_LDS, N_RISK_LDS, M_RISK_LDS, N_GAINS_MAX = 356, 73, 16, 384
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


# ---- expected values from the oracle ------------------------------------------------------------------------------------------
def _rep(a, S):
    return np.ascontiguousarray(np.repeat(a, S, axis=0))  # row r belongs to solve r // S


def _build(O, s, delta, k_scale, score=True):
    """Scene `s` (p, N, X, U, k, K, poly, fl, pose, dim) with offsets delta (S, 4) shared by the solves or (B, S, 4): the oracle's
    rollouts Xr, Ur; with `score` the `_expected` rows (B, S, 8) and c (B, S, M, N, 2) of them, `risk4` = o_risk(rows) and what
    `_reduce` forms from c (risk (B, 6), step_hits, hit_rows)."""
    B, N, M = s["X"].shape[0], s["N"], s["pose"].shape[1]
    S = delta.shape[-2]
    out = dict(s, B=B, M=M, S=S, delta=np.ascontiguousarray(delta), k_scale=k_scale)
    d = np.ascontiguousarray(np.broadcast_to(delta, (B, S, 4)))
    out["Xr"], out["Ur"] = o_rollout(O, s["p"], N, s["X"], s["U"], s["k"], s["K"], d, k_scale)
    if score:
        rows, c = _expected(O, s["p"], N, out["Xr"].reshape(B * S, -1), out["Ur"].reshape(B * S, -1), _rep(s["poly"], S), _rep(s["fl"], S),
                            _rep(s["pose"], S), _rep(s["dim"], S))
        out["rows"], out["c"] = rows.reshape(B, S, 8), c.reshape(B, S, M, N, 2)
        out["risk4"] = o_risk(out["rows"])
        out.update(_reduce(out["c"]))
    return out


def _first_rows(s, S):
    """The first S rows of a built case, reduced again."""
    out = dict(s, S=S, delta=np.ascontiguousarray(s["delta"][:S]), Xr=np.ascontiguousarray(s["Xr"][:, :S]), Ur=np.ascontiguousarray(s["Ur"][:, :S]),
               rows=np.ascontiguousarray(s["rows"][:, :S]), c=np.ascontiguousarray(s["c"][:, :S]))
    out["risk4"] = o_risk(out["rows"])
    out.update(_reduce(out["c"]))
    return out


def _beside(state, ahead, lat):
    x, y, _, th = state
    return [x + ahead * np.cos(th) - lat * np.sin(th), y + ahead * np.sin(th) + lat * np.cos(th), 0.0, th]


def _horizon_scene(O, N, seed, lat):
    from cilqr_amd import scenes
    B, M = 2, 2
    p = O.default_params(N)
    sc = scenes.make_static(B, N, M, p, seed, local_plan=O.local_plan)
    r = O.solve_batch(p, N, M, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], sc["obs_pose"], sc["obs_dim"], None, threads=1)
    plan = r["X"].reshape(B, N + 1, 4)
    pose = sc["obs_pose"].reshape(B, M, N, 4).copy()
    for b in range(B):
        pose[b, 0, :, :] = _beside(plan[b, N - 1], 1.0, lat[0] + 0.4 * b)
        pose[b, 1, :, :] = _beside(plan[b, min(2, N - 1)], 1.0, -(lat[1] + 0.1 * b))
    pose = np.ascontiguousarray(pose.reshape(B, M, 4 * N))
    return dict(p=p, N=N, X=r["X"], U=r["U"], poly=sc["poly"], fl=sc["xplan_fl"], pose=pose, dim=np.ascontiguousarray(sc["obs_dim"]))


def _horizon_case(O, N, seed=None, lat=None):
    from cilqr_amd import scenes
    seed, lat = HORIZON_SCENES[N] if seed is None else (seed, lat)
    s = _horizon_scene(O, N, seed, lat)
    g = lambda lamb: o_gains(O, s["p"], N, s["X"], s["U"], s["poly"], s["fl"], s["pose"], s["dim"], None, lamb)  # noqa: E731
    s["k"], s["K"], s["ok"] = g(1.0)
    s["gains_small"] = g(1e-3)
    s = _build(O, s, scenes.pose_offsets(65, 0.16, 0.16, 0.017, seed), 0.0)
    d = np.ascontiguousarray(np.broadcast_to(s["delta"], (s["B"], s["S"], 4)))
    s["Xr1"], s["Ur1"] = o_rollout(O, s["p"], N, s["X"], s["U"], s["k"], s["K"], d, 1.0)
    s["seed"] = seed
    return s


def _horizon_sampled(O, s):
    """The sampled form on a horizon case: its two obstacles as nominal tables, 3 samples each; gains on the materialised obstacles,
    rollouts with those gains, c and the eight fields by the reduction of tests/test_risk_sampled.py."""
    from cilqr_amd import scenes
    B, N, S, n_obs, ns = s["B"], s["N"], s["S"], 2, 3
    off = np.random.Generator(np.random.PCG64(s["seed"] + 1)).normal(0.0, 1.0, (B, n_obs, ns, 3)) * scenes.POSE_SIGMA
    pose, dim, w = scenes.materialise_samples(s["pose"], s["dim"], off, N)
    pose, dim = np.ascontiguousarray(pose), np.ascontiguousarray(dim)
    k, K, ok = o_gains(O, s["p"], N, s["X"], s["U"], s["poly"], s["fl"], pose, dim, w, 1.0)
    d = np.ascontiguousarray(np.broadcast_to(s["delta"], (B, S, 4)))
    Xr, Ur = o_rollout(O, s["p"], N, s["X"], s["U"], k, K, d, 0.0)
    _, c = _expected(O, s["p"], N, Xr.reshape(B * S, -1), Ur.reshape(B * S, -1), _rep(s["poly"], S), _rep(s["fl"], S), _rep(pose, S), _rep(dim, S))
    c = c.reshape(B, S, n_obs * ns, N, 2)
    out = dict(B=B, N=N, S=S, n_obs=n_obs, ns=ns, X=s["X"], U=s["U"], poly=s["poly"], fl=s["fl"], nom_pose=s["pose"], nom_dim=s["dim"], off=off,
               weight=1.0 / ns, pose=pose, dim=dim, w=w, k=k, K=K, ok=ok, delta=s["delta"], c=c)
    out.update(TS._reduce(c, n_obs, ns))
    return out


def _rows_scene(O):
    """Scene R's solves 0 and 1 cut to 4 steps, 257 rows; `_case` truncates, `_build` adds the rollouts and the row scores."""
    from cilqr_amd import scenes
    r = _scene_r(O)
    r["k"], r["K"], ok = o_gains(O, r["p"], r["N"], r["X"], r["U"], r["poly"], r["fl"], r["pose"], r["dim"], None, 1.0)
    assert np.all(ok == 1)
    two = dict(r, B=2, **{n: np.ascontiguousarray(r[n][:2]) for n in ("X", "U", "k", "K", "poly", "fl", "pose", "dim")})
    cut = _case(O, two, 257, scenes.pose_offsets(257, 0.16, 0.16, 0.017, ROW_SEED), 0.0, N=4)
    s = _build(O, {n: cut[n] for n in ("p", "N", "X", "U", "k", "K", "poly", "fl", "pose", "dim")}, cut["delta"], 0.0)
    assert np.array_equal(_bits(s["c"]), _bits(cut["c"])) and np.array_equal(s["step_hits"], cut["step_hits"])
    return s


def _rows_sampled_scene(O):
    """tests/test_risk_sampled.py's own construction at (B 2, 2 x 4 samples, S 257): entered into its table for the length of the call."""
    TS.SCENES["edge"] = (2, 2, 4, 257, 3.4, 9, ROW_SEED)
    try:
        return TS._scene(O, "edge")
    finally:
        del TS.SCENES["edge"]


def _sampled_first_rows(s, S):
    c = np.ascontiguousarray(s["c"][:, :S])
    return dict(s, S=S, delta=np.ascontiguousarray(s["delta"][:S]), c=c, **TS._reduce(c, s["n_obs"], s["ns"]))


def _wide_offsets():
    rng = np.random.default_rng(77)
    x, y, v, th = rng.normal(0.0, 1.0, 64), rng.normal(0.0, 1.5, 64), rng.uniform(-8.0, 28.0, 64), rng.normal(0.0, 0.3, 64)
    return np.ascontiguousarray(np.stack([x, y, v, th], axis=1))


def _clamp_counts(p, N, Xr, Ur):
    """Per clamp of oracle_forward_simulate — acc = fmax(fmin(u0, acc_max), acc_min); yaw = fmax(fmin(u1, v tan(max)/L), v tan(min)/L);
    v' = fmin(fmax(v + acc dt, 0), speed_max) — at how many row-steps the control or the speed lies beyond the bound it is compared
    with, and the smallest distance of any of them from that bound."""
    B, S = Xr.shape[:2]
    v = Xr.reshape(B, S, N + 1, 4)[:, :, :N, 2]
    u = Ur.reshape(B, S, N, 2)
    hi, lo = v * np.tan(p.steer_angle_max) / p.wheelbase, v * np.tan(p.steer_angle_min) / p.wheelbase
    v_next = v + np.maximum(np.minimum(u[..., 0], p.acc_max), p.acc_min) * p.timestep
    pairs = ((u[..., 0], p.acc_max, 1), (u[..., 0], p.acc_min, -1), (u[..., 1], hi, 1), (u[..., 1], lo, -1), (v_next, 0.0, -1),
             (v_next, p.speed_max, 1))
    counts = [int(np.sum(sign * (value - bound) > 0)) for value, bound, sign in pairs]
    gap = min(float(np.min(np.abs(value - bound))) for value, bound, _ in pairs)
    return counts, gap


def _clamp_cases(O):
    out = {}
    for name, s in (("R", _scene_r(O)), ("L", _scene_l(O))):
        s = {n: s[n] for n in ("p", "N", "X", "U", "poly", "fl", "pose", "dim")}
        s["k"], s["K"], ok = o_gains(O, s["p"], s["N"], s["X"], s["U"], s["poly"], s["fl"], s["pose"], s["dim"], None, 1.0)
        assert np.all(ok == 1)
        out[name] = _build(O, s, _wide_offsets(), 0.0, score=name == "R")
    return out


def _nan_cases(O):
    """Scene R, S = 70, per-solve offsets: the clean set, and the five variants of NAN_VARIANTS in row NAN_ROW of solve NAN_SOLVE."""
    s = _scene_r(O)
    s = {n: s[n] for n in ("p", "N", "X", "U", "poly", "fl", "pose", "dim", "delta")}
    s["k"], s["K"], ok = o_gains(O, s["p"], s["N"], s["X"], s["U"], s["poly"], s["fl"], s["pose"], s["dim"], None, 1.0)
    clean = np.ascontiguousarray(np.broadcast_to(s.pop("delta"), (s["X"].shape[0], 70, 4)))
    out = [_build(O, s, clean, 0.0, score=False)]
    for comp, value in NAN_VARIANTS:
        d = clean.copy()
        d[NAN_SOLVE, NAN_ROW, comp] = value
        out.append(_build(O, s, d, 0.0, score=False))
    return out


def _lds_rollout_case(O):
    from cilqr_amd import scenes
    N = N_ROLLOUT_LDS
    p = O.default_params(N)
    sc = scenes.make_static(1, N, 1, p, 356, local_plan=O.local_plan)
    r = O.solve_batch(p, N, 1, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], sc["obs_pose"], sc["obs_dim"], None, threads=1)
    s = dict(p=p, N=N, X=r["X"], U=r["U"], poly=sc["poly"], fl=sc["xplan_fl"], pose=sc["obs_pose"], dim=sc["obs_dim"])
    s["k"], s["K"], s["ok"] = o_gains(O, p, N, s["X"], s["U"], s["poly"], s["fl"], s["pose"], s["dim"], None, 1.0)
    return _build(O, s, scenes.pose_offsets(65, 0.16, 0.16, 0.017, 356), 0.0, score=False)


LDS_RISK_SEED = 73


def _lds_risk_case(O, seed=LDS_RISK_SEED):
    from cilqr_amd import scenes
    N, M = N_RISK_LDS, M_RISK_LDS
    p = O.default_params(N)
    sc = scenes.make_static(1, N, M, p, seed, local_plan=O.local_plan)
    r = O.solve_batch(p, N, M, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], sc["obs_pose"], sc["obs_dim"], None, threads=1)
    s = dict(p=p, N=N, X=r["X"], U=r["U"], poly=sc["poly"], fl=sc["xplan_fl"], pose=sc["obs_pose"], dim=sc["obs_dim"])
    s["k"], s["K"], s["ok"] = o_gains(O, p, N, s["X"], s["U"], s["poly"], s["fl"], s["pose"], s["dim"], None, 1.0)
    return _build(O, s, scenes.pose_offsets(64, 0.16, 0.16, 0.017, seed), 0.0)


def _lds_gains_case(O):
    from cilqr_amd import scenes
    N = N_GAINS_MAX
    p = O.default_params(N)
    sc = scenes.make_static(1, N, 1, p, 384, local_plan=O.local_plan)
    r = O.solve_batch(p, N, 1, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], sc["obs_pose"], sc["obs_dim"], None, threads=1)
    s = dict(p=p, N=N, X=r["X"], U=r["U"], poly=sc["poly"], fl=sc["xplan_fl"], pose=sc["obs_pose"], dim=sc["obs_dim"])
    s["k"], s["K"], s["ok"] = o_gains(O, p, N, s["X"], s["U"], s["poly"], s["fl"], s["pose"], s["dim"], None, 1.0)
    return s


def _sampled_lds_bytes(N, n_obs, n_samples):
    """include/cilqr.h, cilqr_rollout_risk_sampled."""
    return 8 * (14 * N + 4) + 96 * n_obs * n_samples + 4 * N * (1 + n_obs) + 160


def _largest_sample_count(N, n_obs):
    ns = (LDS_MAX - _sampled_lds_bytes(N, n_obs, 0)) // (96 * n_obs)
    assert _sampled_lds_bytes(N, n_obs, ns) <= LDS_MAX < _sampled_lds_bytes(N, n_obs, ns + 1)
    return ns


def _lds_sampled_case(O):
    """tests/test_risk_sampled.py's construction with B 1, 2 obstacles x the largest sample count that fits, S 2."""
    ns = _largest_sample_count(TS.N_STEPS, 2)
    TS.SCENES["edge"] = (1, 2, ns, 2, 3.4, 12, 7)
    try:
        return TS._scene(O, "edge")
    finally:
        del TS.SCENES["edge"]


class _Cases:
    """Every case of this module, built from the oracle on first use and never modified."""

    def __init__(self, O):
        self.O, self._made = O, {}

    def get(self, kind, key=None):
        if (kind, key) not in self._made:
            O = self.O
            make = {"horizon": lambda: _horizon_case(O, key), "horizon sampled": lambda: _horizon_sampled(O, self.get("horizon", key)),
                    "rows": lambda: _rows_scene(O), "rows sampled": lambda: _rows_sampled_scene(O), "clamps": lambda: _clamp_cases(O),
                    "nan": lambda: _nan_cases(O), "lds rollout": lambda: _lds_rollout_case(O), "lds risk": lambda: _lds_risk_case(O),
                    "lds gains": lambda: _lds_gains_case(O), "lds sampled": lambda: _lds_sampled_case(O)}[kind]
            self._made[(kind, key)] = make()
        return self._made[(kind, key)]


@pytest.fixture(scope="module")
def cases(oracle):
    return _Cases(oracle)


def _conditions(s, what):
    """What keeps the exact comparisons from hiding a failure, on the oracle's numbers alone.  One row is its solve's worst row
    whatever its c; one entry likewise: the gaps are asserted where there are two to tell apart."""
    c, B, S, M, N = s["c"], s["B"], s["S"], s["M"], s["N"]
    assert not np.isnan(c).any() and np.all(np.isfinite(s["Xr"])), what
    finite = c[np.isfinite(c)]
    print("%s: min|c| %.3g, hits per solve %s of %d, first steps %s" % (what, np.min(np.abs(finite)), s["hit_rows"].tolist(), S,
                                                                      s["risk"][:, RR_FIRST_STEP].astype(int).tolist()))
    assert np.min(np.abs(finite)) > MARGIN, what                # every c that decides a hit
    assert np.array_equal(s["rows"][:, :, MAX_C], c.max(axis=(2, 3, 4)))  # (the row scores decide by the same c)
    assert np.all(np.isfinite(s["rows"][:, :, [TRACK, CONTROL, OBSTACLE, UNCERTAINTY]]))
    flat = c.max(axis=4).reshape(B, S, M * N)
    if S > 1:
        row_max = np.sort(flat.max(axis=2), axis=1)
        print("  worst rows %s, smallest row gap %.3g" % (s["risk"][:, RR_WORST_ROW].astype(int).tolist(), np.min(row_max[:, -1] - row_max[:, -2])))
        assert np.min(row_max[:, -1] - row_max[:, -2]) > MARGIN, what  # the worst row of every solve is decided
    if M * N > 1:
        ent = np.sort(np.stack([flat[b, int(s["risk"][b, RR_WORST_ROW])] for b in range(B)]), axis=1)
        print("  worst entries %s, smallest entry gap %.3g" % (s["risk"][:, RR_WORST_ENTRY].astype(int).tolist(), np.min(ent[:, -1] - ent[:, -2])))
        assert np.min(ent[:, -1] - ent[:, -2]) > MARGIN, what          # and the worst entry within it
    assert np.array_equal(s["risk"][:, RR_WORST_ROW], s["risk4"][:, R_WORST_ROW])


def _sampled_conditions(s, what):
    """As test_conditions of tests/test_risk_sampled.py: every c that decides a hit, and the two largest c of every solve."""
    c, B, S = s["c"], s["B"], s["S"]
    assert not np.isnan(c).any()
    top = np.sort(c.max(axis=4).reshape(B, -1), axis=1)
    gap = float(np.min(top[:, -1] - top[:, -2]))
    print("%s: min|c| %.3g, top-two gap %.3g, rows that hit %s of %d, sum of max h %s, pair maxima %s"
          % (what, np.min(np.abs(c[np.isfinite(c)])), gap, s["any_rows"].tolist(), S, s["sum_max"].tolist(), s["pair_max"].tolist()))
    assert np.min(np.abs(c[np.isfinite(c)])) > MARGIN and gap > MARGIN, what


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def _horizon_conditions(s):
    N = s["N"]
    assert (s["B"], s["M"], s["S"]) == (2, 2, 65)
    _conditions(s, "N = %d" % N)
    tile = {1: (2, 1), 7: (0, 7), 8: (1, 0), 9: (2, 1), 15: (0, 7), 16: (1, 0), 63: (0, 7), 64: (1, 0), 65: (2, 1), 130: (3, 2)}[N]
    assert ((N + 1) % 8, N % 8) == tile                        # states and controls of the last rollout tile (0 states: a full one)
    assert (N // 64, (N + 1 + 63) // 64) == {1: (0, 1), 7: (0, 1), 8: (0, 1), 9: (0, 1), 15: (0, 1), 16: (0, 1), 63: (0, 1), 64: (1, 2),
                                             65: (1, 2), 130: (2, 3)}[N]  # full trips over t < N; trips over t <= N
    assert np.all(s["ok"] == 1) and np.all(s["gains_small"][2] == 1)
    hits = s["step_hits"]
    assert np.all(s["risk"][:, RR_FIRST_STEP] >= 0)            # FIRST_STEP decided: every solve has a hit step ...
    assert np.any((s["hit_rows"] > 0) & (s["hit_rows"] < 65))  # ... and a share the offsets decide
    if N > 64:  # (N = 64 scores the states t <= 63: it has no step 64)
        late = [np.nonzero(h[64:])[0] + 64 for h in hits]
        print("  hit steps at t >= 64: %s; below: %s" % ([v.tolist() for v in late], [np.nonzero(h[:64])[0].tolist() for h in hits]))
        assert any(len(v) for v in late) and hits[:, :64].any()  # the second trip of risk_finish carries counts, and the first
    if N == 130:
        assert hits[:, 128:].any()


def _horizon_sampled_conditions(s):
    N = s["N"]
    _sampled_conditions(s, "sampled, N = %d" % N)
    assert np.all(s["ok"] == 1)
    assert np.all(s["risk"][:, TS.FIRST_STEP] >= 0)
    if N > 64:
        pair = s["h"].sum(axis=1)                              # (B, n_obs, N): the (t, o) counters
        assert s["step_hits"][:, 64:].any() and s["step_hits"][:, :64].any() and pair[:, :, 64:].any() and pair[:, :, :64].any()


@pytest.mark.parametrize("N", HORIZONS)
def test_conditions_horizon(cases, N):
    _horizon_conditions(cases.get("horizon", N))


@pytest.mark.parametrize("N", SAMPLED_HORIZONS)
def test_conditions_horizon_sampled(cases, N):
    _horizon_sampled_conditions(cases.get("horizon sampled", N))


def test_conditions_rows(cases):
    full, sampled = cases.get("rows"), cases.get("rows sampled")
    assert (full["B"], full["N"], full["M"], full["S"]) == (2, 4, 3, 257) and (sampled["B"], sampled["ns"], sampled["S"]) == (2, 4, 257)
    hits, shits = {}, {}
    for S in ROW_COUNTS:
        s = _first_rows(full, S)
        _conditions(s, "S = %d" % S)
        hits[S] = s["hit_rows"]
        t = _sampled_first_rows(sampled, S)
        _sampled_conditions(t, "sampled, S = %d" % S)
        shits[S] = t["sum_max"]
        assert (-(-S // 256), min(4, -(-S // 64))) == {1: (1, 1), 63: (1, 1), 64: (1, 1), 65: (1, 2), 128: (1, 2), 255: (1, 4), 256: (1, 4),
                                                       257: (2, 4)}[S]  # workgroups per solve, wavefronts per workgroup
    # the one-row workgroup of S = 257 matters: row 256 hits, or is the worst row, in at least one solve
    last = _first_rows(full, 257)
    row_hits = (last["c"][:, 256].max(axis=3) > 0).any(axis=(1, 2))
    print("row 256: hits %s, worst rows %s; hit rows at 255 / 256 / 257: %s %s %s" % (row_hits.tolist(), last["risk"][:, RR_WORST_ROW].tolist(),
                                                                                     hits[255].tolist(), hits[256].tolist(), hits[257].tolist()))
    assert row_hits.any() or np.any(last["risk"][:, RR_WORST_ROW] == 256)
    assert np.any((hits[255] != hits[256]) & (hits[256] != hits[257]))  # the counts differ across the seam in one solve at least
    assert np.any(shits[256] != shits[257])


def test_conditions_clamps(cases):
    """All six clamps bind in the oracle's rollouts, none within 1e-6 of its bound; scene R's c keeps its margins under these offsets."""
    both = cases.get("clamps")
    for name in ("R", "L"):
        s = both[name]
        counts, gap = _clamp_counts(s["p"], s["N"], s["Xr"], s["Ur"])
        print("scene %s, %d row-steps: %s, smallest distance from a bound %.3g, max|X| %.3g"
              % (name, s["B"] * s["S"] * s["N"], dict(zip(CLAMP_NAMES, counts)), gap, np.max(np.abs(s["Xr"]))))
        assert all(n > 0 for n in counts), (name, counts)
        if name == "R":
            assert counts == [679, 2823, 114, 192, 48, 6]      # (as counted when the offsets were chosen)
        assert gap > MARGIN and np.all(np.isfinite(s["Xr"])) and np.all(np.isfinite(s["Ur"]))
    assert both["R"]["S"] == 64
    _conditions(both["R"], "scene R, wide offsets")


def test_conditions_nan(cases):
    """The oracle defines what a NaN or an infinite offset becomes: only row NAN_ROW of solve NAN_SOLVE changes, and it does."""
    clean, variants = cases.get("nan")[0], cases.get("nan")[1:]
    assert np.all(np.isfinite(clean["Xr"])) and np.all(np.isfinite(clean["Ur"]))
    for (comp, value), s in zip(NAN_VARIANTS, variants):
        bad = ~np.isfinite(s["Xr"])
        print("offset[%d] = %s: %d of %d entries of the row not finite, %d NaN" % (comp, value, bad[NAN_SOLVE, NAN_ROW].sum(), bad.shape[2],
                                                                             np.isnan(s["Xr"][NAN_SOLVE, NAN_ROW]).sum()))
        assert bad[NAN_SOLVE, NAN_ROW].any()
        bad[NAN_SOLVE, NAN_ROW] = False
        assert not bad.any()
        keep = np.ones(s["Xr"].shape[:2], dtype=bool)
        keep[NAN_SOLVE, NAN_ROW] = False
        assert np.array_equal(_bits(s["Xr"][keep]), _bits(clean["Xr"][keep])) and np.array_equal(_bits(s["Ur"][keep]), _bits(clean["Ur"][keep]))


def test_lds_arithmetic_and_conditions(cases):
    """The header's formulas, evaluated here: the largest shapes that fit 64 KiB and the first that do not."""
    h = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    assert int(re.search(r"#define\s+CILQR_MAX_HORIZON\s+(\d+)", h).group(1)) == N_GAINS_MAX
    assert "8*(14*N + 4) + 48*M*N + 4*N + 112 bytes" in h and "8*(14*N + 4) + 96*n_obs*n_samples + 4*N*(1 + n_obs) + 160 bytes" in h
    rollout = lambda N: 112 * N + 25632  # noqa: E731  (14 doubles per step + X_N + 64 x (33 + 17) doubles of staging)
    risk = lambda N, M: 8 * (14 * N + 4) + 48 * M * N + 4 * N + 112  # noqa: E731
    gains = lambda N, path: 8 * (2 * path + 2 * (N + 1) + 16 * N)  # noqa: E731  (cilqr_gains.hip: sx, sy, cos, sin, 16 per step)
    assert rollout(N_ROLLOUT_LDS) <= LDS_MAX < rollout(N_ROLLOUT_LDS + 1) and N_ROLLOUT_LDS + 1 <= N_GAINS_MAX
    assert risk(N_RISK_LDS, M_RISK_LDS) == 64676 <= LDS_MAX < risk(N_RISK_LDS + 1, M_RISK_LDS)
    assert risk(N_GAINS_MAX, 0) <= LDS_MAX
    assert _largest_sample_count(TS.N_STEPS, 2) == 332
    assert gains(N_GAINS_MAX, 200) <= LDS_MAX and cases.O.default_params().num_of_local_wpts * 10 == 200
    s = cases.get("lds rollout")
    assert np.all(s["ok"] == 1) and np.all(np.isfinite(s["Xr"])) and s["Xr"].shape == (1, 65, 4 * (N_ROLLOUT_LDS + 1))
    s = cases.get("lds risk")
    assert (s["B"], s["N"], s["M"], s["S"]) == (1, N_RISK_LDS, M_RISK_LDS, 64)
    _conditions(s, "N = 73, M = 16")
    assert s["hit_rows"][0] > 0 and 0 < np.count_nonzero(s["step_hits"][0]) < N_RISK_LDS  # steps with hits and steps without
    assert s["risk"][0, RR_WORST_ENTRY] >= 8 * N_RISK_LDS     # an obstacle of the table's second half decides the worst c
    s = cases.get("lds sampled")
    assert (s["B"], s["n_obs"], s["ns"], s["S"]) == (1, 2, 332, 2)
    _sampled_conditions(s, "2 x 332 samples")
    assert 0 < s["sum_max"][0] < 2 * 332                       # some samples are hit and some are not
    g = cases.get("lds gains")
    assert np.all(g["ok"] == 1) and np.all(np.isfinite(g["K"])) and np.any(g["K"][0, :8] != 0)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(), max_batch=8 * 70, max_horizon=130, max_obstacles=8, device=0)
    try:
        yield s
    finally:
        s.close()


def _compare_rollouts(sv, s, what, k_scales=(0.0,)):
    """cilqr_rollout_batch fed the oracle's gains against o_rollout.  Returns the k_scale-0 result."""
    first = None
    for ks in k_scales:
        wx, wu = (s["Xr"], s["Ur"]) if ks == 0.0 else (s["Xr1"], s["Ur1"])
        got = sv.rollout_batch(s["N"], s["X"], s["U"], s["k"], s["K"], s["delta"], k_scale=ks)
        _close(got["X"], wx, "%s: rollout, k_scale %g, X" % (what, ks))
        _close(got["U"], wu, "%s: rollout, k_scale %g, U" % (what, ks))
        first = got if first is None else first
    return first


def _compare_risk(cilqr, sv, s, what):
    """cilqr_rollout_risk (host and device form) against `_reduce` of the oracle's c; its WORST_C bit-equal to the worst SCORE_MAX_C of
    cilqr_score_rollouts on the stored rows of the device (the identity of test_against_the_stored_rows_path); cilqr_score_rollouts on
    the oracle's rollouts against `_expected` and o_risk."""
    B, S, N = s["B"], s["S"], s["N"]
    risk, hits, _ = sv.rollout_risk(N, s["X"], s["U"], s["k"], s["K"], s["delta"], s["pose"], s["dim"], k_scale=s["k_scale"])
    _check_against(risk, hits, s, what + ": fused, host form")
    drisk, dhits, _, rows, risk3 = _device(cilqr, sv, s, three_call=True)
    assert _same((risk, hits), (drisk, dhits)), what
    assert np.array_equal(_bits(drisk[:, RR_WORST_C]), _bits(rows[:, :, MAX_C].max(axis=1))), what
    assert np.array_equal(_bits(drisk[:, RR_WORST_C]), _bits(risk3[:, R_WORST_C])), what
    assert np.array_equal(drisk[:, RR_COLLISION], risk3[:, R_COLLISION]) and np.array_equal(drisk[:, RR_WORST_ROW], risk3[:, R_WORST_ROW]), what
    got = sv.score_rollouts(N, s["Xr"], s["Ur"], s["poly"], s["fl"], s["pose"], s["dim"])
    want, want4 = s["rows"], s["risk4"]
    for f, name in ((TRACK, "TRACK"), (CONTROL, "CONTROL"), (OBSTACLE, "OBSTACLE"), (UNCERTAINTY, "UNCERTAINTY")):
        err = np.abs(got["row_score"][:, :, f] - want[:, :, f]) / np.maximum(np.abs(want[:, :, f]), 1e-300)
        print("%s: row %s max relative error %.3g" % (what, name, np.max(err) if np.any(want[:, :, f]) else 0.0))
        assert np.allclose(got["row_score"][:, :, f], want[:, :, f], rtol=SUM_RTOL, atol=0.0), (what, name)
    print("%s: row MAX_C max absolute error %.3g" % (what, np.max(np.abs(got["row_score"][:, :, MAX_C] - want[:, :, MAX_C]))))
    assert np.max(np.abs(got["row_score"][:, :, MAX_C] - want[:, :, MAX_C])) <= ABS_TOL, what
    assert np.array_equal(got["row_score"][:, :, COLLISION], want[:, :, COLLISION]), what
    assert np.array_equal(got["risk"][:, R_COLLISION], want4[:, R_COLLISION]) and np.array_equal(got["risk"][:, R_WORST_ROW], want4[:, R_WORST_ROW]), what
    assert np.max(np.abs(got["risk"][:, R_WORST_C] - want4[:, R_WORST_C])) <= ABS_TOL, what
    assert np.allclose(got["risk"][:, R_MEAN_TOTAL], want4[:, R_MEAN_TOTAL], rtol=SUM_RTOL, atol=0.0), what
    return risk, hits


def _sampled_host(sv, s):
    return sv.rollout_risk_sampled(s["N"], s["X"], s["U"], s["k"], s["K"], s["delta"], s["nom_pose"], s["nom_dim"], s["off"], k_scale=0.0)


@gpu
@pytest.mark.parametrize("N", HORIZONS)
def test_horizon_edges(cilqr, solver, cases, N):
    s = cases.get("horizon", N)
    what = "N = %d" % N
    for lamb, (k, K, ok) in ((1.0, (s["k"], s["K"], s["ok"])), (1e-3, s["gains_small"])):
        got = solver.gains_batch(N, s["X"], s["U"], s["poly"], s["fl"], s["pose"], s["dim"], lamb=lamb)
        assert np.array_equal(got["ok"], ok), (what, lamb)
        _close(got["k"], k, "%s: gains, lamb %g, k" % (what, lamb))
        _close(got["K"], K, "%s: gains, lamb %g, K" % (what, lamb))
    _compare_rollouts(solver, s, what, k_scales=(0.0, 1.0))
    _compare_risk(cilqr, solver, s, what)


@gpu
@pytest.mark.parametrize("N", SAMPLED_HORIZONS)
def test_horizon_edges_sampled(solver, cases, N):
    s = cases.get("horizon sampled", N)
    what = "sampled, N = %d" % N
    got = solver.gains_batch_sampled(N, s["X"], s["U"], s["poly"], s["fl"], s["nom_pose"], s["nom_dim"], s["off"], s["weight"], lamb=1.0)
    assert np.array_equal(got["ok"], s["ok"])
    _close(got["k"], s["k"], what + ": gains, k")
    _close(got["K"], s["K"], what + ": gains, K")
    mat = solver.gains_batch(N, s["X"], s["U"], s["poly"], s["fl"], s["pose"], s["dim"], s["w"], lamb=1.0)
    assert TS._same((got["k"], got["K"], got["ok"]), (mat["k"], mat["K"], mat["ok"]))
    risk, hits, _ = _sampled_host(solver, s)
    TS._check_against(risk, hits, s, what)


@gpu
def test_row_count_edges(cilqr, solver, cases):
    full, sampled = cases.get("rows"), cases.get("rows sampled")
    N = full["N"]
    stored, fused = {}, {}
    for S in ROW_COUNTS:
        s, what = _first_rows(full, S), "S = %d" % S
        stored[S] = _compare_rollouts(solver, s, what)
        fused[S] = _compare_risk(cilqr, solver, s, what)
        t = _sampled_first_rows(sampled, S)
        risk, hits, _ = _sampled_host(solver, t)
        TS._check_against(risk, hits, t, "sampled, " + what)
    # a row depends on its own inputs alone: the first min(S, 63) rows keep their bits whatever S is
    for S in ROW_COUNTS:
        n = min(S, 63)
        for f in ("X", "U"):
            assert np.array_equal(_bits(stored[S][f][:, :n]), _bits(stored[257][f][:, :n])), (S, f)
    # S = 257 (two workgroups, the second with one row) is S = 256 merged with row 256 alone, field for field
    r256, h256 = fused[256]
    r257, h257 = fused[257]
    r1, h1, _ = solver.rollout_risk(N, full["X"], full["U"], full["k"], full["K"], full["delta"][256:257], full["pose"], full["dim"], k_scale=0.0)
    assert np.all(r1[:, RR_WORST_ROW] == 0)
    merged, mhits = np.zeros_like(r257), h256 + h1
    later = r1[:, RR_WORST_C] > r256[:, RR_WORST_C]  # (an equal c leaves the lower row)
    merged[:, RR_COLLISION] = (np.rint(r256[:, RR_COLLISION] * 256) + r1[:, RR_COLLISION]) / 257
    merged[:, RR_WORST_C] = np.where(later, r1[:, RR_WORST_C], r256[:, RR_WORST_C])
    merged[:, RR_WORST_ROW] = np.where(later, 256, r256[:, RR_WORST_ROW])
    merged[:, RR_WORST_ENTRY] = np.where(later, r1[:, RR_WORST_ENTRY], r256[:, RR_WORST_ENTRY])
    merged[:, RR_FIRST_STEP] = np.where((mhits > 0).any(axis=1), (mhits > 0).argmax(axis=1), -1)
    merged[:, RR_STEP_SHARE] = mhits.max(axis=1) / 257
    print("S = 257 against 256 + 1: shares %s / %s, worst rows %s" % (r257[:, RR_COLLISION].tolist(), merged[:, RR_COLLISION].tolist(),
                                                                     r257[:, RR_WORST_ROW].tolist()))
    assert _same((r257, h257), (merged, mhits))


@gpu
def test_clamp_edges(cilqr, solver, cases):
    both = cases.get("clamps")
    for name in ("R", "L"):
        _compare_rollouts(solver, both[name], "scene %s, wide offsets" % name)
    _compare_risk(cilqr, solver, both["R"], "scene R, wide offsets")


@gpu
def test_non_finite_offsets_through_the_stored_rows(solver, cases):
    clean, variants = cases.get("nan")[0], cases.get("nan")[1:]
    N = clean["N"]
    run = lambda s: solver.rollout_batch(N, s["X"], s["U"], s["k"], s["K"], s["delta"], k_scale=0.0)  # noqa: E731
    base = run(clean)
    _close(base["X"], clean["Xr"], "clean, X")
    keep = np.ones(clean["Xr"].shape[:2], dtype=bool)
    keep[NAN_SOLVE, NAN_ROW] = False
    for (comp, value), s in zip(NAN_VARIANTS, variants):
        got = run(s)
        for f, want in (("X", s["Xr"]), ("U", s["Ur"])):
            what = "offset[%d] = %s, %s" % (comp, value, f)
            assert np.array_equal(np.isnan(got[f]), np.isnan(want)), what
            assert np.array_equal(np.isposinf(got[f]), np.isposinf(want)) and np.array_equal(np.isneginf(got[f]), np.isneginf(want)), what
            ok = np.isfinite(want)
            _close(np.where(ok, got[f], 0.0), np.where(ok, want, 0.0), what + " (finite entries)")
            assert np.array_equal(_bits(got[f][keep]), _bits(base[f][keep])), what


def _raw_rollout_risk(cilqr, sv, s, pose, dim):
    """cilqr_rollout_risk through the C-ABI on outputs filled with sentinels."""
    B, N, S = s["X"].shape[0], s["N"], s["delta"].shape[0]
    risk, hits, total, base = np.full((B, 6), SENTINEL), np.full((B, N), SENTINEL_HITS, dtype=np.int32), np.full(B, SENTINEL), np.full(B, BASE)
    obs, M = None, 0
    if pose is not None:
        M, bs, ms, ts, wbs = cilqr.obstacle_strides(pose.shape, dim.shape, None, B, N)
        obs = cilqr.Obstacles(pose.ctypes.data, dim.ctypes.data, None, bs, ms, ts, wbs)
    cilqr._check(cilqr.lib().cilqr_rollout_risk(sv._h, B, N, M, S, _p(s["X"]), _p(s["U"]), _p(s["k"]), _p(s["K"]), _p(s["delta"]), C.c_int64(0),
                                                C.c_double(0.0), None if obs is None else C.byref(obs), C.c_double(1.0), _p(base), _p(risk),
                                                _p(hits, _ip), _p(total)))
    assert not np.any(risk == SENTINEL) and not np.any(hits == SENTINEL_HITS) and np.array_equal(total, base)  # every element written
    return risk, hits


@gpu
def test_rollouts_and_gains_at_the_lds_limit(cilqr, cases):
    """cilqr_rollout_batch: N = 356 takes 65 504 of 65 536 bytes and runs; N = 357 is refused by the host check and leaves the handle
    as it was.  cilqr_gains_batch at N = 384, the longest chain a handle takes.  cilqr_rollout_risk with M = 0 at N = 384."""
    s, g = cases.get("lds rollout"), cases.get("lds gains")
    N, S = s["N"], s["S"]
    sv = cilqr.Solver(cilqr.default_params(N_GAINS_MAX), max_batch=S, max_horizon=N_GAINS_MAX, max_obstacles=1, device=0)
    try:
        first = _compare_rollouts(sv, s, "N = %d" % N)
        z = lambda *shape: np.zeros(shape)  # noqa: E731
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*LDS" % ERR_UNSUPPORTED):
            sv.rollout_batch(N + 1, z(1, 4 * (N + 2)), z(1, 2 * (N + 1)), z(1, 2 * (N + 1)), z(1, 8 * (N + 1)), s["delta"])
        again = sv.rollout_batch(N, s["X"], s["U"], s["k"], s["K"], s["delta"], k_scale=0.0)
        assert _same((again["X"], again["U"]), (first["X"], first["U"]))
        M = N_GAINS_MAX
        got = sv.gains_batch(M, g["X"], g["U"], g["poly"], g["fl"], g["pose"], g["dim"], lamb=1.0)
        assert np.array_equal(got["ok"], g["ok"])
        _close(got["k"], g["k"], "N = %d: gains, k" % M)
        _close(got["K"], g["K"], "N = %d: gains, K" % M)
        none = dict(N=M, X=g["X"], U=g["U"], k=g["k"], K=g["K"], delta=s["delta"][:64])
        risk, hits = _raw_rollout_risk(cilqr, sv, none, None, None)
        assert np.all(np.isneginf(risk[:, RR_WORST_C])) and not hits.any()
        for f, v in ((RR_COLLISION, 0.0), (RR_WORST_ROW, -1.0), (RR_WORST_ENTRY, -1.0), (RR_FIRST_STEP, -1.0), (RR_STEP_SHARE, 0.0)):
            assert np.array_equal(risk[:, f], np.full(1, v)), f
    finally:
        sv.close()


@gpu
def test_fused_risk_at_the_lds_limit(cilqr, cases):
    """cilqr_rollout_risk at N = 73, M = 16: 64 676 of 65 536 bytes, the last obstacle entries and the counters behind them at the top
    of the carve-up; N = 74 is refused by the host check."""
    s = cases.get("lds risk")
    N, M = s["N"], s["M"]
    sv = cilqr.Solver(cilqr.default_params(N + 1), max_batch=64, max_horizon=N + 1, max_obstacles=M, device=0)
    try:
        risk, hits = _raw_rollout_risk(cilqr, sv, s, s["pose"], s["dim"])
        _check_against(risk, hits, s, "N = %d, M = %d" % (N, M))
        z = lambda *shape: np.zeros(shape)  # noqa: E731
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*LDS" % ERR_UNSUPPORTED):
            sv.rollout_risk(N + 1, z(1, 4 * (N + 2)), z(1, 2 * (N + 1)), z(1, 2 * (N + 1)), z(1, 8 * (N + 1)), s["delta"], z(1, M, 4 * (N + 1)),
                            np.ones((1, M, 2 * (N + 1))))
        again = _raw_rollout_risk(cilqr, sv, s, s["pose"], s["dim"])
        assert _same(again, (risk, hits))
    finally:
        sv.close()


@gpu
def test_sampled_risk_at_the_lds_limit(cilqr, cases):
    """cilqr_rollout_risk_sampled at N = 12 with 2 x 332 samples: 65 424 of 65 536 bytes; 2 x 333 samples are refused by the host check."""
    s = cases.get("lds sampled")
    B, N, n_obs, ns, S = s["B"], s["N"], s["n_obs"], s["ns"], s["S"]
    sv = cilqr.Solver(cilqr.default_params(N), max_batch=2, max_horizon=N, max_obstacles=n_obs * (ns + 1), device=0)
    try:
        risk, hits, total, base = np.full((B, 8), SENTINEL), np.full((B, N), SENTINEL_HITS, dtype=np.int32), np.full(B, SENTINEL), np.full(B, BASE)
        cilqr._check(cilqr.lib().cilqr_rollout_risk_sampled(sv._h, B, N, n_obs, ns, S, _p(s["X"]), _p(s["U"]), _p(s["k"]), _p(s["K"]), _p(s["delta"]),
                                                            C.c_int64(0), C.c_double(0.0), _p(s["nom_pose"]), _p(s["nom_dim"]), _p(s["off"]),
                                                            C.c_double(1.0), _p(base), _p(risk), _p(hits, _ip), _p(total)))
        assert not np.any(risk == SENTINEL) and not np.any(hits == SENTINEL_HITS) and np.array_equal(total, base)
        TS._check_against(risk, hits, s, "2 x %d samples" % ns)
        z = lambda *shape: np.zeros(shape)  # noqa: E731
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*LDS" % ERR_UNSUPPORTED):
            sv.rollout_risk_sampled(N, s["X"], s["U"], s["k"], s["K"], s["delta"], s["nom_pose"], s["nom_dim"], z(B, n_obs, ns + 1, 3))
        again = _sampled_host(sv, s)
        assert TS._same(again[:2], (risk, hits))
    finally:
        sv.close()

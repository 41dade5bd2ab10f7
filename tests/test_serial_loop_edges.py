"""Horizons at which the solve's two serial loops change shape (GPU; the HIP path through the C-ABI against the CPU oracle).

Phase R (riccati_mfma) and phase F (forward_smem) run two steps per trip and peel the last one or two; phase F asks for the
record of step i + 1 while step i computes, the last request going to the dump record behind the horizon, and addresses its
records and its LDS stores from positions that move once per trip.  What can go wrong there shows at the trip counts' edges:
N = 1 (no trip, one peeled step), 2 (one trip in F, two peeled steps in R), 3, 4 (odd and even trip counts), 63 and 64 (the
last horizons with one step per lane in phase L), 65 and 127 (two steps per lane).  Every horizon runs on the plan the library
picks by itself (three wavefronts per solve up to N = 64, two above), with two wavefronts per solve, and on a handle created
with CILQR_NO_SHARE_KERNEL (one wavefront per solve): B = 3, M = 2 static obstacles, the scenes' warm-start controls.

Bounds: the suite's (tests/test_gpu_parity.py) — iterations and exit reasons EQUAL to the oracle's, max|dU| ≤ 1e-9 — and the
plans' results bit-identical to each other.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TIGHT = 1e-9
HORIZONS = [1, 2, 3, 4, 63, 64, 65, 127]
B, M = 3, 2
PLANS = {"auto": {}, "two_wavefronts": {"CILQR_SHARE_W": "2"}, "one_wavefront": {"CILQR_NO_SHARE_KERNEL": "1"}}
_cache = {}


def _solver_with_env(cilqr, env, p, batch, N):
    """A handle created under `env` (the plan is decided at create); the environment is put back before the solve."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return cilqr.Solver(p, max_batch=batch, max_horizon=N, max_obstacles=M, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _solve(cilqr, env, p, sc, batch, N):
    s = _solver_with_env(cilqr, env, p, batch, N)
    try:
        return s.solve_batch(N, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], sc["obs_pose"], sc["obs_dim"], sc["obs_weight"]), \
            s.solve_wavefronts(batch, N, M)
    finally:
        s.close()


def _case(cilqr, oracle, N):
    """Scene, oracle result (computed once per horizon) and the result of every plan."""
    if N not in _cache:
        from cilqr_amd import scenes
        p = cilqr.default_params(N)
        sc = scenes.make_static(B, N, M, p, 9400 + N)
        want = oracle.solve_batch(oracle.default_params(N), N, M, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], sc["obs_pose"], sc["obs_dim"],
                                  sc["obs_weight"], threads=min(B, oracle.max_threads()))
        got = {name: _solve(cilqr, env, p, sc, B, N) for name, env in PLANS.items()}
        _cache[N] = (sc, want, got)
    return _cache[N]


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("N", HORIZONS)
def test_edge_horizon_matches_oracle(cilqr, oracle, N, plan):
    _, want, got = _case(cilqr, oracle, N)
    r, wavefronts = got[plan]
    assert wavefronts == {"auto": 3 if N <= 64 else 2, "two_wavefronts": 2, "one_wavefront": 1}[plan]
    du = float(np.max(np.abs(r["U"] - want["U"])))
    dx = float(np.max(np.abs(r["X"] - want["X"])))
    print("N=%d %s (%d wavefronts): max|dU| = %.3e max|dX| = %.3e iters %s" % (N, plan, wavefronts, du, dx, r["iters"].tolist()))
    assert np.array_equal(r["iters"], want["iters"]) and np.array_equal(r["status"], want["status"])
    assert du <= TIGHT
    assert dx <= 100 * TIGHT
    assert np.allclose(r["J"], want["J"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("N", HORIZONS)
def test_edge_horizon_plans_agree_bit_for_bit(cilqr, oracle, N):
    _, _, got = _case(cilqr, oracle, N)
    ref, _ = got["one_wavefront"]
    for plan in ("auto", "two_wavefronts"):
        for k in ("U", "X", "J", "iters", "status"):
            assert np.array_equal(got[plan][0][k], ref[k], equal_nan=(k in ("U", "X", "J"))), "N=%d %s: %s differs" % (N, plan, k)


@pytest.mark.parametrize("plan", list(PLANS))
def test_hand_over_leaves_the_other_solves_untouched(cilqr, oracle, plan):
    """The large-turn scene of test_large_turns_hand_over_to_general_kernel, small: every third ego drives 10-25 m/s on a full-lock
    warm start and turns more than 1/4 rad per step, so phase F reports the turn and the solve is redone by the GENERAL kernel.
    Those solves follow the oracle; the ordinary solves beside them keep the bits they have in a batch without a hand-over."""
    from cilqr_amd import scenes
    N, batch = 50, 12
    p = cilqr.default_params(N)
    sc = scenes.make_static(batch, N, M, p, 8111)
    fast = dict(sc, x0=sc["x0"].copy(), U=sc["U"].copy())
    rng = np.random.default_rng(8112)
    hot = np.arange(0, batch, 3)
    fast["x0"][hot, 2] = rng.uniform(10.0, 25.0, hot.size)
    fast["U"].reshape(batch, N, 2)[hot, :, 1] = np.where(rng.random((hot.size, 1)) < 0.5, 8.0, -8.0)
    assert (fast["x0"][hot, 2] * np.tan(p.steer_angle_max) / p.wheelbase * p.timestep > 0.25).all()  # beyond rotate_heading's bound
    if "large_turn_oracle" not in _cache:
        _cache["large_turn_oracle"] = oracle.solve_batch(oracle.default_params(N), N, M, fast["x0"], fast["U"], fast["poly"], fast["xplan_fl"],
                                                         fast["obs_pose"], fast["obs_dim"], fast["obs_weight"], threads=min(batch, oracle.max_threads()))
    want = _cache["large_turn_oracle"]
    base, _ = _solve(cilqr, PLANS[plan], p, sc, batch, N)
    got, _ = _solve(cilqr, PLANS[plan], p, fast, batch, N)
    ok = np.isfinite(want["U"]).all(axis=1)
    assert ok[hot].sum() >= hot.size // 2
    assert np.array_equal(got["iters"], want["iters"]) and np.array_equal(got["status"], want["status"])
    du = float(np.max(np.abs(got["U"][ok] - want["U"][ok])))
    print("%s: hand-over solves %s, max|dU| = %.3e" % (plan, hot.tolist(), du))
    assert du <= 1e-8  # (the bound of the large-turn test this scene comes from)
    cold = np.setdiff1d(np.arange(batch), hot)
    for k in ("U", "X", "J", "iters", "status"):
        assert np.array_equal(got[k][cold], base[k][cold]), k

"""The control barrier of the two-wavefront share kernel at the edges of its two rounds (GPU; the HIP path through the C-ABI against
the CPU oracle).

cilqr_solve_share_kernel<2, false, …> (tests/test_share_two_rounds.py) deals phase L's records in two rounds, the steps [h, N)
in front of barrier A and the steps [0, h) in front of barrier A2, h = N / 2 from N = 24 on and 0 below.  The control barrier's
record slots (6, 8: acceleration; 7, 9: yaw rate) are main's today; a build that formed them on the aux wavefront's (step, chain)
lanes — the even lane the acceleration barrier, the odd lane the yaw-rate barrier, round by round — was measured slower and is not
in the tree (profiles/r30_main_is_the_pole.txt).  These tests hold whichever wavefront forms the slots, and were written to catch
the wrong lane or the wrong round.  What can go wrong shows
  * at the horizons where the rounds and the lanes change shape: 1, 2, 3, the threshold (23, 24, 25), 32, 33, 50, 63 and 64 (all 64
    lanes on in both rounds), with 0, 1 and 4 obstacles: an odd lane without obstacle entries still has its barrier;
  * where a barrier is live: warm-start controls exactly at a bound and 1 beyond it — acceleration at acc_max and acc_min, yaw rate
    at v·yaw_hi and v·yaw_lo, and an ego at rest (v = 0: both yaw-rate bounds are 0) — at the steps where the wrong lane or the wrong
    round would show: 0, h − 1 and h across the split, N − 1;
  * where a barrier's exponential overflows (argument beyond 710) at a step of round 1 and at a step of round 2: the solve ends as
    the oracle's does.

Every scene runs on the plan the library picks by itself, with two wavefronts per solve (CILQR_SHARE_W=2) and with one
(CILQR_NO_SHARE_KERNEL=1); B = 3.

Bounds: those of tests/test_share_two_rounds.py — iterations and exit reasons EQUAL to the oracle's, max|dU| ≤ 1e-9, max|dX| ≤ 1e-7 —
and the three plans' results bit-identical to each other in U, X, J, iters and status.  The overflow scenes were run through the
oracle first: the cost has no barrier term and stays finite, the first linearisation is accepted, the backward pass meets the
infinite l_u / l_uu, and the solve ends in its first iteration with the numeric exit reason and the warm start as its result, finite
— so the record slots the aux lanes wrote are read by phase R, and the scenes stay in the tolerance comparison (a solve whose oracle
result were not finite would be held to iterations and exit reason only).
"""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TIGHT = 1e-9
HORIZONS = [1, 2, 3, 23, 24, 25, 32, 33, 50, 63, 64]
COUNTS = [0, 1, 4]
B = 3
PLANS = {"auto": {}, "two_wavefronts": {"CILQR_SHARE_W": "2"}, "one_wavefront": {"CILQR_NO_SHARE_KERNEL": "1"}}
KEYS = ("U", "X", "J", "iters", "status")
SPLIT_MIN = 24  # shortest horizon dealt in two rounds (cilqr_solve.hip, SHARE_SPLIT_MIN)
_cache = {}


def _handle(cilqr, env, p, N, n_obs):
    """A handle created under `env` (the plan is decided at create); the environment is put back before any solve."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return cilqr.Solver(p, max_batch=B, max_horizon=N, max_obstacles=max(n_obs, 1), device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _solve_plans(cilqr, p, N, scs):
    """{plan: [result of each scene of `scs`]} (one handle per plan) and the wavefronts each plan ran each scene on."""
    out, waves = {}, {}
    for plan, env in PLANS.items():
        s = _handle(cilqr, env, p, N, max(sc["M"] for sc in scs))
        try:
            out[plan] = [s.solve_batch(N, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], sc["obs_pose"], sc["obs_dim"], sc["obs_weight"]) for sc in scs]
            waves[plan] = [s.solve_wavefronts(B, N, sc["M"]) for sc in scs]
        finally:
            s.close()
    return out, waves


def _oracle(oracle, N, sc):
    return oracle.solve_batch(oracle.default_params(N), N, sc["M"], sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], sc["obs_pose"], sc["obs_dim"],
                              sc["obs_weight"], threads=min(B, oracle.max_threads()))


def _against_oracle(r, want, what):
    """Iterations and exit reasons equal; the solves whose oracle result is finite within the tolerances (every one, in these scenes)."""
    ok = np.isfinite(want["U"]).all(axis=1) & np.isfinite(want["X"]).all(axis=1)
    du = float(np.max(np.abs(r["U"][ok] - want["U"][ok]))) if ok.any() else 0.0
    dx = float(np.max(np.abs(r["X"][ok] - want["X"][ok]))) if ok.any() else 0.0
    print("%s: max|dU| = %.3e max|dX| = %.3e iters %s status %s (oracle finite: %s)" % (what, du, dx, r["iters"].tolist(), r["status"].tolist(), ok.tolist()))
    assert np.array_equal(r["iters"], want["iters"]) and np.array_equal(r["status"], want["status"]), what
    assert du <= TIGHT, what
    assert dx <= 100 * TIGHT, what


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS)


def _check(got, waves, want, i, plan, what):
    if plan != "auto":
        assert waves[plan][i] == {"two_wavefronts": 2, "one_wavefront": 1}[plan]
    _against_oracle(got[plan][i], want[i], "%s, %s (%d wavefronts)" % (what, plan, waves[plan][i]))
    assert _same_bits(got[plan][i], got["one_wavefront"][i]), "%s: %s differs from one wavefront per solve" % (what, plan)


# ------------------------------------------------------------------------------------------------ horizons × obstacle counts
def _grid(cilqr, oracle, N):
    if ("grid", N) not in _cache:
        from cilqr_amd import scenes
        p = cilqr.default_params(N)
        scs = [scenes.make_static(B, N, M, p, 9900 + 10 * N + M) for M in COUNTS]
        want = [_oracle(oracle, N, sc) for sc in scs]
        got, waves = _solve_plans(cilqr, p, N, scs)
        _cache["grid", N] = (want, got, waves)
    return _cache["grid", N]


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("M", COUNTS)
@pytest.mark.parametrize("N", HORIZONS)
def test_horizons_and_obstacle_counts(cilqr, oracle, N, M, plan):
    want, got, waves = _grid(cilqr, oracle, N)
    _check(got, waves, want, COUNTS.index(M), plan, "N=%d M=%d" % (N, M))


# ------------------------------------------------------------------------------------------------ barriers live at the edges of the rounds
LIVE_HORIZONS = [23, 24, 50, 64]  # one round; the first split (h = 12); the production horizon (h = 25); every lane on (h = 32)
BOUNDS = ["acc_max", "acc_min", "yaw_hi", "yaw_lo", "at_rest"]
EDGES = ["0", "h-1", "h", "N-1"]


def _edge_steps(N):
    h = N // 2  # the split of the horizons dealt in two rounds; below them the same steps, all of one round
    return {"0": 0, "h-1": h - 1, "h": h, "N-1": N - 1}


def _speeds(p, sc, N):
    """The speed at every step of the warm start, (B, N), as the model forms it (acceleration and speed clamped)."""
    v = sc["x0"][:, 2].copy()
    U = sc["U"].reshape(B, N, 2)
    out = np.zeros((B, N))
    for t in range(N):
        out[:, t] = v
        v = np.minimum(np.maximum(v + np.clip(U[:, t, 0], p.acc_min, p.acc_max) * p.timestep, 0.0), p.speed_max)
    return out


def _live_scene(cilqr, N, M, bound, step, seed):
    """Solve 0: the control exactly at `bound` at `step`; solve 1: 1 beyond it; solve 2: at the bound at all four edge steps
    (at_rest: v = 0 at `step` in all three, the yaw rate at the bounds' common 0, 1 above and 1 below)."""
    from cilqr_amd import scenes
    p = cilqr.default_params(N)
    sc = scenes.make_static(B, N, M, p, seed)
    sc = dict(sc, x0=sc["x0"].copy(), U=sc["U"].copy())
    if bound == "at_rest":
        sc["x0"][:, 2] = 0.0
    U = sc["U"].reshape(B, N, 2)
    where = [[step], [step], [step] if bound == "at_rest" else sorted(set(_edge_steps(N).values()))]
    beyond = [0.0, 1.0, -1.0 if bound == "at_rest" else 0.0]
    if bound in ("acc_max", "acc_min"):
        for b in range(B):
            U[b, where[b], 0] = p.acc_max + beyond[b] if bound == "acc_max" else p.acc_min - beyond[b]
    else:
        yaw = {"yaw_hi": math.tan(p.steer_angle_max), "yaw_lo": math.tan(p.steer_angle_min), "at_rest": math.tan(p.steer_angle_max)}[bound] / p.wheelbase
        if bound == "at_rest":  # at rest from step 0 on for as long as the ego does not accelerate: u0 = 0 up to the last edge step of the solve
            for b in range(B):
                U[b, :max(where[b]) + 1, 0] = 0.0
        v = _speeds(p, sc, N)
        for b in range(B):
            sign = -1.0 if bound == "yaw_lo" else 1.0
            U[b, where[b], 1] = v[b, where[b]] * yaw + sign * beyond[b]
        if bound == "at_rest":
            assert all((v[b, where[b]] == 0.0).all() for b in range(B))
    return p, sc


def _live(cilqr, oracle, N):
    """Every (bound, edge) scene of horizon N, M = 4 except for the yaw-rate bounds at M = 1 (no entry on the odd lanes)."""
    if ("live", N) not in _cache:
        scs, names = [], []
        for i, bound in enumerate(BOUNDS):
            for j, (edge, step) in enumerate(_edge_steps(N).items()):
                p, sc = _live_scene(cilqr, N, 1 if bound == "yaw_lo" else 4, bound, step, 9800 + 100 * i + 10 * j + N)
                scs.append(sc)
                names.append((bound, edge))
        want = [_oracle(oracle, N, sc) for sc in scs]
        got, waves = _solve_plans(cilqr, p, N, scs)
        _cache["live", N] = (names, want, got, waves)
    return _cache["live", N]


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("N", LIVE_HORIZONS)
def test_live_barriers_at_the_edges_of_the_rounds(cilqr, oracle, N, bound, edge, plan):
    names, want, got, waves = _live(cilqr, oracle, N)
    _check(got, waves, want, names.index((bound, edge)), plan, "N=%d %s at step %s" % (N, bound, edge))


# ------------------------------------------------------------------------------------------------ a barrier's exponential overflows
OVERFLOW = 720.0  # beyond the bound: the barrier's argument is q2 · 720 = 720 > 710 with the default q2 = 1


def _overflow_scene(cilqr, N, control, step):
    """Solve 1's control `control` lies 720 beyond its upper bound at `step`; solves 0 and 2 are ordinary."""
    from cilqr_amd import scenes
    p = cilqr.default_params(N)
    assert p.q2_acc == 1.0 and p.q2_yawrate == 1.0
    sc = scenes.make_static(B, N, 4, p, 9700 + N)
    sc = dict(sc, U=sc["U"].copy())
    U = sc["U"].reshape(B, N, 2)
    if control == 0:
        U[1, step, 0] = p.acc_max + OVERFLOW
    else:
        U[1, step, 1] = _speeds(p, sc, N)[1, step] * math.tan(p.steer_angle_max) / p.wheelbase + OVERFLOW
    return p, sc


def _overflow(cilqr, oracle, N):
    if ("overflow", N) not in _cache:
        scs, names = [], []
        for control in (0, 1):
            for edge, step in _edge_steps(N).items():
                p, sc = _overflow_scene(cilqr, N, control, step)
                scs.append(sc)
                names.append((control, edge))
        want = [_oracle(oracle, N, sc) for sc in scs]
        got, waves = _solve_plans(cilqr, p, N, scs)
        _cache["overflow", N] = (names, want, got, waves)
    return _cache["overflow", N]


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("edge", EDGES)  # 0 and h − 1: steps of round 2; h and N − 1: steps of round 1
@pytest.mark.parametrize("control", [0, 1])
@pytest.mark.parametrize("N", [23, 50, 64])
def test_overflowing_barrier_ends_as_the_oracle_does(cilqr, oracle, N, control, edge, plan):
    """Solve 1 of each scene: the oracle ends it in iteration 1 with the numeric exit reason and returns the warm start.

    Step 0 is the one that needed code: it is the last step of the backward pass, so an infinite l_uu there gives Q_uu = +inf with
    no later step to turn it into a NaN.  +inf passed phase R's PSD test (sign bits, NaN) and the GENERAL kernel's test of det and
    trace for NaN, the forward pass wrote NaN controls, and the solve ended one iteration late with U all NaN, on every plan.  Now
    the fast kernels hand a non-finite det0 of step 0 over and quu_inverse_general rejects an infinite entry, as the oracle's
    isfinite on every entry does."""
    names, want, got, waves = _overflow(cilqr, oracle, N)
    i = names.index((control, edge))
    assert want[i]["status"][1] == 3 and want[i]["iters"][1] == 1, "the oracle no longer meets the overflow in its first backward pass"
    _check(got, waves, want, i, plan, "N=%d control %d overflows at step %s" % (N, control, edge))

"""Phase L of the two-wavefront share kernel in two rounds (GPU; the HIP path through the C-ABI against the CPU oracle).

cilqr_solve_share_kernel<2, false, …> splits the horizon at h = N / 2 from N = 24 on: its aux wavefront forms the obstacle sums and
Jacobians of the steps [h, N) beside main's closest-sample search, and those of the steps [0, h) — with the records' state terms —
while main runs phase R's trips above the split; its lanes are (step, chain) pairs, the even lane summing the obstacle entries of
even index, the odd lane the others.  Below N = 24 there is one round over all steps.  What can go wrong shows
  * at the horizons where the rounds, the lanes and R's two segments change shape: 1 … 8, the threshold (22 … 25), 31 … 33 (h = 16),
    49 … 51 (the production horizon; odd and even splits), 63 and 64 (all 64 lanes in both rounds), and 65 (the LONG form: unchanged);
  * at the obstacle counts 0 … 5: both chains empty, the odd one empty, equal chains, the even one longer;
  * with explicit weights (one of them zero), with every obstacle beside the path (nothing culled) and with all of them far away
    (every entry culled by the wave-wide vote, which now spans two chains and half the steps);
  * on every path through a pass's barriers: accept, rejection of the first forward pass, NaN cost, hand-over out of phase R
    (indefinite Q_uu) and out of phase F (a turn beyond the bound), the last iteration.  A path with unequal barriers would hang.

Every scene runs on the plan the library picks by itself, with two wavefronts per solve (CILQR_SHARE_W=2) and with one
(CILQR_NO_SHARE_KERNEL=1); B = 3 (12 where a scene needs neighbours).

Bounds: the suite's (tests/test_gpu_parity.py) — iterations and exit reasons EQUAL to the oracle's, max|dU| ≤ 1e-9, max|dX| ≤ 1e-7 —
and the three plans' results bit-identical to each other in U, X, J, iters and status.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TIGHT = 1e-9
HORIZONS = [1, 2, 3, 4, 5, 6, 7, 8, 22, 23, 24, 25, 31, 32, 33, 49, 50, 51, 63, 64, 65]
COUNTS = [0, 1, 2, 3, 4, 5]
B = 3
PLANS = {"auto": {}, "two_wavefronts": {"CILQR_SHARE_W": "2"}, "one_wavefront": {"CILQR_NO_SHARE_KERNEL": "1"}}
KEYS = ("U", "X", "J", "iters", "status")
_cache = {}


def _handle(cilqr, env, p, batch, N, n_obs):
    """A handle created under `env` (the plan is decided at create); the environment is put back before any solve."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return cilqr.Solver(p, max_batch=batch, max_horizon=N, max_obstacles=max(n_obs, 1), device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(s, sc, N, flags=0):
    return s.solve_batch(N, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], sc["obs_pose"], sc["obs_dim"], sc["obs_weight"], flags=flags)


def _solve_plans(cilqr, p, N, scs, general=False):
    """{plan: [result of each scene of `scs`]} (one handle per plan), with the wavefronts each plan ran the first scene on;
    general: also the GENERAL kernel alone."""
    batch = max(sc["x0"].shape[0] for sc in scs)
    n_obs = max(sc["M"] for sc in scs)
    out, waves = {}, {}
    for plan, env in PLANS.items():
        s = _handle(cilqr, env, p, batch, N, n_obs)
        try:
            out[plan] = [_run(s, sc, N) for sc in scs]
            waves[plan] = [s.solve_wavefronts(sc["x0"].shape[0], N, sc["M"]) for sc in scs]
            if general and plan == "auto":
                out["general"] = [_run(s, sc, N, flags=cilqr.FLAG_GENERAL_ONLY) for sc in scs]
        finally:
            s.close()
    return out, waves


def _oracle(oracle, N, sc):
    batch = sc["x0"].shape[0]
    return oracle.solve_batch(oracle.default_params(N), N, sc["M"], sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], sc["obs_pose"], sc["obs_dim"],
                              sc["obs_weight"], threads=min(batch, oracle.max_threads()))


def _against_oracle(r, want, what):
    du = float(np.max(np.abs(r["U"] - want["U"])))
    dx = float(np.max(np.abs(r["X"] - want["X"])))
    print("%s: max|dU| = %.3e max|dX| = %.3e iters %s status %s" % (what, du, dx, r["iters"].tolist(), r["status"].tolist()))
    assert np.array_equal(r["iters"], want["iters"]) and np.array_equal(r["status"], want["status"]), what
    assert du <= TIGHT, what
    assert dx <= 100 * TIGHT, what
    assert np.allclose(r["J"], want["J"], rtol=1e-9, atol=1e-9), what


def _same_bits(a, b, rows=slice(None)):
    return all(np.array_equal(a[k][rows], b[k][rows], equal_nan=True) for k in KEYS)


def _ego_positions(p, sc, N):
    """Where the warm start takes the ego: (B, N, 2), by the kinematic model with the scene's controls (close enough to stand beside)."""
    x = sc["x0"].copy()
    U = sc["U"].reshape(x.shape[0], N, 2)
    out = np.zeros((x.shape[0], N, 2))
    for t in range(N):
        out[:, t] = x[:, :2]
        x[:, 0] += x[:, 2] * np.cos(x[:, 3]) * p.timestep
        x[:, 1] += x[:, 2] * np.sin(x[:, 3]) * p.timestep
        x[:, 2] += U[:, t, 0] * p.timestep
        x[:, 3] += U[:, t, 1] * p.timestep
    return out


# ------------------------------------------------------------------------------------------------ horizons × obstacle counts
def _grid(cilqr, oracle, N):
    """Every obstacle count at horizon N: scenes, oracle results, the plans' results (three handles per horizon)."""
    if ("grid", N) not in _cache:
        from cilqr_amd import scenes
        p = cilqr.default_params(N)
        scs = [scenes.make_static(B, N, M, p, 9500 + 10 * N + M) for M in COUNTS]
        want = [_oracle(oracle, N, sc) for sc in scs]
        got, waves = _solve_plans(cilqr, p, N, scs)
        _cache["grid", N] = (want, got, waves)
    return _cache["grid", N]


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("M", COUNTS)
@pytest.mark.parametrize("N", HORIZONS)
def test_horizons_and_obstacle_counts_match_oracle(cilqr, oracle, N, M, plan):
    want, got, waves = _grid(cilqr, oracle, N)
    i = COUNTS.index(M)
    if plan != "auto":
        assert waves[plan][i] == {"two_wavefronts": 2, "one_wavefront": 1}[plan]
    _against_oracle(got[plan][i], want[i], "N=%d M=%d %s (%d wavefronts)" % (N, M, plan, waves[plan][i]))


@pytest.mark.parametrize("M", COUNTS)
@pytest.mark.parametrize("N", HORIZONS)
def test_horizons_and_obstacle_counts_plans_agree_bit_for_bit(cilqr, oracle, N, M):
    _, got, _ = _grid(cilqr, oracle, N)
    i = COUNTS.index(M)
    for plan in ("auto", "two_wavefronts"):
        for k in KEYS:
            assert np.array_equal(got[plan][i][k], got["one_wavefront"][i][k], equal_nan=(k in ("U", "X", "J"))), "N=%d M=%d %s: %s differs" % (N, M, plan, k)


# ------------------------------------------------------------------------------------------------ weights, nothing culled, everything culled
def _special_scene(cilqr, kind):
    from cilqr_amd import scenes
    N, M = 50, 4
    p = cilqr.default_params(N)
    sc = scenes.make_static(B, N, M, p, 9650)
    sc = dict(sc, obs_pose=sc["obs_pose"].copy())
    pose = sc["obs_pose"].reshape(B, M, N, 4)
    if kind == "weights":  # explicit weights, one of them zero in every solve, in an even and in an odd entry
        sc["obs_weight"] = np.array([[0.0, 0.5, 2.0, 1.0], [1.5, 0.0, 1.0, 0.25], [1.0, 3.0, 0.0, 0.0]])
    elif kind == "beside":  # every obstacle 3 m beside the ego's way, spread along it: no entry is negligible at every step
        pos = _ego_positions(p, sc, N)
        for m in range(M):
            t = (m + 1) * N // (M + 1)
            pose[:, m, :, 0] = pos[:, t, 0][:, None]
            pose[:, m, :, 1] = (pos[:, t, 1] + (3.0 if m % 2 == 0 else -3.0))[:, None]
    else:  # "far": every obstacle half a kilometre away: every entry is negligible at every step
        pose[..., 0] += 500.0
        pose[..., 1] -= 500.0
    return N, p, sc


def _special(cilqr, oracle, kind):
    if ("special", kind) not in _cache:
        N, p, sc = _special_scene(cilqr, kind)
        got, waves = _solve_plans(cilqr, p, N, [sc])
        _cache["special", kind] = (N, _oracle(oracle, N, sc), got, waves)
    return _cache["special", kind]


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("kind", ["weights", "beside", "far"])
def test_weights_and_culling_match_oracle(cilqr, oracle, kind, plan):
    N, want, got, waves = _special(cilqr, oracle, kind)
    _against_oracle(got[plan][0], want, "%s, N=%d %s (%d wavefronts)" % (kind, N, plan, waves[plan][0]))
    assert _same_bits(got[plan][0], got["one_wavefront"][0])


# ------------------------------------------------------------------------------------------------ the paths through a pass's barriers
BATCH = 12


def _base12(cilqr, N):
    """The scene of tests/test_psd_check_off_chain.py at horizon N (12 ordinary solves, M = 2, unit weights), solved on every plan."""
    if ("base12", N) not in _cache:
        from test_psd_check_off_chain import _scene
        p, sc = _scene(cilqr, N)
        sc = dict(sc, M=2)
        got, _ = _solve_plans(cilqr, p, N, [sc])
        _cache["base12", N] = (p, sc, got)
    return _cache["base12", N]


def test_rejected_first_pass_follows_the_oracle(cilqr, oracle):
    """Warm starts that are the oracle's own converged controls: the first forward pass raises the cost by 0.1 … 3 (nothing that
    hangs on rounding: the oracle's path stays the same under relative perturbations of the warm start up to 1e-9), is rejected, and
    lamb runs to its maximum — main meets barrier A2 in the reject branch, not in phase R."""
    from cilqr_amd import scenes
    N, M = 50, 4
    p = cilqr.default_params(N)
    sc = scenes.make_static(BATCH, N, M, p, 9701)
    first = _oracle(oracle, N, sc)
    assert np.isfinite(first["U"]).all()
    again = dict(sc, U=first["U"].copy())
    want = _oracle(oracle, N, again)
    rejected = (want["status"] == 1) & (want["iters"] == 7)  # one accepted linearisation, one pass, then lamb to its maximum
    assert rejected.sum() >= BATCH // 2, "the scene no longer rejects its first pass"
    got, waves = _solve_plans(cilqr, p, N, [again])
    assert waves["two_wavefronts"][0] == 2
    for plan in PLANS:
        _against_oracle(got[plan][0], want, "rejected first pass, %s" % plan)
        assert _same_bits(got[plan][0], got["one_wavefront"][0]), plan


@pytest.mark.parametrize("where", ["first step", "last step"])
def test_nan_cost_follows_the_oracle(cilqr, oracle, where):
    """The non-finite scenes of tests/test_psd_check_off_chain.py at N = 50: a NaN in one obstacle entry of solve 5, in a step of round
    2 (the first) or of round 1 (the last).  The solve takes the oracle's path — at the last step the NaN reaches the records and the
    solve ends with the numeric exit reason — and its neighbours keep their bits."""
    N, solve = 50, 5
    p, sc, base = _base12(cilqr, N)
    sn = dict(sc, obs_pose=sc["obs_pose"].copy())
    sn["obs_pose"].reshape(BATCH, 2, N, 4)[solve, 1, 0 if where == "first step" else N - 1, 0] = np.nan
    want = _oracle(oracle, N, sn)
    got, waves = _solve_plans(cilqr, p, N, [sn])
    assert waves["two_wavefronts"][0] == 2
    keep = np.arange(BATCH) != solve
    for plan in PLANS:
        r = got[plan][0]
        print("NaN in the %s, %s: iters %d (oracle %d) status %d (oracle %d)" % (where, plan, r["iters"][solve], want["iters"][solve], r["status"][solve], want["status"][solve]))
        assert np.array_equal(r["iters"], want["iters"]) and np.array_equal(r["status"], want["status"])
        assert _same_bits(r, base[plan][0], keep)
        assert _same_bits(r, got["one_wavefront"][0]), plan


@pytest.mark.parametrize("N,step", [(50, 0), (50, 25), (50, 49), (64, 0), (64, 32), (64, 63)])
def test_hand_over_out_of_phase_r_ends_and_agrees(cilqr, N, step):
    """The indefinite-Q_uu scenes of tests/test_psd_check_off_chain.py (obstacle weight -40 on solves 3 and 8, both of their obstacles
    0.3 m beside the ego's position at `step`: below the split, at it, above it): phase R's PSD test behind its loop, i.e. behind
    barrier A2, hands the solve over.  Each ends, comes back with the GENERAL kernel's bits, and the plans agree bit for bit."""
    from test_psd_check_off_chain import NEGATIVE, _indefinite_scene
    p, _, base = _base12(cilqr, N)
    _, sb = _indefinite_scene(cilqr, N, step)
    got, waves = _solve_plans(cilqr, p, N, [dict(sb, M=2)], general=True)
    assert waves["two_wavefronts"][0] == 2
    keep = np.setdiff1d(np.arange(BATCH), NEGATIVE)
    for plan in PLANS:
        r = got[plan][0]
        for b in NEGATIVE:
            assert r["status"][b] in (0, 1, 2, 3) and 1 <= r["iters"][b] <= p.max_iterations
            assert _same_bits(r, got["general"][0], [b]), "%s: solve %d did not come back with the GENERAL kernel's results: not handed over" % (plan, b)
        assert _same_bits(r, base[plan][0], keep)
        assert _same_bits(r, got["one_wavefront"][0]), plan


def test_hand_over_out_of_phase_f_ends_and_agrees(cilqr, oracle):
    """The large-turn scene of test_hand_over_leaves_the_other_solves_untouched (tests/test_serial_loop_edges.py): every third ego
    drives 10-25 m/s on a full-lock warm start, phase F reports the turn and the solve is redone by the GENERAL kernel."""
    from cilqr_amd import scenes
    N, M = 50, 2
    p = cilqr.default_params(N)
    sc = scenes.make_static(BATCH, N, M, p, 8111)
    fast = dict(sc, x0=sc["x0"].copy(), U=sc["U"].copy())
    rng = np.random.default_rng(8112)
    hot = np.arange(0, BATCH, 3)
    fast["x0"][hot, 2] = rng.uniform(10.0, 25.0, hot.size)
    fast["U"].reshape(BATCH, N, 2)[hot, :, 1] = np.where(rng.random((hot.size, 1)) < 0.5, 8.0, -8.0)
    assert (fast["x0"][hot, 2] * np.tan(p.steer_angle_max) / p.wheelbase * p.timestep > 0.25).all()  # beyond rotate_heading's bound
    want = _oracle(oracle, N, fast)
    got, waves = _solve_plans(cilqr, p, N, [sc, fast])
    assert waves["two_wavefronts"][1] == 2
    ok = np.isfinite(want["U"]).all(axis=1)
    assert ok[hot].sum() >= hot.size // 2
    cold = np.setdiff1d(np.arange(BATCH), hot)
    for plan in PLANS:
        base, r = got[plan]
        assert np.array_equal(r["iters"], want["iters"]) and np.array_equal(r["status"], want["status"])
        du = float(np.max(np.abs(r["U"][ok] - want["U"][ok])))
        print("%s: hand-over solves %s, max|dU| = %.3e" % (plan, hot.tolist(), du))
        assert du <= 1e-8  # (the bound of the large-turn test this scene comes from)
        assert _same_bits(r, base, cold)
        assert _same_bits(r, got["one_wavefront"][1]), plan

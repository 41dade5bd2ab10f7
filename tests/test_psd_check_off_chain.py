"""The PSD test of the backward pass, made behind its loop (GPU; the HIP path through the C-ABI).

The scalar-path form of phase R (riccati_mfma_smem, csrc/cilqr_solve.hip) no longer tests Q_uu on its serial chain: every step stores
a, b, d of its Q_uu into the LDS record it has just used up, and one pass by lanes behind the loop forms det0 and looks at the sign
bits (two rounds of that pass above N = 64).  A solve whose Q_uu fails the test anywhere, or turns non-finite, is handed to the
GENERAL kernel exactly as before.  What can go wrong shows where the stored slots end and where the loop changes shape, so the
scenes here fail the test at step 0, at step N - 1 and in the middle, at N = 1, 2, 3, 4 (no trip, peeled steps, odd and even trip
counts), 50, 64 and 65 (one and two rounds) and 127 — on the plan the library picks by itself, with two wavefronts per solve and with
one (CILQR_NO_SHARE_KERNEL).  B = 12, M = 2.

Bounds: those of the tests these scenes come from.  Indefinite Q_uu (obstacle weight -40, test_general_kernel_paths (b)): no value
parity with the oracle is claimed for the chaotic solves, only a legal status and 1 <= iters <= max — and the GENERAL kernel's own bits,
which shows that they were handed over; the other solves keep the bits they have in the batch without negative weights; the three
plans agree bit for bit on every output.  Non-finite input: iterations and status EQUAL to
the oracle's, the neighbours keep their bits.  Ill-conditioned but positive definite (tests/test_quu_conditioning.py's three solves):
that file's bound against the EXACT form of the oracle, and no hand-over.
"""
import os

import numpy as np
import pytest

from test_gpu_fuzz import _compare
from test_quu_conditioning import HOT, draw  # noqa: F401  (the fixture: draw 138 and its oracle solves)

pytestmark = pytest.mark.gpu

B, M = 12, 2
PLANS = {"auto": {}, "two_wavefronts": {"CILQR_SHARE_W": "2"}, "one_wavefront": {"CILQR_NO_SHARE_KERNEL": "1"}}
KEYS = ("U", "X", "J", "iters", "status")
NEGATIVE = (3, 8)  # the solves with obstacle weight -40
_cache = {}


def _solve(cilqr, env, p, sc, N, n_obs=M, flags=0, passes=False):
    """One solve of the scene on a handle created under `env` (the plan is decided at create) → results [, pass counts]."""
    import torch
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        batch = sc["x0"].shape[0]
        s = cilqr.Solver(p, max_batch=batch, max_horizon=N, max_obstacles=n_obs, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        ps = torch.full((batch,), -1, dtype=torch.int32, device="cuda:0")
        s.set_pass_count_buffer(ps.data_ptr())
        r = s.solve_batch(N, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], sc["obs_pose"], sc["obs_dim"], sc["obs_weight"], flags=flags)
        torch.cuda.synchronize()
        s.set_pass_count_buffer(0)
        return (r, ps.cpu().numpy().copy()) if passes else r
    finally:
        s.close()


def _same_bits(a, b, rows=slice(None)):
    return all(np.array_equal(a[k][rows], b[k][rows], equal_nan=True) for k in KEYS)


def _scene(cilqr, N):
    from cilqr_amd import scenes
    if ("scene", N) not in _cache:
        p = cilqr.default_params(N)
        sc = scenes.make_static(B, N, M, p, 9800 + N)
        sc["obs_weight"] = np.full((B, M), 1.0)
        _cache["scene", N] = (p, sc)
    return _cache["scene", N]


def _base(cilqr, N, plan):
    """The scene without negative weights and without NaN, solved on `plan` (once per horizon and plan)."""
    if ("base", N, plan) not in _cache:
        p, sc = _scene(cilqr, N)
        _cache["base", N, plan] = _solve(cilqr, PLANS[plan], p, sc, N)
    return _cache["base", N, plan]


# ------------------------------------------------------------------------------------------------ indefinite Q_uu
def _ego_positions(p, sc, N):
    """Where the warm start takes the ego: (B, N, 2), by the kinematic model with the scene's controls (close enough to stand beside)."""
    x = sc["x0"].copy()
    U = sc["U"].reshape(B, N, 2)
    out = np.zeros((B, N, 2))
    for t in range(N):
        out[:, t] = x[:, :2]
        x[:, 0] += x[:, 2] * np.cos(x[:, 3]) * p.timestep
        x[:, 1] += x[:, 2] * np.sin(x[:, 3]) * p.timestep
        x[:, 2] += U[:, t, 0] * p.timestep
        x[:, 3] += U[:, t, 1] * p.timestep
    return out


INDEFINITE = [(N, k) for N in (1, 2, 3, 4, 50, 64, 65, 127) for k in sorted({0, N // 2, N - 1})]


BESIDE = 0.3  # m to either side of the ego: inside the obstacles' ellipses, where the barrier's curvature is large enough to make Q_uu
# indefinite at weight -40 even through the dt² of a one-step horizon (at 1.5 m the horizons up to 4 stayed positive definite)


def _indefinite_scene(cilqr, N, step):
    """Obstacle weight -40 on two solves, both of their obstacles beside the ego's position at `step`."""
    p, sc = _scene(cilqr, N)
    sb = dict(sc, obs_weight=sc["obs_weight"].copy(), obs_pose=sc["obs_pose"].copy())
    pos = _ego_positions(p, sc, N)
    pose = sb["obs_pose"].reshape(B, M, N, 4)
    for b in NEGATIVE:
        sb["obs_weight"][b, :] = -40.0
        for m in range(M):
            pose[b, m, :, 0] = pos[b, step, 0] + 0.5 * m
            pose[b, m, :, 1] = pos[b, step, 1] + (BESIDE if m == 0 else -BESIDE)
    return p, sb


def _indefinite(cilqr, N, step):
    """Results of the three plans on that scene, and of the GENERAL kernel alone."""
    if ("indef", N, step) not in _cache:
        p, sb = _indefinite_scene(cilqr, N, step)
        _cache["indef", N, step] = {plan: _solve(cilqr, env, p, sb, N) for plan, env in PLANS.items()}
        _cache["indef", N, step]["general"] = _solve(cilqr, {}, p, sb, N, flags=cilqr.FLAG_GENERAL_ONLY)
    return _cache["indef", N, step]


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("N,step", INDEFINITE)
def test_indefinite_quu_is_contained(cilqr, N, step, plan):
    p, _ = _scene(cilqr, N)
    got, base = _indefinite(cilqr, N, step)[plan], _base(cilqr, N, plan)
    print("N=%d obstacle at step %d, %s: status %s iters %s" % (N, step, plan, got["status"][list(NEGATIVE)].tolist(), got["iters"][list(NEGATIVE)].tolist()))
    for b in NEGATIVE:
        assert got["status"][b] in (0, 1, 2, 3) and 1 <= got["iters"][b] <= p.max_iterations
    keep = np.setdiff1d(np.arange(B), NEGATIVE)
    assert _same_bits(got, base, keep)
    # The moved test must FIRE.  A solve that is handed over is redone by the GENERAL kernel from the same inputs and comes back with
    # that kernel's bits (CILQR_FLAG_GENERAL_ONLY solves the whole batch there); were the test never to fail, the fast kernels would
    # go on with an indefinite Q_uu, which the GENERAL kernel clamps: other values altogether.  So each of the two solves has the
    # GENERAL kernel's bits, or — its Q_uu stayed positive definite — the same path and the same values to the suite's tight bound.
    # The latter can only be at the shortest horizons: with N = 1 Q_uu is l_uu itself, and the states' curvature reaches Q_uu through
    # B'VB with B's position rows of order dt², so up to N = 3 nothing is claimed; from N = 4 on both must have been handed over.
    general = _indefinite(cilqr, N, step)["general"]
    for b in NEGATIVE:
        if _same_bits(got, general, [b]):
            continue
        assert N < 4, "solve %d did not come back with the GENERAL kernel's results: not handed over" % b
        assert got["iters"][b] == general["iters"][b] and got["status"][b] == general["status"][b]
        assert np.max(np.abs(got["U"][b] - general["U"][b])) <= 1e-9, "solve %d: neither handed over nor the GENERAL kernel's values" % b


@pytest.mark.parametrize("N,step", INDEFINITE)
def test_indefinite_quu_plans_agree_bit_for_bit(cilqr, N, step):
    got = _indefinite(cilqr, N, step)
    for plan in ("auto", "two_wavefronts"):
        for k in KEYS:
            assert np.array_equal(got[plan][k], got["one_wavefront"][k], equal_nan=True), "N=%d step %d %s: %s differs" % (N, step, plan, k)


# ------------------------------------------------------------------------------------------------ non-finite input
NAN_SOLVE = 5


def _non_finite(cilqr, oracle, N, where):
    if ("nan", N, where) not in _cache:
        p, sc = _scene(cilqr, N)
        sn = dict(sc, x0=sc["x0"].copy(), obs_pose=sc["obs_pose"].copy())
        if where == "x0":
            sn["x0"][NAN_SOLVE, 1] = np.nan
        else:
            sn["obs_pose"].reshape(B, M, N, 4)[NAN_SOLVE, 1, 0 if where == "first step" else N - 1, 0] = np.nan
        want = oracle.solve_batch(oracle.default_params(N), N, M, sn["x0"], sn["U"], sn["poly"], sn["xplan_fl"], sn["obs_pose"], sn["obs_dim"],
                                  sn["obs_weight"], threads=min(B, oracle.max_threads()))
        _cache["nan", N, where] = (want, {plan: _solve(cilqr, env, p, sn, N) for plan, env in PLANS.items()})
    return _cache["nan", N, where]


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("where", ["x0", "first step", "last step"])
@pytest.mark.parametrize("N", [2, 4, 50, 65])
def test_non_finite_input_follows_the_oracle(cilqr, oracle, N, where, plan):
    want, got = _non_finite(cilqr, oracle, N, where)
    r, base = got[plan], _base(cilqr, N, plan)
    print("N=%d NaN in %s, %s: iters %d (oracle %d) status %d (oracle %d)" % (
        N, where, plan, r["iters"][NAN_SOLVE], want["iters"][NAN_SOLVE], r["status"][NAN_SOLVE], want["status"][NAN_SOLVE]))
    assert np.array_equal(r["iters"], want["iters"]) and np.array_equal(r["status"], want["status"])
    keep = np.arange(B) != NAN_SOLVE
    assert _same_bits(r, base, keep)


# ------------------------------------------------------------------------------------------------ ill-conditioned, positive definite
@pytest.mark.parametrize("plan", list(PLANS))
def test_ill_conditioned_quu_does_not_hand_over(cilqr, draw, plan):  # noqa: F811
    """Solves 208, 282 and 325 of draw 138 (Q_uu = [[1e10, b], [b, d]] on the way, condition 1e10, both eigenvalues positive): within
    test_quu_conditioning's bound of the EXACT form on every plan, the plans bit-identical to each other, the pass counts those of the
    GENERAL kernel.  Whether a solve was handed over cannot be read from the pass-count buffer — it holds the passes of whichever
    kernel finished the solve, and a solve that is handed over is redone by the GENERAL kernel from the same inputs — so a hand-over
    shows in the outputs alone, where the two kernels differ.  Measured: they differ on solve 208 (3.3e-13 in U) and agree bit for
    bit on 282 and 325, so 208 is shown not to hand over, and for the other two a hand-over would be neither visible nor of
    consequence.  (tools/handover_ab.py compares two builds on scenes that do hand over.)"""
    N, n_obs, sc = draw["N"], draw["M"], draw["sc"]
    p = cilqr.default_params(N)
    for name, _ in type(draw["po"])._fields_:  # the draw's parameter set is off the defaults
        setattr(p, name, getattr(draw["po"], name))
    idx = np.array(HOT)
    sub = {k: (None if sc[k] is None else np.ascontiguousarray(sc[k][idx])) for k in ("x0", "U", "poly", "xplan_fl", "obs_pose", "obs_dim", "obs_weight")}
    env = dict(PLANS[plan], CILQR_FORCE_G="64")  # (the wavefront family, as in test_quu_conditioning)
    got, passes = _solve(cilqr, env, p, sub, N, n_obs, passes=True)
    if "general" not in _cache:
        _cache["general"] = _solve(cilqr, {"CILQR_FORCE_G": "64"}, p, sub, N, n_obs, flags=cilqr.FLAG_GENERAL_ONLY, passes=True)
    general, general_passes = _cache["general"]
    want = {k: v[idx] for k, v in draw["forms"]["exact"].items()}
    print("%s: max|dU| vs exact %.3e, vs the GENERAL kernel %.3e; passes %s (GENERAL %s)" % (
        plan, np.max(np.abs(got["U"] - want["U"])), np.max(np.abs(got["U"] - general["U"])), passes.tolist(), general_passes.tolist()))
    _compare(got, want, "%s, draw 138, solves %s against quu='exact'" % (plan, list(HOT)))
    assert np.array_equal(passes, general_passes) and (passes >= 1).all()
    if "ill one_wavefront" not in _cache:
        _cache["ill one_wavefront"] = _solve(cilqr, dict(PLANS["one_wavefront"], CILQR_FORCE_G="64"), p, sub, N, n_obs)
    assert _same_bits(got, _cache["ill one_wavefront"])
    shown = [k for i, k in enumerate(HOT) if not np.array_equal(got["U"][i], general["U"][i])]
    assert 208 in shown, "solve 208 came back with the GENERAL kernel's bits: handed over"

"""The local plan fit (local_plan.hip + vandermonde_qr.hpp) pinned bit for bit at every abscissa, and at the inputs where the column
pivoting and the rank cut-off decide the answer.

The oracle's own fit forms x^j with libm's pow, which glibc misrounds about once in a thousand calls, so against it the device fit
can only be held to "most fits bit-equal".  Here the oracle takes its Vandermonde entries from `oracle.exact_powers` (exact rational
power, rounded once), the value the kernel's double-double recurrence returns; both sides then run the same algorithm in the same
order from the same matrix, and every comparison below is on bits, in every fit, with no tolerance.

CPU part (no mark): the libm path is unchanged by the split; the oracle agrees with the reference's Eigen on the degenerate fits
recorded in tests/golden/ref_polyfit_edges.json; the kernel's power recurrence, emulated exactly, returns the correctly rounded
power at every abscissa the GPU tests use; the host pre-step gives the oracle's slice and coefficients at exact-power edge cases.
GPU part (`gpu` mark): general paths, magnitudes, degenerate abscissae, ties, slice lengths 1..34 (34 fills the 64 KiB LDS slot
exactly; 35 is refused), batch sizes around the 32-lane workgroup and the three path layouts.

Each comparison prints one line `local_plan_edges <label>: fits=… bit_equal=… patterns=…` before it asserts.
"""
import ctypes as C
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from conftest import load_golden

dp = C.POINTER(C.c_double)
W0 = 20  # num_of_local_wpts of the default parameters


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _pattern(c):
    return "".join("0" if v == 0.0 else "x" for v in c)


# ------------------------------------------------------------------------------------------------ inputs of the GPU tests
# Built once, seeded, and shared between the GPU tests and the CPU check of the power recurrence (C.3 reads every abscissa).
def _sine_y(rng, x, B):
    A, w, ph = rng.uniform(0, 1.5, (B, 1)), rng.uniform(0.02, 0.08, (B, 1)), rng.uniform(0, 2 * np.pi, (B, 1))
    return A * np.sin(w * x + ph)


def _egos_near(rng, paths, k, dx, dy):
    B = paths.shape[0]
    r = np.arange(B)
    return np.stack([paths[r, k, 0] + rng.uniform(-dx, dx, B), paths[r, k, 1] + rng.uniform(-dy, dy, B), rng.uniform(0, 8, B),
                     rng.uniform(-1, 1, B)], axis=1)


@functools.lru_cache(maxsize=None)
def general_case(B=256, P=60, seed=2912):
    """Drawn as test_gpu_parity.test_local_plan_batch_general_paths draws them."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-300, 300, (B, 1)) + np.cumsum(rng.uniform(0.5, 1.5, (B, P)), axis=1)
    paths = np.stack([x, _sine_y(rng, x, B)], axis=2)
    return paths, _egos_near(rng, paths, rng.integers(0, P, B), 0.4, 2.0)


@functools.lru_cache(maxsize=None)
def magnitude_groups(B=64, P=60):
    rng = np.random.default_rng(2913)
    groups = {}

    def put(name, x, scale=1.0):
        paths = np.stack([x, _sine_y(rng, x / scale, B)], axis=2)
        groups[name] = (paths, _egos_near(rng, paths, rng.integers(0, P, B), 0.4 * scale, 2.0))

    for x0 in (1e3, 1e4, 5.3e5, -4.2e5):
        put("at_%g" % x0, x0 + rng.uniform(-50, 50, (B, 1)) + np.cumsum(rng.uniform(0.5, 1.5, (B, P)), axis=1))
    put("at_1e-3", 1e-3 + np.cumsum(rng.uniform(0.5e-4, 1.5e-4, (B, P)), axis=1), scale=1e-4)
    half = np.cumsum(rng.uniform(0.5, 1.5, (B, P // 2)), axis=1)
    put("symmetric", np.concatenate([-half[:, ::-1], half], axis=1))
    c = np.cumsum(rng.uniform(0.5, 1.5, (B, P)), axis=1)
    x = c - c[np.arange(B), rng.integers(0, P, B)][:, None]  # one waypoint of each path at exactly 0.0 …
    assert (x == 0.0).sum() == B
    x[1::2][x[1::2] == 0.0] = -0.0                            # … and -0.0 in every other path
    put("with_zero", x)
    return groups


DEGENERATE_N = (20, 1, 2, 5, 6, 7)


@functools.lru_cache(maxsize=None)
def degenerate_case():
    """One 20-waypoint path per (pattern, n): the ego stands on waypoint 20 - n, so the slice is the path's last n waypoints.
    Repeated abscissae carry distinct ordinates (a vertical stretch), so every waypoint is a distinct point."""
    rng = np.random.default_rng(2914)
    i = np.arange(20.0)
    up = 3.3 + np.cumsum(rng.uniform(0.5, 1.5, 20))
    pats = {"all_equal": np.full(20, 7.3), "all_zero": np.zeros(20), "two_distinct": np.repeat([3.7, 4.9], 10),
            # every power of ±1 is ±1: the column norms tie exactly and the first maximum has to be the pivot
            "all_one": np.ones(20), "all_minus_one": -np.ones(20), "plus_minus_one": np.tile([1.0, -1.0], 10),
            "near_one": 1.0 + rng.uniform(-1e-6, 1e-6, 20)}  # … and norms that tie to a few parts in a million
    for k, at in ((2, 18), (4, 16), (19, 1)):  # a run of k equal abscissae; the short slices of each path include it
        x = up.copy()
        x[at:at + k] = x[at]
        pats["run_of_%d" % k] = x
    out = 10.1 + np.cumsum(rng.uniform(0.5, 1.5, 12))
    pats["doubled_back"] = np.concatenate([out, out[-2:2:-1]])
    names, paths, egos = [], [], []
    for name, x in pats.items():
        y = 0.7 * i + 0.3 * np.sin(0.9 * i)  # strictly increasing
        for n in DEGENERATE_N:
            names.append((name, n))
            paths.append(np.stack([x, y], axis=1))
            egos.append([x[20 - n], y[20 - n], 2.0, 0.1])
    return names, np.array(paths), np.array(egos)


@functools.lru_cache(maxsize=None)
def tie_cases():
    i = np.arange(40.0)
    straight = np.stack([i, 0.5 * i], axis=1)
    ks = np.array([0, 5, 19, 20, 21, 33, 37, 38])  # the last three: slices cut short by the path's end
    # on the perpendicular bisector of waypoints k and k+1, (0.5, -1) off their midpoint: squared distance 1.5625 to both, exactly
    off = np.stack([ks + 1.0, 0.5 * ks - 0.75, np.full(ks.size, 3.0), np.zeros(ks.size)], axis=1)
    on = np.stack([ks + 0.5, 0.5 * ks + 0.25, np.full(ks.size, 3.0), np.zeros(ks.size)], axis=1)  # the midpoint itself: 0.3125 to both
    midway, ks = np.concatenate([on, off]), np.concatenate([ks, ks])
    th = 2 * np.pi * np.arange(24) / 24
    closed = np.stack([30.0 * np.cos(th) + 4.1, 30.0 * np.sin(th) - 2.7], axis=1)
    closed = np.concatenate([closed, closed[:1]])  # the last waypoint is the first
    on_seam = np.array([[closed[0, 0], closed[0, 1], 3.0, 0.0]] * 2)
    rng = np.random.default_rng(2915)
    x = 12.3 + np.cumsum(rng.uniform(0.5, 1.5, 30))
    wavy = np.stack([x, 0.8 * np.sin(0.07 * x)], axis=1)
    nan_egos = np.array([[np.nan, 0.3, 3.0, 0.0], [20.0, np.nan, 3.0, 0.0], [np.nan, np.nan, 3.0, 0.0], [wavy[0, 0], wavy[0, 1], 3.0, 0.0]])
    return dict(midway=(straight, midway, ks), seam=(closed, on_seam), nan=(wavy, nan_egos))


SLICE_LENGTHS = (1, 2, 5, 6, 7, 19, 21, 34)


@functools.lru_cache(maxsize=None)
def slice_length_case(W, B=64, P=40):
    """Non-integer abscissae; egos on the last W waypoints give every n from 1 to W, the rest are drawn."""
    rng = np.random.default_rng(2916 + W)
    x = rng.uniform(-40, 40) + np.cumsum(rng.uniform(0.5, 1.5, P))
    path = np.stack([x, 0.9 * np.sin(0.06 * x + 0.4)], axis=1)
    k = np.concatenate([P - 1 - np.arange(W), rng.integers(0, P, B - W)])
    egos = np.stack([x[k] + rng.uniform(-0.2, 0.2, B), path[k, 1] + rng.uniform(-0.2, 0.2, B), np.full(B, 3.0), np.zeros(B)], axis=1)
    return path, egos


BATCHES = (31, 32, 33, 65)
WINDOW_P, WINDOW_STRIDE = 30, 2  # doubles: each candidate's window starts one waypoint after the previous one's


@functools.lru_cache(maxsize=None)
def stride_case(B):
    rng = np.random.default_rng(2917 + B)
    P = WINDOW_P
    L = (B - 1) * WINDOW_STRIDE // 2 + P
    x = rng.uniform(-100, 100) + np.cumsum(rng.uniform(0.5, 1.5, L))
    long_path = np.stack([x, 1.1 * np.sin(0.05 * x + 1.0)], axis=1)
    xs = rng.uniform(-300, 300, (B, 1)) + np.cumsum(rng.uniform(0.5, 1.5, (B, P)), axis=1)
    per = np.stack([xs, _sine_y(rng, xs, B)], axis=2)
    k = rng.integers(0, P, B)
    k[:3] = [0, P - 1, P - 3]
    win = np.stack([long_path[b:b + P] for b in range(B)])
    mk = lambda paths: _egos_near(rng, paths, k, 0.4, 1.0)  # noqa: E731
    return dict(long_path=long_path, per=per, egos_shared=mk(np.broadcast_to(long_path[:P], (B, P, 2))), egos_per=mk(per),
                egos_win=mk(win), win=win)


def gpu_abscissae():
    """Every abscissa of every path a GPU test of this file sends to the device."""
    xs = [general_case()[0][..., 0]]
    xs += [g[0][..., 0] for g in magnitude_groups().values()]
    xs.append(degenerate_case()[1][..., 0])
    xs += [v[0][:, 0] for v in tie_cases().values()]
    xs += [slice_length_case(W)[0][:, 0] for W in SLICE_LENGTHS + (35,)]
    for B in BATCHES:
        s = stride_case(B)
        xs += [s["long_path"][:, 0], s["per"][..., 0]]
    return np.concatenate([np.ravel(x) for x in xs])


# ------------------------------------------------------------------------------------------------ C.1  the libm path is unchanged
def _libm_vandermonde(x, degree):
    return np.array([[math.pow(xi, float(j)) for j in range(degree + 1)] for xi in x.tolist()]).reshape(len(x), degree + 1)


def test_polyfit_powers_with_libm_powers_is_polyfit(oracle):
    """`oracle_polyfit` is now `oracle_polyfit_powers` behind a libm-filled matrix: handed the same matrix from outside, the powers
    form returns `oracle_polyfit`'s bits on every case of both golden files."""
    n = 0
    for name in ("ref_polyfit.json", "ref_polyfit_edges.json"):
        for c in load_golden(name)["cases"]:
            x, y = np.array(c["x"]), np.array(c["y"])
            assert _same_bits(oracle.polyfit_powers(_libm_vandermonde(x, c["degree"]), y, c["degree"]), oracle.polyfit(x, y, c["degree"])), c
            n += 1
    assert n >= 31


def test_local_plan_exact_is_local_plan_where_libm_is_exact(oracle):
    """At integer abscissae libm's powers are exact: the powers form and the libm form of the local plan agree on every bit."""
    p = oracle.default_params(50)
    i = np.arange(60.0)
    path = np.stack([i, 0.5 * np.sin(0.05 * i)], axis=1)
    for ego in ([0.0, 0.1], [17.4, 0.3], [41.0, -0.2], [55.2, 0.0], [59.0, 0.0], [np.nan, 0.0]):
        c1, r1 = oracle.local_plan(p, path, np.array(ego + [3.0, 0.0]))
        c2, r2 = oracle.local_plan_exact(p, path, np.array(ego + [3.0, 0.0]))
        assert _same_bits(c1, c2) and _same_bits(r1, r2), ego


# ------------------------------------------------------------------------------------------------ C.2  the degenerate fits
def test_polyfit_edges_vs_reference_eigen(oracle):
    """The rule of test_oracle.test_polyfit_vs_reference_eigen on the degenerate fits: the reference's zeroed-column pattern, its
    fitted values within 1e-9·max(1, max|y|), and the live reference equal to the recording where it is built.  Both the libm form
    and the exact-power form of the oracle are held to it."""
    cases = load_golden("ref_polyfit_edges.json")["cases"]
    assert [c["name"] for c in cases] == ["all_equal", "all_zero", "two_distinct", "run_of_four", "doubled_back", "at_1000", "at_10000",
                                          "at_530000", "at_-420000", "symmetric_no_zero", "symmetric_with_zero", "at_1e-3", "n_1",
                                          "n_2", "n_3", "n_5", "n_6", "n_7", "all_one", "all_minus_one", "plus_minus_one",
                                          "plus_minus_one_n_5"]
    live = oracle.ref_lib("eigen")
    for c in cases:
        x, y = np.array(c["x"]), np.array(c["y"])
        ref = np.array(c["coeffs"])
        V = np.vander(x, c["degree"] + 1, increasing=True)
        bound = 1e-9 * max(1.0, np.max(np.abs(y)))
        for form, got in (("libm", oracle.polyfit(x, y, c["degree"])),
                          ("exact", oracle.polyfit_powers(oracle.exact_powers(x, c["degree"]), y, c["degree"]))):
            err = np.max(np.abs(V @ got - V @ ref))
            print("local_plan_edges golden %-20s %-5s pattern=%s share_of_bound=%.3g" % (c["name"], form, _pattern(got), err / bound))
            assert np.array_equal(got == 0.0, ref == 0.0), (c["name"], form)
            assert err < bound, (c["name"], form, err)
        if live is not None:
            chk = np.zeros(c["degree"] + 1)
            live.ref_polyfit(x.ctypes.data_as(dp), y.ctypes.data_as(dp), len(x), c["degree"], chk.ctypes.data_as(dp))
            assert _same_bits(chk, ref), c["name"]
    assert len({_pattern(c["coeffs"]) for c in cases}) >= 5  # the recording spans ranks 1 to 6


# ------------------------------------------------------------------------------------------------ C.3  the kernel's powers are exact
def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # one rounding: Python's big-integer division rounds to nearest even


def pow_small_int_emulated(x, degree):
    """local_plan.hip's `pow_small_int(x, j)` for j = 0..degree, operation for operation: (hi + lo)·x kept as an unevaluated sum.
    (The loop's state after t rounds does not depend on j, so one pass yields every j.)"""
    out = [1.0, x]
    hi, lo = x, 0.0
    for _ in range(2, degree + 1):
        p = hi * x
        e = _fma(hi, x, -p)
        e = _fma(lo, x, e)
        s = p + e
        lo = e - (s - p)
        hi = s
        out.append(hi)
    return out[:degree + 1]


def test_power_recurrence_is_exact_at_every_gpu_abscissa(oracle):
    """A condition on the inputs of the GPU tests, not a tolerance: at each of their abscissae the kernel's double-double recurrence
    (emulated with an exact fma) returns `exact_powers`' value for j = 0..5 — zero mismatches.  (Values are compared; at x = ±0.0
    every power above the zeroth is a zero on both sides.  The recurrence returns +0.0 for (-0.0)^3 and (-0.0)^5 where the rounded
    exact power and libm give -0.0; a zero's sign in the matrix reaches no output bit, which the `with_zero` group of the
    magnitudes test shows on the device.)"""
    x = np.unique(gpu_abscissae())
    x = np.concatenate([x, [-0.0]])  # np.unique keeps one of ±0.0
    assert np.isfinite(x).all() and x.size > 20000
    want = oracle.exact_powers(x, 5)
    bad = [(xi, j) for xi, w in zip(x.tolist(), want.tolist()) for j, g in enumerate(pow_small_int_emulated(xi, 5)) if g != w[j]]
    print("local_plan_edges powers: abscissae=%d powers_checked=%d mismatches=%d" % (x.size, 4 * x.size, len(bad)))
    assert not bad, bad[:5]
    assert np.all(want[:, 0] == 1.0) and _same_bits(want[:, 1], x)
    tiny = np.abs(want[:, 5][x != 0.0]).min()
    assert tiny > 2.3e-308  # every fifth power is a normal double: the domain in which the recurrence is exact


def test_exact_powers_is_the_rounded_rational_power(oracle):
    """`exact_powers` against its definition and against cases with a known answer."""
    x = np.array([3.0, -2.5, 1.3, 1e3 + 1 / 3, -4.2e5 - 0.7, 1.234e-3, 0.0, -0.0])
    got = oracle.exact_powers(x, 5)
    for xi, row in zip(x.tolist(), got):
        for j in range(6):
            assert row[j] == float(Fraction(xi) ** j)
    assert got[0].tolist() == [1.0, 3.0, 9.0, 27.0, 81.0, 243.0] and got[1].tolist() == [1.0, -2.5, 6.25, -15.625, 39.0625, -97.65625]
    assert _same_bits(got[6], [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]) and _same_bits(got[7], [1.0, -0.0, 0.0, -0.0, 0.0, -0.0])
    assert got[2, 2] == 1.3 * 1.3 and got[2, 3] != 1.3 * 1.3 * 1.3  # the cube of the double 1.3 is not what two roundings give


# ------------------------------------------------------------------------------------------------ C.4  the host pre-step
def _host_cases():
    q = np.arange(40.0) * 0.25 + 100.5  # dyadic: ten significant bits, every power to the fifth is exact
    i = np.arange(40.0)
    y = 0.4 * np.sin(0.3 * i) + 0.05 * i
    straight = np.stack([i, np.zeros(40)], axis=1)
    cases = [("tie", straight, [k + 0.5, 1.0], k) for k in (0, 7, 20, 36, 38)]
    dup = q.copy()
    dup[10:14] = dup[10]
    cases += [("duplicated", np.stack([dup, y], axis=1), [dup[k], y[k]], k) for k in (0, 8, 12, 25)]
    eq = np.stack([np.full(40, 6.75), y], axis=1)
    cases += [("all_equal", eq, [6.75, y[k]], k) for k in (0, 19, 35, 39)]
    zero = np.stack([np.zeros(40), y], axis=1)
    cases += [("all_zero", zero, [0.0, y[k]], k) for k in (3, 37)]
    one, pm = np.stack([np.ones(40), y], axis=1), np.stack([np.tile([1.0, -1.0], 20), y], axis=1)  # the column norms tie exactly
    cases += [("all_one", one, [1.0, y[k]], k) for k in (0, 35)] + [("plus_minus_one", pm, [pm[k, 0], y[k]], k) for k in (1, 20, 35)]
    wavy = np.stack([q, y], axis=1)
    cases += [("nan_ego", wavy, e, 0) for e in ([np.nan, 0.0], [101.0, np.nan], [np.nan, np.nan])]
    cases += [("short", wavy, [q[40 - n], y[40 - n]], 40 - n) for n in (1, 2, 3, 4, 5, 6, 7)]
    return cases


def test_host_pre_step_is_the_oracle_at_exact_power_edges(cilqr, oracle):
    """`cilqr_local_plan` (local_planner.cpp, the host instantiation of vandermonde_qr.hpp; no device) at integer and dyadic
    abscissae, where libm's powers are exact: the exact tie (strict-< first minimum), duplicated x, all-equal x, all-zero x, a NaN
    ego (index 0) and n < 6.  The oracle's slice; coefficients and fitted row bit for bit, against both forms of the oracle."""
    p, po = cilqr.default_params(), oracle.default_params()
    seen = set()
    for name, path, exy, first in _host_cases():
        ego = np.array(list(exy) + [3.0, 0.0])
        c, ref = cilqr.local_plan(p, path, ego)
        ce, re = oracle.local_plan_exact(po, path, ego)
        cl, rl = oracle.local_plan(po, path, ego)
        n = min(W0, len(path) - first)
        assert ref.shape == re.shape == (n, 2) and _same_bits(ref[:, 0], path[first:first + n, 0]), (name, first)
        assert _same_bits(c, ce) and _same_bits(c, cl), (name, first, c, ce)
        assert _same_bits(ref, re) and _same_bits(ref, rl), (name, first)
        seen.add(_pattern(c))
    assert len(seen) >= 4, seen


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(10), max_batch=256, max_horizon=10, max_obstacles=0, device=0)
    yield s
    s.close()


def _exact_plans(O, p, paths, egos, powers=None):
    """The oracle with exactly rounded powers, candidate by candidate.  paths: (P, 2) shared or (B, P, 2)."""
    B = egos.shape[0]
    shared = paths.ndim == 2
    if powers is None:
        powers = O.exact_powers(paths[..., 0], p.poly_order).reshape(paths.shape[:-1] + (p.poly_order + 1,))
    polys, fls, ns, refs = [], [], [], []
    for b in range(B):
        c, ref = O.local_plan_exact(p, paths if shared else paths[b], egos[b], powers if shared else powers[b])
        polys.append(c)
        fls.append([ref[0, 0], ref[-1, 0]])
        ns.append(ref.shape[0])
        refs.append(ref)
    return dict(poly=np.array(polys), xplan_fl=np.array(fls), n=np.array(ns, dtype=np.int32), refs=refs)


def _compare(label, got, want, W=W0):
    """n, xplan_fl, poly and ref_traj[:n] on bits in every fit; the host form's ref_traj zero past n.  Returns the patterns seen."""
    B = want["n"].size
    ok = np.zeros(B, dtype=bool)
    for b in range(B):
        n = int(want["n"][b])
        ok[b] = (int(got["n"][b]) == n and _same_bits(got["xplan_fl"][b], want["xplan_fl"][b]) and _same_bits(got["poly"][b], want["poly"][b])
                 and _same_bits(got["ref_traj"][b, :n], want["refs"][b]) and not _bits(got["ref_traj"][b, n:]).any())
    pats = sorted({_pattern(c) for c in want["poly"]})
    print("local_plan_edges %s: fits=%d bit_equal=%d n=%d..%d patterns=%s" % (label, B, int(ok.sum()), want["n"].min(), want["n"].max(),
                                                                             ",".join(pats)))
    assert got["ref_traj"].shape == (B, W, 2) and got["poly"].shape == (B, 6)
    assert ok.all(), "%s: fits that differ from the exact-power oracle: %s" % (label, np.nonzero(~ok)[0][:16].tolist())
    return set(pats)


@pytest.mark.gpu
def test_general_paths_every_fit_bit_equal(cilqr, oracle, solver):
    """256 paths in global coordinates of a few hundred metres, non-integer abscissae: all 256 fits."""
    paths, egos = general_case()
    want = _exact_plans(oracle, oracle.default_params(50), paths, egos)
    assert want["n"].min() < 6 and want["n"].max() == W0
    _compare("general", solver.local_plan_batch(paths, egos), want)


@pytest.mark.gpu
def test_magnitudes_every_fit_bit_equal(cilqr, oracle, solver):
    """First abscissae near 1e3, 1e4, 5.3e5 (UTM size), -4.2e5, at 1e-3, symmetric about zero, and through an exact 0.0 / -0.0:
    the rank cut-off removes a different set of columns from group to group."""
    p = oracle.default_params(50)
    seen = set()
    for name, (paths, egos) in magnitude_groups().items():
        want = _exact_plans(oracle, p, paths, egos)
        seen |= _compare("magnitude " + name, solver.local_plan_batch(paths, egos), want)
    x = magnitude_groups()["with_zero"][0][..., 0]
    assert (_bits(x) == _bits(np.array([-0.0]))[0]).sum() == 32 and (_bits(x) == 0).sum() == 32
    assert len(seen) >= 3, seen


@pytest.mark.gpu
def test_degenerate_abscissae_every_fit_bit_equal(cilqr, oracle, solver):
    """All 20 abscissae equal, all zero, two distinct values, all 1, all -1, alternating ±1 (the column norms tie exactly: the first
    maximum is the pivot), all within 1e-6 of 1, a run of 2, 4 and 19 equal, a doubled-back path; each at the full slice and cut
    short by the path's end to n = 1, 2, 5, 6, 7."""
    names, paths, egos = degenerate_case()
    want = _exact_plans(oracle, oracle.default_params(50), paths, egos)
    assert want["n"].tolist() == [n for _, n in names]
    assert _pattern(want["poly"][names.index(("all_equal", 20))]) == "00000x" and _pattern(want["poly"][names.index(("all_zero", 20))]) == "x00000"
    _compare("degenerate", solver.local_plan_batch(paths, egos), want)


@pytest.mark.gpu
def test_ties_every_fit_bit_equal(cilqr, oracle, solver):
    """The strict-< first-minimum rule: an ego exactly midway between waypoints k and k+1 takes k; on the seam of a closed path
    it takes 0, not the equal last waypoint; a NaN in the ego compares false everywhere and takes 0."""
    p = oracle.default_params(50)
    t = tie_cases()
    straight, egos, ks = t["midway"]
    want = _exact_plans(oracle, p, straight, egos)
    assert np.array_equal(want["xplan_fl"][:, 0], ks.astype(float)) and want["n"].tolist() == [min(W0, 40 - k) for k in ks]
    _compare("tie midway", solver.local_plan_batch(straight, egos), want)
    closed, egos = t["seam"]
    want = _exact_plans(oracle, p, closed, egos)
    assert want["n"].tolist() == [W0, W0] and _same_bits(want["xplan_fl"][:, 0], closed[[0, 0], 0])
    _compare("tie seam", solver.local_plan_batch(closed, egos), want)
    wavy, egos = t["nan"]
    want = _exact_plans(oracle, p, wavy, egos)
    assert _same_bits(want["xplan_fl"][:, 0], wavy[[0] * 4, 0]) and all(_same_bits(want["poly"][b], want["poly"][3]) for b in range(3))
    _compare("tie nan ego", solver.local_plan_batch(wavy, egos), want)


@pytest.mark.gpu
@pytest.mark.parametrize("W", SLICE_LENGTHS)
def test_slice_lengths_every_fit_bit_equal(cilqr, oracle, W):
    """num_of_local_wpts other than 20 (the plain-loop instantiation of the kernel) at non-integer abscissae, every n from 1 to W
    in one batch.  34 is the largest whose LDS slot fits: 32·((34·7 + 12)·8 + 48) = 65 536 bytes."""
    p, po = cilqr.default_params(10), oracle.default_params(10)
    p.num_of_local_wpts = po.num_of_local_wpts = W
    path, egos = slice_length_case(W)
    want = _exact_plans(oracle, po, path, egos)
    assert set(want["n"].tolist()) == set(range(1, W + 1))
    s = cilqr.Solver(p, max_batch=64, max_horizon=10, max_obstacles=0, device=0)
    try:
        got = s.local_plan_batch(path, egos)
    finally:
        s.close()
    _compare("slice W=%d" % W, got, want, W)


@pytest.mark.gpu
def test_slice_length_35_is_refused_and_touches_nothing(cilqr, oracle, solver):
    """One past the LDS slot: CILQR_ERR_UNSUPPORTED, outputs as they were; a default handle afterwards still gives the oracle's fit."""
    p = cilqr.default_params(10)
    p.num_of_local_wpts = 35
    path, egos = slice_length_case(35)
    B, P = egos.shape[0], path.shape[0]
    path, egos = np.ascontiguousarray(path), np.ascontiguousarray(egos)
    poly, fl, ref = np.full((B, 6), 1234.5), np.full((B, 2), 1234.5), np.full((B, 35, 2), 1234.5)
    n = np.full(B, -7, dtype=np.int32)
    s = cilqr.Solver(p, max_batch=64, max_horizon=10, max_obstacles=0, device=0)
    try:
        rc = cilqr.lib().cilqr_local_plan_batch(s._h, B, P, path.ctypes.data_as(dp), C.c_int64(0), egos.ctypes.data_as(dp), poly.ctypes.data_as(dp),
                                                fl.ctypes.data_as(dp), ref.ctypes.data_as(dp), n.ctypes.data_as(C.POINTER(C.c_int32)))
        with pytest.raises(cilqr.CilqrError):
            s.local_plan_batch(path, egos)
    finally:
        s.close()
    assert rc == -4  # CILQR_ERR_UNSUPPORTED (include/cilqr.h)
    assert (poly == 1234.5).all() and (fl == 1234.5).all() and (ref == 1234.5).all() and (n == -7).all()
    want = _exact_plans(oracle, oracle.default_params(50), path, egos)
    _compare("after refusal", solver.local_plan_batch(path, egos), want)


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
def test_batch_and_stride_shapes_every_fit_bit_equal(cilqr, oracle, solver, B):
    """Batches one short of, on and one past the 32-lane workgroup, and two workgroups and one lane; a shared path (stride 0), one
    path per candidate, and overlapping windows over one long path (stride 2 doubles = one waypoint, through the device form): each
    candidate gets the oracle's answer for its own window.  The device form without ref_traj and n_out writes the same rest."""
    import torch
    p = oracle.default_params(50)
    sc = stride_case(B)
    P = WINDOW_P
    shared = np.ascontiguousarray(sc["long_path"][:P])
    _compare("B=%d shared" % B, solver.local_plan_batch(shared, sc["egos_shared"]), _exact_plans(oracle, p, shared, sc["egos_shared"]))
    _compare("B=%d per-candidate" % B, solver.local_plan_batch(sc["per"], sc["egos_per"]), _exact_plans(oracle, p, sc["per"], sc["egos_per"]))

    want = _exact_plans(oracle, p, sc["win"], sc["egos_win"])
    assert len({tuple(f) for f in want["xplan_fl"].tolist()}) > B // 2  # the windows really differ
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_path, d_ego = t(sc["long_path"]), t(sc["egos_win"])
    assert d_path.numel() == (B - 1) * WINDOW_STRIDE + 2 * P  # the last window ends on the path's last waypoint
    z = lambda *shape, dt=torch.float64: torch.zeros(*shape, dtype=dt, device=dev)  # noqa: E731
    poly, fl, ref, n = z(B, 6), z(B, 2), z(B, W0, 2), z(B, dt=torch.int32)
    poly2, fl2 = z(B, 6), z(B, 2)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    solver.local_plan_batch_device(st, B, P, d_path.data_ptr(), WINDOW_STRIDE, d_ego.data_ptr(), poly.data_ptr(), fl.data_ptr(),
                                   ref.data_ptr(), n.data_ptr())
    solver.local_plan_batch_device(st, B, P, d_path.data_ptr(), WINDOW_STRIDE, d_ego.data_ptr(), poly2.data_ptr(), fl2.data_ptr())
    torch.cuda.synchronize()
    got = dict(poly=poly.cpu().numpy(), xplan_fl=fl.cpu().numpy(), ref_traj=ref.cpu().numpy(), n=n.cpu().numpy())
    _compare("B=%d windows" % B, got, want)
    assert _same_bits(poly2.cpu().numpy(), want["poly"]) and _same_bits(fl2.cpu().numpy(), want["xplan_fl"])

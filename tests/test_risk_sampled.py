"""Gains and fused rollout risk for sampled obstacles in compact form (cilqr_gains_batch_sampled*, cilqr_rollout_risk_sampled*,
include/cilqr.h): n_obs moving obstacles x n_samples Gaussian pose samples, taken as nominal tables + sample offsets.

Expected values come from the CPU oracle's exported pieces alone, through the helpers of the suite: gains from oracle_backward_pass
(o_gains) on the MATERIALISED obstacles (scenes.materialise_samples), rollouts from o_rollout, c from `_expected(...)[1]` of
tests/test_candidate_score.py on the materialised obstacles per rollout row, and the eight fields by numpy from that c:
h(r, t, o) = #{samples j of obstacle o : max(c_front, c_rear) > 0 at state t of row r}.
Tolerances are the suite's: gains |d| <= 1e-9 * max(1, max|oracle value| of that solve); WORST_C 1e-9 absolute; every count, share,
row, entry, step and pick exact.  What makes the exact comparisons meaningful is asserted on the oracle's numbers in a CPU test:
every c that decides a hit is more than 1e-6 from 0, and the two largest c of every solve are more than 1e-6 apart (which decides the
worst row and the worst entry at once).

Scenes, N = 12: make_static(B, 12, n_obs, p, 7); nominal obstacle 0 of solve b starts 1.0 m ahead of the start and (lat0 + 0.1 b) m to
its left, heading = start heading, moving along it at 1.5 m/s; sample offsets PCG64(oseed).normal(0, 1, (B, n_obs, n_samples, 3)) *
POSE_SIGMA; ego offsets pose_offsets(S, 0.16, 0.16, 0.017, dseed) shared by all solves; trajectories solved by the oracle on the
materialised obstacles with weight 1/n_samples; gains at lamb 1, rollouts at k_scale 0.
  S  B 6, 2 x 8 samples,  S = 70  (lat0 3.4, oseed 9,  dseed 5): a partial second wavefront
  T  B 3, 3 x 32 samples, S = 5   (lat0 3.4, oseed 10, dseed 6): 96 entries per step built by 64 lanes, 59 lanes without a row
  V  B 2, 3 x 5 samples,  S = 300 (lat0 3.5, oseed 11, dseed 8): two workgroups per solve, the second with 44 rows (three wavefronts
     of it have no row at all)
"""
import ctypes as C
import itertools
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_candidate_score import _bits, _expected, _totals
from test_rollout_risk import _close, _pick, o_gains, o_rollout

gpu = pytest.mark.gpu

ABS_TOL, MARGIN = 1e-9, 1e-6
ERR_ARG, ERR_UNSUPPORTED = -1, -4
ENTRY_POINTS = ("cilqr_gains_batch_sampled", "cilqr_gains_batch_sampled_device", "cilqr_rollout_risk_sampled",
                "cilqr_rollout_risk_sampled_device")
FIELD_NAMES = ("COLLISION", "WORST_C", "WORST_ROW", "WORST_ENTRY", "FIRST_STEP", "STEP_SHARE", "ANY_SHARE", "PAIR_SHARE")
COLLISION, WORST_C, WORST_ROW, WORST_ENTRY, FIRST_STEP, STEP_SHARE, ANY_SHARE, PAIR_SHARE = range(8)
EXACT = (COLLISION, WORST_ROW, WORST_ENTRY, FIRST_STEP, STEP_SHARE, ANY_SHARE, PAIR_SHARE)
RR_COLLISION, RR_WORST_C, RR_WORST_ROW, RR_WORST_ENTRY, RR_FIRST_STEP = range(5)  # cilqr_rollout_risk_field
N_STEPS = 12
SCENES = {  # B, n_obs, n_samples, S, lat0, oseed, dseed
    "S": (6, 2, 8, 70, 3.4, 9, 5),
    "T": (3, 3, 32, 5, 3.4, 10, 6),
    "V": (2, 3, 5, 300, 3.5, 11, 8),
}
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


# ---- expected values from the oracle ------------------------------------------------------------------------------------------
def _reduce(c, n_obs, ns, lost=None):
    """c (B, S, M, N, 2) of `_expected` on the materialised obstacles, m = o*ns + j -> what the call returns, by numpy.  lost (B, S, N)
    bool: rows whose state or control is not finite at a step (h = ns for every obstacle there); such rows must carry c = -inf."""
    B, S, M, N = c.shape[:4]
    per_entry = c.max(axis=4)                                                   # (B, S, M, N): max(c_front, c_rear)
    h = (per_entry > 0).reshape(B, S, n_obs, ns, N).sum(axis=3)                 # (B, S, n_obs, N)
    if lost is not None:
        h = np.where(lost[:, :, None, :], ns, h)
    step_hits = h.max(axis=2).sum(axis=1).astype(np.int32)                      # (B, N): sum over rows of max_o h
    pair = h.sum(axis=1)                                                        # (B, n_obs, N): sum over rows of h
    row_max = h.max(axis=(2, 3))                                                # (B, S)
    risk = np.zeros((B, 8))
    risk[:, COLLISION] = row_max.sum(axis=1) / (S * ns)
    any_step = step_hits > 0
    risk[:, FIRST_STEP] = np.where(any_step.any(axis=1), any_step.argmax(axis=1), -1)
    risk[:, STEP_SHARE] = step_hits.max(axis=1) / (S * ns)
    risk[:, ANY_SHARE] = (row_max > 0).sum(axis=1) / S
    risk[:, PAIR_SHARE] = pair.max(axis=(1, 2)) / (S * ns)
    flat = per_entry.reshape(B, S, M * N)                                       # entry index m*N + t
    rows = flat.max(axis=2).argmax(axis=1)
    risk[:, WORST_C] = flat.max(axis=(1, 2))
    risk[:, WORST_ROW] = rows
    risk[:, WORST_ENTRY] = [int(flat[b, rows[b]].argmax()) for b in range(B)]
    return dict(risk=risk, step_hits=step_hits, h=h, any_rows=(row_max > 0).sum(axis=1), sum_max=row_max.sum(axis=1), pair_max=pair.max(axis=(1, 2)))


def _scene(O, name):
    """Scene `name` solved by the oracle, with the oracle's gains, rollouts, c and the fields reduced from it."""
    from cilqr_amd import scenes
    B, n_obs, ns, S, lat0, oseed, dseed = SCENES[name]
    N, M = N_STEPS, n_obs * ns
    p = O.default_params(N)
    sc = scenes.make_static(B, N, n_obs, p, 7, local_plan=O.local_plan)
    nom = sc["obs_pose"].reshape(B, n_obs, N, 4).copy()
    t = np.arange(N) * p.timestep
    for b in range(B):
        x, y, _, th = sc["x0"][b]
        lat = lat0 + 0.1 * b
        nom[b, 0, :, 0] = x + 1.0 * np.cos(th) - lat * np.sin(th) + (1.5 * np.cos(th)) * t
        nom[b, 0, :, 1] = y + 1.0 * np.sin(th) + lat * np.cos(th) + (1.5 * np.sin(th)) * t
        nom[b, 0, :, 2] = 1.5
        nom[b, 0, :, 3] = th
    nom_pose, nom_dim = np.ascontiguousarray(nom.reshape(B, n_obs, 4 * N)), np.ascontiguousarray(sc["obs_dim"].reshape(B, n_obs, 2 * N))
    off = np.random.Generator(np.random.PCG64(oseed)).normal(0.0, 1.0, (B, n_obs, ns, 3)) * scenes.POSE_SIGMA
    pose, dim, w = scenes.materialise_samples(nom_pose, nom_dim, off, N)
    pose, dim = np.ascontiguousarray(pose), np.ascontiguousarray(dim)
    r = O.solve_batch(p, N, M, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], pose, dim, w, threads=min(8, O.max_threads()))
    X, U, poly, fl = r["X"], r["U"], sc["poly"], sc["xplan_fl"]
    k, K, ok = o_gains(O, p, N, X, U, poly, fl, pose, dim, w, 1.0)
    assert np.all(ok == 1)
    delta = scenes.pose_offsets(S, 0.16, 0.16, 0.017, seed=dseed)
    Xr, Ur = o_rollout(O, p, N, X, U, k, K, np.ascontiguousarray(np.broadcast_to(delta, (B, S, 4))), 0.0)
    rep = lambda a: np.ascontiguousarray(np.repeat(a, S, axis=0))  # noqa: E731  (row r belongs to solve r // S)
    _, c = _expected(O, p, N, Xr.reshape(B * S, -1), Ur.reshape(B * S, -1), rep(poly), rep(fl), rep(pose), rep(dim))
    c = c.reshape(B, S, M, N, 2)
    nominal, _ = _expected(O, p, N, X, U, poly, fl, pose, dim, w, n_samples=ns)
    out = dict(name=name, p=p, B=B, N=N, M=M, n_obs=n_obs, ns=ns, S=S, X=X, U=U, k=k, K=K, poly=poly, fl=fl, nom_pose=nom_pose, nom_dim=nom_dim,
               off=off, weight=1.0 / ns, pose=pose, dim=dim, w=w, delta=delta, c=c, base=_totals(nominal))
    out.update(_reduce(c, n_obs, ns))
    return out


@pytest.fixture(scope="module")
def cases(oracle):
    """Scenes S, T and V from the oracle.  Computed once; never modified."""
    return {name: _scene(oracle, name) for name in SCENES}


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_facade_export_the_calls(cilqr):
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cilqr.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert name in cilqr.ABI_SYMBOLS, name
        assert hasattr(cilqr.lib(), name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    assert cilqr.lib().cilqr_abi_version() == 2  # additive: the ABI number stays
    assert re.search(r"#define\s+CILQR_ABI_VERSION\s+2\b", h)
    assert re.search(r"#define\s+CILQR_RRS_FIELDS\s+8\b", h)
    for i, name in enumerate(FIELD_NAMES):
        assert re.search(r"\bCILQR_RRS_%s\s*=\s*%d\b" % (name, i), h), name
        assert getattr(cilqr, "RRS_" + name) == i
    assert cilqr.RRS_FIELDS == 8
    for name in ("gains_batch_sampled", "rollout_risk_sampled"):
        assert callable(getattr(cilqr.Solver, name)) and callable(getattr(cilqr.Solver, name + "_device"))
    f = open(os.path.join(PKG, "host", "ilqr_adapter.h")).read()
    assert re.search(r"void\s+set_obstacle_samples\s*\(\s*const\s+std::vector<double>&\s+offsets\s*,\s*int\s+n_samples\s*\)", f)


@pytest.mark.parametrize("name", ["S", "T", "V"])
def test_conditions(cases, name):
    """What keeps the exact comparisons of the GPU tests from hiding a failure, on the oracle's numbers alone; and the oracle's counts
    for the three scenes, as recorded when the scenes were designed."""
    s = cases[name]
    c, B, S, M, N = s["c"], s["B"], s["S"], s["M"], s["N"]
    assert not np.isnan(c).any()
    finite = c[np.isfinite(c)]
    top = np.sort(c.max(axis=4).reshape(B, S * M * N), axis=1)
    gap = float(np.min(top[:, -1] - top[:, -2]))
    print("scene %s: min|c| %.3g, smallest top-two gap %.3g, rows that hit %s of %d, sum of max h %s of %d, pair maxima %s"
          % (name, np.min(np.abs(finite)), gap, s["any_rows"].tolist(), S, s["sum_max"].tolist(), S * s["ns"], s["pair_max"].tolist()))
    assert np.min(np.abs(finite)) >= MARGIN  # every c that decides a hit
    assert gap >= MARGIN                     # the worst c of every solve, hence its row and its entry
    want = {"S": ([67, 12, 68, 9, 0, 18], [243, 23, 133, 18, 0, 18], [242, 23, 116, 17, 0, 18]),
            "T": ([5, 5, 5], [121, 64, 53], [93, 48, 41]),
            "V": ([111, 61], [259, 113], [254, 98])}[name]
    assert (s["any_rows"].tolist(), s["sum_max"].tolist(), s["pair_max"].tolist()) == tuple(map(list, want))


def test_argument_errors_need_no_device(cilqr):
    """NULL required pointers, total without base, S < 1, a negative stride, a NaN k_scale or max_risk, a lamb that is not finite, fewer
    than two samples: CILQR_ERR_ARG, decided before the handle is looked at (there is none here)."""
    L = cilqr.lib()
    B, N, n_obs, ns, S = 2, 4, 1, 2, 3
    X, U, k, K = np.zeros((B, 4 * (N + 1))), np.zeros((B, 2 * N)), np.zeros((B, 2 * N)), np.zeros((B, 8 * N))
    poly, fl = np.zeros((B, 6)), np.zeros((B, 2))
    pose, dim, off, delta = np.zeros((B, n_obs, 4 * N)), np.ones((B, n_obs, 2 * N)), np.zeros((B, n_obs, ns, 3)), np.zeros((S, 4))
    risk, hits, total, base, ok = np.zeros((B, 8)), np.zeros((B, N), dtype=np.int32), np.zeros(B), np.zeros(B), np.zeros(B, dtype=np.int32)
    no_handle = C.c_void_p()
    d = C.c_double

    def risk_call(dev, S_=S, ns_=ns, n_obs_=n_obs, stride=0, ks=0.0, mr=1.0, **nulls):
        a = dict(X=X, U=U, k=k, K=K, delta=delta, pose=pose, dim=dim, off=off, risk=risk, base=base, total=total)
        a.update(nulls)
        f = L.cilqr_rollout_risk_sampled_device if dev else L.cilqr_rollout_risk_sampled
        head = (no_handle, None) if dev else (no_handle,)
        return f(*head, B, N, n_obs_, ns_, S_, _p(a["X"]), _p(a["U"]), _p(a["k"]), _p(a["K"]), _p(a["delta"]), C.c_int64(stride), d(ks),
                 _p(a["pose"]), _p(a["dim"]), _p(a["off"]), d(mr), _p(a["base"]), _p(a["risk"]), _p(hits, _ip), _p(a["total"]))

    def gains_call(dev, ns_=ns, n_obs_=n_obs, lamb=1.0, **nulls):
        a = dict(X=X, U=U, poly=poly, fl=fl, pose=pose, dim=dim, off=off, k=k, K=K)
        a.update(nulls)
        f = L.cilqr_gains_batch_sampled_device if dev else L.cilqr_gains_batch_sampled
        head = (no_handle, None) if dev else (no_handle,)
        return f(*head, B, N, n_obs_, ns_, _p(a["X"]), _p(a["U"]), _p(a["poly"]), _p(a["fl"]), _p(a["pose"]), _p(a["dim"]), _p(a["off"]), d(0.5),
                 d(lamb), _p(a["k"]), _p(a["K"]), _p(ok, _ip))

    for dev in (False, True):
        for name in ("X", "U", "k", "K", "delta", "pose", "dim", "off", "risk"):
            assert risk_call(dev, **{name: None}) == ERR_ARG and b"null required pointer" in L.cilqr_last_error(), name
        assert risk_call(dev, base=None) == ERR_ARG and b"total needs base" in L.cilqr_last_error()
        assert risk_call(dev, S_=0) == ERR_ARG and b"S >= 1" in L.cilqr_last_error()
        assert risk_call(dev, stride=-1) == ERR_ARG and b"negative stride" in L.cilqr_last_error()
        assert risk_call(dev, ks=float("nan")) == ERR_ARG and b"NaN" in L.cilqr_last_error()
        assert risk_call(dev, mr=float("nan")) == ERR_ARG and b"NaN" in L.cilqr_last_error()
        assert risk_call(dev, ns_=1) == ERR_ARG and b"n_samples >= 2" in L.cilqr_last_error()
        assert risk_call(dev, n_obs_=0) == ERR_ARG and b"n_obs >= 1" in L.cilqr_last_error()
        assert risk_call(dev) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid arguments, no handle
        assert risk_call(dev, base=None, total=None) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # neither: valid too
        for name in ("X", "U", "poly", "fl", "pose", "dim", "off", "k", "K"):
            assert gains_call(dev, **{name: None}) == ERR_ARG and b"null required pointer" in L.cilqr_last_error(), name
        for lamb in (float("nan"), float("inf")):
            assert gains_call(dev, lamb=lamb) == ERR_ARG and b"not finite" in L.cilqr_last_error()
        assert gains_call(dev, ns_=1) == ERR_ARG and b"n_samples >= 2" in L.cilqr_last_error()
        assert gains_call(dev) == ERR_ARG and b"null handle" in L.cilqr_last_error()


def test_the_two_host_plans(tmp_path):
    """csrc/cilqr_host_plan.h, plan_gains_sampled and plan_rollout_risk_sampled through tests/cpp/host_plan_sampled_dump.cpp: offsets
    16-byte aligned and back to back, inputs a prefix and outputs a suffix (one copy each way moves a packed call), every array of the
    size the header gives it, obstacle weights dropped, and `end` within the arena host_arena_bytes gives the smallest handle that takes
    the call."""
    exe = str(tmp_path / "host_plan_sampled_dump")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "host_plan_sampled_dump.cpp")], check=True)
    shapes, wants = [], []
    for B, N, n_obs, ns, opt in itertools.product([1, 3, 64], [1, 5, 50], [1, 3], [2, 5], [0, 1]):
        X, U, K = B * 4 * (N + 1) * 8, B * 2 * N * 8, B * 8 * N * 8
        samp = {"nom_pose": B * n_obs * N * 32, "nom_dim": B * n_obs * N * 16, "samp_off": B * n_obs * ns * 24}
        common = dict(B=B, N=N, n_obs=n_obs, n_samples=ns, opt=opt)
        shapes.append(dict(form="gains_batch_sampled", **common))
        wants.append((dict(X=X, U=U, poly=B * 48, xplan_fl=B * 16, **samp), dict(k_out=U, K_out=K, ok_out=B * 4 if opt else 0)))
        for S, delta_sets in itertools.product([1, 3], [1, B]):
            shapes.append(dict(form="rollout_risk_sampled", S=S, delta_sets=delta_sets, **common))
            wants.append((dict(X=X, U=U, k=U, K=K, delta=delta_sets * S * 32, base=B * 8 if opt else 0, **samp),
                          dict(risk=B * 8 * 8, step_hits=B * N * 4 if opt else 0, total=B * 8 if opt else 0)))
    args = [",".join("%s=%s" % kv for kv in s.items()) for s in shapes]
    plans = [json.loads(line) for line in subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.splitlines()]
    assert len(plans) == len(shapes)
    for shape, (ins, outs), p in zip(shapes, wants, plans):
        assert p["ok"] == 1, shape
        entries, at = p["entries"], 0
        for off, nbytes, _, _ in entries:
            assert off % 16 == 0 and off == at and nbytes > 0, (shape, entries)
            at = (off + nbytes + 15) // 16 * 16
        assert p["end"] == at and len(entries) <= 12, shape
        n_in = len([b for b in ins.values() if b])
        assert all(i and not o for _, _, i, o in entries[:n_in]) and all(o and not i for _, _, i, o in entries[n_in:]), (shape, entries)
        assert p["in_end"] == p["out_begin"] == (entries[n_in][0] if n_in < len(entries) else p["end"]), shape
        by_off = {off: nbytes for off, nbytes, _, _ in entries}
        assert len(entries) == len([b for b in list(ins.values()) + list(outs.values()) if b]), (shape, entries)
        for name, nbytes in list(ins.items()) + list(outs.items()):
            assert (p["at"][name] == -1) if nbytes == 0 else (by_off[p["at"][name]] == nbytes), (shape, name)
        assert p["at"]["obs_weight"] == -1, shape  # neither kernel reads per-obstacle weights: they do not travel
        assert p["end"] <= p["cap"], (shape, p["end"], p["cap"])


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(N_STEPS), max_batch=16, max_horizon=N_STEPS, max_obstacles=96, device=0)
    yield s
    s.close()


def _host(solver, s, sel=slice(None), delta=None, max_risk=1.0, base=None):
    return solver.rollout_risk_sampled(s["N"], s["X"][sel], s["U"][sel], s["k"][sel], s["K"][sel], s["delta"] if delta is None else delta,
                                       s["nom_pose"][sel], s["nom_dim"][sel], s["off"][sel], k_scale=0.0, max_risk=max_risk, base=base)


def _device(cilqr, solver, s, base=None, max_risk=1.0, materialised=False):
    """The device form on torch buffers: (risk, step_hits, total); materialised: cilqr_rollout_risk_device on the materialised
    obstacles and the same buffers instead."""
    import torch
    B, N, S = s["B"], s["N"], s["S"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    t = {n: torch.from_numpy(np.ascontiguousarray(s[n])).to(dev) for n in ("X", "U", "k", "K", "delta", "nom_pose", "nom_dim", "off", "pose", "dim")}
    z = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    risk, hits, total = z(B, 6 if materialised else 8), z(B, N, dt=torch.int32), z(B)
    tb = None if base is None else torch.from_numpy(np.ascontiguousarray(base)).to(dev)
    opt = dict(step_hits=hits.data_ptr(), total=total.data_ptr() if tb is not None else 0, base=tb.data_ptr() if tb is not None else 0, k_scale=0.0,
               max_risk=max_risk)
    head = [t[n].data_ptr() for n in ("X", "U", "k", "K", "delta")] + [0]
    if materialised:
        strides = cilqr.obstacle_strides(s["pose"].shape, s["dim"].shape, None, B, N)[1:]
        solver.rollout_risk_device(stream, B, N, s["M"], S, *head, t["pose"].data_ptr(), t["dim"].data_ptr(), strides, risk.data_ptr(), **opt)
    else:
        solver.rollout_risk_sampled_device(stream, B, N, s["n_obs"], s["ns"], S, *head, t["nom_pose"].data_ptr(), t["nom_dim"].data_ptr(),
                                           t["off"].data_ptr(), risk.data_ptr(), **opt)
    torch.cuda.synchronize(dev)
    out = [a.cpu().numpy() for a in (risk, hits, total)]
    if tb is None:
        out[2] = None
    return out


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) if x.dtype == np.float64 else np.array_equal(x, y) for x, y in zip(a, b))


def _check_against(got_risk, got_hits, want, what):
    risk, hits = want["risk"], want["step_hits"]
    print("%s: COLLISION %s, PAIR_SHARE %s, |WORST_C - oracle| max %.3g" % (what, got_risk[:, COLLISION].tolist(), got_risk[:, PAIR_SHARE].tolist(),
                                                                          np.max(np.abs(got_risk[:, WORST_C] - risk[:, WORST_C]))))
    assert got_hits.dtype == np.int32 and np.array_equal(got_hits, hits), (what, got_hits, hits)
    for f in EXACT:
        assert np.array_equal(got_risk[:, f], risk[:, f]), (what, FIELD_NAMES[f], got_risk[:, f], risk[:, f])
    assert np.max(np.abs(got_risk[:, WORST_C] - risk[:, WORST_C])) <= ABS_TOL, what


@gpu
@pytest.mark.parametrize("name", ["S", "T"])
def test_sampled_gains(cilqr, solver, cases, name):
    """Against oracle_backward_pass on the materialised obstacles, and bit for bit cilqr_gains_batch on them; host form = device form."""
    import torch
    s = cases[name]
    B, N = s["B"], s["N"]
    got = solver.gains_batch_sampled(N, s["X"], s["U"], s["poly"], s["fl"], s["nom_pose"], s["nom_dim"], s["off"], s["weight"], lamb=1.0)
    assert np.all(got["ok"] == 1)
    _close(got["k"], s["k"], "scene %s: k" % name)
    _close(got["K"], s["K"], "scene %s: K" % name)
    mat = solver.gains_batch(N, s["X"], s["U"], s["poly"], s["fl"], s["pose"], s["dim"], s["w"], lamb=1.0)
    assert _same((got["k"], got["K"], got["ok"]), (mat["k"], mat["K"], mat["ok"]))
    dev = torch.device("cuda", 0)
    t = {n: torch.from_numpy(np.ascontiguousarray(s[n])).to(dev) for n in ("X", "U", "poly", "fl", "nom_pose", "nom_dim", "off")}
    k, K, ok = (torch.zeros(shape, dtype=dt, device=dev) for shape, dt in (((B, 2 * N), torch.float64), ((B, 8 * N), torch.float64), ((B,), torch.int32)))
    solver.gains_batch_sampled_device(torch.cuda.current_stream(dev).cuda_stream, B, N, s["n_obs"], s["ns"], *(t[n].data_ptr() for n in t), s["weight"],
                                      k.data_ptr(), K.data_ptr(), ok.data_ptr(), lamb=1.0)
    torch.cuda.synchronize(dev)
    assert _same((got["k"], got["K"], got["ok"]), (k.cpu().numpy(), K.cpu().numpy(), ok.cpu().numpy()))
    # another regularisation reaches the kernel: the gains move, and still equal the materialised call's
    g2 = solver.gains_batch_sampled(N, s["X"], s["U"], s["poly"], s["fl"], s["nom_pose"], s["nom_dim"], s["off"], s["weight"], lamb=10.0)
    m2 = solver.gains_batch(N, s["X"], s["U"], s["poly"], s["fl"], s["pose"], s["dim"], s["w"], lamb=10.0)
    assert _same((g2["k"], g2["K"]), (m2["k"], m2["K"])) and not np.array_equal(g2["K"], got["K"])


@gpu
@pytest.mark.parametrize("name", ["S", "T", "V"])
def test_fields_against_the_oracle(cilqr, solver, cases, name):
    """Fed the oracle's gains: all eight fields and step_hits against numpy on the oracle's c; total with max_risk between two solves'
    shares; the host form and the device form give the same bits."""
    s = cases[name]
    share = np.sort(s["risk"][:, COLLISION])
    assert share[-1] - share[-2] > 1e-3
    max_risk = 0.5 * (share[-1] + share[-2])  # rejects exactly the solve with the largest share
    want_total = np.where(s["risk"][:, COLLISION] > max_risk, np.nan, s["base"])
    assert np.isnan(want_total).sum() == 1
    risk, hits, total = _host(solver, s, max_risk=max_risk, base=s["base"])
    _check_against(risk, hits, s, "scene %s, host form" % name)
    drisk, dhits, dtotal = _device(cilqr, solver, s, base=s["base"], max_risk=max_risk)
    _check_against(drisk, dhits, s, "scene %s, device form" % name)
    assert _same((risk, hits, total), (drisk, dhits, dtotal))
    assert np.array_equal(np.isnan(total), np.isnan(want_total))
    assert np.array_equal(_bits(total[~np.isnan(want_total)]), _bits(s["base"][~np.isnan(want_total)]))
    assert _pick(total) == _pick(want_total)
    none = _host(solver, s)  # no base: no total, the same fields
    assert none[2] is None and _same(none[:2], (risk, hits))


@gpu
@pytest.mark.parametrize("name", ["S", "V"])
def test_against_the_ordinary_call_on_the_materialised_obstacles(cilqr, solver, cases, name):
    """cilqr_rollout_risk_device on the M = n_obs*n_samples materialised obstacles (M*N = 192 and 180 entries fit that kernel's LDS):
    ANY_SHARE, WORST_ROW, WORST_ENTRY and FIRST_STEP equal its fields, WORST_C bit for bit."""
    s = cases[name]
    risk, _, _ = _device(cilqr, solver, s)
    mat, _, _ = _device(cilqr, solver, s, materialised=True)
    print("scene %s: WORST_C sampled %s\n        materialised %s" % (name, risk[:, WORST_C].tolist(), mat[:, RR_WORST_C].tolist()))
    assert np.array_equal(risk[:, ANY_SHARE], mat[:, RR_COLLISION])
    assert np.array_equal(risk[:, WORST_ROW], mat[:, RR_WORST_ROW])
    assert np.array_equal(risk[:, WORST_ENTRY], mat[:, RR_WORST_ENTRY])
    assert np.array_equal(risk[:, FIRST_STEP], mat[:, RR_FIRST_STEP])
    assert np.array_equal(_bits(risk[:, WORST_C]), _bits(mat[:, RR_WORST_C]))


@gpu
def test_a_result_depends_on_its_own_solve_alone(solver, cases):
    """A subset and the reversed batch of scene S, and scene V's solves alone (two workgroups and the finish kernel): the same bits."""
    s = cases["S"]
    risk, hits, total = _host(solver, s, max_risk=0.2, base=s["base"])
    sub = [4, 1]
    r1, h1, t1 = _host(solver, dict(s, **{n: np.ascontiguousarray(s[n][sub]) for n in ("X", "U", "k", "K", "nom_pose", "nom_dim", "off")}),
                       max_risk=0.2, base=s["base"][sub])
    assert _same((r1, h1, t1), (risk[sub], hits[sub], total[sub]))
    rev = slice(None, None, -1)
    r2, h2, t2 = _host(solver, dict(s, **{n: np.ascontiguousarray(s[n][rev]) for n in ("X", "U", "k", "K", "nom_pose", "nom_dim", "off")}),
                       max_risk=0.2, base=np.ascontiguousarray(s["base"][rev]))
    assert _same((r2, h2, t2), (risk[rev], hits[rev], total[rev]))
    r3, h3, _ = _host(solver, s, delta=np.ascontiguousarray(np.broadcast_to(s["delta"], (s["B"], s["S"], 4))))  # delta_batch_stride 1
    assert _same((r3, h3), (risk, hits))
    v = cases["V"]
    rv, hv, _ = _host(solver, v)
    for b in range(v["B"]):
        ra, ha, _ = _host(solver, v, sel=slice(b, b + 1))
        assert _same((ra[0], ha[0]), (rv[b], hv[b])), b


@gpu
def test_a_nan_offset_row_counts_every_sample_at_every_step(solver, cases):
    """One row of scene S with a NaN offset: h = n_samples for every obstacle at every step of that row, the other rows' contributions
    unchanged, the row never the worst; a base that is NaN gives a NaN total."""
    s = cases["S"]
    B, S, N, ns = s["B"], s["S"], s["N"], s["ns"]
    row = 7
    assert not np.any(s["risk"][:, WORST_ROW] == row)
    delta = s["delta"].copy()
    delta[row] = np.nan
    c = s["c"].copy()
    c[:, row] = -np.inf
    lost = np.zeros((B, S, N), dtype=bool)
    lost[:, row] = True
    want = _reduce(c, s["n_obs"], ns, lost)
    assert np.all(want["risk"][:, FIRST_STEP] == 0) and np.all(want["step_hits"] >= ns)
    assert np.array_equal(want["step_hits"] - ns, _reduce(c, s["n_obs"], ns)["step_hits"])  # (the other rows alone)
    base = s["base"].copy()
    base[2] = np.nan
    risk, hits, total = _host(solver, s, delta=delta, base=base)
    _check_against(risk, hits, want, "one NaN offset row")
    clean = _host(solver, s)
    assert np.array_equal(_bits(risk[:, WORST_C]), _bits(clean[0][:, WORST_C]))
    assert np.isnan(total[2]) and np.array_equal(_bits(np.delete(total, 2)), _bits(np.delete(base, 2)))


@gpu
def test_error_calls_leave_the_handle_usable(cilqr, solver, cases):
    """Limits beyond cilqr_create and the LDS bound are refused; the handle then computes scene T as before."""
    s = cases["T"]
    N = s["N"]
    z = lambda *shape: np.zeros(shape)  # noqa: E731
    with pytest.raises(cilqr.CilqrError, match="cilqr error %d: M=128" % ERR_ARG):  # 4 x 32 samples on a handle of 96 obstacles
        solver.rollout_risk_sampled(N, z(1, 4 * (N + 1)), z(1, 2 * N), z(1, 2 * N), z(1, 8 * N), z(5, 4), z(1, 4, 4 * N), np.ones((1, 4, 2 * N)), z(1, 4, 32, 3))
    with pytest.raises(cilqr.CilqrError, match="cilqr error %d: M=128" % ERR_ARG):
        solver.gains_batch_sampled(N, z(1, 4 * (N + 1)), z(1, 2 * N), z(1, 6), z(1, 2), z(1, 4, 4 * N), np.ones((1, 4, 2 * N)), z(1, 4, 32, 3), 1.0)
    with pytest.raises(cilqr.CilqrError, match="cilqr error %d: B=17" % ERR_ARG):
        solver.rollout_risk_sampled(N, z(17, 4 * (N + 1)), z(17, 2 * N), z(17, 2 * N), z(17, 8 * N), z(5, 4), z(17, 1, 4 * N), np.ones((17, 1, 2 * N)), z(17, 1, 2, 3))
    with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*delta_batch_stride 0 or 1" % ERR_ARG):
        cilqr._check(cilqr.lib().cilqr_rollout_risk_sampled(solver._h, 1, N, 1, 2, 1, _p(z(1, 4 * (N + 1))), _p(z(1, 2 * N)), _p(z(1, 2 * N)), _p(z(1, 8 * N)),
                                                            _p(z(2, 4)), C.c_int64(2), C.c_double(0.0), _p(z(1, 1, 4 * N)), _p(np.ones((1, 1, 2 * N))),
                                                            _p(z(1, 1, 2, 3)), C.c_double(1.0), None, _p(z(1, 8)), None, None))
    big = cilqr.Solver(cilqr.default_params(N_STEPS), max_batch=1, max_horizon=N_STEPS, max_obstacles=700, device=0)
    try:  # 8*(14*12 + 4) + 96*700 + 4*12*3 + 160 = 68 880 bytes of LDS
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*LDS" % ERR_UNSUPPORTED):
            big.rollout_risk_sampled(N, z(1, 4 * (N + 1)), z(1, 2 * N), z(1, 2 * N), z(1, 8 * N), z(5, 4), z(1, 2, 4 * N), np.ones((1, 2, 2 * N)), z(1, 2, 350, 3))
    finally:
        big.close()
    risk, hits, _ = _host(solver, s)
    _check_against(risk, hits, s, "scene T after the refused calls")


def _read_dump(path):
    v = open(path).read().split()
    B, N, n_obs, ns, S = (int(x) for x in v[:5])
    max_risk, best = float(v[5]), int(v[6])
    a = np.array([float(x) for x in v[7:]])
    take = lambda *shape, at=[0]: (a[at[0]:at[0] + int(np.prod(shape))].reshape(shape), at.__setitem__(0, at[0] + int(np.prod(shape))))[0]  # noqa: E731
    d = dict(B=B, N=N, n_obs=n_obs, ns=ns, S=S, max_risk=max_risk, best=best)
    for name, shape in (("x0", (B, 4)), ("U0", (B, 2 * N)), ("poly", (B, 6)), ("fl", (B, 2)), ("X", (B, 4 * (N + 1))), ("U", (B, 2 * N)),
                        ("nom_pose", (n_obs, 4 * N)), ("nom_dim", (n_obs, 2 * N)), ("off", (n_obs, ns, 3)), ("delta", (S, 4)), ("risk", (B, 8)),
                        ("hits", (B, N)), ("scores", (B, 8))):
        d[name] = np.ascontiguousarray(take(*shape))
    return d


@gpu
def test_cpp_facade_sampled_risk_checked_candidates(cilqr, tmp_path):
    """tests/cpp/candidates_risk_sampled.cpp: iLQR::run_candidates with set_obstacle_samples under set_pose_noise_check_fused against the
    C-ABI sequence called by hand and the unsampled façade (inside the program), and against the Python calls on the same inputs (here):
    the solve, last_scores, last_risk and last_step_hits bit for bit, and the pick."""
    exe, dump = str(tmp_path / "candidates_risk_sampled"), str(tmp_path / "dump.txt")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "candidates_risk_sampled.cpp"), "-L" + os.path.join(PKG, "lib"), "-lcilqr_hip",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([exe, dump], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sampled risk pick ok" in r.stdout, r.stdout
    d = _read_dump(dump)
    B, N, n_obs, ns = d["B"], d["N"], d["n_obs"], d["ns"]
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))  # noqa: E731  (one obstacle set for every candidate)
    pose, dim, off = rep(d["nom_pose"]), rep(d["nom_dim"]), rep(d["off"])
    p = cilqr.default_params(N)
    w = p.w_obstacle / ns
    sv = cilqr.Solver(p, max_batch=B, max_horizon=N, max_obstacles=n_obs * ns, device=0)
    try:
        sol = sv.solve_batch_sampled(N, d["x0"], d["U0"], d["poly"], d["fl"], pose, dim, off, w)
        assert _same((sol["X"], sol["U"]), (d["X"], d["U"]))
        g = sv.gains_batch_sampled(N, d["X"], d["U"], d["poly"], d["fl"], pose, dim, off, w, lamb=1.0)
        sc = sv.score_batch_sampled(N, d["X"], d["U"], d["poly"], d["fl"], pose, dim, off, w, max_collision=1.0)
        risk, hits, total = sv.rollout_risk_sampled(N, d["X"], d["U"], g["k"], g["K"], d["delta"], pose, dim, off, k_scale=0.0, max_risk=d["max_risk"],
                                                    base=sc["total"])
    finally:
        sv.close()
    print("shares %s, max_risk %g, pick %d" % (risk[:, COLLISION].tolist(), d["max_risk"], d["best"]))
    assert _same((risk, sc["score"]), (d["risk"], d["scores"])) and np.array_equal(hits, d["hits"].astype(np.int32))
    assert 0 < np.isnan(total).sum() < B  # the bound separates the candidates
    assert d["best"] == _pick(total) and d["best"] != _pick(sc["total"])  # and the check changes the pick

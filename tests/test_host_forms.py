"""Every host-buffer form of a batched call goes through one transport (csrc/cilqr_host_io.cpp): its arrays are copied into the
handle's device arena, its `_device` form runs on them, the results are copied back.  So a host form must return what its `_device`
form returns on the same inputs, bit for bit — on the packed path (arrays ≤ the pinned staging buffer: one copy each way), on the
direct path (one copy per array), with optional outputs given and null, and after a failed call on the same handle."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, M, B, S = 5, 2, 3, 3  # the handle is created with exactly these: every call runs at the arena's limit
MIB = 1 << 20  # the pinned staging buffer: min(arena, 1 MiB)
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def P(a):
    """A host array (or None) as the pointer the C-ABI takes."""
    return None if a is None else a.ctypes.data_as(_ip if a.dtype == np.int32 else _dp)


def obstacles(cilqr, pose, dim, weight, strides):
    return cilqr.Obstacles(pose.ctypes.data, dim.ctypes.data, None if weight is None else weight.ctypes.data, *strides)


class Dev:
    """Device copies of host arrays and device outputs, on the current stream of device 0."""

    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        self.keep = []

    def put(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.keep.append(t)
        return t.data_ptr()

    def out(self, *shape, dtype=np.float64):
        t = self.torch.zeros(shape, dtype=self.torch.int32 if dtype == np.int32 else self.torch.float64, device=self.dev)
        self.keep.append(t)
        return t

    def run(self, device_form, *args, **kw):
        """A `_device` form on the stream, waited for: the host form that follows runs on the handle's own stream, and a handle's
        workspaces serve one call at a time (include/cilqr.h)."""
        device_form(self.stream, *args, **kw)
        self.torch.cuda.synchronize(self.dev)

    def get(self, *tensors):
        self.torch.cuda.synchronize(self.dev)
        return [t.cpu().numpy() for t in tensors]


def same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def make_scene(cilqr, b, n, m, seed):
    """Paths, starts, warm starts and m static obstacles near the start (cilqr_amd.scenes), with weights."""
    from cilqr_amd import scenes
    sc = scenes.make_static(b, n, m, cilqr.default_params(n), seed)
    pose = sc["obs_pose"].copy()
    pose[:, :, 0::4] -= 8.0  # (the generator places obstacles 10 m and more ahead: a short horizon would never come near them)
    w = np.linspace(0.5, 1.5, b * m).reshape(b, m)
    return dict(x0=sc["x0"], U0=sc["U"], poly=sc["poly"], fl=sc["xplan_fl"], pose=pose, dim=sc["obs_dim"].copy(), w=w)


def device_chain(solver, s, b, n, m, rows):
    """The `_device` forms on the scene: solve -> X, U; gains at (X, U) -> k, K; `rows` rollouts of solve 0 -> X_roll, U_roll."""
    d = Dev()
    U, X, J, it, st = d.out(b, 2 * n), d.out(b, 4 * (n + 1)), d.out(b), d.out(b, dtype=np.int32), d.out(b, dtype=np.int32)
    U.copy_(d.torch.from_numpy(s["U0"]))
    poly, fl, pose, dim, w = d.put(s["poly"]), d.put(s["fl"]), d.put(s["pose"]), d.put(s["dim"]), d.put(s["w"])
    solver.solve_batch_device(d.stream, b, n, m, d.put(s["x0"]), U.data_ptr(), poly, fl, pose, dim, w, X.data_ptr(), J.data_ptr(), it.data_ptr(),
                              st.data_ptr())
    k, K, ok = d.out(b, 2 * n), d.out(b, 8 * n), d.out(b, dtype=np.int32)
    solver.gains_batch_device(d.stream, b, n, m, X.data_ptr(), U.data_ptr(), poly, fl, pose, dim, w, (m * n, n, 1, m), k.data_ptr(), K.data_ptr(),
                              ok.data_ptr())
    Xr, Ur = d.out(rows, 4 * (n + 1)), d.out(rows, 2 * n)
    solver.rollout_batch_device(d.stream, 1, n, rows, X.data_ptr(), U.data_ptr(), k.data_ptr(), K.data_ptr(), d.put(s["delta"][0]), 0, Xr.data_ptr(),
                                Ur.data_ptr(), k_scale=1.0)
    names = ("U", "X", "J", "iters", "status", "k", "K", "ok", "X_roll", "U_roll")
    return dict(zip(names, d.get(U, X, J, it, st, k, K, ok, Xr, Ur)))


@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(N), max_batch=B, max_horizon=N, max_obstacles=M)
    yield s
    s.close()


@pytest.fixture(scope="module")
def scene(cilqr, solver):
    s = make_scene(cilqr, B, N, M, 77)
    rng = np.random.Generator(np.random.PCG64(5))
    s["delta"] = rng.normal(0.0, 0.2, (B, S, 4))
    s["off"] = rng.normal(0.0, 0.2, (B, 1, 2, 3))  # sampled forms: the first obstacle as n_obs = 1 with n_samples = 2 pose samples
    s.update(device_chain(solver, s, B, N, M, S))
    return s


@pytest.mark.parametrize("opt", [True, False], ids=["optional-given", "optional-null"])
@pytest.mark.parametrize("form", ["solve_batch", "solve_batch_obstacles", "solve_batch_sampled"])
def test_solve_forms_equal_their_device_forms(cilqr, solver, scene, form, opt):
    s, L, h, d = scene, cilqr.lib(), solver._h, Dev()
    U, X, J, it, st = d.out(B, 2 * N), d.out(B, 4 * (N + 1)), d.out(B), d.out(B, dtype=np.int32), d.out(B, dtype=np.int32)
    U.copy_(d.torch.from_numpy(s["U0"]))
    hU, hX = s["U0"].copy(), np.zeros((B, 4 * (N + 1)))
    hJ, hit, hst = (np.zeros(B), np.zeros(B, np.int32), np.zeros(B, np.int32)) if opt else (None, None, None)
    dev_args = (d.put(s["x0"]), U.data_ptr(), d.put(s["poly"]), d.put(s["fl"]))
    dev_outs = (X.data_ptr(), J.data_ptr(), it.data_ptr(), st.data_ptr())
    host_args, host_outs = (P(s["x0"]), P(hU), P(s["poly"]), P(s["fl"])), (P(hX), P(hJ), P(hit), P(hst), C.c_uint32(0))
    if form == "solve_batch":
        d.run(solver.solve_batch_device, B, N, M, *dev_args, d.put(s["pose"]), d.put(s["dim"]), d.put(s["w"]), *dev_outs)
        cilqr._check(L.cilqr_solve_batch(h, B, N, M, *host_args, P(s["pose"]), P(s["dim"]), P(s["w"]), *host_outs))
    elif form == "solve_batch_obstacles":  # one static scene and one weight vector for the batch: M entries travel
        pose, dim, w = (np.ascontiguousarray(a) for a in (s["pose"][0, :, :4], s["dim"][0, :, :2], s["w"][0]))
        d.run(solver.solve_batch_obstacles_device, B, N, M, *dev_args, d.put(pose), d.put(dim), d.put(w), (0, 1, 0, 0), *dev_outs)
        o = obstacles(cilqr, pose, dim, w, (0, 1, 0, 0))
        cilqr._check(L.cilqr_solve_batch_obstacles(h, B, N, M, *host_args, C.byref(o), *host_outs))
    else:
        pose, dim = np.ascontiguousarray(s["pose"][:, :1]), np.ascontiguousarray(s["dim"][:, :1])
        d.run(solver.solve_batch_sampled_device, B, N, 1, 2, *dev_args, d.put(pose), d.put(dim), d.put(s["off"]), 0.5, *dev_outs)
        cilqr._check(L.cilqr_solve_batch_sampled(h, B, N, 1, 2, *host_args, P(pose), P(dim), P(s["off"]), C.c_double(0.5), *host_outs))
    wU, wX, wJ, wit, wst = d.get(U, X, J, it, st)
    assert np.all(np.isfinite(wX)) and not same(wU, s["U0"])  # (the solve did something)
    assert same(hU, wU) and same(hX, wX)
    if opt:
        assert same(hJ, wJ) and same(hit, wit) and same(hst, wst)


@pytest.mark.parametrize("opt", [True, False], ids=["optional-given", "optional-null"])
@pytest.mark.parametrize("form", ["score_batch", "score_batch_sampled"])
def test_score_forms_equal_their_device_forms(cilqr, solver, scene, form, opt):
    s, L, h, d = scene, cilqr.lib(), solver._h, Dev()
    score, total = d.out(B, cilqr.SCORE_FIELDS), d.out(B)
    hscore, htotal = np.zeros((B, cilqr.SCORE_FIELDS)), np.zeros(B) if opt else None
    dev_args = (d.put(s["X"]), d.put(s["U"]), d.put(s["poly"]), d.put(s["fl"]))
    host_args = (P(s["X"]), P(s["U"]), P(s["poly"]), P(s["fl"]))
    if form == "score_batch":
        d.run(solver.score_batch_device, B, N, M, *dev_args, d.put(s["pose"]), d.put(s["dim"]), d.put(s["w"]), (M * N, N, 1, M), score.data_ptr(),
              total.data_ptr(), max_collision=0.5)
        o = obstacles(cilqr, s["pose"], s["dim"], s["w"], (M * N, N, 1, M))
        cilqr._check(L.cilqr_score_batch(h, B, N, M, *host_args, C.byref(o), C.c_double(0.5), P(hscore), P(htotal)))
    else:
        pose, dim = np.ascontiguousarray(s["pose"][:, :1]), np.ascontiguousarray(s["dim"][:, :1])
        d.run(solver.score_batch_sampled_device, B, N, 1, 2, *dev_args, d.put(pose), d.put(dim), d.put(s["off"]), 0.5, score.data_ptr(),
              total.data_ptr(), max_collision=0.5)
        cilqr._check(L.cilqr_score_batch_sampled(h, B, N, 1, 2, *host_args, P(pose), P(dim), P(s["off"]), C.c_double(0.5), C.c_double(0.5), P(hscore),
                                                 P(htotal)))
    wscore, wtotal = d.get(score, total)
    assert np.any(wscore != 0.0) and same(hscore, wscore) and (not opt or same(htotal, wtotal))


def run_gains(cilqr, solver, s, b, n, m, opt):
    """cilqr_gains_batch and its _device form on (X, U) of s with dense weighted obstacles: ((k, K, ok) host, (k, K, ok) device)."""
    d = Dev()
    k, K, ok = d.out(b, 2 * n), d.out(b, 8 * n), d.out(b, dtype=np.int32)
    d.run(solver.gains_batch_device, b, n, m, d.put(s["X"]), d.put(s["U"]), d.put(s["poly"]), d.put(s["fl"]), d.put(s["pose"]), d.put(s["dim"]),
          d.put(s["w"]), (m * n, n, 1, m), k.data_ptr(), K.data_ptr(), ok.data_ptr(), lamb=2.0)
    hk, hK, hok = np.zeros((b, 2 * n)), np.zeros((b, 8 * n)), np.full(b, -1, np.int32) if opt else None
    o = obstacles(cilqr, s["pose"], s["dim"], s["w"], (m * n, n, 1, m))
    cilqr._check(cilqr.lib().cilqr_gains_batch(solver._h, b, n, m, P(s["X"]), P(s["U"]), P(s["poly"]), P(s["fl"]), C.byref(o), C.c_double(2.0), P(hk),
                                               P(hK), P(hok)))
    return (hk, hK, hok), d.get(k, K, ok)


def run_rollout_risk(cilqr, solver, s, b, n, m, opt, shared_delta):
    """cilqr_rollout_risk and its _device form: ((risk, step_hits, total) host, the same from the device form)."""
    d = Dev()
    delta = np.ascontiguousarray(s["delta"][0] if shared_delta else s["delta"])
    rows, stride = delta.shape[-2], 0 if shared_delta else 1
    base = np.ascontiguousarray(s["J"]) if opt else None
    risk, hits, total = d.out(b, cilqr.ROLLOUT_RISK_FIELDS), d.out(b, n, dtype=np.int32), d.out(b)
    d.run(solver.rollout_risk_device, b, n, m, rows, d.put(s["X"]), d.put(s["U"]), d.put(s["k"]), d.put(s["K"]), d.put(delta), stride,
          d.put(s["pose"]), d.put(s["dim"]), (m * n, n, 1, m), risk.data_ptr(), hits.data_ptr(), total.data_ptr() if opt else 0,
          d.put(base) if opt else 0, k_scale=1.0, max_risk=0.5)
    hrisk = np.zeros((b, cilqr.ROLLOUT_RISK_FIELDS))
    hhits, htotal = (np.full((b, n), -1, np.int32), np.zeros(b)) if opt else (None, None)
    o = obstacles(cilqr, s["pose"], s["dim"], s["w"], (m * n, n, 1, m))  # (weights given: they are not read and do not travel)
    cilqr._check(cilqr.lib().cilqr_rollout_risk(solver._h, b, n, m, rows, P(s["X"]), P(s["U"]), P(s["k"]), P(s["K"]), P(delta), C.c_int64(stride),
                                                C.c_double(1.0), C.byref(o), C.c_double(0.5), P(base), P(hrisk), P(hhits), P(htotal)))
    return (hrisk, hhits, htotal), d.get(risk, hits, total)


def all_same(got, want):
    return all(g is None or same(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("opt", [True, False], ids=["optional-given", "optional-null"])
def test_gains_form_equals_its_device_form(cilqr, solver, scene, opt):
    got, want = run_gains(cilqr, solver, scene, B, N, M, opt)
    assert np.any(want[1] != 0.0) and all_same(got, want) and same(want[0], scene["k"]) is False  # (lamb = 2 here, 1 in the chain)


@pytest.mark.parametrize("opt", [True, False], ids=["optional-given", "optional-null"])
def test_rollout_risk_form_equals_its_device_form(cilqr, solver, scene, opt):
    got, want = run_rollout_risk(cilqr, solver, scene, B, N, M, opt, shared_delta=not opt)
    assert np.all(want[0][:, cilqr.RR_WORST_ROW] >= 0) and all_same(got, want)


def test_rollout_form_equals_its_device_form(cilqr, solver, scene):
    """B = 1 with S = 3 rows: B*S = max_batch.  (Both outputs are required.)"""
    s = scene
    hX, hU = np.zeros((S, 4 * (N + 1))), np.zeros((S, 2 * N))
    delta = np.ascontiguousarray(s["delta"][0])
    cilqr._check(cilqr.lib().cilqr_rollout_batch(solver._h, 1, N, S, P(s["X"]), P(s["U"]), P(s["k"]), P(s["K"]), P(delta), C.c_int64(0), C.c_double(1.0),
                                                 P(hX), P(hU)))
    assert not same(s["X_roll"][1], s["X_roll"][0]) and same(hX, s["X_roll"]) and same(hU, s["U_roll"])


@pytest.mark.parametrize("opt", [True, False], ids=["optional-given", "optional-null"])
def test_score_rollouts_form_equals_its_device_form(cilqr, solver, scene, opt):
    s, d = scene, Dev()
    rows, risk, total = d.out(S, cilqr.SCORE_FIELDS), d.out(1, cilqr.RISK_FIELDS), d.out(1)
    d.run(solver.score_rollouts_device, 1, N, M, S, d.put(s["X_roll"]), d.put(s["U_roll"]), d.put(s["poly"]), d.put(s["fl"]), d.put(s["pose"]),
          d.put(s["dim"]), d.put(s["w"]), (M * N, N, 1, M), rows.data_ptr(), risk.data_ptr(), total.data_ptr(), max_risk=0.5)
    hrows, hrisk, htotal = np.zeros((S, cilqr.SCORE_FIELDS)), np.zeros((1, cilqr.RISK_FIELDS)), np.zeros(1) if opt else None
    o = obstacles(cilqr, s["pose"], s["dim"], s["w"], (M * N, N, 1, M))
    cilqr._check(cilqr.lib().cilqr_score_rollouts(solver._h, 1, N, M, S, P(s["X_roll"]), P(s["U_roll"]), P(s["poly"]), P(s["fl"]), C.byref(o),
                                                  C.c_double(0.5), P(hrows), P(hrisk), P(htotal)))
    assert np.any(d.get(rows)[0] != 0.0) and all_same((hrows, hrisk, htotal), d.get(rows, risk, total))


from test_host_plan import dump  # noqa: E402,F401  (the fixture that builds tests/cpp/host_plan_dump.cpp: the plans themselves, on the host)


@pytest.mark.parametrize("form", ["gains_batch", "rollout_risk"])
def test_direct_path_equals_the_device_form(cilqr, dump, form):  # noqa: F811
    """N = 50, M = 4 and the smallest B whose plan (csrc/cilqr_host_plan.h, through host_plan_dump) ends beyond the 1 MiB staging
    buffer of a handle of max_batch = B: every array is copied on its own, where the shapes above, a few KiB, travel packed."""
    n, m = 50, 4

    def shape(b, n, m):
        return dict(form=form, B=b, N=n, M=m, S=S, delta_sets=b, span=b * m * n, w_span=b * m if form == "gains_batch" else 0, weights=1, opt=1,
                    max_B=b, max_N=n, max_M=m)
    plans = dump([shape(b, n, m) for b in range(1, 129)])
    b = next(i + 1 for i, p in enumerate(plans) if p["end"] > min(p["cap"], MIB))
    assert 1 < b < 128 and plans[b - 2]["end"] <= MIB < plans[b - 1]["end"] <= plans[b - 1]["cap"]
    small = dump([shape(B, N, M)])[0]
    assert small["end"] <= min(small["cap"], MIB)  # (the packed cases of this file)
    s = make_scene(cilqr, b, n, m, 78)
    s["delta"] = np.random.Generator(np.random.PCG64(6)).normal(0.0, 0.2, (b, S, 4))
    big = cilqr.Solver(cilqr.default_params(n), max_batch=b, max_horizon=n, max_obstacles=m)
    try:
        s.update(device_chain(big, s, b, n, m, S))
        got, want = run_gains(cilqr, big, s, b, n, m, True) if form == "gains_batch" else run_rollout_risk(cilqr, big, s, b, n, m, True, False)
        assert np.any(want[0] != 0.0) and all_same(got, want)
    finally:
        big.close()


def test_a_forced_solve_enqueue_failure_is_followed_by_working_host_calls(cilqr, scene):
    """cilqr_debug_fail_enqueue(h, 1): the next host solve fails after its input copies were enqueued.  The shared failure path
    drains the stream and clears the in-flight mark, so a host score call and a host gains call on the same handle then succeed
    and equal their _device forms.  The hook counts solves only: with cilqr_debug_fail_enqueue(h, 2) a score and a gains call pass
    uncounted, the first solve after them succeeds and the second fails."""
    s, L = scene, cilqr.lib()
    solver = cilqr.Solver(cilqr.default_params(N), max_batch=B, max_horizon=N, max_obstacles=M)
    hU, hX = s["U0"].copy(), np.zeros((B, 4 * (N + 1)))

    def host_solve():
        hU[...] = s["U0"]
        return L.cilqr_solve_batch(solver._h, B, N, M, P(s["x0"]), P(hU), P(s["poly"]), P(s["fl"]), P(s["pose"]), P(s["dim"]), P(s["w"]), P(hX), None,
                                   None, None, C.c_uint32(0))

    def score_and_gains_equal_their_device_forms():
        d = Dev()
        score, total = d.out(B, cilqr.SCORE_FIELDS), d.out(B)
        d.run(solver.score_batch_device, B, N, M, d.put(s["X"]), d.put(s["U"]), d.put(s["poly"]), d.put(s["fl"]), d.put(s["pose"]), d.put(s["dim"]),
              d.put(s["w"]), (M * N, N, 1, M), score.data_ptr(), total.data_ptr())
        hscore, htotal = np.zeros((B, cilqr.SCORE_FIELDS)), np.zeros(B)
        o = obstacles(cilqr, s["pose"], s["dim"], s["w"], (M * N, N, 1, M))
        cilqr._check(L.cilqr_score_batch(solver._h, B, N, M, P(s["X"]), P(s["U"]), P(s["poly"]), P(s["fl"]), C.byref(o), C.c_double(1.0), P(hscore),
                                         P(htotal)))
        assert all_same((hscore, htotal), d.get(score, total))
        got, want = run_gains(cilqr, solver, s, B, N, M, True)
        assert all_same(got, want)

    try:
        cilqr._check(L.cilqr_debug_fail_enqueue(solver._h, 1))
        assert host_solve() != 0 and b"forced failure" in L.cilqr_last_error()
        score_and_gains_equal_their_device_forms()
        assert host_solve() == 0 and same(hU, s["U"]) and same(hX, s["X"])  # the hook is spent
        cilqr._check(L.cilqr_debug_fail_enqueue(solver._h, 2))
        score_and_gains_equal_their_device_forms()  # not solves: not counted
        assert host_solve() == 0 and same(hU, s["U"]) and same(hX, s["X"])
        assert host_solve() != 0 and b"forced failure" in L.cilqr_last_error()
        score_and_gains_equal_their_device_forms()
        assert host_solve() == 0 and same(hU, s["U"]) and same(hX, s["X"])
    finally:
        solver.close()

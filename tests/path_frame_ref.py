"""The path-aligned planning frame of include/cilqr.h restated in numpy: plain float64, the header's order of operations
(numpy rounds every elementwise product, sum and difference on its own, as the kernels do with contraction off), `math.sqrt`
and `math.atan2`.  Test infrastructure only; tests/test_path_frame.py and tests/test_path_frame_gpu.py compare against it.
"""
import functools
import math

import numpy as np

FRAME_DOUBLES = 5
DEGENERATE, NOT_MONOTONE = 1, 2
TO, FROM = 0, 1
GLOBAL_INFLATION = 1


def closest_and_slice(path, ego, W):
    """`first` (strict-< first minimum of the squared distance; a NaN compares false and leaves 0) and the slice length n."""
    path = np.asarray(path, dtype=np.float64).reshape(-1, 2)
    ex, ey = float(ego[0]), float(ego[1])
    dx, dy = ex - path[:, 0], ey - path[:, 1]
    d = dx * dx + dy * dy
    first, best = 0, d[0]
    for i in range(1, len(d)):
        if d[i] < best:
            first, best = i, d[i]
    return first, min(W, len(path) - first)


def make_frame(origin, end, n):
    """(ox, oy, c, s, phi), info from the slice's first and last waypoint."""
    ox, oy = float(origin[0]), float(origin[1])
    dx, dy = float(end[0]) - ox, float(end[1]) - oy
    q = np.float64(dx) * np.float64(dx) + np.float64(dy) * np.float64(dy)
    h = math.sqrt(q) if q >= 0.0 else float("nan")
    if n < 2 or h == 0.0 or not math.isfinite(h):
        return np.array([ox, oy, 1.0, 0.0, 0.0]), DEGENERATE
    c, s = dx / h, dy / h
    return np.array([ox, oy, c, s, math.atan2(s, c)]), 0


def point_to(f, x, y):
    """f: (..., 5) broadcast against x, y."""
    f = np.asarray(f, dtype=np.float64)
    ox, oy, c, s = f[..., 0], f[..., 1], f[..., 2], f[..., 3]
    ux, uy = x - ox, y - oy
    return (c * ux) + (s * uy), (c * uy) - (s * ux)


def point_from(f, xf, yf):
    f = np.asarray(f, dtype=np.float64)
    ox, oy, c, s = f[..., 0], f[..., 1], f[..., 2], f[..., 3]
    return ((c * xf) - (s * yf)) + ox, ((s * xf) + (c * yf)) + oy


def local_plan_frames(O, p, path, ego):
    """One candidate.  O: the oracle module, p: its parameters.  Returns dict(first, n, info, frame (5,), ego (4,), x (n,), y (n,)
    the framed slice, poly (6,), xplan_fl (2,), ref (n, 2))."""
    path = np.asarray(path, dtype=np.float64).reshape(-1, 2)
    ego = np.asarray(ego, dtype=np.float64)
    W, deg = p.num_of_local_wpts, p.poly_order
    first, n = closest_and_slice(path, ego, W)
    w = path[first:first + n]
    f, info = make_frame(w[0], w[-1], n)
    with np.errstate(invalid="ignore", over="ignore"):
        x, y = point_to(f, w[:, 0], w[:, 1])
        if n > 1 and not np.all(x[1:] > x[:-1]):
            info |= NOT_MONOTONE
        V = O.exact_powers(x, deg)
        c = O.polyfit_powers(V, y, deg)
        fy = np.zeros(n)
        for j in range(deg + 1):
            fy = fy + c[j] * V[:, j]
        ex, ey = point_to(f, ego[0], ego[1])
    poly = np.zeros(6)
    poly[:deg + 1] = c
    return dict(first=first, n=n, info=info, frame=f, ego=np.array([ex, ey, ego[2], ego[3] - f[4]]), x=x, y=y, poly=poly,
                xplan_fl=np.array([x[0], x[-1]]), ref=np.stack([x, fy], axis=1))


def _np_sincos(th):
    return np.sin(th), np.cos(th)


def frame_obstacles(frames, pose, dim, cov=None, t_safe=0.0, flags=0, sincos=_np_sincos):
    """frames (B, 5); pose (B, M, N, 4), dim (B, M, N, 2), cov None or (B, M, N, 3): the dense expansion of the inputs.
    sincos(theta) -> (sin, cos): numpy's by default; the GPU tests hand in the kernels' own (Solver.debug_math)."""
    f = np.asarray(frames, dtype=np.float64)[:, None, None, :]
    pose, dim = np.asarray(pose, dtype=np.float64), np.asarray(dim, dtype=np.float64)
    x, y = point_to(f, pose[..., 0], pose[..., 1])
    v, th = pose[..., 2], pose[..., 3]
    thf = th - f[..., 4]
    L, Wd = dim[..., 0], dim[..., 1]
    if flags & GLOBAL_INFLATION:
        sg, cg = sincos(th)
        sf, cf = sincos(thf)
        two = 2.0 * t_safe
        L = L + two * (np.abs(v * cg) - np.abs(v * cf))
        Wd = Wd + two * (np.abs(v * sg) - np.abs(v * sf))
    out = dict(pose=np.stack([x, y, v, thf], axis=-1), dim=np.stack([L, Wd], axis=-1), cov=None)
    if cov is not None:
        cov = np.asarray(cov, dtype=np.float64)
        c, s = f[..., 2], f[..., 3]
        xx, xy, yy = cov[..., 0], cov[..., 1], cov[..., 2]
        m00, m01 = (c * xx) + (s * xy), (c * xy) + (s * yy)
        m10, m11 = (c * xy) - (s * xx), (c * yy) - (s * xy)
        out["cov"] = np.stack([(m00 * c) + (m01 * s), (m01 * c) - (m00 * s), (m11 * c) - (m10 * s)], axis=-1)
    return out


def frame_states(frames, X, direction, S=1):
    """X (B*S, N+1, 4) -> the same shape."""
    X = np.asarray(X, dtype=np.float64)
    f = np.repeat(np.asarray(frames, dtype=np.float64), S, axis=0)[:, None, :]
    if direction == TO:
        x, y = point_to(f, X[..., 0], X[..., 1])
        th = X[..., 3] - f[..., 4]
    else:
        x, y = point_from(f, X[..., 0], X[..., 1])
        th = X[..., 3] + f[..., 4]
    return np.stack([x, y, X[..., 2], th], axis=-1)


def frame_poses(frames, poses):
    """poses (B, K, 3) -> (B, K, 3)."""
    poses = np.asarray(poses, dtype=np.float64)
    f = np.asarray(frames, dtype=np.float64)[:, None, :]
    x, y = point_to(f, poses[..., 0], poses[..., 1])
    return np.stack([x, y, poses[..., 2] - f[..., 4]], axis=-1)


def move_scene(a, t, path, ego, obs_pose=None):
    """The scene turned by `a` about the map origin, then moved by t: (path (P, 2), ego (4,), obs_pose (..., 4)) in the new place.
    Quarter turns are exact (their sines and cosines are set, not computed)."""
    exact = {0.0: (1.0, 0.0), math.pi / 2: (0.0, 1.0), math.pi: (-1.0, 0.0), -math.pi / 2: (0.0, -1.0)}
    c, s = exact.get(a, (math.cos(a), math.sin(a)))

    def pt(x, y):
        return c * x - s * y + t[0], s * x + c * y + t[1]

    path = np.asarray(path, dtype=np.float64)
    px, py = pt(path[:, 0], path[:, 1])
    ego = np.asarray(ego, dtype=np.float64)
    ex, ey = pt(ego[0], ego[1])
    out_obs = None
    if obs_pose is not None:
        obs_pose = np.asarray(obs_pose, dtype=np.float64)
        ox, oy = pt(obs_pose[..., 0], obs_pose[..., 1])
        out_obs = np.stack([ox, oy, obs_pose[..., 2], obs_pose[..., 3] + a], axis=-1)
    return np.stack([px, py], axis=1), np.array([ex, ey, ego[2], ego[3] + a]), out_obs


def framed_solve(O, p, N, path, ego, U, obs_pose=None, obs_dim=None, flags=0):
    """The framed pipeline on the CPU oracle: restated pre-step -> obstacle rows into the frame -> the oracle's solve -> X back
    to the map frame.  obs_pose (M, 4) / obs_dim (M, 2) static, or (M, N, 4) / (M, N, 2).  Returns the oracle's dict plus
    X_map (N+1, 4), plan (the restated pre-step)."""
    plan = local_plan_frames(O, p, path, ego)
    fp = fd = None
    if obs_pose is not None:
        obs_pose, obs_dim = np.asarray(obs_pose, dtype=np.float64), np.asarray(obs_dim, dtype=np.float64)
        M = obs_pose.shape[0]
        if obs_pose.ndim == 2:
            obs_pose = np.broadcast_to(obs_pose[:, None, :], (M, N, 4))
            obs_dim = np.broadcast_to(obs_dim[:, None, :], (M, N, 2))
        fo = frame_obstacles(plan["frame"][None], obs_pose[None], obs_dim[None], t_safe=p.t_safe, flags=flags)
        fp, fd = fo["pose"][0].reshape(M, 4 * N), fo["dim"][0].reshape(M, 2 * N)
    r = O.solve(p, N, plan["ego"], U, plan["poly"], plan["xplan_fl"][0], plan["xplan_fl"][1], fp, fd)
    r["X_map"] = frame_states(plan["frame"][None], r["X"].reshape(1, N + 1, 4), FROM)[0]
    r["plan"] = plan
    return r


def turned(path, a, t=(0.0, 0.0)):
    return move_scene(a, t, path, np.zeros(4))[0]


@functools.lru_cache(maxsize=None)
def prestep_cases():
    """The pre-step cases of tests/test_path_frame_gpu.py, which tools/path_frame_ab.py measures too.
    (label, paths (P, 2) shared or (B, P, 2), egos (B, 4)): B around the 32-lane workgroup, P of 1, 2 and 25, egos that put
    `first` at 0, mid-path and P - 3, a NaN ego, coincident waypoints, slices heading north and west, through a sine's crest, and
    around a hairpin (not monotone)."""
    rng = np.random.default_rng(3201)
    i = np.arange(25.0)
    wavy = np.stack([7.3 + 1.1 * i, 0.9 * np.sin(0.21 * i + 0.4)], axis=1)
    cases = []

    def egos_at(path, ks, B):
        k = np.resize(np.asarray(ks), B)
        return np.stack([path[k, 0] + rng.uniform(-0.3, 0.3, B), path[k, 1] + rng.uniform(-0.3, 0.3, B), rng.uniform(0, 8, B),
                         rng.uniform(-3, 3, B)], axis=1)

    for B in (1, 31, 32, 33):  # one path for the batch (path_stride 0), turned by an odd angle and moved
        path = turned(wavy, 0.3 + 0.4 * B, (130.5, -77.25))
        cases.append(("shared B=%d" % B, path, egos_at(path, (0, 12, 22, 5, 24), B)))
    north, west = turned(wavy, math.pi / 2, (3.0, 0.0)), turned(wavy, math.pi, (-40.0, 6.5))
    crest = np.stack([100.0 + 0.7 * i, 5.0 * np.sin(math.pi * i / 24.0)], axis=1)  # the slice from 2 runs over the crest at i = 12
    th = 1.7 * math.pi * np.arange(25) / 24.0
    hairpin = np.stack([20.0 + 6.0 * np.sin(th), 6.0 - 6.0 * np.cos(th)], axis=1)  # most of a circle: the framed abscissae turn back
    straight_n = np.stack([np.full(25, 3.0), 1.5 * i], axis=1)  # x = 3 everywhere
    per = np.stack([north, west, crest, hairpin, straight_n, turned(crest, 2.4, (1e5, 5e5))])
    cases.append(("per-candidate", per, np.stack([egos_at(p, (k,), 1)[0] for p, k in zip(per, (0, 12, 2, 3, 22, 2))])))
    nan_ego = egos_at(north, (7, 7, 7), 3)
    nan_ego[0, 0], nan_ego[1, 1], nan_ego[2, 3] = np.nan, np.nan, np.nan
    cases.append(("nan ego", north, nan_ego))
    two = np.array([[[4.0, 1.0], [4.0, 1.0]], [[4.0, 1.0], [3.5, 2.75]], [[-2.0, 0.0], [-2.0, -9.0]]])  # P = 2: coincident, oblique, south
    cases.append(("P=2", two, np.array([[4.1, 1.0, 2.0, 0.3], [3.4, 2.7, 2.0, 0.3], [-2.0, -0.1, 2.0, -1.5]])))
    cases.append(("P=1", np.array([[12.5, -3.25]]), np.array([[12.0, -3.0, 1.0, 0.2], [13.0, 0.0, 1.0, 2.9]])))
    return cases


def restated(O, paths, egos):
    """The restated pre-step of every candidate of a case (default parameters)."""
    p = O.default_params(30)
    shared = paths.ndim == 2
    return [local_plan_frames(O, p, paths if shared else paths[b], egos[b]) for b in range(egos.shape[0])]

#!/usr/bin/env python3
"""The analytic map-risk launch (cilqr_chance_risk_map_device) beside the map rollout-risk launch (cilqr_rollout_risk_map_device) and the
chance launch (cilqr_chance_risk_device) of the same batch, in one process, alternated round by round so that all see the same clocks and
neighbours:

  config-2 scenes   B = 1024, N = 50, M = 4 static obstacles, the node's 150 x 100 map at 0.2 m shared by the batch, probes 3 x 3
  planner's shape   B = 16 of the same scenes
  new launch        Q = 75 (the 5 x 5 x 3 Gauss-Hermite rule) and Q = 1024 (equal-weight standard-normal draws), on Sigma_t of the
                    chance launch from Sigma_0 = diag(0.16^2, 0.16^2, 0, 0.017^2)
  beside it         the map rollout risk at S = 64 and S = 1024 offsets shared by the batch, and the chance launch itself

Before anything is timed, r_t, u_t and e_t of the new launch are asserted equal to a numpy restatement of the header's definition on the
first --check solves (1e-9 on r_t and u_t, 1e-7 on e_t).  Times are device events; the launches are short, so a window holds --reps launches
back to back and is divided by their number.  Nothing is promised in advance: the file reports the medians.

    python tools/chance_map_ab.py [--rounds R] [--reps K] [--out profiles/r15_chance_map.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uncertainty-aware-cilqr-for-trajectory-optimization_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime first, tests/conftest.py)

import cilqr_amd  # noqa: E402
from cilqr_amd import scenes  # noqa: E402
from risk_map_ab import GEOM, POSE, SAFE, THRESHOLD, median, smooth_layer, spread  # noqa: E402

SIX = (0, 4, 5, 12, 13, 15)


def numpy_chance_map(g, layer, pose, probes, X, sigma, nodes, weights):
    """The header's definition: X (B, N+1, 4), sigma (B, N+1, 16) -> r_t, u_t, e_t (B, N)."""
    B, N = X.shape[0], X.shape[1] - 1
    nl, nw = probes
    a = np.array([-0.5 * SAFE[0] + k * (SAFE[0] / (nl - 1)) if nl > 1 else 0.0 for k in range(nl)])
    b = np.array([-0.5 * SAFE[1] + l * (SAFE[1] / (nw - 1)) if nw > 1 else 0.0 for l in range(nw)])
    a, b = np.repeat(a, nw), np.tile(b, nl)
    c00, c10, c11, c20, c21, c22 = (sigma[:, :N, i] for i in SIX)
    with np.errstate(invalid="ignore", divide="ignore"):
        l00 = np.sqrt(np.fmax(c00, 0.0))
        l10, l20 = np.where(l00 > 0, c10 / l00, 0.0), np.where(l00 > 0, c20 / l00, 0.0)
        l11 = np.sqrt(np.fmax(c11 - l10 * l10, 0.0))
        l21 = np.where(l11 > 0, (c21 - l20 * l10) / l11, 0.0)
        l22 = np.sqrt(np.fmax(c22 - l20 * l20 - l21 * l21, 0.0))
    zx, zy, zt = nodes[:, 0], nodes[:, 1], nodes[:, 2]
    x = (X[:, :N, 0:1] + l00[..., None] * zx)[..., None]                                  # (B, N, Q, 1)
    y = (X[:, :N, 1:2] + (l10[..., None] * zx + l11[..., None] * zy))[..., None]
    th = (X[:, :N, 3:4] + (l20[..., None] * zx + l21[..., None] * zy + l22[..., None] * zt))[..., None]
    ct, st = np.cos(th), np.sin(th)
    dx, dy = x + (a * ct - b * st) - pose[0], y + (a * st + b * ct) - pose[1]
    cp, sp = np.cos(pose[2]), np.sin(pose[2])
    x_first, y_first, inv = g.pos_x + (0.5 * g.len_x - 0.5 * g.res), g.pos_y + (0.5 * g.len_y - 0.5 * g.res), 1.0 / g.res
    fi, fj = (x_first - (cp * dx + sp * dy)) * inv, (y_first - (cp * dy - sp * dx)) * inv
    inside = (fi >= 0.0) & (fj >= 0.0) & (fi < g.rows - 1.0) & (fj < g.cols - 1.0)
    i0, j0 = np.where(inside, fi, 0.0).astype(np.int64), np.where(inside, fj, 0.0).astype(np.int64)
    ti, tj = fi - i0, fj - j0
    lay = layer.astype(np.float64)
    f00, f10, f01, f11 = lay[i0, j0], lay[i0 + 1, j0], lay[i0, j0 + 1], lay[i0 + 1, j0 + 1]
    ok = inside & np.isfinite(f00) & np.isfinite(f10) & np.isfinite(f01) & np.isfinite(f11)
    with np.errstate(invalid="ignore"):
        a0, a1 = f00 + ti * (f10 - f00), f01 + ti * (f11 - f01)
        occ = np.where(ok, a0 + tj * (a1 - a0), -np.inf)                                   # (B, N, Q, P)
    hit, unknown = (occ > THRESHOLD).any(axis=3), (~ok).any(axis=3)
    m = occ.max(axis=3)
    r = np.minimum(1.0, (weights * hit).sum(axis=2))
    u = np.minimum(1.0, (weights * unknown).sum(axis=2))
    e = (weights * np.where(ok.any(axis=3), m, 0.0)).sum(axis=2)
    return r, u, e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--check", type=int, default=32, help="solves whose per-step values numpy restates before timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, N, M = args.batch, 50, 4
    Bp = 16  # the planner's shape
    Bc = min(args.check, B)
    p = cilqr_amd.default_params(N)
    p.safe_length, p.safe_width = SAFE
    sc = scenes.make_c2(B, p)
    s = cilqr_amd.Solver(p, max_batch=4 * B, max_horizon=N, max_obstacles=M, device=0)  # (S = 1024 takes four partial records per solve)
    g = cilqr_amd.map_geom(*GEOM)
    layer = smooth_layer(g.rows, g.cols, 1)
    rules = {75: cilqr_amd.pose_quadrature(5, 5, 3)}
    draws = scenes.pose_offsets(1024, 1.0, 1.0, 1.0, seed=5)
    rules[1024] = (np.ascontiguousarray(draws[:, [0, 1, 3]]), np.full(1024, 1.0 / 1024))
    sigma0 = np.zeros(16)
    sigma0[0], sigma0[5], sigma0[15] = 0.16 ** 2, 0.16 ** 2, 0.017 ** 2
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    zeros = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device="cuda")  # noqa: E731
    t = dict(x0=dv(sc["x0"]), U0=dv(sc["U"]), poly=dv(sc["poly"]), fl=dv(sc["xplan_fl"]), pose=dv(sc["obs_pose"]), dim=dv(sc["obs_dim"]),
             d64=dv(scenes.pose_offsets(64, 0.16, 0.16, 0.017, seed=5)), d1024=dv(scenes.pose_offsets(1024, 0.16, 0.16, 0.017, seed=5)),
             layer=dv(np.asfortranarray(layer).flatten(order="F")), s0=dv(sigma0))
    for q, (nodes, weights) in rules.items():
        t["n%d" % q], t["w%d" % q] = dv(nodes), dv(weights)
    t["U"] = t["U0"].clone()
    t.update(X=zeros(B, 4 * (N + 1)), J=zeros(B), it=zeros(B, dtype=torch.int32), st=zeros(B, dtype=torch.int32),
             k=zeros(B, 2 * N), K=zeros(B, 8 * N), ok=zeros(B, dtype=torch.int32), sigma=zeros(B, N + 1, 16),
             crisk=zeros(B, cilqr_amd.CHANCE_FIELDS), ctotal=zeros(B),
             mrisk=zeros(B, cilqr_amd.MAP_RISK_FIELDS), mhits=zeros(B, N, dtype=torch.int32), munk=zeros(B, N, dtype=torch.int32), mtotal=zeros(B),
             qrisk=zeros(B, cilqr_amd.CHANCE_MAP_FIELDS), qr=zeros(B, N), qe=zeros(B, N), qu=zeros(B, N), qtotal=zeros(B))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    ptr = {k: v.data_ptr() for k, v in t.items()}
    strides = (M * N, N, 1, 0)
    s.set_uncertainty_map_device(ptr["layer"], g, POSE, (3, 3))

    def solve():
        s.solve_batch_device(stream, B, N, M, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, ptr["X"], ptr["J"],
                             ptr["it"], ptr["st"])

    def gains():
        s.gains_batch_device(stream, B, N, M, ptr["X"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, strides, ptr["k"],
                             ptr["K"], ptr["ok"], lamb=1.0)

    def chance(b=B):
        s.chance_risk_device(stream, b, N, M, ptr["X"], ptr["U"], ptr["K"], ptr["s0"], 0, 0, ptr["pose"], ptr["dim"], strides, ptr["crisk"],
                             sigma_out=ptr["sigma"], total=ptr["ctotal"], base=ptr["J"], max_risk=0.05)

    def rollout_map(b, n_s):
        s.rollout_risk_map_device(stream, b, N, n_s, ptr["X"], ptr["U"], ptr["k"], ptr["K"], ptr["d%d" % n_s], 0, THRESHOLD, ptr["mrisk"],
                                  ptr["mhits"], ptr["munk"], ptr["mtotal"], ptr["ctotal"], k_scale=0.0, max_risk=0.05)

    def chance_map(b, q, steps=True):
        s.chance_risk_map_device(stream, b, N, q, ptr["X"], ptr["sigma"], ptr["n%d" % q], ptr["w%d" % q], THRESHOLD, ptr["qrisk"],
                                 ptr["qr"] if steps else 0, ptr["qe"] if steps else 0, ptr["qu"] if steps else 0, ptr["qtotal"], ptr["ctotal"],
                                 max_risk=0.05)

    steps = []
    for b in (B, Bp):
        steps += [("chance launch, B=%d" % b, lambda b=b: chance(b)),
                  ("map rollout S=64, B=%d" % b, lambda b=b: rollout_map(b, 64)),
                  ("map rollout S=1024, B=%d" % b, lambda b=b: rollout_map(b, 1024)),
                  ("chance map Q=75, B=%d" % b, lambda b=b: chance_map(b, 75)),
                  ("chance map Q=1024, B=%d" % b, lambda b=b: chance_map(b, 1024))]
    steps.append(("chance map Q=75, B=%d, no per-step output" % Bp, lambda: chance_map(Bp, 75, False)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):  # warm-up of every launch
        t["U"].copy_(t["U0"])
        solve()
        gains()
        chance()
        for _, f in steps:
            f()
    torch.cuda.synchronize()
    # ---- agreement with the numpy restatement on the first Bc solves, before anything is timed
    X, sigma = t["X"].cpu().numpy().reshape(B, N + 1, 4), t["sigma"].cpu().numpy()
    figures = {}
    for q, (nodes, weights) in rules.items():
        chance_map(B, q)
        torch.cuda.synchronize()
        n = Bc if q <= 128 else max(1, Bc // 8)  # (numpy holds every probe of every node at once)
        r, u, e = numpy_chance_map(g, layer, POSE, (3, 3), X[:n], sigma[:n], nodes, weights)
        got = [t[name].cpu().numpy() for name in ("qr", "qu", "qe")]
        assert np.max(np.abs(got[0][:n] - r)) <= 1e-9 and np.max(np.abs(got[1][:n] - u)) <= 1e-9, "r_t or u_t differs from numpy's (Q = %d)" % q
        assert np.max(np.abs(got[2][:n] - e)) <= 1e-7, "e_t differs from numpy's (Q = %d)" % q
        risk = t["qrisk"].cpu().numpy()
        figures[q] = (risk[:, cilqr_amd.CM_STEP_RISK].copy(), int(np.isnan(t["qtotal"].cpu().numpy()).sum()))
    first = None
    times = {name: [] for name in ("solve",) + tuple(st[0] for st in steps)}
    same = True
    for _ in range(args.rounds):
        t["U"].copy_(t["U0"])
        torch.cuda.synchronize()
        e0.record()
        solve()
        e1.record()
        torch.cuda.synchronize()
        times["solve"].append(e0.elapsed_time(e1))
        gains()
        chance()
        for name, f in steps:
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.reps)
            if name == "chance map Q=75, B=%d" % B:
                if first is None:
                    first = t["qrisk"].clone()
                same = same and torch.equal(t["qrisk"].view(torch.int64), first.view(torch.int64))
    lines = ["analytic map-risk launch beside the map rollout-risk launch and the chance launch of the same batch: device events, %d alternated "
             "rounds, one process" % args.rounds,
             "config-2 scenes: N=%d, M=%d static obstacles (dense tables); map %d x %d cells of %.1f m shared by the batch, probes 3 x 3, "
             "threshold %g; Sigma_0 = diag(0.16^2, 0.16^2, 0, 0.017^2); Q=75: Gauss-Hermite 5 x 5 x 3, Q=1024: equal-weight draws"
             % (N, M, g.rows, g.cols, g.res, THRESHOLD),
             "r_t, u_t within 1e-9 and e_t within 1e-7 of a numpy restatement on the first %d solves at Q = 75 and the first %d at Q = 1024: asserted "
             "before timing" % (Bc, max(1, Bc // 8)),
             "   solve launch with the map set, B=%d, ms            %s" % (B, spread(times["solve"]))]
    for name, _ in steps:
        b = int(name.split("B=")[1].split(",")[0])
        ref = "map rollout S=64, B=%d" % b
        lines.append("   %-42s ms (%2d per window)   %s   = %.2f x the map rollout launch at S = 64 of that batch"
                     % (name + ",", args.reps, spread(times[name]), median(times[name]) / median(times[ref])))
    lines.append("   chance map rows bit-identical over the rounds: %s" % same)
    for q, (step, rej) in figures.items():
        lines.append("   Q=%d: solves with CM_STEP_RISK 0: %d, strictly between 0 and 1: %d, 1: %d; NaN totals at max_risk 0.05 (the chance call's "
                     "included): %d of %d" % (q, int((step == 0).sum()), int(((step > 0) & (step < 1)).sum()), int((step >= 1).sum()), rej, B))
    s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

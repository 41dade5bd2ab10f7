#!/usr/bin/env python3
"""The analytic pose-noise risk launch (cilqr_chance_risk_device) beside the gains launch (cilqr_gains_batch_device) and the fused
rollout-risk launch (cilqr_rollout_risk_device, S = 64 start offsets) of the same batch, in one process, alternated round by round so
that all see the same clocks and neighbours:

  config-2 scenes   B = 1024, N = 50, M = 4 static obstacles; Sigma_0 = diag(0.16^2, 0.16^2, 0, 0.017^2) shared by the batch, process
                    noise W = diag(1e-4, 1e-4, 4e-4, 1e-6); every optional output asked for, and none
  planner's shape   B = 16 of the same scenes

Times are device events; the launches are short, so a window holds --reps launches back to back and is divided by their number.
Nothing is promised in advance: the file reports the medians.

It then prints, for scenes R and L of tests/test_rollout_risk.py (restated here; trajectories and gains by the device's own solve and
gains calls), CR_STEP_RISK and CR_SUM_RISK beside RR_COLLISION and RR_STEP_SHARE of cilqr_rollout_risk at S = 70 (S = 64 for scene L: the
scenes' own offset sets) and at S = 4096 offsets of the same sigmas.  These figures are recorded, not asserted.

    python tools/chance_risk_ab.py [--rounds R] [--reps K] [--out profiles/r13_chance_risk.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uncertainty-aware-cilqr-for-trajectory-optimization_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime first, tests/conftest.py)

import cilqr_amd  # noqa: E402
from cilqr_amd import scenes  # noqa: E402

SIGMA0 = np.diag([0.16 ** 2, 0.16 ** 2, 0.0, 0.017 ** 2]).reshape(16)
W = np.diag([1e-4, 1e-4, 4e-4, 1e-6]).reshape(16)


def spread(ts):
    ts = sorted(ts)
    return "min %.4f  median %.4f  max %.4f" % (ts[0], ts[len(ts) // 2], ts[-1])


def median(ts):
    return sorted(ts)[len(ts) // 2]


def scene_r(p):
    """make_static(8, 12, 3, seed 7) with obstacle 0 of solve b 1.0 m ahead of the start and (3.4 + 0.1 b) m to its left (tests/test_rollout_risk.py)."""
    B, N, M = 8, 12, 3
    sc = scenes.make_static(B, N, M, p, 7)
    pose, dim = sc["obs_pose"].reshape(B, M, N, 4).copy(), sc["obs_dim"].reshape(B, M, N, 2)
    for b in range(B):
        x, y, _, th = sc["x0"][b]
        lat = 3.4 + 0.1 * b
        pose[b, 0, :, :] = [x + 1.0 * np.cos(th) - lat * np.sin(th), y + 1.0 * np.sin(th) + lat * np.cos(th), 0.0, th]
    return dict(B=B, N=N, M=M, S=70, seed=5, sc=sc, pose=pose.reshape(B, M, 4 * N), dim=np.ascontiguousarray(dim.reshape(B, M, 2 * N)))


def scene_l(p):
    B, N, M = 6, 50, 4
    sc = scenes.make_static(B, N, M, p, 11)
    return dict(B=B, N=N, M=M, S=64, seed=6, sc=sc, pose=np.ascontiguousarray(sc["obs_pose"]).reshape(B, M, 4 * N),
                dim=np.ascontiguousarray(sc["obs_dim"]).reshape(B, M, 2 * N))


def analytic_beside_rollouts(name, make):
    """Lines of the table for one scene: host forms on a solver of its own."""
    p = cilqr_amd.default_params()
    s = make(p)
    B, N, M = s["B"], s["N"], s["M"]
    p = cilqr_amd.default_params(N)
    sv = cilqr_amd.Solver(p, max_batch=512, max_horizon=N, max_obstacles=M, device=0)  # (holds B * 16 partial records and 4096 offsets)
    sc = s["sc"]
    r = sv.solve_batch(N, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], s["pose"], s["dim"])
    g = sv.gains_batch(N, r["X"], r["U"], sc["poly"], sc["xplan_fl"], s["pose"], s["dim"], lamb=1.0)
    c = sv.chance_risk(N, r["X"], r["U"], g["K"], SIGMA0, None, s["pose"], s["dim"], want_entry_p=False, want_sigma=False)["risk"]
    lines = ["scene %s (B %d, N %d, M %d), Sigma_0 = diag(0.16^2, 0.16^2, 0, 0.017^2), W = 0, gains at lamb = 1 (ok on %d of %d solves):"
             % (name, B, N, M, int(g["ok"].sum()), B),
             "   solve                      " + "".join("%10d" % b for b in range(B)),
             "   CR_STEP_RISK               " + "".join("%10.5f" % v for v in c[:, cilqr_amd.CR_STEP_RISK]),
             "   CR_SUM_RISK                " + "".join("%10.5f" % v for v in c[:, cilqr_amd.CR_SUM_RISK]),
             "   CR_MAX_POS_SIGMA, m        " + "".join("%10.5f" % v for v in c[:, cilqr_amd.CR_MAX_POS_SIGMA])]
    for S in (s["S"], 4096):
        delta = scenes.pose_offsets(S, 0.16, 0.16, 0.017, seed=s["seed"])
        rr, _, _ = sv.rollout_risk(N, r["X"], r["U"], g["k"], g["K"], delta, s["pose"], s["dim"], None, k_scale=0.0)
        lines.append("   RR_COLLISION,  S = %-6d   " % S + "".join("%10.5f" % v for v in rr[:, cilqr_amd.RR_COLLISION]))
        lines.append("   RR_STEP_SHARE, S = %-6d   " % S + "".join("%10.5f" % v for v in rr[:, cilqr_amd.RR_STEP_SHARE]))
    sv.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, S, N, M = args.batch, args.samples, 50, 4
    Bp = 16  # the planner's shape
    p = cilqr_amd.default_params(N)
    sc = scenes.make_c2(B, p)
    s = cilqr_amd.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M, device=0)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    zeros = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device="cuda")  # noqa: E731
    t = dict(x0=dv(sc["x0"]), U0=dv(sc["U"]), poly=dv(sc["poly"]), fl=dv(sc["xplan_fl"]), pose=dv(sc["obs_pose"]), dim=dv(sc["obs_dim"]),
             delta=dv(scenes.pose_offsets(S, 0.16, 0.16, 0.017, seed=5)), s0=dv(SIGMA0), W=dv(W))
    t["U"] = t["U0"].clone()
    t.update(X=zeros(B, 4 * (N + 1)), J=zeros(B), it=zeros(B, dtype=torch.int32), st=zeros(B, dtype=torch.int32),
             k=zeros(B, 2 * N), K=zeros(B, 8 * N), ok=zeros(B, dtype=torch.int32),
             frisk=zeros(B, cilqr_amd.ROLLOUT_RISK_FIELDS), fhits=zeros(B, N, dtype=torch.int32), ftotal=zeros(B),
             crisk=zeros(B, cilqr_amd.CHANCE_FIELDS), cstep=zeros(B, N), cep=zeros(B, M * N), csig=zeros(B, N + 1, 16), ctotal=zeros(B))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    ptr = {k: v.data_ptr() for k, v in t.items()}
    strides = (M * N, N, 1, 0)

    def solve():
        s.solve_batch_device(stream, B, N, M, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, ptr["X"], ptr["J"],
                             ptr["it"], ptr["st"])

    def gains(b=B):
        s.gains_batch_device(stream, b, N, M, ptr["X"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, strides, ptr["k"],
                             ptr["K"], ptr["ok"], lamb=1.0)

    def rollout_risk(b=B):
        s.rollout_risk_device(stream, b, N, M, S, ptr["X"], ptr["U"], ptr["k"], ptr["K"], ptr["delta"], 0, ptr["pose"], ptr["dim"], strides,
                              ptr["frisk"], ptr["fhits"], ptr["ftotal"], ptr["J"], k_scale=0.0, max_risk=0.05)

    def chance(b=B, full=True):
        s.chance_risk_device(stream, b, N, M, ptr["X"], ptr["U"], ptr["K"], ptr["s0"], 0, ptr["W"], ptr["pose"], ptr["dim"], strides,
                             ptr["crisk"], ptr["cstep"] if full else 0, ptr["cep"] if full else 0, ptr["csig"] if full else 0, ptr["ctotal"],
                             ptr["J"], max_risk=0.05)

    steps = [("gains", gains), ("rollout_risk, S=%d" % S, rollout_risk), ("chance_risk, every output", chance),
             ("chance_risk, risk + total", lambda: chance(B, False)),
             ("gains, B=%d" % Bp, lambda: gains(Bp)), ("rollout_risk, B=%d S=%d" % (Bp, S), lambda: rollout_risk(Bp)),
             ("chance_risk, B=%d, every output" % Bp, lambda: chance(Bp)), ("chance_risk, B=%d, risk + total" % Bp, lambda: chance(Bp, False))]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):  # warm-up of every launch: code objects loaded, the solve's schedule hint built
        t["U"].copy_(t["U0"])
        solve()
        for _, f in steps:
            f()
    torch.cuda.synchronize()
    chance()
    torch.cuda.synchronize()
    first = t["crisk"].clone()
    same = True
    times = {name: [] for name in ("solve",) + tuple(st[0] for st in steps)}
    for _ in range(args.rounds):
        t["U"].copy_(t["U0"])
        torch.cuda.synchronize()
        e0.record()
        solve()
        e1.record()
        torch.cuda.synchronize()
        times["solve"].append(e0.elapsed_time(e1))
        gains()
        for name, f in steps:
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.reps)
            if name == steps[2][0]:
                same = same and torch.equal(t["crisk"].view(torch.int64), first.view(torch.int64))
    gains()
    chance()
    rollout_risk()
    torch.cuda.synchronize()
    cr, rr, ok = t["crisk"].cpu().numpy(), t["frisk"].cpu().numpy(), t["ok"].cpu().numpy()
    lines = ["analytic pose-noise risk launch (cilqr_chance_risk_device) beside the gains launch and the fused rollout-risk launch of the same "
             "batch: device events, %d alternated rounds, one process" % args.rounds,
             "config-2 scenes: B=%d, N=%d, M=%d static obstacles (dense tables); rollout risk with S=%d start offsets shared by the batch "
             "(%d rows); chance risk with one shared Sigma_0 and process noise; solve on %d lanes per solve, %d wavefront(s)"
             % (B, N, M, S, B * S, s.solve_family(B, N, M), s.solve_wavefronts(B, N, M)),
             "   solve launch, ms                                          %s" % spread(times["solve"])]
    ms = median(times["solve"])
    for i, (name, _) in enumerate(steps):
        ref = median(times[steps[1 if i < 4 else 5][0]])
        lines.append("   %-34s ms (%2d per window)     %s   = %.3f of the solve launch, %.2f x the rollout risk launch of that batch"
                     % (name + ",", args.reps, spread(times[name]), median(times[name]) / ms, median(times[name]) / ref))
    lines.append("   chance risk rows bit-identical over the rounds: %s; gains ok on %d of %d solves" % (same, int(ok.sum()), B))
    lines.append("   B=%d: solves with CR_STEP_RISK <= 0.05: %d, with RR_COLLISION <= 0.05: %d, both: %d; rank correlation of CR_STEP_RISK "
                 "with RR_COLLISION over the batch: %.4f" % (
                     B, int((cr[:, 0] <= 0.05).sum()), int((rr[:, 0] <= 0.05).sum()), int(((cr[:, 0] <= 0.05) & (rr[:, 0] <= 0.05)).sum()),
                     float(np.corrcoef(np.argsort(np.argsort(cr[:, 0])), np.argsort(np.argsort(rr[:, 0])))[0, 1])))
    s.close()
    lines.append("")
    for name, make in (("R", scene_r), ("L", scene_l)):
        lines += analytic_beside_rollouts(name, make)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

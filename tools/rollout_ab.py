#!/usr/bin/env python3
"""The gains, rollout and rollout-score launches (cilqr_gains_batch_device, cilqr_rollout_batch_device, cilqr_score_rollouts_device)
beside the solve launch of the same batch, in one process, alternated round by round so that all see the same clocks and neighbours:

  config-2 scenes   B = 1024, N = 50, M = 4 static obstacles, S = 64 start offsets shared by the batch (65 536 rollout rows)

Times are device events.  A solve launch is timed alone (its warm start is restored outside the window); the other launches are
short, so a window holds --reps launches back to back and is divided by their number.  Nothing is promised in advance: the file
reports the medians and each launch as a fraction of the solve launch.

    python tools/rollout_ab.py [--rounds R] [--reps K] [--out profiles/r09_rollout.txt]
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


def spread(ts):
    ts = sorted(ts)
    return "min %.4f  median %.4f  max %.4f" % (ts[0], ts[len(ts) // 2], ts[-1])


def median(ts):
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, S, N, M = args.batch, args.samples, 50, 4
    p = cilqr_amd.default_params(N)
    sc = scenes.make_c2(B, p)
    delta = scenes.pose_offsets(S, 0.16, 0.16, 0.017, seed=5)
    s = cilqr_amd.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M, device=0)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    zeros = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device="cuda")  # noqa: E731
    t = dict(x0=dv(sc["x0"]), U0=dv(sc["U"]), poly=dv(sc["poly"]), fl=dv(sc["xplan_fl"]), pose=dv(sc["obs_pose"]), dim=dv(sc["obs_dim"]),
             delta=dv(delta))
    t["U"] = t["U0"].clone()
    t.update(X=zeros(B, 4 * (N + 1)), J=zeros(B), it=zeros(B, dtype=torch.int32), st=zeros(B, dtype=torch.int32),
             k=zeros(B, 2 * N), K=zeros(B, 8 * N), ok=zeros(B, dtype=torch.int32),
             Xr=zeros(B * S, 4 * (N + 1)), Ur=zeros(B * S, 2 * N), rows=zeros(B * S, cilqr_amd.SCORE_FIELDS),
             risk=zeros(B, cilqr_amd.RISK_FIELDS), total=zeros(B), pair=zeros(2))
    stream = torch.cuda.current_stream().cuda_stream
    ptr = {k: v.data_ptr() for k, v in t.items()}
    strides = (M * N, N, 1, 0)

    def solve():
        s.solve_batch_device(stream, B, N, M, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, ptr["X"], ptr["J"],
                             ptr["it"], ptr["st"])

    def gains():
        s.gains_batch_device(stream, B, N, M, ptr["X"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, strides, ptr["k"],
                             ptr["K"], ptr["ok"], lamb=1.0)

    def rollout():
        s.rollout_batch_device(stream, B, N, S, ptr["X"], ptr["U"], ptr["k"], ptr["K"], ptr["delta"], 0, ptr["Xr"], ptr["Ur"], k_scale=0.0)

    def score():
        s.score_rollouts_device(stream, B, N, M, S, ptr["Xr"], ptr["Ur"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, strides,
                                ptr["rows"], ptr["risk"], ptr["total"], max_risk=0.05)

    steps = (("gains", gains), ("rollout", rollout), ("score_rollouts", score))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):  # warm-up of every launch: code objects loaded, the solve's schedule hint built
        t["U"].copy_(t["U0"])
        solve()
        for _, f in steps:
            f()
    torch.cuda.synchronize()
    first = (t["risk"].clone(), t["Xr"].clone())
    times = {name: [] for name in ("solve",) + tuple(n for n, _ in steps)}
    same = True
    for _ in range(args.rounds):
        t["U"].copy_(t["U0"])
        torch.cuda.synchronize()
        e0.record()
        solve()
        e1.record()
        torch.cuda.synchronize()
        times["solve"].append(e0.elapsed_time(e1))
        for name, f in steps:
            e0.record()
            for _ in range(args.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.reps)
        same = same and torch.equal(t["risk"].view(torch.int64), first[0].view(torch.int64)) and \
            torch.equal(t["Xr"].view(torch.int64), first[1].view(torch.int64))
    s.argmin_device(stream, B, ptr["total"], ptr["pair"])
    torch.cuda.synchronize()
    risk, total, ok = t["risk"].cpu().numpy(), t["total"].cpu().numpy(), t["ok"].cpu().numpy()
    lines = ["gains, rollout and rollout-score launches beside the solve launch of the same batch: device events, %d alternated rounds, "
             "one process" % args.rounds,
             "config-2 scenes: B=%d, N=%d, M=%d static obstacles (dense tables), S=%d start offsets shared by the batch (%d rows); solve on "
             "%d lanes per solve, %d wavefront(s)" % (B, N, M, S, B * S, s.solve_family(B, N, M), s.solve_wavefronts(B, N, M)),
             "   solve launch, ms                          %s" % spread(times["solve"])]
    ms = median(times["solve"])
    together = 0.0
    for name, _ in steps:
        lines.append("   %-15s ms (%2d per window)        %s   = %.3f of the solve launch" % (name + ",", args.reps, spread(times[name]),
                                                                                            median(times[name]) / ms))
        together += median(times[name])
    lines.append("   the three together (medians)              %.4f ms = %.3f of the solve launch" % (together, together / ms))
    lines.append("   rollout rows and risk bit-identical over the rounds: %s; gains ok on %d of %d solves" % (same, int(ok.sum()), B))
    share = risk[:, cilqr_amd.RISK_COLLISION]
    lines.append("   solves with risk 0: %d, with 0 < risk < 1: %d, with risk 1: %d; rejected at max_risk 0.05: %d of %d; pick %d"
                 % (int((share == 0).sum()), int(((share > 0) & (share < 1)).sum()), int((share == 1).sum()), int(np.isnan(total).sum()), B,
                    int(t["pair"].cpu().numpy()[1])))
    s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The fused rollout-risk launch (cilqr_rollout_risk_device) beside the pair of launches it stands in for (cilqr_rollout_batch_device +
cilqr_score_rollouts_device) and the solve launch of the same batch, in one process, alternated round by round so that all see the same
clocks and neighbours:

  config-2 scenes   B = 1024, N = 50, M = 4 static obstacles, S = 64 start offsets shared by the batch (65 536 rollout rows): fused
                    against the pair
  planner's shape   B = 16 of the same scenes with S = 1024 and S = 4096: the fused launch alone (the pair would have to store up to
                    65 536 rows for 16 candidates)

Before anything is timed, the shares, worst rows and worst c of the fused launch are asserted equal to the pair's (worst c bit for bit).
Times are device events; the launches are short, so a window holds --reps launches back to back and is divided by their number.  Nothing
is promised in advance: the file reports the medians.

    python tools/risk_fused_ab.py [--rounds R] [--reps K] [--out profiles/r10_risk_fused.txt]
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
    Bp, Sp = 16, (1024, 4096)  # the planner's shape
    p = cilqr_amd.default_params(N)
    sc = scenes.make_c2(B, p)
    s = cilqr_amd.Solver(p, max_batch=max(B, Bp * (max(Sp) // 256)), max_horizon=N, max_obstacles=M, device=0)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    zeros = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device="cuda")  # noqa: E731
    t = dict(x0=dv(sc["x0"]), U0=dv(sc["U"]), poly=dv(sc["poly"]), fl=dv(sc["xplan_fl"]), pose=dv(sc["obs_pose"]), dim=dv(sc["obs_dim"]),
             delta=dv(scenes.pose_offsets(S, 0.16, 0.16, 0.017, seed=5)))
    for n in Sp:
        t["delta%d" % n] = dv(scenes.pose_offsets(n, 0.16, 0.16, 0.017, seed=5))
    t["U"] = t["U0"].clone()
    t.update(X=zeros(B, 4 * (N + 1)), J=zeros(B), it=zeros(B, dtype=torch.int32), st=zeros(B, dtype=torch.int32),
             k=zeros(B, 2 * N), K=zeros(B, 8 * N), ok=zeros(B, dtype=torch.int32),
             Xr=zeros(B * S, 4 * (N + 1)), Ur=zeros(B * S, 2 * N), rows=zeros(B * S, cilqr_amd.SCORE_FIELDS),
             risk=zeros(B, cilqr_amd.RISK_FIELDS), total=zeros(B),
             frisk=zeros(B, cilqr_amd.ROLLOUT_RISK_FIELDS), fhits=zeros(B, N, dtype=torch.int32), ftotal=zeros(B))
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

    def fused(b=B, n_s=S, delta="delta"):
        s.rollout_risk_device(stream, b, N, M, n_s, ptr["X"], ptr["U"], ptr["k"], ptr["K"], ptr[delta], 0, ptr["pose"], ptr["dim"], strides,
                              ptr["frisk"], ptr["fhits"], ptr["ftotal"], ptr["J"], k_scale=0.0, max_risk=0.05)

    steps = [("rollout", rollout), ("score_rollouts", score), ("fused rollout_risk", fused)]
    for n in Sp:
        steps.append(("fused, B=%d S=%d" % (Bp, n), lambda n=n: fused(Bp, n, "delta%d" % n)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):  # warm-up of every launch: code objects loaded, the solve's schedule hint built
        t["U"].copy_(t["U0"])
        solve()
        gains()
        for _, f in steps[:3]:
            f()
    torch.cuda.synchronize()
    # ---- agreement with the pair, before anything is timed
    risk, rows, frisk = t["risk"].cpu().numpy(), t["rows"].cpu().numpy().reshape(B, S, -1), t["frisk"].cpu().numpy()
    worst = risk[:, cilqr_amd.RISK_WORST_ROW].astype(int)
    assert np.array_equal(frisk[:, cilqr_amd.RR_COLLISION], risk[:, cilqr_amd.RISK_COLLISION]), "shares differ from the pair's"
    assert np.array_equal(frisk[:, cilqr_amd.RR_WORST_ROW], risk[:, cilqr_amd.RISK_WORST_ROW]), "worst rows differ from the pair's"
    assert np.array_equal(frisk[:, cilqr_amd.RR_WORST_C].view(np.int64), risk[:, cilqr_amd.RISK_WORST_C].view(np.int64)), "worst c differs"
    assert np.array_equal(frisk[:, cilqr_amd.RR_WORST_ENTRY], rows[np.arange(B), worst, cilqr_amd.SCORE_MAX_C_ENTRY]), "worst entries differ"
    assert np.array_equal(np.isnan(t["ftotal"].cpu().numpy()), np.isnan(t["total"].cpu().numpy())), "rejections differ"
    first = t["frisk"].clone()
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
        gains()
        for name, f in steps[:3]:
            e0.record()
            for _ in range(args.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.reps)
        same = same and torch.equal(t["frisk"].view(torch.int64), first.view(torch.int64))
        for name, f in steps[3:]:
            e0.record()
            for _ in range(args.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.reps)
    planner = {}
    for n in Sp:  # what the planner's shape reports (the last launch of each is not the last one run: run them once more)
        fused(Bp, n, "delta%d" % n)
        torch.cuda.synchronize()
        planner[n] = t["frisk"].cpu().numpy()[:Bp].copy()
    ok = t["ok"].cpu().numpy()
    lines = ["fused rollout-risk launch beside the rollout + rollout-score pair it stands in for and the solve launch of the same batch: "
             "device events, %d alternated rounds, one process" % args.rounds,
             "config-2 scenes: B=%d, N=%d, M=%d static obstacles (dense tables), S=%d start offsets shared by the batch (%d rows); solve on "
             "%d lanes per solve, %d wavefront(s)" % (B, N, M, S, B * S, s.solve_family(B, N, M), s.solve_wavefronts(B, N, M)),
             "shares, worst rows, worst entries and rejections equal to the pair's, worst c bit for bit: asserted before timing",
             "   solve launch, ms                                %s" % spread(times["solve"])]
    ms = median(times["solve"])
    for name, _ in steps:
        lines.append("   %-22s ms (%2d per window)       %s   = %.3f of the solve launch" % (name + ",", args.reps, spread(times[name]),
                                                                                          median(times[name]) / ms))
    pair = median(times["rollout"]) + median(times["score_rollouts"])
    lines.append("   the pair together (medians)                     %.4f ms = %.3f of the solve launch; fused / pair = %.3f"
                 % (pair, pair / ms, median(times["fused rollout_risk"]) / pair))
    lines.append("   fused risk rows bit-identical over the rounds: %s; gains ok on %d of %d solves" % (same, int(ok.sum()), B))
    share = frisk[:, cilqr_amd.RR_COLLISION]
    lines.append("   solves with risk 0: %d, with 0 < risk < 1: %d, with risk 1: %d; rejected at max_risk 0.05: %d of %d"
                 % (int((share == 0).sum()), int(((share > 0) & (share < 1)).sum()), int((share == 1).sum()),
                    int(np.isnan(t["ftotal"].cpu().numpy()).sum()), B))
    for n in Sp:
        sh = planner[n][:, cilqr_amd.RR_COLLISION]
        lines.append("   B=%d, S=%d: shares min %.5f max %.5f (steps of 1/%d), %d of %d above 0.05" % (Bp, n, sh.min(), sh.max(), n,
                                                                                                 int((sh > 0.05).sum()), Bp))
    s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

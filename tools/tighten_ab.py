#!/usr/bin/env python3
"""The chance-constraint tightening launch (cilqr_tighten_obstacles_device) beside the gains launch and the chance-risk launch of the
same batch, one full round of the loop beside the first solve, and the solve on obstacles inflated by their own position covariance
beside the sampled solve — in one process, alternated round by round so that all see the same clocks and neighbours:

  config-2 scenes   B = 1024, N = 50, M = 4 static obstacles; Sigma_0 = diag(0.16^2, 0.16^2, 0, 0.017^2) shared by the batch, no process
                    noise, kappa = cilqr_chance_kappa(0.05), max_inflate 2; the three launches, and
                    solve  |  round = gains + chance risk (sigma_out) + tighten (pose_out, dim_out) + re-solve from the first solve's U
  planner's shape   B = 16 of the same scenes
  config-3 scenes   B = --batch3, N = 50, 8 moving obstacles: cilqr_solve_batch_sampled_device on 8 x 32 pose samples (sigma 0.16 m,
                    0.16 m, 0.017 rad) beside cilqr_solve_batch_obstacles_device on the 8 nominal obstacles inflated ONCE by
                    obs_cov = diag(0.16^2, 0.16^2) and no ego covariance (the tighten launch is counted with that solve); each plan's
                    collision share against the samples (cilqr_score_batch_sampled) says what the cheaper form gives up.

Times are device events; the short launches are timed --reps back to back and divided by their number, solves and rounds one per window
(each from the cold warm start).  Nothing is promised in advance: the file reports the medians.

    python tools/tighten_ab.py [--rounds R] [--reps K] [--batch3 B] [--out profiles/r14_tighten.txt]
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
EPS, CAP = 0.05, 2.0


def spread(ts):
    ts = sorted(ts)
    return "min %.4f  median %.4f  max %.4f" % (ts[0], ts[len(ts) // 2], ts[-1])


def median(ts):
    return sorted(ts)[len(ts) // 2]


dv = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()  # noqa: E731
zeros = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device="cuda")  # noqa: E731


def timed(f, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def config2(args, kappa):
    B, N, M, Bp = args.batch, 50, 4, 16
    p = cilqr_amd.default_params(N)
    sc = scenes.make_c2(B, p)
    s = cilqr_amd.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M, device=0)
    t = dict(x0=dv(sc["x0"]), U0=dv(sc["U"]), poly=dv(sc["poly"]), fl=dv(sc["xplan_fl"]), pose=dv(sc["obs_pose"]), dim=dv(sc["obs_dim"]), s0=dv(SIGMA0))
    t["U"] = t["U0"].clone()
    t.update(X=zeros(B, 4 * (N + 1)), J=zeros(B), it=zeros(B, dtype=torch.int32), st=zeros(B, dtype=torch.int32),
             k=zeros(B, 2 * N), K=zeros(B, 8 * N), ok=zeros(B, dtype=torch.int32), crisk=zeros(B, cilqr_amd.CHANCE_FIELDS),
             csig=zeros(B, N + 1, 16), tpose=zeros(B, M, 4 * N), tdim=zeros(B, M, 2 * N), tg=zeros(B, cilqr_amd.TIGHTEN_FIELDS),
             it1=zeros(B, dtype=torch.int32))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    ptr = {k: v.data_ptr() for k, v in t.items()}
    strides = (M * N, N, 1, 0)

    def solve(b=B, pose="pose", dim="dim"):
        s.solve_batch_obstacles_device(stream, b, N, M, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr[pose], ptr[dim], 0, strides, ptr["X"],
                                       ptr["J"], ptr["it"], ptr["st"])

    def gains(b=B):
        s.gains_batch_device(stream, b, N, M, ptr["X"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, strides, ptr["k"],
                             ptr["K"], ptr["ok"], lamb=1.0)

    def chance(b=B):
        s.chance_risk_device(stream, b, N, M, ptr["X"], ptr["U"], ptr["K"], ptr["s0"], 0, 0, ptr["pose"], ptr["dim"], strides, ptr["crisk"],
                             sigma_out=ptr["csig"])

    def tighten(b=B, pose_out=True):
        s.tighten_obstacles_device(stream, b, N, M, ptr["X"], ptr["csig"], ptr["pose"], ptr["dim"], strides, ptr["tdim"], ptr["tg"],
                                   pose_out=ptr["tpose"] if pose_out else 0, kappa=kappa, max_inflate=CAP)

    def one_round(b=B):
        gains(b)
        chance(b)
        tighten(b)
        solve(b, "tpose", "tdim")

    launches = [("gains", gains), ("chance_risk, sigma_out", chance), ("tighten, pose_out + dim_out", tighten),
                ("tighten, dim_out alone", lambda: tighten(B, False)),
                ("gains, B=%d" % Bp, lambda: gains(Bp)), ("chance_risk, B=%d, sigma_out" % Bp, lambda: chance(Bp)),
                ("tighten, B=%d, pose_out + dim_out" % Bp, lambda: tighten(Bp))]
    for _ in range(3):  # warm-up of every launch: code objects loaded, the solve's schedule hint built
        for b in (B, Bp):
            t["U"].copy_(t["U0"])
            solve(b)
            one_round(b)
    torch.cuda.synchronize()
    names = ["solve", "round", "solve, B=%d" % Bp, "round, B=%d" % Bp] + [n for n, _ in launches]
    times = {n: [] for n in names}
    first_tg, same = None, True
    iters = {}
    for _ in range(args.rounds):
        for b, tag in ((B, ""), (Bp, ", B=%d" % Bp)):
            t["U"].copy_(t["U0"])
            times["solve" + tag].append(timed(lambda: solve(b)))
            t["it1"].copy_(t["it"])
            times["round" + tag].append(timed(lambda: one_round(b)))
            iters[b] = (t["it1"][:b].cpu().numpy().copy(), t["it"][:b].cpu().numpy().copy())
        # the short launches, on the plan of a fresh first solve
        t["U"].copy_(t["U0"])
        solve()
        gains()
        chance()
        for name, f in launches:
            times[name].append(timed(f, args.reps))
        tighten()
        torch.cuda.synchronize()
        if first_tg is None:
            first_tg = (t["tg"].clone(), t["tdim"].clone())
        same = same and torch.equal(t["tg"].view(torch.int64), first_tg[0].view(torch.int64)) and torch.equal(t["tdim"].view(torch.int64), first_tg[1].view(torch.int64))
    tg = t["tg"].cpu().numpy()
    lines = ["chance-constraint tightening (cilqr_tighten_obstacles_device) beside the gains and chance-risk launches and the solve of the same "
             "batch: device events, %d alternated rounds, one process" % args.rounds,
             "config-2 scenes: B=%d, N=%d, M=%d static obstacles (dense tables); one shared Sigma_0, no process noise, kappa %.6f (eps %.2f), "
             "max_inflate %.1f; solve on %d lanes per solve, %d wavefront(s)" % (B, N, M, kappa, EPS, CAP, s.solve_family(B, N, M), s.solve_wavefronts(B, N, M))]
    for b, tag in ((B, ""), (Bp, ", B=%d" % Bp)):
        ms, mr = median(times["solve" + tag]), median(times["round" + tag])
        lines.append("   %-38s ms (1 per window)      %s" % ("first solve" + tag + ",", spread(times["solve" + tag])))
        lines.append("   %-38s ms (1 per window)      %s   = %.3f of the first solve; iterations: first solve mean %.2f max %d, re-solve mean %.2f max %d"
                     % ("round" + tag + ",", spread(times["round" + tag]), mr / ms, iters[b][0].mean(), iters[b][0].max(), iters[b][1].mean(), iters[b][1].max()))
    for i, (name, _) in enumerate(launches):
        ms = median(times["solve" if i < 4 else "solve, B=%d" % Bp])
        lines.append("   %-38s ms (%2d per window)     %s   = %.4f of the first solve of that batch" % (name + ",", args.reps, spread(times[name]), median(times[name]) / ms))
    lines.append("   tighten rows and dim_out bit-identical over the rounds: %s; B=%d: MAX_DA %.4f .. %.4f, MAX_DB %.4f .. %.4f, capped entries %d"
                 % (same, B, tg[:, 0].min(), tg[:, 0].max(), tg[:, 1].min(), tg[:, 1].max(), int(tg[:, 3].sum())))
    s.close()
    return lines


def config3(args, kappa):
    B, N, n_obs, n_samples = args.batch3, 50, 8, 32
    p = cilqr_amd.default_params(N)
    sc = scenes.make_c3(B, p, n_dyn=n_obs, n_samples=n_samples)
    s = cilqr_amd.Solver(p, max_batch=B, max_horizon=N, max_obstacles=n_obs * n_samples, device=0)
    cov = np.zeros((B, n_obs, N, 3))
    cov[..., 0], cov[..., 2] = 0.16 ** 2, 0.16 ** 2
    t = dict(x0=dv(sc["x0"]), U0=dv(sc["U"]), poly=dv(sc["poly"]), fl=dv(sc["xplan_fl"]), pose=dv(sc["nom_pose"]), dim=dv(sc["nom_dim"]),
             off=dv(sc["offsets"]), cov=dv(cov))
    t["U"] = t["U0"].clone()
    t.update(X=zeros(B, 4 * (N + 1)), J=zeros(B), it=zeros(B, dtype=torch.int32), st=zeros(B, dtype=torch.int32),
             sig=zeros(B, N + 1, 16), tdim=zeros(B, n_obs, 2 * N), tg=zeros(B, cilqr_amd.TIGHTEN_FIELDS))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    ptr = {k: v.data_ptr() for k, v in t.items()}
    strides = (n_obs * N, N, 1, 0)
    w = float(sc["sample_weight"])

    def sampled():
        s.solve_batch_sampled_device(stream, B, N, n_obs, n_samples, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], ptr["off"], w,
                                     ptr["X"], ptr["J"], ptr["it"], ptr["st"])

    def inflated():  # (Sigma = 0: the ego's heading plays no part in the inflation, any finite X serves)
        s.tighten_obstacles_device(stream, B, N, n_obs, ptr["X"], ptr["sig"], ptr["pose"], ptr["dim"], strides, ptr["tdim"], ptr["tg"],
                                   obs_cov=ptr["cov"], kappa=kappa, max_inflate=CAP)
        s.solve_batch_obstacles_device(stream, B, N, n_obs, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["tdim"], 0, strides, ptr["X"],
                                       ptr["J"], ptr["it"], ptr["st"])

    def nominal():
        s.solve_batch_obstacles_device(stream, B, N, n_obs, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, strides, ptr["X"],
                                       ptr["J"], ptr["it"], ptr["st"])

    forms = [("sampled solve, 8 x 32", sampled), ("tighten + solve on 8 inflated", inflated), ("solve on the 8 nominal", nominal)]
    for _ in range(3):
        for _, f in forms:
            t["U"].copy_(t["U0"])
            f()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in forms}
    plans = {}
    for _ in range(args.rounds):
        for name, f in forms:
            t["U"].copy_(t["U0"])
            times[name].append(timed(f))
            plans[name] = (t["X"].cpu().numpy().copy(), t["U"].cpu().numpy().copy(), t["it"].cpu().numpy().copy())
    lines = ["config-3 scenes: B=%d, N=%d, %d moving obstacles x %d pose samples (sigma 0.16 m, 0.16 m, 0.017 rad); the inflated form: obs_cov = "
             "diag(0.16^2, 0.16^2), Sigma = 0, kappa %.6f; collision share = SCORE_COLLISION of cilqr_score_batch_sampled against the samples"
             % (B, N, n_obs, n_samples, kappa)]
    ms = median(times[forms[0][0]])
    for name, _ in forms:
        X, U, it = plans[name]
        sb = min(B, 256)  # (the score rows of the first solves say enough, and fit every arena)
        score = s.score_batch_sampled(N, X[:sb], U[:sb], sc["poly"][:sb], sc["xplan_fl"][:sb], sc["nom_pose"][:sb], sc["nom_dim"][:sb], sc["offsets"][:sb], w)["score"]
        col = score[:, cilqr_amd.SCORE_COLLISION]
        lines.append("   %-32s ms (1 per window)   %s   = %.3f of the sampled solve; iterations mean %.2f max %d; first %d solves: collision share mean "
                     "%.4f, max %.4f, solves with any contact %d; max c mean %.4f"
                     % (name + ",", spread(times[name]), median(times[name]) / ms, it.mean(), it.max(), sb, col.mean(), col.max(), int((col > 0).sum()),
                        score[:, cilqr_amd.SCORE_MAX_C].mean()))
    s.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--batch3", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    kappa = cilqr_amd.chance_kappa(EPS)
    lines = config2(args, kappa) + [""] + config3(args, kappa)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

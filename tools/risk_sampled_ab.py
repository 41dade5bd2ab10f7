#!/usr/bin/env python3
"""The two calls that take sampled obstacles in compact form beyond the solve and the score, on config-3 scenes (make_c3: 8 moving
obstacles x 32 pose samples, N = 50), in one process, alternated round by round so that all see the same clocks and neighbours:

  1. cilqr_gains_batch_sampled_device beside cilqr_gains_batch_device on the materialised obstacles (M = 256, weights 1/32) of the same
     batch: the same arithmetic on 1/24 of the obstacle bytes;
  2. cilqr_rollout_risk_sampled_device beside the sampled solve launch of the same batch and, at B = 16, S = 64 where its rows fit,
     beside the only path there was before it: cilqr_rollout_batch_device + cilqr_score_rollouts_device on the materialised obstacles.

Shapes: B = 16 with S = 64 and S = 1024 ego offsets (the planner's), B = 1024 with S = 64.  Before anything is timed the sampled gains
are asserted bit-equal to the materialised call's and, at B = 16, S = 64, the sampled risk's ANY_SHARE, WORST_ROW and WORST_C (bit for
bit) equal to the stored-rows pair's.  Times are device events; the short launches are timed in windows of --reps launches.  Nothing is
promised in advance: the file reports the medians.

    python tools/risk_sampled_ab.py [--rounds R] [--reps K] [--out profiles/r11_risk_sampled.txt]
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
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    Bw, Bp, N, n_obs, ns = args.batch, 16, 50, 8, 32  # the wide batch and the planner's
    M = n_obs * ns
    shapes = [(Bp, 64), (Bp, 1024), (Bw, 64)]
    p = cilqr_amd.default_params(N)
    sc = scenes.make_c3(Bw, p, n_dyn=n_obs, n_samples=ns)
    w = sc["sample_weight"]
    s = cilqr_amd.Solver(p, max_batch=Bw, max_horizon=N, max_obstacles=M, device=0)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    zeros = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device="cuda")  # noqa: E731
    t = dict(x0=dv(sc["x0"]), U0=dv(sc["U"]), poly=dv(sc["poly"]), fl=dv(sc["xplan_fl"]), npose=dv(sc["nom_pose"]), ndim=dv(sc["nom_dim"]),
             off=dv(sc["offsets"]), pose=dv(sc["obs_pose"]), dim=dv(sc["obs_dim"]), wts=dv(sc["obs_weight"]))
    for S in (64, 1024):
        t["delta%d" % S] = dv(scenes.pose_offsets(S, 0.16, 0.16, 0.017, seed=5))
    t["U"] = t["U0"].clone()
    R = Bp * 64  # rows of the stored-rows pair
    t.update(X=zeros(Bw, 4 * (N + 1)), J=zeros(Bw), it=zeros(Bw, dtype=torch.int32), st=zeros(Bw, dtype=torch.int32),
             k=zeros(Bw, 2 * N), K=zeros(Bw, 8 * N), ok=zeros(Bw, dtype=torch.int32), km=zeros(Bw, 2 * N), Km=zeros(Bw, 8 * N),
             okm=zeros(Bw, dtype=torch.int32), score=zeros(Bw, cilqr_amd.SCORE_FIELDS), base=zeros(Bw),
             risk=zeros(Bw, cilqr_amd.RRS_FIELDS), hits=zeros(Bw, N, dtype=torch.int32), total=zeros(Bw),
             Xr=zeros(R, 4 * (N + 1)), Ur=zeros(R, 2 * N), rows=zeros(R, cilqr_amd.SCORE_FIELDS), risk3=zeros(Bp, cilqr_amd.RISK_FIELDS),
             total3=zeros(Bp))
    stream = torch.cuda.current_stream().cuda_stream
    ptr = {k: v.data_ptr() for k, v in t.items()}
    strides = (M * N, N, 1, M)

    def solve(B):
        s.solve_batch_sampled_device(stream, B, N, n_obs, ns, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr["npose"], ptr["ndim"], ptr["off"],
                                     w, ptr["X"], ptr["J"], ptr["it"], ptr["st"])

    def gains(B):
        s.gains_batch_sampled_device(stream, B, N, n_obs, ns, ptr["X"], ptr["U"], ptr["poly"], ptr["fl"], ptr["npose"], ptr["ndim"], ptr["off"],
                                     w, ptr["k"], ptr["K"], ptr["ok"], lamb=1.0)

    def gains_mat(B):
        s.gains_batch_device(stream, B, N, M, ptr["X"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], ptr["wts"], strides, ptr["km"],
                             ptr["Km"], ptr["okm"], lamb=1.0)

    def score(B):
        s.score_batch_sampled_device(stream, B, N, n_obs, ns, ptr["X"], ptr["U"], ptr["poly"], ptr["fl"], ptr["npose"], ptr["ndim"], ptr["off"],
                                     w, ptr["score"], ptr["base"], max_collision=1.0)

    def risk(B, S):
        s.rollout_risk_sampled_device(stream, B, N, n_obs, ns, S, ptr["X"], ptr["U"], ptr["k"], ptr["K"], ptr["delta%d" % S], 0, ptr["npose"],
                                      ptr["ndim"], ptr["off"], ptr["risk"], ptr["hits"], ptr["total"], ptr["base"], k_scale=0.0, max_risk=0.25)

    def pair():  # B = 16, S = 64 on the materialised obstacles
        s.rollout_batch_device(stream, Bp, N, 64, ptr["X"], ptr["U"], ptr["k"], ptr["K"], ptr["delta64"], 0, ptr["Xr"], ptr["Ur"], k_scale=0.0)
        s.score_rollouts_device(stream, Bp, N, M, 64, ptr["Xr"], ptr["Ur"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], ptr["wts"], strides,
                                ptr["rows"], ptr["risk3"], ptr["total3"], max_risk=0.25)

    def prepare(B):  # the solved batch, its gains and nominal totals
        t["U"].copy_(t["U0"])
        solve(B)
        gains(B)
        score(B)

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(f, reps):
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    lines = ["gains and fused rollout risk for sampled obstacles in compact form, config-3 scenes (n_obs %d x n_samples %d, N = %d; materialised "
             "M = %d): device events, %d alternated rounds, one process" % (n_obs, ns, N, M, args.rounds)]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for B in (Bp, Bw):
        for _ in range(2):  # warm-up: code objects loaded, the solve's schedule hint built
            prepare(B)
            gains_mat(B)
            for b, S in shapes:
                if b == B:
                    risk(B, S)
        torch.cuda.synchronize()
        # ---- agreement, before anything is timed
        assert torch.equal(t["k"][:B].view(torch.int64), t["km"][:B].view(torch.int64)), "sampled gains k differ from the materialised call's"
        assert torch.equal(t["K"][:B].view(torch.int64), t["Km"][:B].view(torch.int64)), "sampled gains K differ from the materialised call's"
        assert torch.equal(t["ok"][:B], t["okm"][:B])
        if B == Bp:
            risk(Bp, 64)
            pair()
            torch.cuda.synchronize()
            r, r3 = t["risk"][:Bp].cpu().numpy(), t["risk3"].cpu().numpy()
            assert np.array_equal(r[:, cilqr_amd.RRS_ANY_SHARE], r3[:, cilqr_amd.RISK_COLLISION]), "ANY_SHARE differs from the stored-rows pair's share"
            assert np.array_equal(r[:, cilqr_amd.RRS_WORST_ROW], r3[:, cilqr_amd.RISK_WORST_ROW]), "worst rows differ from the stored-rows pair's"
            assert np.array_equal(r[:, cilqr_amd.RRS_WORST_C].view(np.int64), r3[:, cilqr_amd.RISK_WORST_C].view(np.int64)), "worst c differs"
        mine = [S for b, S in shapes if b == B]
        names = ["solve", "gains sampled", "gains materialised"] + ["risk S=%d" % S for S in mine] + (["stored-rows pair S=64"] if B == Bp else [])
        times = {n: [] for n in names}
        for _ in range(args.rounds):
            t["U"].copy_(t["U0"])
            torch.cuda.synchronize()
            times["solve"].append(window(lambda: solve(B), 1))
            gains(B)
            score(B)
            times["gains sampled"].append(window(lambda: gains(B), args.reps))
            times["gains materialised"].append(window(lambda: gains_mat(B), args.reps))
            for S in mine:
                times["risk S=%d" % S].append(window(lambda S=S: risk(B, S), args.reps))
            if B == Bp:
                times["stored-rows pair S=64"].append(window(pair, args.reps))
        ms = median(times["solve"])
        lines.append("B = %d (sampled solve on %d wavefront(s) per solve); gains ok on %d of %d solves" % (B, s.solve_sampled_wavefronts(B, N, n_obs),
                                                                                                   int(t["ok"][:B].sum().item()), B))
        for n in names:
            reps = 1 if n == "solve" else args.reps
            lines.append("   %-24s ms (%d per window)   %s   = %.3f of the solve launch" % (n + ",", reps, spread(times[n]), median(times[n]) / ms))
        lines.append("   gains sampled / materialised = %.3f (medians); input bytes per solve: %d against %d"
                     % (median(times["gains sampled"]) / median(times["gains materialised"]), 8 * (6 * n_obs * N + 3 * n_obs * ns),
                        8 * (6 * M * N + M)))
        for S in mine:
            G = (S + 255) // 256
            risk(B, S)
            torch.cuda.synchronize()
            r = t["risk"][:B].cpu().numpy()
            lines.append("   risk S=%d: %d workgroups of %d lanes on %d CUs; COLLISION min %.4f max %.4f, ANY_SHARE max %.4f, PAIR_SHARE max %.4f, "
                         "rejected at max_risk 0.25: %d of %d" % (S, B * G, 64 * min(4, (S + 63) // 64), cus, r[:, cilqr_amd.RRS_COLLISION].min(),
                                                                  r[:, cilqr_amd.RRS_COLLISION].max(), r[:, cilqr_amd.RRS_ANY_SHARE].max(),
                                                                  r[:, cilqr_amd.RRS_PAIR_SHARE].max(), int(np.isnan(t["total"][:B].cpu().numpy()).sum()), B))
        if B == Bp:
            lines.append("   risk S=64 / stored-rows pair = %.3f (medians); the pair stores %d rows of %d doubles"
                         % (median(times["risk S=64"]) / median(times["stored-rows pair S=64"]), R, 4 * (N + 1) + 2 * N + cilqr_amd.SCORE_FIELDS))
    s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

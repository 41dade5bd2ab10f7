#!/usr/bin/env python3
"""The analytic chance risk against sampled obstacles (the M = 0 cilqr_chance_risk_device launch that supplies Sigma_t + the two launches
of cilqr_chance_risk_sampled_device) beside cilqr_rollout_risk_sampled_device at S = 64 on the same batch, on config-3 scenes (make_c3:
8 moving obstacles x 32 pose samples, N = 50), in one process, alternated round by round so that all see the same clocks and neighbours:

  planner's shape   B = 16
  wide batch        B = 1024

Before anything is timed, pair_p and step_risk of the new call are asserted equal (1e-9) to a numpy restatement of the header's sums on
the call's own entry_p for the first --check solves — q = mean over the samples, r_t = min(1, sum over the obstacles) — and the nominal
share equal to CILQR_SCORE_COLLISION of the sampled score on the same plans.  (entry_p itself is checked against the materialised call
and a restatement in tests/test_chance_risk_sampled.py.)  Times are device events; the launches are short, so a window holds --reps
launches back to back and is divided by their number.  Nothing is promised in advance: the file reports the medians.

    python tools/chance_sampled_ab.py [--rounds R] [--reps K] [--out profiles/r16_chance_sampled.txt]
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
from risk_sampled_ab import median, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--check", type=int, default=16, help="solves whose sums numpy restates before timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    Bw, Bp, N, n_obs, ns, S = args.batch, 16, 50, 8, 32, 64
    E = n_obs * ns
    p = cilqr_amd.default_params(N)
    sc = scenes.make_c3(Bw, p, n_dyn=n_obs, n_samples=ns)
    w = sc["sample_weight"]
    s = cilqr_amd.Solver(p, max_batch=Bw, max_horizon=N, max_obstacles=E, device=0)
    sigma0 = np.zeros(16)
    sigma0[0], sigma0[5], sigma0[15] = 0.16 ** 2, 0.16 ** 2, 0.017 ** 2
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    zeros = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device="cuda")  # noqa: E731
    Bc = min(args.check, Bp)
    t = dict(x0=dv(sc["x0"]), U0=dv(sc["U"]), poly=dv(sc["poly"]), fl=dv(sc["xplan_fl"]), npose=dv(sc["nom_pose"]), ndim=dv(sc["nom_dim"]),
             off=dv(sc["offsets"]), delta=dv(scenes.pose_offsets(S, 0.16, 0.16, 0.017, seed=5)), s0=dv(sigma0))
    t["U"] = t["U0"].clone()
    t.update(X=zeros(Bw, 4 * (N + 1)), J=zeros(Bw), it=zeros(Bw, dtype=torch.int32), st=zeros(Bw, dtype=torch.int32),
             k=zeros(Bw, 2 * N), K=zeros(Bw, 8 * N), ok=zeros(Bw, dtype=torch.int32), score=zeros(Bw, cilqr_amd.SCORE_FIELDS), base=zeros(Bw),
             rrisk=zeros(Bw, cilqr_amd.RRS_FIELDS), hits=zeros(Bw, N, dtype=torch.int32), rtotal=zeros(Bw),
             sigma=zeros(Bw, N + 1, 16), crisk=zeros(Bw, cilqr_amd.CHANCE_FIELDS), ctotal=zeros(Bw),
             srisk=zeros(Bw, cilqr_amd.CRS_FIELDS), step=zeros(Bw, N), pair=zeros(Bw, n_obs, N), stotal=zeros(Bw), entry=zeros(Bc, E, N))
    stream = torch.cuda.current_stream().cuda_stream
    ptr = {k: v.data_ptr() for k, v in t.items()}

    def prepare(B):  # the solved batch, its gains and nominal totals
        t["U"].copy_(t["U0"])
        s.solve_batch_sampled_device(stream, B, N, n_obs, ns, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr["npose"], ptr["ndim"], ptr["off"],
                                     w, ptr["X"], ptr["J"], ptr["it"], ptr["st"])
        s.gains_batch_sampled_device(stream, B, N, n_obs, ns, ptr["X"], ptr["U"], ptr["poly"], ptr["fl"], ptr["npose"], ptr["ndim"], ptr["off"],
                                     w, ptr["k"], ptr["K"], ptr["ok"], lamb=1.0)
        s.score_batch_sampled_device(stream, B, N, n_obs, ns, ptr["X"], ptr["U"], ptr["poly"], ptr["fl"], ptr["npose"], ptr["ndim"], ptr["off"],
                                     w, ptr["score"], ptr["base"], max_collision=1.0)

    def rollout(B):
        s.rollout_risk_sampled_device(stream, B, N, n_obs, ns, S, ptr["X"], ptr["U"], ptr["k"], ptr["K"], ptr["delta"], 0, ptr["npose"],
                                      ptr["ndim"], ptr["off"], ptr["rrisk"], ptr["hits"], ptr["rtotal"], ptr["base"], k_scale=0.0, max_risk=0.25)

    def chain(B):  # the M = 0 chance launch: Sigma_t, and its total as the next call's base
        s.chance_risk_device(stream, B, N, 0, ptr["X"], ptr["U"], ptr["K"], ptr["s0"], 0, 0, 0, 0, (0, 0, 0, 0), ptr["crisk"],
                             sigma_out=ptr["sigma"], total=ptr["ctotal"], base=ptr["base"], max_risk=0.25)

    def sampled(B, steps=True, entry=False):
        s.chance_risk_sampled_device(stream, B, N, n_obs, ns, ptr["X"], ptr["sigma"], ptr["npose"], ptr["ndim"], ptr["off"], ptr["srisk"],
                                     ptr["step"] if steps else 0, ptr["pair"] if steps else 0, ptr["entry"] if entry else 0, ptr["stotal"],
                                     ptr["ctotal"], max_risk=0.25)

    def both(B):
        chain(B)
        sampled(B)

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(f, reps):
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = ["analytic chance risk against sampled obstacles beside the fused rollout risk of the same batch, config-3 scenes (n_obs %d x "
             "n_samples %d, N = %d): device events, %d alternated rounds, one process" % (n_obs, ns, N, args.rounds),
             "Sigma_0 = diag(0.16^2, 0.16^2, 0, 0.017^2), no W; rollout risk at S = %d ego offsets shared by the batch; %d CUs" % (S, cus)]
    for B in (Bp, Bw):
        for _ in range(2):  # warm-up: code objects loaded, the solve's schedule hint built
            prepare(B)
            rollout(B)
            both(B)
        torch.cuda.synchronize()
        if B == Bp:  # ---- agreement, before anything is timed
            sampled(Bc, entry=True)
            torch.cuda.synchronize()
            ep = t["entry"].cpu().numpy().reshape(Bc, n_obs, ns, N)
            q = ep.mean(axis=2)
            r = np.fmin(1.0, q.sum(axis=1))
            assert np.max(np.abs(t["pair"][:Bc].cpu().numpy() - q)) <= 1e-9, "pair_p differs from the mean of entry_p over the samples"
            assert np.max(np.abs(t["step"][:Bc].cpu().numpy() - r)) <= 1e-9, "step_risk differs from the sum of pair_p over the obstacles"
            both(B)
            torch.cuda.synchronize()
        assert np.array_equal(t["srisk"][:B, cilqr_amd.CRS_NOMINAL_SHARE].cpu().numpy(), t["score"][:B, cilqr_amd.SCORE_COLLISION].cpu().numpy()), \
            "CRS_NOMINAL_SHARE differs from the sampled score's collision share"
        names = ["rollout risk S=%d" % S, "chance M=0 (Sigma_t)", "chance sampled", "chance M=0 + chance sampled", "chance sampled, no per-step output"]
        calls = [lambda: rollout(B), lambda: chain(B), lambda: sampled(B), lambda: both(B), lambda: sampled(B, steps=False)]
        times = {n: [] for n in names}
        first, same = None, True
        for _ in range(args.rounds):
            prepare(B)
            chain(B)
            torch.cuda.synchronize()
            for n, f in zip(names, calls):
                times[n].append(window(f, args.reps))
            sampled(B)
            torch.cuda.synchronize()
            if first is None:
                first = t["srisk"][:B].clone()
            same = same and torch.equal(t["srisk"][:B].view(torch.int64), first.view(torch.int64))
        ref = median(times[names[0]])
        G = (N + 3) // 4
        lines.append("B = %d: %d workgroups of 256 lanes (chance sampled), %d (rollout risk); gains ok on %d of %d solves"
                     % (B, B * G, B * ((S + 255) // 256), int(t["ok"][:B].sum().item()), B))
        for n in names:
            lines.append("   %-36s ms (%2d per window)   %s   = %.3f x the rollout risk launch of that batch"
                         % (n + ",", args.reps, spread(times[n]), median(times[n]) / ref))
        sr, rr = t["srisk"][:B].cpu().numpy(), t["rrisk"][:B].cpu().numpy()
        lines.append("   chance sampled rows bit-identical over the rounds: %s" % same)
        lines.append("   CRS_STEP_RISK min %.4f median %.4f max %.4f; CRS_MAX_PAIR_P max %.4f beside RRS_PAIR_SHARE max %.4f; NaN totals at max_risk "
                     "0.25: %d (analytic) and %d (rollouts) of %d" % (sr[:, cilqr_amd.CRS_STEP_RISK].min(), np.median(sr[:, cilqr_amd.CRS_STEP_RISK]),
                                                                      sr[:, cilqr_amd.CRS_STEP_RISK].max(), sr[:, cilqr_amd.CRS_MAX_PAIR_P].max(),
                                                                      rr[:, cilqr_amd.RRS_PAIR_SHARE].max(),
                                                                      int(np.isnan(t["stotal"][:B].cpu().numpy()).sum()),
                                                                      int(np.isnan(t["rtotal"][:B].cpu().numpy()).sum()), B))
    s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

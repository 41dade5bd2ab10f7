#!/usr/bin/env python3
"""The path-aligned planning frame measured: what its one inexact routine differs by, and what its launches cost.

Part 1, headings.  phi = atan2(s, c) is the one value of a frame record the device and the host's libm may round differently.
Over the pre-step cases of tests/test_path_frame_gpu.py and --chords seeded chords (two-waypoint paths, headings uniform on the
circle and packed around the axes and diagonals, lengths from 1e-3 m to 1e5 m, origins up to 5e5 m out) it reports the largest
|phi_device - math.atan2(s, c)| and the largest difference of the ego heading theta - phi, in spacings of doubles at max(|phi|,
|value|).  (ox, oy, c, s) must be bit-equal to the numpy restatement on every chord, or the tool stops.  The tests assert twice
the figure printed here.

Part 2, times.  Config-2 scenes at N = 50, M = 4 static obstacles, a P = 200 path shared by the batch, B = 16 and B = 1024, in one
process, alternated round by round: the framed pre-step beside cilqr_local_plan_batch_device; cilqr_frame_obstacles_device beside
the page-locked upload of the same dense table; cilqr_frame_states_device; and the framed sequence (pre-step, obstacle rows, solve,
states back) beside the unframed one (pre-step, solve).  Device events; a window holds --reps calls back to back; every launch of
the new code is timed twice per round (an A/A pair: what the difference of two equal things looks like here).  Nothing is promised
in advance: the file reports the medians.

    python tools/path_frame_ab.py [--rounds R] [--reps K] [--chords C] [--out profiles/r32_path_frame.txt]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uncertainty-aware-cilqr-for-trajectory-optimization_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime first, tests/conftest.py)

import cilqr_amd  # noqa: E402
from cilqr_amd import scenes  # noqa: E402

import path_frame_ref as R  # noqa: E402  (tests/: the restatement the suite checks against)


def spread(ts):
    ts = sorted(ts)
    return "min %.4f  median %.4f  max %.4f" % (ts[0], ts[len(ts) // 2], ts[-1])


def median(ts):
    return sorted(ts)[len(ts) // 2]


def ulps(got, want, phi):
    unit = np.spacing(np.maximum(np.abs(phi), np.abs(want)))
    return np.abs(got - want) / unit


def seeded_chords(n, seed=3299):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-math.pi, math.pi, n)
    k = n // 4  # a quarter of them within 1e-6 ... 1e-12 rad of a multiple of pi/4
    a[:k] = rng.integers(-4, 5, k) * (math.pi / 4) + rng.choice([-1.0, 1.0], k) * 10.0 ** rng.uniform(-12, -6, k)
    length = 10.0 ** rng.uniform(-3, 5, n)
    o = rng.uniform(-1.0, 1.0, (n, 2)) * 10.0 ** rng.uniform(0, 5.7, (n, 1))
    e = o + length[:, None] * np.stack([np.cos(a), np.sin(a)], axis=1)
    paths = np.stack([o, e], axis=1)
    egos = np.stack([o[:, 0], o[:, 1], np.full(n, 3.0), a + rng.uniform(-0.3, 0.3, n)], axis=1)  # the ego stands on the origin: first = 0
    return paths, egos


def heading_part(lines, n_chords):
    from oracle import oracle as O
    O.build(ref=False)
    worst_phi = worst_ego = 0.0
    where = None
    s = cilqr_amd.Solver(cilqr_amd.default_params(30), max_batch=max(n_chords, 64), max_horizon=30, max_obstacles=0, device=0)
    n_cases = 0
    for label, paths, egos in R.prestep_cases():
        got = s.local_plan_frames(paths, egos)
        for b, w in enumerate(R.restated(O, paths, egos)):
            n_cases += 1
            u = float(ulps(got["frames"][b, 4], w["frame"][4], w["frame"][4]))
            worst_phi = max(worst_phi, u)
            if not math.isnan(egos[b, 3]):
                worst_ego = max(worst_ego, float(ulps(got["ego"][b, 3], w["ego"][3], w["frame"][4])))
    paths, egos = seeded_chords(n_chords)
    got = s.local_plan_frames(paths, egos)
    s.close()
    want = np.array([R.make_frame(paths[b, 0], paths[b, 1], 2)[0] for b in range(n_chords)])
    if not np.array_equal(got["frames"][:, :4].view(np.uint64), want[:, :4].view(np.uint64)):
        raise SystemExit("(ox, oy, c, s) differ from the restatement on a seeded chord")
    assert not got["info"].any() and not got["first"].any()
    u = ulps(got["frames"][:, 4], want[:, 4], want[:, 4])
    ue = ulps(got["ego"][:, 3], egos[:, 3] - want[:, 4], want[:, 4])
    if u.max() > worst_phi:
        where = int(np.argmax(u))
    worst_phi, worst_ego = max(worst_phi, float(u.max())), max(worst_ego, float(ue.max()))
    lines.append("headings: %d pre-step cases of tests/test_path_frame_gpu.py and %d seeded chords; (ox, oy, c, s) bit-equal to the restatement on all"
                 % (n_cases, n_chords))
    lines.append("   phi = atan2(s, c), device against math.atan2: largest difference %.3f ulp; chords that differ at all: %d of %d%s"
                 % (worst_phi, int((u > 0).sum()), n_chords, "" if where is None else " (largest at s = %r, c = %r)" % (want[where, 3], want[where, 2])))
    lines.append("   ego heading theta - phi, device against the restatement: largest difference %.3f spacings at max(|phi|, |theta - phi|)" % worst_ego)
    lines.append("   HEADING_ULPS of the tests = 2 x max of the two = %.3f" % (2.0 * max(worst_phi, worst_ego)))


def timing_part(lines, rounds, reps):
    N, M, P = 50, 4, 200
    p = cilqr_amd.default_params(N)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    zeros = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device="cuda")  # noqa: E731
    i = np.arange(float(P))
    path = np.stack([i, 0.5 * np.sin(0.05 * i)], axis=1)
    lines.append("times: device events, %d alternated rounds of %d calls per window, one process; N=%d, M=%d static obstacles (strides (M, 1, 0)), "
                 "P=%d shared path; launches of the new code timed twice per round (A/A)" % (rounds, reps, N, M, P))
    for B in (16, 1024):
        sc = scenes.make_c2(B, p)
        s = cilqr_amd.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M, device=0)
        obs_pose, obs_dim = sc["obs_pose"].reshape(B, M, N, 4)[:, :, 0, :], sc["obs_dim"].reshape(B, M, N, 2)[:, :, 0, :]
        t = dict(path=dv(path), ego=dv(sc["x0"]), U0=dv(sc["U"]), pose=dv(obs_pose), dim=dv(obs_dim), dense_pose=dv(sc["obs_pose"]), dense_dim=dv(sc["obs_dim"]))
        t["U"] = t["U0"].clone()
        t.update(fr=zeros(B, 5), info=zeros(B, dtype=torch.int32), x0=zeros(B, 4), poly=zeros(B, 6), fl=zeros(B, 2), oP=zeros(B, M, 4 * N),
                 oD=zeros(B, M, 2 * N), X=zeros(B, 4 * (N + 1)), J=zeros(B), it=zeros(B, dtype=torch.int32), st=zeros(B, dtype=torch.int32),
                 poly_u=zeros(B, 6), fl_u=zeros(B, 2))
        pin_pose, pin_dim = torch.from_numpy(sc["obs_pose"]).pin_memory(), torch.from_numpy(sc["obs_dim"]).pin_memory()
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        ptr = {k: v.data_ptr() for k, v in t.items()}

        def pre_framed():
            s.local_plan_frames_device(stream, B, P, ptr["path"], 0, ptr["ego"], ptr["fr"], ptr["info"], ptr["x0"], ptr["poly"], ptr["fl"])

        def pre_plain():
            s.local_plan_batch_device(stream, B, P, ptr["path"], 0, ptr["ego"], ptr["poly_u"], ptr["fl_u"])

        def obstacles():
            s.frame_obstacles_device(stream, B, N, M, ptr["fr"], 5, ptr["pose"], ptr["dim"], (M, 1, 0), ptr["oP"], ptr["oD"])

        def upload():
            t["dense_pose"].copy_(pin_pose, non_blocking=True)
            t["dense_dim"].copy_(pin_dim, non_blocking=True)

        def states():
            s.frame_states_device(stream, B, 1, N, ptr["fr"], 5, cilqr_amd.FRAME_FROM, ptr["X"], ptr["X"])

        def seq_framed():
            t["U"].copy_(t["U0"])
            pre_framed()
            obstacles()
            s.solve_batch_obstacles_device(stream, B, N, M, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr["oP"], ptr["oD"], 0, (M * N, N, 1, 0),
                                           ptr["X"], ptr["J"], ptr["it"], ptr["st"])
            states()

        def seq_plain():
            t["U"].copy_(t["U0"])
            pre_plain()
            s.solve_batch_obstacles_device(stream, B, N, M, ptr["ego"], ptr["U"], ptr["poly_u"], ptr["fl_u"], ptr["pose"], ptr["dim"], 0, (M, 1, 0, 0),
                                           ptr["X"], ptr["J"], ptr["it"], ptr["st"])

        steps = [("pre-step, unframed", pre_plain, reps), ("pre-step, framed", pre_framed, reps), ("pre-step, framed (A/A)", pre_framed, reps),
                 ("frame_obstacles", obstacles, reps), ("frame_obstacles (A/A)", obstacles, reps), ("pinned upload of the table", upload, reps),
                 ("frame_states", states, reps), ("frame_states (A/A)", states, reps), ("sequence, unframed", seq_plain, 1),
                 ("sequence, framed", seq_framed, 1), ("sequence, framed (A/A)", seq_framed, 1)]
        for _ in range(3):
            for _, f, _ in steps:
                f()
        torch.cuda.synchronize()
        it_f = None
        times = {name: [] for name, _, _ in steps}
        for _ in range(rounds):
            for name, f, k in steps:
                torch.cuda.synchronize()
                e0.record()
                for _ in range(k):
                    f()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / k)
                if name == "sequence, framed":
                    it_f = t["it"].cpu().numpy().copy()
                if name == "sequence, unframed":
                    it_u = t["it"].cpu().numpy().copy()
        lines.append("B=%d; the solve runs on %d lanes per solve, %d wavefront(s); iterations summed over the batch: unframed %d, framed %d"
                     % (B, s.solve_family(B, N, M), s.solve_wavefronts(B, N, M), int(it_u.sum()), int(it_f.sum())))
        for name, _, k in steps:
            lines.append("   %-30s ms (%2d per window)    %s" % (name + ",", k, spread(times[name])))
        lines.append("   framed sequence / unframed sequence, medians: %.3f" % (median(times["sequence, framed"]) / median(times["sequence, unframed"])))
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--chords", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32_path_frame.txt"))
    args = ap.parse_args()
    lines = []
    heading_part(lines, args.chords)
    timing_part(lines, args.rounds, args.reps)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

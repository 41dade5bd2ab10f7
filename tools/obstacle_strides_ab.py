#!/usr/bin/env python3
"""Obstacles by strides (cilqr_solve_batch_obstacles*) against the dense tables of cilqr_solve_batch*, the two variants alternated
in one process so that both see the same clocks and the same neighbours:

  A  host-buffer solves/s, config 2 (B = 1024, N = 50, M = 4): dense [B][M][4N] tables against static per solve (B, M, 4), from
     pageable and from page-locked memory (cilqr_host_alloc); copies in and out included;
  B  one grouped-family launch (B = 8192, N = 80, M = 16, config-5 paths) with ONE obstacle scene: shared (M, 4), whose table is
     built once in front of the solves, against the same scene replicated B times (dense device tables); kernel time by events.

    python tools/obstacle_strides_ab.py [--rounds R] [--out profiles/r04_obstacle_strides.txt]
    python tools/obstacle_strides_ab.py --launch shared|replicated [--reps K]   one variant of B only (a counter-collection run)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uncertainty-aware-cilqr-for-trajectory-optimization_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime first, tests/conftest.py)

import cilqr_amd  # noqa: E402
from cilqr_amd import scenes  # noqa: E402


def spread(ts):
    ts = sorted(ts)
    return "min %.3f  median %.3f  max %.3f" % (ts[0], ts[len(ts) // 2], ts[-1])


def host_ab(rounds, lines):
    N, M, B = 50, 4, 1024
    p = cilqr_amd.default_params(N)
    sc = scenes.make_c2(B, p)
    s = cilqr_amd.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M, device=0)
    st_pose = np.ascontiguousarray(sc["obs_pose"].reshape(B, M, N, 4)[:, :, 0])
    st_dim = np.ascontiguousarray(sc["obs_dim"].reshape(B, M, N, 2)[:, :, 0])
    srcs = {"pageable": dict(sc, st_pose=st_pose, st_dim=st_dim)}
    srcs["pinned"] = {k: cilqr_amd.pinned_copy(v) for k, v in srcs["pageable"].items()
                      if k in ("x0", "U", "poly", "xplan_fl", "obs_pose", "obs_dim", "st_pose", "st_dim")}
    outs = {"pageable": None, "pinned": dict(U=cilqr_amd.pinned_empty((B, 2 * N)), X=cilqr_amd.pinned_empty((B, 4 * (N + 1))),
                                             J=cilqr_amd.pinned_empty((B,)), iters=cilqr_amd.pinned_empty((B,), np.int32),
                                             status=cilqr_amd.pinned_empty((B,), np.int32))}

    def call(kind, mem):
        src, out = srcs[mem], outs[mem]
        if out is not None:
            out["U"][...] = src["U"]
        t = time.perf_counter()
        if kind == "dense":
            r = s.solve_batch(N, src["x0"], src["U"], src["poly"], src["xplan_fl"], src["obs_pose"], src["obs_dim"], out=out)
        else:
            r = s.solve_batch_obstacles(N, src["x0"], src["U"], src["poly"], src["xplan_fl"], src["st_pose"], src["st_dim"], out=out)
        dt = time.perf_counter() - t
        return dt, r["U"].copy(), r["iters"].copy()

    lines.append("A. host-buffer entry points, config 2 (B=%d, N=%d, M=%d), copies in and out included; %d alternated rounds, M solves/s"
                 % (B, N, M, rounds))
    lines.append("   inputs per solve: dense %d bytes, static per solve %d bytes; outputs %d bytes"
                 % (8 * (4 + 6 + 2 + 2 * N + M * 6 * N), 8 * (4 + 6 + 2 + 2 * N + M * 6), 8 * (2 * N + 4 * (N + 1) + 1) + 8))
    for mem in ("pageable", "pinned"):
        res = {"dense": [], "static": []}
        ref = {}
        for kind in ("dense", "static"):
            _, ref[kind], _ = call(kind, mem)  # first call untimed
        same = np.array_equal(ref["dense"], ref["static"])
        for _ in range(rounds):
            for kind in ("dense", "static"):
                dt, U, _ = call(kind, mem)
                res[kind].append(B / dt / 1e6)
                same = same and np.array_equal(U, ref["dense"])
        for kind in ("dense", "static"):
            lines.append("   %-8s %-7s %s" % (mem, kind, spread(res[kind])))
        lines.append("   %-8s results bit-identical: %s" % (mem, same))
    s.close()


def launch_setup():
    N, M, B = 80, 16, 8192
    p = cilqr_amd.default_params(N)
    sc = scenes.make_c5(B, p)
    s = cilqr_amd.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M, device=0)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    pose0 = sc["obs_pose"].reshape(B, M, N, 4)[0, :, 0]  # solve 0's (static) obstacles: the one scene
    dim0 = sc["obs_dim"].reshape(B, M, N, 2)[0, :, 0]
    t = dict(x0=dv(sc["x0"]), U0=dv(sc["U"]), poly=dv(sc["poly"]), fl=dv(sc["xplan_fl"]), sh_pose=dv(pose0), sh_dim=dv(dim0),
             rep_pose=dv(np.broadcast_to(np.repeat(pose0[:, None], N, 1).reshape(M, 4 * N), (B, M, 4 * N))),
             rep_dim=dv(np.broadcast_to(np.repeat(dim0[:, None], N, 1).reshape(M, 2 * N), (B, M, 2 * N))))
    t["U"] = t["U0"].clone()
    t["X"] = torch.zeros(B, 4 * (N + 1), dtype=torch.float64, device="cuda")
    t["J"] = torch.zeros(B, dtype=torch.float64, device="cuda")
    t["it"] = torch.zeros(B, dtype=torch.int32, device="cuda")
    t["st"] = torch.zeros(B, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def launch(kind):
        t["U"].copy_(t["U0"])
        if kind == "shared":
            s.solve_batch_obstacles_device(stream, B, N, M, t["x0"].data_ptr(), t["U"].data_ptr(), t["poly"].data_ptr(), t["fl"].data_ptr(),
                                           t["sh_pose"].data_ptr(), t["sh_dim"].data_ptr(), 0, (0, 1, 0, 0), t["X"].data_ptr(),
                                           t["J"].data_ptr(), t["it"].data_ptr(), t["st"].data_ptr())
        else:
            s.solve_batch_device(stream, B, N, M, t["x0"].data_ptr(), t["U"].data_ptr(), t["poly"].data_ptr(), t["fl"].data_ptr(),
                                 t["rep_pose"].data_ptr(), t["rep_dim"].data_ptr(), 0, t["X"].data_ptr(), t["J"].data_ptr(),
                                 t["it"].data_ptr(), t["st"].data_ptr())
    return s, t, launch, (B, N, M)


def launch_ab(rounds, lines):
    s, t, launch, (B, N, M) = launch_setup()
    assert s.solve_family(B, N, M) < 64
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {"shared": [], "replicated": []}
    ref = {}
    for kind in ("replicated", "shared"):
        launch(kind)
        torch.cuda.synchronize()
        ref[kind] = (t["U"].clone(), t["it"].clone())
    same = bool(torch.equal(ref["shared"][0], ref["replicated"][0]) and torch.equal(ref["shared"][1], ref["replicated"][1]))
    for _ in range(rounds):
        for kind in ("replicated", "shared"):
            t["U"].copy_(t["U0"])
            torch.cuda.synchronize()
            e0.record()
            launch(kind)
            e1.record()
            torch.cuda.synchronize()
            res[kind].append(e0.elapsed_time(e1))
    lines.append("B. grouped family, one obstacle scene (B=%d, N=%d, M=%d, G=%d lanes per solve, config-5 paths); %d alternated rounds, "
                 "ms per launch (events; the shared variant includes its table kernel)" % (B, N, M, s.solve_family(B, N, M), rounds))
    for kind in ("replicated", "shared"):
        lines.append("   %-10s %s" % (kind, spread(res[kind])))
    lines.append("   results bit-identical: %s" % same)
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--launch", choices=("shared", "replicated"), default=None)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if args.launch:  # one variant only, for a counter-collection run
        s, t, launch, _ = launch_setup()
        for _ in range(args.reps):
            launch(args.launch)
        torch.cuda.synchronize()
        s.close()
        return
    lines = []
    host_ab(args.rounds, lines)
    launch_ab(args.rounds, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Wall time per call of the HOST-BUFFER forms of the risk family at the planner's smallest shape — one candidate (B = 1, N = 50,
M = 4 static obstacles, S = 64 shared start offsets) — where a call is a handful of DMA latencies around a short launch:

  cilqr_gains_batch    X, U, path, obstacles in; k, K, ok back
  cilqr_rollout_risk   X, U, k, K, offsets, obstacles, base in; risk, step_hits, total back

One process times one library (CILQR_LIB in the environment chooses an A/B build, cilqr_amd/__init__.py); run it once per build,
alternating, on one box.  The arguments are marshalled once, outside the timed loop.  Prints one JSON line.

    [CILQR_LIB=other/libcilqr_hip.so] python tools/host_transport_ab.py [--calls 2000] [--label NAME]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uncertainty-aware-cilqr-for-trajectory-optimization_amd")]
import numpy as np  # noqa: E402

import cilqr_amd  # noqa: E402
from cilqr_amd import scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--label", default=os.environ.get("CILQR_LIB", "lib/libcilqr_hip.so"))
    args = ap.parse_args()
    B, N, M, S = 1, 50, 4, 64
    p = cilqr_amd.default_params(N)
    sc = scenes.make_c2(B, p)
    s = cilqr_amd.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M, device=0)
    sol = s.solve_batch(N, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], sc["obs_pose"], sc["obs_dim"])
    X, U, J = sol["X"], sol["U"], sol["J"]
    poly, fl = np.ascontiguousarray(sc["poly"]), np.ascontiguousarray(sc["xplan_fl"])
    pose, dim = np.ascontiguousarray(sc["obs_pose"]), np.ascontiguousarray(sc["obs_dim"])
    delta = scenes.pose_offsets(S, 0.16, 0.16, 0.017, seed=5)
    k, K, ok = np.zeros((B, 2 * N)), np.zeros((B, 8 * N)), np.zeros(B, np.int32)
    risk, hits, total = np.zeros((B, cilqr_amd.ROLLOUT_RISK_FIELDS)), np.zeros((B, N), np.int32), np.zeros(B)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    P = lambda a: a.ctypes.data_as(ip if a.dtype == np.int32 else dp)  # noqa: E731
    obs = cilqr_amd.Obstacles(pose.ctypes.data, dim.ctypes.data, None, M * N, N, 1, 0)
    L, h = cilqr_amd.lib(), s._h
    gains_args = (h, B, N, M, P(X), P(U), P(poly), P(fl), C.byref(obs), C.c_double(1.0), P(k), P(K), P(ok))
    risk_args = (h, B, N, M, S, P(X), P(U), P(k), P(K), P(delta), C.c_int64(0), C.c_double(0.0), C.byref(obs), C.c_double(0.05), P(J), P(risk),
                 P(hits), P(total))
    out = {"label": args.label, "shape": "B=%d N=%d M=%d S=%d" % (B, N, M, S), "calls": args.calls, "unit": "us per call"}
    for name, fn, a in (("gains_batch", L.cilqr_gains_batch, gains_args), ("rollout_risk", L.cilqr_rollout_risk, risk_args)):
        for _ in range(50):
            cilqr_amd._check(fn(*a))
        ts = []
        for _ in range(args.calls):
            t = time.perf_counter()
            rc = fn(*a)
            ts.append(time.perf_counter() - t)
            if rc:
                cilqr_amd._check(rc)
        ts.sort()
        out[name] = {"min": round(1e6 * ts[0], 2), "median": round(1e6 * ts[len(ts) // 2], 2), "p90": round(1e6 * ts[len(ts) * 9 // 10], 2)}
    out["risk_row"] = [float(v) for v in risk[0]]  # (the same in every build: the transport changes no bit)
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""One-off CPU sweep: on which draws of the randomised parity sweep does the form of the Q_uu inverse matter?

Solves every draw of test_random_static_scenes_wavefront_family (tests/test_gpu_fuzz.py, wavefront_family_scene) with the oracle's
`reference` form (the EigenSolver restatement) and its `exact` form (the closed form in quad precision) and lists the draws and
solves on which the two leave each other by more than --bar in U: the scenes on which a kernel, right to rounding, would miss the
`reference` oracle.  No GPU.  tests/test_quu_conditioning.py pins the draw this found at twelve times the committed number of draws.

    python tools/quu_form_sweep.py --scale 12          (result: profiles/r21_quu_conditioning.txt, section 5)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uncertainty-aware-cilqr-for-trajectory-optimization_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=int, default=12, help="as CILQR_FUZZ_SCALE: 12 draws per unit")
    ap.add_argument("--bar", type=float, default=1e-9, help="max|dU| between the forms that is reported")
    args = ap.parse_args()
    from oracle import oracle as O
    from test_gpu_fuzz import wavefront_family_scene
    O.build(ref=False)
    threads = min(16, O.max_threads())
    t0, found, paths = time.time(), [], 0
    print("# draw  N  M  B  solves beyond %.0e (index: max|dU| reference vs exact) ; other solves' max" % args.bar)
    for seed in range(12 * args.scale):
        N, M, B, _, po, sc = wavefront_family_scene(seed, O.default_params, O.default_params, O.local_plan)
        r = {f: O.solve_batch(po, N, M, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], sc["obs_pose"], sc["obs_dim"], sc["obs_weight"],
                              threads=threads, quu=f) for f in ("reference", "exact")}
        same = (r["reference"]["iters"] == r["exact"]["iters"]) & (r["reference"]["status"] == r["exact"]["status"])
        paths += int((~same).sum())
        fin = np.isfinite(r["reference"]["U"]).all(axis=1) & np.isfinite(r["exact"]["U"]).all(axis=1)
        du = np.where(fin, np.max(np.abs(np.where(fin[:, None], r["reference"]["U"] - r["exact"]["U"], 0.0)), axis=1), 0.0)
        hot = np.nonzero(du > args.bar)[0]
        if hot.size or not same.all():
            found.append(seed)
            print("%4d %4d %3d %4d   %s ; %.2e%s" % (seed, N, M, B, ", ".join("%d: %.3e" % (k, du[k]) for k in hot),
                                                   np.delete(du, hot).max() if hot.size < B else 0.0,
                                                   "" if same.all() else " ; %d solves on another accept/reject path" % int((~same).sum())))
    print("# %d draws, %d with a solve beyond the bar or on another path: %s; %.0f s" % (12 * args.scale, len(found), found, time.time() - t0))


if __name__ == "__main__":
    main()

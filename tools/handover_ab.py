#!/usr/bin/env python3
"""A/B of two BUILDS of the library on the hand-over scenes of tests/test_psd_check_off_chain.py: the scenes whose Q_uu fails the PSD
test (obstacle weight -40 beside the ego at step 0, in the middle and at step N - 1; N = 1 ... 127) and the non-finite ones, on the
three plans of that file.  A solve that is handed to the GENERAL kernel in one build and not in the other shows up here, since the
GENERAL kernel agrees with the fast passes only to rounding: U, X, J, iters, status and the pass-count buffer must agree bit for bit.

    [CILQR_LIB=path/to/libcilqr_hip.so] python tools/handover_ab.py dump FILE.npz     once per build
    python tools/handover_ab.py compare A.npz B.npz                                  exit code 1 when an array differs
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uncertainty-aware-cilqr-for-trajectory-optimization_amd"), os.path.join(ROOT, "tests")]
import numpy as np


def dump(path):
    import torch  # noqa: F401  (before the library: tests/conftest.py)
    import cilqr_amd
    import test_psd_check_off_chain as T
    out = {}
    for N, step in T.INDEFINITE:
        p, sb = T._indefinite_scene(cilqr_amd, N, step)
        for plan, env in T.PLANS.items():
            r, passes = T._solve(cilqr_amd, env, p, sb, N, passes=True)
            for k in T.KEYS:
                out["indefinite N=%d step=%d %s %s" % (N, step, plan, k)] = r[k]
            out["indefinite N=%d step=%d %s passes" % (N, step, plan)] = passes
    for N in (2, 4, 50, 65):
        for where in ("x0", "first step", "last step"):
            p, sc = T._scene(cilqr_amd, N)
            sn = dict(sc, x0=sc["x0"].copy(), obs_pose=sc["obs_pose"].copy())
            if where == "x0":
                sn["x0"][T.NAN_SOLVE, 1] = np.nan
            else:
                sn["obs_pose"].reshape(T.B, T.M, N, 4)[T.NAN_SOLVE, 1, 0 if where == "first step" else N - 1, 0] = np.nan
            for plan, env in T.PLANS.items():
                r, passes = T._solve(cilqr_amd, env, p, sn, N, passes=True)
                for k in T.KEYS:
                    out["non-finite N=%d %s %s %s" % (N, where, plan, k)] = r[k]
                out["non-finite N=%d %s %s passes" % (N, where, plan)] = passes
    np.savez(path, **out)
    print("%s: %d arrays of %s" % (path, len(out), os.path.relpath(cilqr_amd.LIB_PATH, ROOT)))


def compare(a, b):
    A, Bz = np.load(a), np.load(b)
    bad = [k for k in A.files if k not in Bz.files or not np.array_equal(A[k], Bz[k], equal_nan=True)]
    print("%d arrays, %d different%s" % (len(A.files), len(bad), "".join("\n    " + k for k in bad[:20])))
    return 1 if bad or set(A.files) != set(Bz.files) else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        raise SystemExit(__doc__)

#!/usr/bin/env python3
"""Kernel time of the config-2 solve by HIP events, for an A/B of two BUILDS of the library (tools/share_ab.py compares two
plans of one build): the library named by CILQR_LIB — or the tree's own — solves the same seeded batch REPS times on the plan
the library picks; minimum, median and mean of the launches (fast kernel + GENERAL hand-over).  Run it once per build and round,
the builds taking turns; the minimum decides (a process can sit in the alternating state, worth 3 % of a mean).

    [CILQR_LIB=path/to/libcilqr_hip.so] python tools/solve_time.py [B] [N] [M]      default 1024 50 4
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uncertainty-aware-cilqr-for-trajectory-optimization_amd")]
import numpy as np, torch
import cilqr_amd
from cilqr_amd import scenes

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
N = int(sys.argv[2]) if len(sys.argv) > 2 else 50
M = int(sys.argv[3]) if len(sys.argv) > 3 else 4
REPS = 16
p = cilqr_amd.default_params(N)
sc = scenes.make_static(B, N, M, p, scenes.SEED0 + 2)
s = cilqr_amd.Solver(p, max_batch=B, max_horizon=N, max_obstacles=max(M, 1))
dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
x0, U0, poly, xpl = dv(sc["x0"]), dv(sc["U"]), dv(sc["poly"]), dv(sc["xplan_fl"])
pose, dim = (dv(sc["obs_pose"]), dv(sc["obs_dim"])) if M else (None, None)
X = torch.zeros(B, 4 * (N + 1), dtype=torch.float64, device="cuda"); J = torch.zeros(B, dtype=torch.float64, device="cuda")
it = torch.zeros(B, dtype=torch.int32, device="cuda"); st = torch.zeros(B, dtype=torch.int32, device="cuda")
U = U0.clone()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
ms = []
for r in range(REPS + 2):
    U.copy_(U0)
    torch.cuda.synchronize(); e0.record()
    s.solve_batch_device(torch.cuda.current_stream().cuda_stream, B, N, M, x0.data_ptr(), U.data_ptr(), poly.data_ptr(), xpl.data_ptr(),
                         pose.data_ptr() if M else 0, dim.data_ptr() if M else 0, 0, X.data_ptr(), J.data_ptr(), it.data_ptr(), st.data_ptr())
    e1.record(); torch.cuda.synchronize()
    if r >= 2:
        ms.append(e0.elapsed_time(e1))
t = sorted(ms)
print("%s: B = %d N = %d M = %d, %d wavefronts per solve: min %.4f median %.4f mean %.4f ms of %d launches; checksum U %.17g"
      % (os.path.relpath(cilqr_amd.LIB_PATH, ROOT), B, N, M, s.solve_wavefronts(B, N, M), t[0], t[len(t) // 2], sum(t) / len(t), REPS,
         float(U.sum().item())), flush=True)
s.close()

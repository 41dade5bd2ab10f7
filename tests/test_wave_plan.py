"""The launch plan of the one-wavefront-per-solve family (csrc/cilqr_wave_plan.h) — which kernel, how many wavefronts per solve, the
obstacle table where, how much LDS — is plain integer arithmetic on the host: checked here without a GPU through
tests/cpp/wave_plan_dump.cpp, for a device of 1024 SIMDs (an MI355X) and the default 200 path samples."""
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

FAITHFUL_ITERS = 1  # CILQR_FLAG_FAITHFUL_ITERS (include/cilqr.h)
SIMDS = 1024


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wave_plan") / "wave_plan_dump")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "wave_plan_dump.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def plan(exe):
    def run(B, N, M, **kw):
        shape = ",".join("%s=%d" % kv for kv in dict(B=B, N=N, M=M, **kw).items())
        r = subprocess.run([exe, shape], check=True, capture_output=True, text=True)
        return json.loads(r.stdout)
    return run


def test_header_is_plain_cpp():
    """The plan header compiles without HIP (its only include beyond the C library is include/cilqr.h)."""
    text = open(os.path.join(PKG, "csrc", "cilqr_wave_plan.h")).read()
    assert "#include <hip" not in text and "__device__" not in text and "__global__" not in text


def test_flag_value_matches_the_header():
    import re
    m = re.search(r"#define\s+CILQR_FLAG_FAITHFUL_ITERS\s+(\S+)", open(os.path.join(ROOT, "include", "cilqr.h")).read())
    assert m and int(m.group(1).rstrip("uU"), 0) == FAITHFUL_ITERS


def test_solve_wavefronts_values_of_the_gpu_tests(plan):
    """Every cilqr_solve_wavefronts value the GPU tests assert on a device (tests/test_gpu_parity.py, tests/test_obstacle_strides.py)."""
    w = lambda B, N, M, **kw: plan(B, N, M, **kw)["solve_wavefronts"]  # noqa: E731
    # test_share_kernel_weights_warm_starts_and_hand_over
    assert w(160, 50, 6) == 3 and w(160, 50, 30) == 3 and w(160, 50, 6, share_off=1) == 1
    assert w(64, 128, 4) == 1 and w(64, 127, 4) == 2 and w(64, 65, 4) == 2 and w(64, 64, 4) == 3
    assert w(64, 63, 4) == 3 and w(64, 63, 1) == 2
    assert w(3 * SIMDS // 4, 50, 4) == 3 and w(3 * SIMDS // 4 + 1, 50, 4) == 2
    assert w(2 * SIMDS, 50, 4) == 2 and w(2 * SIMDS + 1, 50, 4) == 1
    assert w(64, 50, 80) == 1
    assert w(512, 50, 12) == 3 and w(1024, 50, 12) == 1 and w(1024, 50, 8) == 2
    assert w(64, 50, 40) == 3 and w(300, 50, 40) == 1
    # test_share_kernel_changes_no_bit: its parameter list and its rule
    for N, M, B in [(50, 4, 1024), (50, 4, 768), (50, 4, 2048), (50, 12, 300), (50, 8, 1024), (50, 30, 64), (50, 20, 400), (80, 16, 64), (64, 3, 100),
                    (64, 1, 40), (65, 2, 50), (127, 2, 30), (100, 6, 300), (30, 2, 200), (2, 1, 9), (1, 1, 3), (3, 0, 5), (17, 5, 64), (63, 4, 96),
                    (33, 9, 70), (40, 3, 33)]:
        want = 3 if B <= 768 and M >= 2 and N <= 64 else 2
        assert (w(B, N, M), w(B, N, M, share_off=1)) == (want, 1), (N, M, B)
        if want == 3:
            assert w(B, N, M, share_w=2) == 2
    # test_schedule_hint_changes_nothing_but_the_order
    assert w(1800, 50, 4) == 2 and w(3000, 50, 4) == 1
    assert plan(1800, 50, 4)["hinted"] == 1 and plan(3000, 50, 4)["hinted"] == 1 and plan(1024, 50, 4)["hinted"] == 0
    assert plan(3000, 50, 4, hint_off=1)["hinted"] == 0
    # test_obstacle_strides.py: config 2 on the share kernel; M = 40 at B = 1024 on one wavefront with the table in the workspace
    assert w(1024, 50, 4) > 1
    p = plan(1024, 50, 40)
    assert (p["family"], p["solve_wavefronts"], p["kernel"], p["tab"]) == (64, 1, "ONE", 0)
    # under CILQR_PAIR_KERNEL the query answers 1 (include/cilqr.h)
    assert w(256, 50, 4, pair_on=1) == 1 and w(2048, 50, 4, pair_on=1) == 1


def test_solve_family_values_of_the_gpu_tests(plan):
    """test_family_rule_on_measured_shapes, test_pass_count_buffer, test_grouped_family, test_lane_sharing_changes_no_bit."""
    fam = lambda B, N, M, **kw: plan(B, N, M, **kw)["family"]  # noqa: E731
    assert fam(1024, 50, 4) == 64 and fam(4096, 50, 4) == 64 and fam(8192, 50, 4) == 8 and fam(4096, 50, 8) == 64 and fam(8192, 50, 8) == 8
    assert fam(8192, 30, 2) == 64 and fam(16384, 30, 2) == 4 and fam(2048, 64, 4) == 64 and fam(4096, 64, 4) == 16
    assert fam(2048, 80, 16) == 64 and fam(4096, 80, 16) == 16 and fam(8192, 80, 16) == 8 and fam(65536, 80, 16) == 4 and fam(65536, 50, 4) == 2
    assert fam(4096, 120, 4) == 64 and fam(16384, 160, 16) == 64 and fam(4096, 50, 256) == 64
    assert fam(96, 50, 4) == 64 and fam(8192, 50, 4) < 64 and fam(8192, 80, 16) < 64
    for G, B, N, M in [(8, 520, 80, 16), (1, 300, 30, 2), (4, 333, 50, 4), (16, 90, 50, 5), (32, 40, 64, 3), (2, 257, 20, 0)]:
        assert fam(B, N, M, force_g=G) == G
    assert fam(1024, 50, 4, force_g=3) == 64  # (not a lane count: ignored)


def test_solve_sampled_wavefronts_values_of_the_gpu_tests(plan):
    """test_split_kernel_with_uncertainty_map: CILQR_SPLIT_W and CILQR_NO_SPLIT_KERNEL; and the automatic rule."""
    sw = lambda B, N, n_obs, **kw: plan(B, N, n_obs, **kw)["solve_sampled_wavefronts"]  # noqa: E731
    for B, W in [(160, 4), (300, 2)]:
        assert sw(B, 50, 5, split_w=W, map=1) == W and sw(B, 50, 5, split_off=1, map=1) == 1
    assert sw(1024, 50, 8) == 4 and sw(1025, 50, 8) == 2 and sw(4096, 50, 8) == 2
    assert sw(256, 65, 8) == 1 and sw(256, 50, 3) == 1 and sw(4096, 50, 1) == 1 and sw(4096, 50, 2) == 2
    # the plan of the shapes of test_split_kernel_against_one_wavefront_per_solve
    for B, N, n_dyn, S, W in [(200, 50, 8, 32, 4), (1200, 50, 8, 8, 2), (33, 30, 3, 5, 2), (40, 64, 2, 4, 2), (17, 12, 5, 2, 4), (9, 20, 7, 3, 4)]:
        p = plan(B, N, n_dyn, n_samples=S, split_w=W)
        assert (p["kernel"], p["W"], p["tab"]) == ("SPLIT", W, 2), (B, N, n_dyn, S, W)
        assert plan(B, N, n_dyn, n_samples=S, split_off=1)["kernel"] == "ONE"


def test_fall_backs(plan):
    """Where a kernel with further wavefronts per solve does not apply, the plan is the one-wavefront kernel."""
    assert plan(1024, 50, 4)["kernel"] == "SHARE"
    p = plan(1024, 50, 4, flags=FAITHFUL_ITERS)
    assert (p["kernel"], p["W"], p["tab"]) == ("ONE", 1, 1)
    assert plan(64, 127, 4)["kernel"] == "SHARE" and plan(64, 127, 4)["long_form"] == 1 and plan(64, 64, 4)["long_form"] == 0
    assert plan(64, 128, 4)["kernel"] == "ONE"
    # sampled obstacles
    assert plan(256, 64, 8, n_samples=8)["kernel"] == "SPLIT" and plan(256, 65, 8, n_samples=8)["kernel"] == "ONE"
    assert plan(256, 50, 3, n_samples=8)["kernel"] == "ONE" and plan(256, 50, 4, n_samples=8)["W"] == 4  # (four wavefronts need four obstacles)
    assert plan(256, 50, 8, n_samples=8, flags=FAITHFUL_ITERS)["kernel"] == "ONE"
    p = plan(256, 50, 8, n_samples=128)  # 49 280 B of offset records: 63 952 B beside the general kernel, 65 920 B beside four wavefronts
    assert (p["kernel"], p["tab"], p["lds_fast"], p["lds_general"], p["solve_sampled_wavefronts"]) == ("ONE", 2, 10624 + 49280, 14672 + 49280, 4)
    assert plan(256, 50, 8, n_samples=64)["kernel"] == "SPLIT"
    assert plan(256, 50, 8, n_samples=32, map=1)["kernel"] == "SPLIT"  # (a map: its term on the last wavefront)
    # one scene for the batch: the table is built in front of the kernels only where they read it from the workspace
    assert plan(1024, 50, 40, shared=1)["shared_table"] == 1 and plan(1024, 50, 40)["shared_table"] == 0
    p = plan(1024, 50, 4, shared=1)
    assert (p["tab"], p["shared_table"]) == (1, 0)
    p = plan(1024, 50, 4, shared=1, share_off=1)
    assert (p["kernel"], p["tab"], p["shared_table"]) == ("ONE", 1, 0)
    # CILQR_PAIR_KERNEL: up to one solve per SIMD, without a map, within the default 64 KiB
    assert plan(1024, 50, 4, pair_on=1)["kernel"] == "PAIR" and plan(1024, 50, 4, pair_on=1)["W"] == 2
    assert plan(1025, 50, 4, pair_on=1)["kernel"] == "SHARE"  # (beyond: the ordinary rule)
    assert plan(256, 50, 4, pair_on=1, map=1)["kernel"] == "ONE"
    assert plan(256, 50, 4, pair_on=1, flags=FAITHFUL_ITERS)["kernel"] == "ONE"
    p = plan(160, 50, 30, pair_on=1)  # 72 000 B of table: 83 056 B with the pair kernel's arrays
    assert (p["kernel"], p["W"], p["tab"], p["lds_fast"], p["lds_general"]) == ("ONE", 1, 1, 82624, 86672)
    # a map set: the share kernel up to one solve per SIMD
    assert plan(512, 50, 4, map=1)["W"] == 3 and plan(1024, 50, 4, map=1)["W"] == 2 and plan(1025, 50, 4, map=1)["kernel"] == "ONE"
    # beyond the LDS of a CU
    assert plan(64, 1000, 0)["too_large"] == 1 and plan(64, 127, 4)["too_large"] == 0
    assert plan(64, 50, 8, n_samples=400)["too_large"] == 1


def test_lds_bytes(plan):
    """Dynamic LDS per solve of the first kernel and of the GENERAL kernel behind it: literal byte counts, computed by hand from the
    formulas the launcher had before the plan existed.  Per-solve arrays at N = 50 with 200 path samples: 200 + 406 + 50·14 + 22 = 1328
    doubles compact, 200 + 2·406 + 50·16 + 22 = 1834 with candidate buffers."""
    p = plan(1024, 50, 4)  # config 2: 9600 B of table; two wavefronts: 250 partial sums + 4 control doubles
    assert (p["kernel"], p["W"], p["lds_fast"], p["lds_general"]) == ("SHARE", 2, 10624 + 9600 + 2032, 14672 + 9600)
    assert (p["lds_fast"], p["lds_general"]) == (22256, 24272)
    p = plan(1024, 50, 4, share_off=1)
    assert (p["kernel"], p["lds_fast"], p["lds_general"]) == ("ONE", 20224, 24272)
    p = plan(1024, 50, 4, flags=FAITHFUL_ITERS)  # the reference loop keeps candidate buffers in the first kernel too
    assert (p["lds_fast"], p["lds_general"]) == (24272, 24272)
    p = plan(160, 50, 30)  # "87 KB": 72 000 B of table; three wavefronts: 500 partial sums + 4 control doubles
    assert (p["kernel"], p["W"], p["tab"], p["lds_fast"], p["lds_general"]) == ("SHARE", 3, 1, 86656, 86672)
    p = plan(4096, 50, 8, n_samples=32)  # config 3: (8·32·6 + 16)·8 = 12 416 B of sample records; two wavefronts: 250 + 2 doubles
    assert (p["family"], p["kernel"], p["W"], p["tab"], p["lds_fast"], p["lds_general"]) == (64, "SPLIT", 2, 2, 25056, 27088)
    p = plan(1024, 50, 4, pair_on=1)  # the pair kernel: 50 + 4 doubles behind the table
    assert (p["kernel"], p["lds_fast"], p["lds_general"]) == ("PAIR", 10624 + 9600 + 432, 24272)


SOLVE_LDS_MAX = 160 * 1024  # cilqr::SOLVE_LDS_MAX: the LDS of one CU


def _enumerate(exe):
    """Every shape of the static-obstacle sweep through `wave_plan_dump --stdin` → (shapes (n, 6), plans (n, 8)); plan columns:
    kernel (2 = SHARE), W, long_form, tab, lds_fast, lds_general, too_large, solve_wavefronts."""
    shapes = np.array(list(itertools.product(range(1, 128), (2, 44, 50, 200), range(0, 65), (1, 256, 257, 512, 513, 1024), (0, 1), (0, 2, 3))))
    text = "".join("N=%d,path_samples=%d,M=%d,B=%d,map=%d,share_w=%d\n" % tuple(s) for s in shapes)
    r = subprocess.run([exe, "--stdin"], input=text, check=True, capture_output=True, text=True)
    plans = np.array(r.stdout.split(), dtype=np.int64).reshape(-1, 8)
    assert plans.shape[0] == shapes.shape[0] == 127 * 4 * 65 * 6 * 2 * 3
    return shapes, plans


def test_every_plan_fits_the_lds_of_a_cu(exe):
    """No plan asks for more dynamic LDS than a CU has: launch_solve_wave hands max(lds_fast, lds_general) to hipFuncSetAttribute, which
    refuses more than 160 KiB, so an over-limit plan turns a valid call into CILQR_ERR_HIP.  Before the share kernel's candidate was
    bounded, B=256 N=53 M=58 with a map and 44 path samples planned three wavefronts with 163 856 B (limit 163 840) while the GENERAL
    kernel's 161 744 B fit; two wavefronts need 161 728 B.  Also: cilqr_solve_wavefronts answers the W of the plan that will run."""
    shapes, plans = _enumerate(exe)
    kernel, W, lds_fast, lds_general, too_large, query = plans[:, 0], plans[:, 1], plans[:, 4], plans[:, 5], plans[:, 6], plans[:, 7]
    over = (too_large == 0) & ((lds_fast > SOLVE_LDS_MAX) | (lds_general > SOLVE_LDS_MAX))
    assert not over.any(), "%d plans beyond the LDS of a CU, first (N, path_samples, M, B, map, share_w) = %s: %s" % (
        int(over.sum()), shapes[over][0].tolist(), plans[over][0].tolist())
    assert ((too_large == 1) == (lds_general > SOLVE_LDS_MAX)).all()
    share = kernel == 2
    assert (query[share] == W[share]).all() and (query[~share] == 1).all() and (W[share] >= 2).all() and (W[~share] == 1).all()
    # the sweep reaches two and three wavefronts, the short and the long form, tables in LDS and in the workspace, and plans within a
    # few bytes of the limit (no horizon up to 127 is too large on its own: a table that does not fit goes to the workspace)
    assert (W == 2).sum() > 10000 and (W == 3).sum() > 10000 and (plans[share, 2] == 1).sum() > 10000 and (plans[:, 3] == 0).sum() > 10000
    assert np.max(np.maximum(lds_fast, lds_general)) > SOLVE_LDS_MAX - 64 and too_large.sum() == 0


def test_share_plan_steps_down_at_the_lds_limit(plan):
    """The shape above and the one tests/test_quu_conditioning.py solves on a device (50 path samples: the nearest a parameter set
    reaches, path samples being 10·num_of_local_wpts): three wavefronts do not fit, two do, and the query says two."""
    p = plan(256, 53, 58, map=1, path_samples=44)
    assert (p["kernel"], p["W"], p["tab"], p["lds_fast"], p["lds_general"], p["too_large"], p["solve_wavefronts"]) == ("SHARE", 2, 1, 161728, 161744, 0, 2)
    p = plan(4, 53, 58, map=1, path_samples=50)
    assert (p["kernel"], p["W"], p["tab"], p["lds_fast"], p["lds_general"], p["too_large"], p["solve_wavefronts"]) == ("SHARE", 2, 1, 161776, 161792, 0, 2)
    assert plan(4, 53, 57, map=1, path_samples=50)["W"] == 3  # (one obstacle fewer: three fit)
    # (only three wavefronts with a map can pass the GENERAL kernel's size: their 15N partial sums against its 10N + 6 doubles of
    # candidate buffers; 10N + 4 for two with a map or three without always fit where it does)
    assert plan(256, 53, 58, path_samples=44)["W"] == 3 and plan(256, 53, 58, path_samples=44)["lds_fast"] <= SOLVE_LDS_MAX

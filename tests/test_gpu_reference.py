"""The reference's own kernels, compiled for gfx950 (oracle/_ref/libstm_ref_hip.so, recipe oracle/build_ref.py), against the
oracle and the HIP library: the same input arrays on all three sides, stage by stage (cases: tests/ref_cases.py).

The reference runs in a CHILD process per case (python -m oracle.pyref, under `timeout`), because it ends the process with
exit(1) on a failed runtime call and checks no launch status; the child synchronises and reads hipGetLastError after every
call.  If a child ends abnormally the test fails and `_BROKEN` makes every later reference test fail at once without starting
anything on the GPU: the cause is then to be found from the code, not by running it again.

Why each admitted stage stays inside its tiles and buffers on the shapes of tests/ref_cases.py (oracle/pyref.admit asserts
the conditions before a launch; IDs are SURVEY Appendix A):

  ci_adcensus        W % 160 == 0, so every 160-thread block is full and fills its whole tile before the barrier (A-L4); global
                     reads are clamped to the row; the tile indices tx+pad+-(d-zd) reach at most one element outside their half
                     of the tile (A-Q7), which is still inside the launch's own 2 x sm_sz LDS request; writes are guarded by
                     gx < W.  LDS request (160+D-1)*16 B < 4 KB.
  ca_cross           arms: one block of W <= 1024 threads per row, every neighbour test is preceded by a border test.  Sums: W/2
                     resp. H/2 threads per line (even sizes, A-L2), the line tile holds the whole line, and a window [x-armL,
                     x+armR) cannot leave the line because the arm kernel stops arms at the border; arms come from the arm kernel
                     of the same call.  Transposes: grid (W/32, H/8/4) of 32 x 32 tiles covers the plane exactly when W % 32 ==
                     H % 32 == 0 (A-L3) and has no partial tile.  LDS (3*max(W,H)+1)*4 B < 13 KB.
  dc_wta, dr_dcc     one block of W <= 1024 threads per row, guarded; the cross-view column is clamped to [0, W-1].
  filter_bilateral_1 32 x 30 blocks with H % 30 == 0, W % 32 == 0: no thread leaves before the barrier (A-L6), tile reads stay
                     within radius of the block; the colour table of D entries is indexed by (int)|a-b| with no clamp, so the
                     inputs are maps whose value range is below D (asserted by the loader).  LDS < 10 KB.
  filter_gaussian_1  32 x 32 blocks, H % 32 == W % 32 == 0 (A-L5), barrier after the clamped tile fill; the dead reflecting kernel
                     the host wrapper runs first mirrors indices into [0, W-1] for radius < W.  LDS < 13 KB.
  filter_bleed_1     guarded; mirrored neighbour indices stay in the plane for radius < min(H, W).
  dibr_occl, dibr_occl_to_mask   guarded; the target column is clamped.
  dibr_dbm           guarded; sample x is clamped to [0, W-1] before the nearest / +1 fetch, which is clamped again; runs
                     filter_gaussian_1(7, 10) on the mask (H % 32 == W % 32 == 0).
  mux_multiview      Hout % N == 0 takes the strided kernel, which writes columns N*tx+v: inside the row only if Wout % N == 0
                     (asserted); otherwise the guarded 32 x 32 kernel.  Sample coordinates are clamped.
  tx_scale           (d_tx_scale, which takes host pointers despite its name) guarded 32 x 32 blocks over the output; sample
                     coordinates are clamped to the input, the +1 neighbours clamped again.
  grey, census       run inside ci_adcensus (their only caller); clamped 9 x 7 window.

Left out, and why:
  dr_irv             the vote kernel fills its LDS tile and reads it with NO barrier in between (A-Q17 i).  A wave that runs ahead
                     reads whatever an earlier kernel left in LDS, and uses (int)value + zd as an index into `int dhist[65]` in
                     private memory, unclamped: an out-of-bounds WRITE whose address the inputs do not bound.  It cannot be shown
                     to stay in bounds for any shape, so it is not run on a shared machine.
  adcensus_stm,      the frame functions call d_dr_irv five times per view (d_io.cu:147-148): left out for the same reason.
  adcensus_stm_2
  filter_median      reads in[(x+dx) + (y+dy)*W] for dx, dy in -1..1 with no border rule: elements before the start and after the
                     end of the buffer at every border pixel (flat-index sampling, which the oracle models inside a padded copy).
  demux_sbs,         exist only as kernels / inside the frame functions (no host-flavour entry point of their own).
  tx_disp_scale
  dc_hslo            a stub in the reference (A-Q25).      dibr_dfm   a racy scatter (A-Q23).      transposes   gone in our design.
"""
import subprocess

import numpy as np
import pytest

import ref_cases as rc
from conftest import ROOT

pytestmark = pytest.mark.gpu

_BROKEN = []  # the first child that ended abnormally; once set, nothing more of the reference is started


def run_reference(tmp_path, stage, params, arrays):
    """One reference stage call in a child process.  Returns its outputs; fails the test, and every later one, if it ends
    abnormally."""
    from oracle import pyref
    assert not _BROKEN, "an earlier reference child ended abnormally (%s): nothing more is started" % _BROKEN[0]
    assert pyref.available(), "oracle/_ref/libstm_ref_hip.so is missing: build() makes it where the reference tree exists"
    status, out, tail = rc.reference_child(tmp_path, stage, params, arrays)
    if status != 0:
        _BROKEN.append("%s: status %d" % (stage, status))
        pytest.fail("reference child for %s ended with status %d\n%s" % (stage, status, tail))
    return out


def admit_case(stage, p, a):
    """The envelope, asserted in the test module before anything is launched (the loader asserts it again)."""
    from oracle import pyref
    first = a[sorted(a)[0]] if stage != "mux_multiview" else a["views"][0]
    H, W = (first.shape[-2], first.shape[-1]) if first.ndim == 2 or stage in ("dc_wta",) else first.shape[:2]
    if stage == "ca_cross":
        H, W = a["img"].shape[:2]
    pyref.admit(stage, H, W, p.get("D", 1), p.get("zd", 0), p.get("usd", 1), radius=p.get("radius", 0),
                Hout=p.get("Hout"), Wout=p.get("Wout"), N=len(a["views"]) if stage == "mux_multiview" else 8)


@pytest.mark.parametrize("name,stage,params,build", rc.CASES + rc.GPU_ONLY_CASES, ids=rc.CASE_IDS + [c[0] for c in rc.GPU_ONLY_CASES])
def test_stage_three_ways(gpu_ready, stm, orc, tmp_path, name, stage, params, build):
    """reference == oracle == HIP library under the stage's rule (ref_cases.RULES), on the same input arrays."""
    arrays = build(orc, params)
    admit_case(stage, params, arrays)
    ref = run_reference(tmp_path, stage, params, arrays)
    want = rc.run_oracle(orc, stage, params, arrays)
    hip = rc.run_hip(stm, stage, params, arrays)
    rc.check(stage, ref, want, "reference vs oracle")
    rc.check(stage, ref, hip, "reference vs HIP library")
    for k in want:  # HIP library against oracle stays exact, as in test_gpu_parity.py
        assert rc.same_with_nans(hip[k], want[k]), "HIP library vs oracle: %s differs" % k
    if stage == "ca_cross":
        assert np.array_equal(arrays["cost"], build(orc, params)["cost"], equal_nan=True)  # inputs untouched on all sides
    if stage == "ci_adcensus":
        clean = rc.run_oracle(orc, stage, params, arrays, quirks=False)
        shape = want["cost_l"].shape
        rc.check_q7(name, shape, ref, clean, want, rc.TOL[stage], "reference vs oracle")
        hclean = rc.run_hip(stm, stage, params, arrays, quirks=False)
        assert all(np.array_equal(hclean[k], clean[k]) for k in clean)


def test_reference_library_exports_the_33_symbols():
    """The compiled reference stands behind the same 33 names as the drop-in layer (tests/test_abi.py)."""
    import re
    from oracle import pyref
    from test_abi import REFERENCE_HOST_SYMBOLS
    assert pyref.available(), "oracle/_ref/libstm_ref_hip.so is missing"
    out = subprocess.check_output(["nm", "-D", "--defined-only", pyref.LIB_PATH]).decode()
    have = set(re.findall(r" T (_Z\S+)", out))
    assert not [w for w in REFERENCE_HOST_SYMBOLS if w not in have]

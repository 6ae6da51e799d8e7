"""The oracle against what the reference's own kernels computed on an MI355X (tests/golden/ref_gfx950_*.npz, recorded by
tests/golden/make_golden_ref.py from the reference compiled for gfx950).  No GPU and no reference tree are needed: the inputs
are rebuilt from the committed fixtures and seeds (tests/ref_cases.py), the oracle runs, and its outputs are compared with the
recorded ones under the rules of tests/test_gpu_reference.py: exact for the integer and order-defined stages, within
ref_cases.TOL for cost init (fast exp against the rho tables, A-Q8) and the bilateral.  A change to oracle/stm_oracle.c that
departs from the reference fails here.

Not pinned (the reference cannot be shown to stay in bounds there, see tests/test_gpu_reference.py): dr_irv, the frame
functions, filter_median; and by nature dc_hslo, dibr_dfm, the transposes.
"""
import numpy as np
import pytest

import ref_cases as rc
from conftest import load_golden


@pytest.fixture(scope="module")
def recorded():
    return load_golden("ref_gfx950")


def _of(recorded, name):
    got = {k.split("/", 1)[1]: v for k, v in recorded.items() if k.split("/", 1)[0] == name}
    assert got, "no recorded reference output for %s" % name
    return got


def test_every_case_is_recorded(recorded):
    assert sorted({k.split("/", 1)[0] for k in recorded}) == sorted(rc.CASE_IDS)
    assert len(rc.CASES) >= 2 * len(rc.RULES)  # at least two cases per stage
    for stage in rc.RULES:
        assert sum(1 for c in rc.CASES if c[1] == stage) >= 2, stage


def test_tolerances_come_from_the_measurement():
    for stage, tol in rc.TOL.items():
        assert tol == min(4.0 * rc.MEASURED_MAX[stage], 1e-4) and tol <= 1e-4


@pytest.mark.parametrize("name,stage,params,build", rc.CASES, ids=rc.CASE_IDS)
def test_oracle_equals_recorded_reference(orc, recorded, name, stage, params, build):
    arrays = build(orc, params)
    want = rc.run_oracle(orc, stage, params, arrays)
    ref = _of(recorded, name)
    rc.check(stage, ref, rc.views_of(name, want), "recorded reference vs oracle")
    if stage == "ci_adcensus":
        clean = rc.run_oracle(orc, stage, params, arrays, quirks=False)
        rc.check_q7(name, want["cost_l"].shape, ref, rc.views_of(name, clean), rc.views_of(name, want), rc.TOL[stage],
                    "recorded reference vs oracle")


def test_recorded_nonfinite_cases_hold_what_they_are_for(recorded):
    """The FLT_MAX-run case really overflows inside one window, and only there: the reference poisons the windows that contain
    the markers (d_ca_cross_sum.cu:189-194, 284-289), not whole tiles."""
    for name in ("agg_rand_160x64_D8_fltmax_run", "agg_bud_96x64_D6_inf_nan"):
        got = _of(recorded, name)
        vals = np.concatenate([v.reshape(-1) for k, v in got.items() if k.startswith("acost")])
        assert (~np.isfinite(vals)).any() and np.isfinite(vals).mean() > 0.5

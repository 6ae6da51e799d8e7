"""Records what the reference's own kernels compute on the MI355X into tests/golden/ref_gfx950_*.npz.

The reference's programs, compiled for gfx950 (oracle/_ref/libstm_ref_hip.so, recipe oracle/build_ref.py), run every case of
tests/ref_cases.py in a child process each; what is kept is ref_cases.views_of() of their outputs (small maps whole, of a volume
a fixed seeded sample plus the d = 0 plane), keyed "<case>/<output>".  The inputs are not stored: tests/ref_cases.py rebuilds
them from the committed fixtures and seeds, and the parameters live in its CASES table.  Files are split below the size limit for
a committed file; conftest.load_golden("ref_gfx950") merges them.  tests/test_oracle_vs_reference.py compares the oracle with
these vectors on any machine.

It also measures max |reference - oracle| and the number of differing elements per case and output and writes them next to the
fixtures as ref_parity_measured.json (the source of profiles/ref_parity.json and of ref_cases.MEASURED_MAX).

Run on a machine with an MI355X, from the repo root:  python tests/golden/make_golden_ref.py [--dir OUT_DIR] [--new]
It stops at the first child that ends abnormally and starts nothing after it.

--new records only the cases of ref_cases.CASES that tests/golden/ has no vector for yet, into files of their own with the next
part numbers; ref_parity_measured.json then holds their measurements only.  The recorded files stay as they are, byte for byte.
"""
import glob
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stm_amd  # noqa: E402,F401
import ref_cases as rc  # noqa: E402
from oracle import pyoracle as orc  # noqa: E402
from oracle import pyref  # noqa: E402

LIMIT = 900 * 1024


def main(argv):
    out_dir = argv[argv.index("--dir") + 1] if "--dir" in argv else os.path.join(ROOT, "tests", "golden")
    os.makedirs(out_dir, exist_ok=True)
    assert pyref.available(), "oracle/_ref/libstm_ref_hip.so is missing"
    recorded, measured = {}, {}
    only_new = "--new" in argv
    golden = os.path.join(ROOT, "tests", "golden")
    cases = rc.CASES + rc.GPU_ONLY_CASES
    if only_new:
        have = set()
        for f in glob.glob(os.path.join(golden, "ref_gfx950_*.npz")):
            have |= {k.split("/", 1)[0] for k in np.load(f).files}
        cases = [c for c in rc.CASES if c[0] not in have]
        print("--new: %s" % [c[0] for c in cases], flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        for name, stage, params, build in cases:
            arrays = build(orc, params)
            status, ref, tail = rc.reference_child(tmp, stage, params, arrays, tag=name)
            if status != 0:
                print("STOP: reference child for %s ended with status %d\n%s" % (name, status, tail), flush=True)
                return 1
            want = rc.run_oracle(orc, stage, params, arrays)
            m = {}
            for k in sorted(ref):
                g, w = ref[k], want[k]
                fin = np.isfinite(g.astype(np.float64)) & np.isfinite(w.astype(np.float64))
                m[k] = {"max_abs_diff": rc.max_abs_diff(g[fin], w[fin]), "differing": int((~rc_eq(g, w)).sum()),
                        "elements": int(g.size),
                        "nonfinite_at_same_places": bool(np.array_equal(np.isfinite(g.astype(np.float64)), np.isfinite(w.astype(np.float64))))}
            measured[name] = {"stage": stage, "outputs": m}
            print(name, json.dumps(m), flush=True)
            if name in rc.CASE_IDS:  # the large GPU-only cases are measured, not recorded
                for k, v in rc.views_of(name, ref).items():
                    recorded[name + "/" + k] = v
    if only_new:
        part = len(glob.glob(os.path.join(golden, "ref_gfx950_*.npz")))  # the parts are numbered from 0 without gaps
    else:
        for f in glob.glob(os.path.join(out_dir, "ref_gfx950_*.npz")):
            os.remove(f)
        part = 0
    first, group, size = part, {}, 0

    def flush():
        nonlocal part, group, size
        if group:
            np.savez_compressed(os.path.join(out_dir, "ref_gfx950_%02d.npz" % part), **group)
            assert os.path.getsize(os.path.join(out_dir, "ref_gfx950_%02d.npz" % part)) < 1024 * 1024
            part, group, size = part + 1, {}, 0

    for k in sorted(recorded):
        if size + recorded[k].nbytes > LIMIT:
            flush()
        group[k] = recorded[k]
        size += recorded[k].nbytes
    flush()
    with open(os.path.join(out_dir, "ref_parity_measured.json"), "w") as fh:
        json.dump(measured, fh, indent=1, sort_keys=True)
    print("recorded %d arrays in %d files" % (len(recorded), part - first))
    return 0


def rc_eq(g, w):
    """element equality with NaN == NaN"""
    if g.dtype.kind == "f":
        return (g == w) | (np.isnan(g) & np.isnan(w))
    return g == w


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

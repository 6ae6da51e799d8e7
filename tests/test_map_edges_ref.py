"""The oracle's map-taking stages on huge and non-finite disparities (tests/map_edge_cases.py), without a GPU.

1. Restatement: dr_dcc, dr_irv, filter_bilateral_1, filter_median, dibr_occl and dibr_dfm written again in numpy with 64-bit
   integers, which the sums of a saturated conversion and an image coordinate cannot overflow, from the rules of
   include/stm_hip.h ("Map values a stage cannot place"): every float -> int of a map value is f2i_sat, the target column is
   clamp(x +- f2i_sat(v), 0, W - 1) taken without overflow, the bilateral's table index is min(f2i_sat(|va - vs|), D - 1).
   Integer outputs must be equal, float outputs equal with NaNs compared by position.
2. Conditions on the inputs: the same restatements with every such sum wrapped to 32 bits (what a kernel that adds in a register
   computes) differ from the defined result on the cases, on an element with x > 0; every class of dr_dcc occurs; region voting
   accepts and rejects outliers that carry planted values; the bilateral's cases hold a NaN difference and one of 2^31 or more.
3. A stand-alone program (tools/oracle_map_edges.c) runs the oracle on the same cases under AddressSanitizer and UBSan with
   -fsanitize=float-cast-overflow, which a plain (int) of such a value trips.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import map_edge_cases as mc
from map_edge_cases import f2i_sat, same, wrap32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFTS = [0.0, 0.4, 1.0, -1.0]
BIL = [(7, 5.0, 10.0), (2, 1.5, 1.0)]
IRV_THRESH = [(0, 0.0), (4, 0.1), (0, 0.1), (4, 0.0)]


def _add(a, b, wrap):
    s = np.asarray(a, np.int64) + np.asarray(b, np.int64)
    return wrap32(s) if wrap else s


def _col(x, sd, W, wrap):
    return np.clip(_add(x, sd, wrap), 0, W - 1)


# ---------------------------------------------------------------- restatements
def dcc_py(dl, dr, wrap=False):
    H, W = dl.shape
    x = np.arange(W, dtype=np.int64)[None, :].repeat(H, 0)
    rows = np.arange(H)[:, None].repeat(W, 1)
    il, ir = f2i_sat(dl), f2i_sat(dr)
    cl, cr = _col(x, il, W, wrap), _col(x, -ir if not wrap else wrap32(-ir), W, wrap)
    with np.errstate(invalid="ignore", over="ignore"):
        out_l = (np.abs(dl - dr[rows, cl]) > np.float32(1.0)).astype(np.uint8)
        out_r = (np.abs(dr - dl[rows, cr]) > np.float32(1.0)).astype(np.uint8)
    hit_l, hit_r = np.ones((H, W), np.uint8), np.ones((H, W), np.uint8)
    hit_r[rows, cl] = 0
    hit_l[rows, cr] = 0
    out_l[(out_l == 1) & (hit_l == 1)] = 2
    out_r[(out_r == 1) & (hit_r == 1)] = 2
    return out_l, out_r


def occl_py(dl, dr, wrap=False):
    H, W = dl.shape
    x = np.arange(W, dtype=np.int64)[None, :].repeat(H, 0)
    rows = np.arange(H)[:, None].repeat(W, 1)
    ol, orr = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    orr[rows, _col(x, f2i_sat(dl * np.float32(1.0)), W, wrap)] = 1
    ol[rows, _col(x, f2i_sat(dr * np.float32(-1.0)), W, wrap)] = 1
    return ol, orr


def dfm_py(img_l, dl, shift, wrap=False):
    """sources in ascending x: of the sources that land on one target the largest x wins; three bytes per pixel are copied"""
    H, W, E = img_l.shape
    with np.errstate(invalid="ignore", over="ignore"):
        sd = f2i_sat(dl * np.float32(shift))
    out = np.zeros((H, W, E), np.uint8)
    rows = np.arange(H)
    for x in range(W):
        out[rows, _col(x, sd[:, x], W, wrap), :3] = img_l[:, x, :3]
    return out


def median_py(img):
    H, W = img.shape
    flat = img.reshape(-1)
    ty, tx = np.mgrid[0:H, 0:W]
    v = []
    for y in (-1, 0, 1):
        for x in (-1, 0, 1):
            q = np.clip((tx + x) + (ty + y) * W, 0, H * W - 1)   # flat index, no border rule; outside the buffer: clamped
            v.append(flat[q].copy())
    for i in range(9):
        cur = f2i_sat(v[i])
        for j in range(i, 9):
            comp = f2i_sat(v[j])
            m = comp < cur
            v[j] = np.where(m, cur.astype(np.float32), v[j])
            v[i] = np.where(m, comp.astype(np.float32), v[i])
            cur = np.where(m, comp, cur)
    return v[4].astype(np.float32)


def bilateral_py(orc, img, radius, sigma_color, sigma_spatial, D):
    """one f32 operation per line, taps in row-major order, as the oracle's loop states them"""
    H, W = img.shape
    sk = orc.gaussian_kernel_2d(radius, sigma_spatial)
    ck = orc.gaussian_kernel_1d(D, sigma_color)
    gy, gx = np.mgrid[0:H, 0:W]
    norm, res = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for y in range(-radius, radius + 1):
            sy = np.clip(gy + y, 0, H - 1)
            for x in range(-radius, radius + 1):
                vs = img[sy, np.clip(gx + x, 0, W - 1)]
                ci = np.minimum(f2i_sat(np.abs(img - vs)), D - 1)
                w = sk[y + radius, x + radius] * ck[ci]
                norm = norm + w
                t = vs * w
                res = res + t
        return (res / norm).astype(np.float32)


def _irv_vote_py(disp, outl, cross, D, zd, usd, wrap):
    H, W = disp.shape
    aU, aD, aL, aR = [cross[i].astype(np.int64) for i in range(4)]
    nb = max(D, 65)
    d = f2i_sat(disp)
    b = _add(d, zd, wrap)
    ys, xs = np.nonzero(outl)
    n = len(ys)
    idx = np.arange(n)
    cu, cd = np.minimum(aU[ys, xs], usd), aD[ys, xs]
    hist, total = np.zeros((n, nb), np.int64), np.zeros(n, np.int64)
    if n:
        assert (ys - cu).min() >= 0 and (ys + cd).max() <= H - 1   # arms of the image: the rows of a region exist
        for dy in range(-int(cu.max()), int(cd.max()) + 1):
            rowok = (dy >= -cu) & (dy <= cd)
            qy = np.clip(ys + dy, 0, H - 1)
            cl, cr = aL[qy, xs], aR[qy, xs]
            for dx in range(-int(aL.max()), int(aR.max()) + 1):
                sx = np.clip(xs + dx, 0, W - 1)
                rel = rowok & (dx >= -cl) & (dx <= cr) & (outl[qy, sx] == 0)
                bb = b[qy, sx]
                inr = rel & (bb >= 0) & (bb < nb)
                np.add.at(hist, (idx[inr], bb[inr]), 1)
                total += rel
    max_cnt = hist.max(1) if n else np.zeros(0, np.int64)
    max_d = np.where(max_cnt > 0, hist.argmax(1) - zd, d[ys, xs]) if n else np.zeros(0, np.int64)   # first of equal bins
    return ys, xs, max_d, max_cnt, total


def irv_py(disp, outl, cross, thresh_s, thresh_h, D, zd, usd, iterations, device_flavour, paper=False, wrap=False):
    disp, outl = disp.copy(), outl.copy()
    votes = None
    for _ in range(iterations):
        if device_flavour or votes is None:      # host flavour: one vote, `iterations` applies
            votes = _irv_vote_py(disp, outl, cross, D, zd, usd, wrap)
        ys, xs, max_d, max_cnt, total = votes
        still = outl[ys, xs] != 0
        num = (max_cnt if paper else _add(max_d, zd, wrap)).astype(np.float32)
        with np.errstate(invalid="ignore", divide="ignore"):
            ok = still & (total > thresh_s) & (num / total.astype(np.float32) > np.float32(thresh_h))
        outl[ys[ok], xs[ok]] = 0
        disp[ys[ok], xs[ok]] = max_d[ok].astype(np.float32)
    return disp, outl


# ---------------------------------------------------------------- 1. the oracle against the restatement
@pytest.mark.parametrize("H,W", mc.SHAPES)
def test_oracle_dcc_occl_dfm_equal_the_restatement(orc, H, W):
    il, ir = mc.images(H, W, 3)
    il4, ir4 = mc.images(H, W, 4)
    for n, (name, dl, dr, _) in enumerate(mc.pair_cases(H, W)):
        got, want = orc.dr_dcc(dl, dr), dcc_py(dl, dr)
        assert same(got[0], want[0]) and same(got[1], want[1]), name
        got, want = orc.dibr_occl(dl, dr), occl_py(dl, dr)
        assert same(got[0], want[0]) and same(got[1], want[1]), name
        for shift in SHIFTS:
            assert same(orc.dibr_dfm(il, ir, dl, dr, shift), dfm_py(il, dl, shift)), (name, shift)
        shift = SHIFTS[n % 4]
        assert same(orc.dibr_dfm(il4, ir4, dl, dr, shift), dfm_py(il4, dl, shift)), (name, shift, "elem_sz 4")


@pytest.mark.parametrize("H,W", mc.SHAPES)
def test_oracle_median_and_bilateral_equal_the_restatement(orc, H, W):
    for name, dl, dr, _ in mc.pair_cases(H, W):
        for m in (dl, dr):
            assert same(orc.filter_median(m), median_py(m)), name
    for name, dl, dr, _ in mc.pair_cases(H, W, whole=True):
        for (r, sc, ss) in BIL:
            assert same(orc.filter_bilateral_1(dl, r, sc, ss, mc.BIL_D), bilateral_py(orc, dl, r, sc, ss, mc.BIL_D)), (name, r)


@pytest.mark.parametrize("D,zd", mc.IRV_RANGES)
@pytest.mark.parametrize("H,W", mc.SHAPES)
def test_oracle_irv_equals_the_restatement(orc, H, W, D, zd):
    for n, (name, _, disp, outl, cross, _) in enumerate(mc.irv_cases(orc, H, W, D, zd)):
        ts, th = IRV_THRESH[n % 4]
        for (it, dev) in ((2, True), (3, False)):
            got = orc.dr_irv(disp, outl, cross, ts, th, D, zd, mc.USD, it, device_flavour=dev)
            want = irv_py(disp, outl, cross, ts, th, D, zd, mc.USD, it, dev)
            assert same(got[0], want[0]) and same(got[1], want[1]), (name, ts, th, it, dev)
    orc.set_irv_paper_ratio(1)
    try:
        for name, _, disp, outl, cross, _ in mc.irv_cases(orc, H, W, D, zd)[::7]:
            got = orc.dr_irv(disp, outl, cross, 0, 0.1, D, zd, mc.USD, 2, device_flavour=True)
            want = irv_py(disp, outl, cross, 0, 0.1, D, zd, mc.USD, 2, True, paper=True)
            assert same(got[0], want[0]) and same(got[1], want[1]), (name, "paper ratio")
    finally:
        orc.set_irv_paper_ratio(0)


# ---------------------------------------------------------------- 2. the cases see what they are for
def _differs_right_of_column_0(a, b):
    """(elements that differ, those of them with x > 0); the column is axis 1"""
    bad = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b)))) if a.dtype.kind == "f" else np.argwhere(a != b)
    return len(bad), int((bad[:, 1] > 0).sum()) if len(bad) else 0


def wrap_mutant_counts(orc):
    """per stage: (cases on which the 32-bit-sum restatement differs from the defined one, differing elements, those with x > 0)"""
    counts = {k: [0, 0, 0] for k in ("dcc", "occl", "dfm", "irv")}

    def tally(stage, pairs):
        n = nx = 0
        for a, b in pairs:
            k, kx = _differs_right_of_column_0(a, b)
            n, nx = n + k, nx + kx
        c = counts[stage]
        c[0], c[1], c[2] = c[0] + (n > 0), c[1] + n, c[2] + nx

    for H, W in mc.SHAPES:
        il, _ = mc.images(H, W, 3)
        for _, dl, dr, _ in mc.pair_cases(H, W):
            tally("dcc", zip(dcc_py(dl, dr), dcc_py(dl, dr, wrap=True)))
            tally("occl", zip(occl_py(dl, dr), occl_py(dl, dr, wrap=True)))
            tally("dfm", [(dfm_py(il, dl, s), dfm_py(il, dl, s, wrap=True)) for s in SHIFTS])
        for D, zd in mc.IRV_RANGES:
            for n, (_, _, disp, outl, cross, _) in enumerate(mc.irv_cases(orc, H, W, D, zd)):
                ts, th = IRV_THRESH[n % 4]
                tally("irv", zip(irv_py(disp, outl, cross, ts, th, D, zd, mc.USD, 2, True),
                                 irv_py(disp, outl, cross, ts, th, D, zd, mc.USD, 2, True, wrap=True)))
    return counts


def test_sums_wrapped_to_32_bits_change_every_stage(orc):
    """A restatement that adds in 32 bits gives another result than the defined one for dr_dcc, dibr_occl, dibr_dfm and dr_irv, and
    not only in column 0: the cases would catch a kernel that adds a saturated conversion to a coordinate in a register."""
    counts = wrap_mutant_counts(orc)
    print("wrap mutants (cases, elements, elements with x > 0):", counts)
    for stage, (cases, elements, right) in counts.items():
        assert cases > 0 and elements > 0 and right > 0, (stage, counts)


def test_every_dcc_class_occurs():
    seen = set()
    for H, W in mc.SHAPES:
        for _, dl, dr, _ in mc.pair_cases(H, W):
            for o in dcc_py(dl, dr):
                seen |= set(np.unique(o).tolist())
    assert seen == {0, 1, 2}


def test_irv_accepts_and_rejects_planted_outliers(orc):
    """among the outliers that carry a planted value (`own`, `alone`) some are accepted and some are not, in both ranges; and in a
    case whose planted values vote, an outlier is accepted and another is rejected"""
    for D, zd in mc.IRV_RANGES:
        acc = rej = vote_acc = vote_rej = 0
        for H, W in mc.SHAPES:
            for n, (_, kind, disp, outl, cross, planted) in enumerate(mc.irv_cases(orc, H, W, D, zd)):
                ts, th = IRV_THRESH[n % 4]
                _, o = orc.dr_irv(disp, outl, cross, ts, th, D, zd, mc.USD, 2, device_flavour=True)
                if kind == "vote":
                    vote_acc += int(((outl != 0) & (o == 0)).sum())
                    vote_rej += int((o != 0).sum())
                else:
                    for _, y, x, _ in planted:
                        acc += o[y, x] == 0
                        rej += o[y, x] != 0
        assert acc > 0 and rej > 0 and vote_acc > 0 and vote_rej > 0, (D, zd, acc, rej, vote_acc, vote_rej)


def test_bilateral_cases_hold_a_nan_and_a_huge_difference():
    nan = huge = inf = 0
    for H, W in mc.SHAPES:
        if W < 2:
            continue
        for _, dl, _, planted in mc.pair_cases(H, W, whole=True):
            for m, y, x, v in planted:
                if m != 0:
                    continue
                other = dl[y, x + 1] if x + 1 < W else dl[y, x - 1]      # a tap of the planted pixel's own window
                with np.errstate(invalid="ignore", over="ignore"):
                    diff = np.abs(np.float32(v) - other)
                nan += bool(np.isnan(diff))
                inf += bool(np.isinf(diff))
                huge += bool(diff >= 2147483648.0)
    assert nan > 0 and huge > 0 and inf > 0


# ---------------------------------------------------------------- 3. the oracle under the sanitizers
def write_sanitizer_cases(orc, d):
    """the cases as raw files and a list of runs, one per line, for tools/oracle_map_edges.c"""
    lines = []

    def put(name, arrs, dtype):
        a = np.ascontiguousarray(np.stack(arrs), dtype)
        a.tofile(os.path.join(d, name))
        return name

    for H, W in mc.SHAPES:
        tag = "%dx%d" % (H, W)
        frac, whole = mc.pair_cases(H, W), mc.pair_cases(H, W, whole=True)
        fl = put(tag + "_l.f32", [c[1] for c in frac], np.float32)
        fr = put(tag + "_r.f32", [c[2] for c in frac], np.float32)
        wl = put(tag + "_wl.f32", [c[1] for c in whole], np.float32)
        lines.append("bilateral %d %d %d %d %s" % (H, W, len(whole), mc.BIL_D, wl))   # first: the one conversion that indexed a table
        lines.append("pair %d %d %d %s %s" % (H, W, len(frac), fl, fr))
        for D, zd in mc.IRV_RANGES:
            cases = mc.irv_cases(orc, H, W, D, zd)
            t = "%s_D%d" % (tag, D)
            fd = put(t + "_disp.f32", [c[2] for c in cases], np.float32)
            fo = put(t + "_outl.u8", [c[3] for c in cases], np.uint8)
            fx = put(t + "_cross.u8", [cases[0][4]], np.uint8)
            lines.append("irv %d %d %d %d %d %d %s %s %s" % (H, W, len(cases), D, zd, mc.USD, fd, fo, fx))
    with open(os.path.join(d, "runs.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def test_oracle_under_sanitizers(orc, tmp_path):
    """gcc's `undefined` group leaves float-cast-overflow out, so it is named: an (int) of a NaN or of a value beyond +-2^31 is
    what this run is for.  Passes only when the program exits 0 and writes nothing to stderr."""
    gcc = shutil.which("gcc")
    asan = subprocess.run([gcc, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip() if gcc else ""
    if not gcc or not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("gcc -print-file-name=libasan.so finds no AddressSanitizer runtime")
    exe = str(tmp_path / "oracle_map_edges")
    subprocess.check_call([gcc, "-O1", "-g", "-fopenmp", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tools", "oracle_map_edges.c"), os.path.join(ROOT, "oracle", "stm_oracle.c"), "-lm"])
    cases = tmp_path / "cases"
    cases.mkdir()
    write_sanitizer_cases(orc, str(cases))
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", "exit %d\n%s" % (r.returncode, r.stderr[-3000:])
    assert r.stdout.startswith("ok:"), r.stdout

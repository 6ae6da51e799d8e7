"""The numpy statement of the rectification (include/stm_rectify.h): coords_ref is steps A to C, rectify_ref
the whole remap.  Tied here to a plain scalar loop, to known answers and to stm_amd.rectify's helpers; tests/test_gpu_rectify.py
compares the GPU with it bit for bit.  No GPU is needed here."""
import importlib.util
import math
import os

import numpy as np
import pytest

from conftest import ROOT

QMAX = np.float32(1048576.0)
SHAPES = [(1, 1), (1, 5), (2, 2), (3, 7), (5, 64), (5, 65), (4, 257), (9, 37), (33, 300)]


def identity():
    rec = np.zeros(18, np.float32)
    rec[[0, 4, 8, 9, 10]] = 1.0
    return rec


def coords_ref(rec, H, W):
    """steps A to C, one float32 operation per line.  Returns a dict: qu, qv (int32, 0 where not ok), ok, and the intermediates u,
    v and Wd the cases below are judged by"""
    c = np.asarray(rec, np.float32)
    assert c.shape == (18,)
    m00, m01, m02, m10, m11, m12, m20, m21, m22, fx, fy, cx, cy, k1, k2, p1, p2, k3 = c
    with np.errstate(all="ignore"):
        xf = np.tile(np.arange(W, dtype=np.float32), (H, 1))
        yf = np.tile(np.arange(H, dtype=np.float32)[:, None], (1, W))
        X = m00 * xf; t = m01 * yf; X = X + t; X = X + m02
        Y = m10 * xf; t = m11 * yf; Y = Y + t; Y = Y + m12
        Wd = m20 * xf; t = m21 * yf; Wd = Wd + t; Wd = Wd + m22
        xn = X / Wd; yn = Y / Wd
        xx = xn * xn; yy = yn * yn; xy = xn * yn; r2 = xx + yy
        rad = k3 * r2; rad = rad + k2; rad = rad * r2; rad = rad + k1; rad = rad * r2; rad = rad + np.float32(1)
        a = xy + xy; a = p1 * a; b = xx + xx; b = r2 + b; b = p2 * b; xd = xn * rad; xd = xd + a; xd = xd + b
        a = yy + yy; a = r2 + a; a = p1 * a; b = xy + xy; b = p2 * b; yd = yn * rad; yd = yd + a; yd = yd + b
        u = fx * xd; u = u + cx
        v = fy * yd; v = v + cy
        mu = u * np.float32(32); mu = mu + np.float32(0.5); mu = np.floor(mu)
        mv = v * np.float32(32); mv = mv + np.float32(0.5); mv = np.floor(mv)
        ok = (mu >= -QMAX) & (mu <= QMAX) & (mv >= -QMAX) & (mv <= QMAX)
    for arr in (X, Wd, xn, rad, xd, yd, u, v, mu, mv):
        assert arr.dtype == np.float32
    qu = np.where(ok, mu, 0).astype(np.int32)
    qv = np.where(ok, mv, 0).astype(np.int32)
    return {"qu": qu, "qv": qv, "ok": ok, "u": u, "v": v, "Wd": Wd}


def quv_ref(rec, H, W):
    """what stm_rectify_coords hands out: [H][W][2] int32, INT32_MIN twice where not ok"""
    c = coords_ref(rec, H, W)
    lo = np.int32(-2 ** 31)
    return np.stack([np.where(c["ok"], c["qu"], lo), np.where(c["ok"], c["qv"], lo)], axis=-1).astype(np.int32)


def rectify_ref(img, rec, border):
    """steps A to E: the [H][W][3] uint8 remap of img's first three channels"""
    assert border in (0, 1)
    H, W = img.shape[:2]
    src = np.asarray(img)[:, :, :3].astype(np.int64)
    c = coords_ref(rec, H, W)
    x0, y0 = (c["qu"] >> 5).astype(np.int64), (c["qv"] >> 5).astype(np.int64)
    fu, fv = (c["qu"] & 31).astype(np.int64)[..., None], (c["qv"] & 31).astype(np.int64)[..., None]

    def tap(ty, tx):
        inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        p = src[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)]
        return p if border == 1 else p * inside[..., None]
    top = (32 - fu) * tap(y0, x0) + fu * tap(y0, x0 + 1)
    bot = (32 - fu) * tap(y0 + 1, x0) + fu * tap(y0 + 1, x0 + 1)
    out = ((32 - fv) * top + fv * bot + 512) >> 10
    out[~c["ok"]] = 0
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def taps_outside(rec, H, W):
    """per side (left, right, top, bottom): whether an ok pixel has a tap beyond it"""
    c = coords_ref(rec, H, W)
    x0, y0, ok = c["qu"] >> 5, c["qv"] >> 5, c["ok"]
    return bool((ok & (x0 < 0)).any()), bool((ok & (x0 + 1 > W - 1)).any()), bool((ok & (y0 < 0)).any()), bool((ok & (y0 + 1 > H - 1)).any())


# ------------------------------------------------------------------------------------------------- the records of the GPU cases
def rot_z(deg):
    a = math.radians(deg)
    return np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])


def camera(f, cx, cy, ratio=1.0):
    return np.array([[f, 0.0, cx], [0.0, f * ratio, cy], [0.0, 0.0, 1.0]])


def case_records(H, W):
    """name -> record, the cases of tests/test_gpu_rectify.py; test_the_cases_do_what_their_names_say proves each on the statement"""
    from stm_amd import rectify
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    recs = {"identity": identity()}
    r = identity(); r[11], r[12] = 3.0, -2.0
    recs["shift 3 -2"] = r
    for name, v in (("cx +1/32", 1.0 / 32), ("cx -1/32", -1.0 / 32), ("cx +31/32", 31.0 / 32), ("cx -31/32", -31.0 / 32)):
        r = identity(); r[11] = v
        recs[name] = r
    f = float(max(W, 8))
    recs["roll 2"] = rectify.record(camera(f, cx, cy, 1.03), None, rot_z(2.0), camera(f, cx, cy))
    r = identity(); r[6] = np.float32(-1.0 / 18.0)
    recs["Wd crosses zero"] = r
    r = identity(); r[9] = 1.0e6
    recs["fx 1e6"] = r
    recs["barrel"] = rectify.record(camera(0.93 * W, cx, cy), [-0.2, 0.05, 1e-3, -2e-3, 0.01], np.eye(3), camera(0.75 * W, cx + 0.3, cy - 0.2))
    for r in recs.values():
        assert r.dtype == np.float32 and r.shape == (18,) and np.isfinite(r).all()
    return recs


def texture(H, W, seed, E=3):
    """smooth colour under noise, no two neighbours alike"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([40 + 5 * xx + 3 * yy, 200 - 2 * xx + 7 * yy, 90 + 11 * ((xx + yy) % 13)], axis=-1)
    img = np.full((H, W, E), 0xC3, np.uint8)
    img[:, :, :3] = ((base + rng.randint(0, 64, size=(H, W, 3))) % 256).astype(np.uint8)
    return img


# ------------------------------------------------------------------------------------------------- the statement against a scalar loop
def _scalar(img, c, border):
    f = np.float32
    H, W = img.shape[:2]
    out = np.zeros((H, W, 3), np.uint8)
    quv = np.zeros((H, W, 2), np.int64)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                xf, yf = f(x), f(y)
                X = c[0] * xf; t = c[1] * yf; X = f(X + t); X = f(X + c[2])
                Y = c[3] * xf; t = c[4] * yf; Y = f(Y + t); Y = f(Y + c[5])
                Wd = c[6] * xf; t = c[7] * yf; Wd = f(Wd + t); Wd = f(Wd + c[8])
                xn = f(X / Wd); yn = f(Y / Wd)
                xx = f(xn * xn); yy = f(yn * yn); xy = f(xn * yn); r2 = f(xx + yy)
                rad = f(c[17] * r2); rad = f(rad + c[14]); rad = f(rad * r2); rad = f(rad + c[13]); rad = f(rad * r2); rad = f(rad + f(1))
                a = f(xy + xy); a = f(c[15] * a); b = f(xx + xx); b = f(r2 + b); b = f(c[16] * b)
                xd = f(xn * rad); xd = f(xd + a); xd = f(xd + b)
                a = f(yy + yy); a = f(r2 + a); a = f(c[15] * a); b = f(xy + xy); b = f(c[16] * b)
                yd = f(yn * rad); yd = f(yd + a); yd = f(yd + b)
                u = f(c[9] * xd); u = f(u + c[11]); v = f(c[10] * yd); v = f(v + c[12])
                mu = f(u * f(32)); mu = f(mu + f(0.5)); mu = f(math.floor(mu)) if np.isfinite(mu) else mu
                mv = f(v * f(32)); mv = f(mv + f(0.5)); mv = f(math.floor(mv)) if np.isfinite(mv) else mv
                if not (mu >= -QMAX and mu <= QMAX and mv >= -QMAX and mv <= QMAX):
                    quv[y, x] = -2 ** 31
                    continue
                qu, qv = int(mu), int(mv)
                quv[y, x] = (qu, qv)
                x0, fu, y0, fv = qu >> 5, qu & 31, qv >> 5, qv & 31

                def tap(ty, tx, ch):
                    if border == 0 and not (0 <= tx < W and 0 <= ty < H):
                        return 0
                    return int(img[min(max(ty, 0), H - 1), min(max(tx, 0), W - 1), ch])
                for ch in range(3):
                    top = (32 - fu) * tap(y0, x0, ch) + fu * tap(y0, x0 + 1, ch)
                    bot = (32 - fu) * tap(y0 + 1, x0, ch) + fu * tap(y0 + 1, x0 + 1, ch)
                    out[y, x, ch] = ((32 - fv) * top + fv * bot + 512) >> 10
    return out, quv


@pytest.mark.parametrize("name", ["barrel", "roll 2", "Wd crosses zero", "cx -31/32"])
def test_the_statement_is_the_scalar_loop(name):
    H, W = 7, 23
    rec = case_records(H, W)[name]
    img = texture(H, W, 3)
    for border in (0, 1):
        out, quv = _scalar(img, rec, border)
        assert np.array_equal(rectify_ref(img, rec, border), out), (name, border)
        assert np.array_equal(quv_ref(rec, H, W), quv), name


def test_the_library_module_states_the_same_chain():
    from stm_amd import rectify
    for (H, W) in [(9, 37), (5, 65)]:
        for name, rec in case_records(H, W).items():
            qu, qv, ok = rectify.coords(rec, H, W)
            c = coords_ref(rec, H, W)
            assert np.array_equal(qu, c["qu"]) and np.array_equal(qv, c["qv"]) and np.array_equal(ok, c["ok"]), name
    assert np.array_equal(rectify.identity(), identity())


# ------------------------------------------------------------------------------------------------- known answers
def test_the_identity_is_a_copy():
    for (H, W) in SHAPES:
        img = texture(H, W, H + W, 4)
        for border in (0, 1):
            assert np.array_equal(rectify_ref(img, identity(), border), img[:, :, :3])
        c = coords_ref(identity(), H, W)
        assert c["ok"].all() and not (c["qu"] & 31).any() and not (c["qv"] & 31).any()


def test_half_scale_doubles_the_width():
    H, W = 5, 40
    img = texture(H, W, 1)
    rec = identity(); rec[0] = 0.5
    out = rectify_ref(img, rec, 1)
    a = img[:, :, :3].astype(np.int32)
    assert np.array_equal(out[:, 0::2], a[:, :W // 2])  # even columns are copies
    assert np.array_equal(out[:, 1::2], (a[:, :W // 2] + a[:, 1:W // 2 + 1] + 1) >> 1)  # odd columns are (a + b + 1) >> 1


def test_a_flat_image_stays_flat_with_the_clamped_border():
    for (H, W) in [(9, 37), (33, 300)]:
        flat = np.full((H, W, 3), (17, 130, 251), np.uint8)
        for name, rec in case_records(H, W).items():
            ok = coords_ref(rec, H, W)["ok"]
            out = rectify_ref(flat, rec, 1)
            assert np.array_equal(out[ok], flat[ok]), name
            assert not out[~ok].any(), name


def test_integer_translations():
    H, W = 9, 37
    img = texture(H, W, 2)[:, :, :3]
    for (dx, dy) in [(3, -2), (-5, 4), (0, 8), (36, 0), (40, 0)]:
        rec = identity(); rec[11], rec[12] = dx, dy
        ys, xs = np.arange(H)[:, None] + dy, np.arange(W)[None, :] + dx
        inside = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
        moved = img[np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)]
        assert np.array_equal(rectify_ref(img, rec, 1), moved), (dx, dy)
        assert np.array_equal(rectify_ref(img, rec, 0), moved * inside[..., None]), (dx, dy)


def test_not_ok_pixels_are_zero_with_either_border():
    H, W = 9, 37
    img = texture(H, W, 4)
    for bad in (np.float32(2.0 ** 15 + 1), np.float32(-(2.0 ** 15) - 1)):  # just beyond +-2^20 / 32
        rec = identity(); rec[11] = bad
        assert not coords_ref(rec, H, W)["ok"][:, 0].any()
        for border in (0, 1):
            assert not rectify_ref(img, rec, border)[:, 0].any()
    rec = identity(); rec[11] = np.float32(2.0 ** 15) - np.float32(W)  # the last ok value: mu = 2^20 at the last column
    c = coords_ref(rec, H, W)
    assert c["ok"].all() and c["qu"].max() < 2 ** 20
    rec = identity(); rec[11] = np.float32(2.0 ** 15)
    c = coords_ref(rec, H, W)
    assert c["ok"][:, 0].all() and c["qu"][0, 0] == 2 ** 20 and not c["ok"][:, 1:].any()
    assert (quv_ref(rec, H, W)[:, 1:] == -2 ** 31).all()


def test_the_cases_do_what_their_names_say():
    for (H, W) in [(9, 37), (33, 300)]:
        recs = case_records(H, W)
        for name, frac in (("cx +1/32", 1), ("cx -1/32", 31), ("cx +31/32", 31), ("cx -31/32", 1)):
            c = coords_ref(recs[name], H, W)
            assert ((c["qu"] & 31) == frac).all() and (c["qu"].min() < 0) == ("-" in name), name
        c = coords_ref(recs["Wd crosses zero"], H, W)
        assert (~np.isfinite(c["u"])).any() and (c["Wd"] < 0).all(axis=0).any() and c["ok"].any() and not c["ok"].all()
        c = coords_ref(recs["fx 1e6"], H, W)
        assert np.isfinite(c["u"]).all() and np.array_equal(c["ok"], c["u"] == recs["fx 1e6"][11]) and c["ok"].any() and not c["ok"].all()
        for name in ("barrel", "roll 2"):
            c = coords_ref(recs[name], H, W)
            assert c["ok"].all(), name
            assert len(set((c["qu"] & 31).ravel().tolist())) > 8 and len(set((c["qv"] & 31).ravel().tolist())) > 8, name
            assert any(taps_outside(recs[name], H, W)), name
        c = coords_ref(recs["shift 3 -2"], H, W)
        assert (c["qu"][0] == 32 * (np.arange(W) + 3)).all() and (c["qv"][:, 0] == 32 * (np.arange(H) - 2)).all()


# ------------------------------------------------------------------------------------------------- stm_amd.rectify
def test_record_of_a_pure_roll():
    """K = newK = [[f, 0, cx], [0, f, cy], [0, 0, 1]], R a roll by t: inv(K R) = R^T K^-1, by hand"""
    from stm_amd import rectify
    f, cx, cy, t = 50.0, 20.0, 10.0, math.radians(30.0)
    K = camera(f, cx, cy)
    rec = rectify.record(K, [0.1, -0.02], rot_z(30.0), K)
    co, si = math.cos(t), math.sin(t)
    rows = [[co / f, si / f, (-co * cx - si * cy) / f], [-si / f, co / f, (si * cx - co * cy) / f], [0.0, 0.0, 1.0]]
    want = np.array(sum(rows, []) + [f, f, cx, cy, 0.1, -0.02, 0.0, 0.0, 0.0])
    assert rec.dtype == np.float32 and rec.shape == (18,)
    assert np.allclose(rec, want, rtol=1e-6, atol=1e-9)
    assert np.array_equal(rectify.record(K, None, np.eye(3), K)[9:], np.array([f, f, cx, cy, 0, 0, 0, 0, 0], np.float32))
    with pytest.raises(ValueError):
        rectify.record(K, [0.0] * 8, np.eye(3), K)  # the rational model is not this one
    with pytest.raises(ValueError):
        rectify.record(K, None, np.eye(3), np.zeros((3, 3)) + np.nan)


def _brute_inner_rect(good):
    H, W = good.shape
    best, rect = 0, (0, 0, 0, 0)
    s = np.zeros((H + 1, W + 1), np.int64)
    s[1:, 1:] = good.cumsum(0).cumsum(1)
    for b in range(1, H + 1):
        for l in range(W):
            for t in range(b):
                for r in range(l + 1, W + 1):
                    area = (b - t) * (r - l)
                    if area > best and s[b, r] - s[t, r] - s[b, l] + s[t, l] == area:
                        best, rect = area, (t, b, l, r)
    return best, rect


def test_inner_rect_against_brute_force():
    from stm_amd import rectify
    for (H, W) in [(9, 37), (7, 12)]:
        for name, rec in case_records(H, W).items():
            c = coords_ref(rec, H, W)
            x0, y0 = c["qu"] >> 5, c["qv"] >> 5
            good = c["ok"] & (x0 >= 0) & (x0 + 1 <= W - 1) & (y0 >= 0) & (y0 + 1 <= H - 1)
            t, b, l, r = rectify.inner_rect(rec, H, W)
            area, _ = _brute_inner_rect(good)
            assert (b - t) * (r - l) == area, (name, H, W)
            assert area == 0 or good[t:b, l:r].all(), name
    assert rectify.inner_rect(identity(), 9, 37) == (0, 8, 0, 36)  # the last row and column have taps beyond the eye
    bad = identity(); bad[11] = 1.0e9
    assert rectify.inner_rect(bad, 4, 5) == (0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------- the two drivers
def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_take_rectify_option(tmp_path):
    from stm_amd import video
    good = str(tmp_path / "good.npy")
    np.save(good, np.stack([identity(), identity()]))
    argv = ["x", "--rectify", good, "1", "y"]
    rec_l, rec_r, border = video.take_rectify_option(argv)
    assert argv == ["x", "y"] and border == 1 and np.array_equal(rec_l, identity()) and np.array_equal(rec_r, identity())
    argv = ["x", "--rectify", good]
    assert video.take_rectify_option(argv)[2] == 0 and argv == ["x"]
    assert video.take_rectify_option(["x"]) is None


def test_the_tools_refuse_a_malformed_rectify_option(tmp_path, capsys):
    good, shape, dtype, nan, text = (str(tmp_path / n) for n in ("good.npy", "shape.npy", "dtype.npy", "nan.npy", "text.npy"))
    np.save(good, np.stack([identity(), identity()]))
    np.save(shape, np.zeros((18,), np.float32))
    np.save(dtype, np.zeros((2, 18), np.float64))
    bad = np.stack([identity(), identity()]); bad[1, 13] = np.nan
    np.save(nan, bad)
    open(text, "w").write("not an array")
    plane = str(tmp_path / "plane.npy")
    np.save(plane, np.zeros((2, 4, 6), np.uint8))
    vid, img = _tool("stm_video"), _tool("stm_image")
    for tail in (["--rectify"], ["--rectify", shape], ["--rectify", dtype], ["--rectify", nan], ["--rectify", text],
                 ["--rectify", str(tmp_path / "missing.npy")], ["--rectify", good, "2"]):
        assert vid.main(["stm_video"] + ["x"] * 16 + tail) == -1, tail  # (no frame directory "x" exists: nothing was read)
        assert "--rectify FILE.npy" in capsys.readouterr().out
        assert img.main(["stm_image"] + ["x"] * 17 + tail) == -1, tail
        assert "--rectify FILE.npy" in capsys.readouterr().out
    assert vid.main(["stm_video"] + ["x"] * 16 + ["--depth-input", plane, "0", "16", "--rectify", good]) == -1
    capsys.readouterr()

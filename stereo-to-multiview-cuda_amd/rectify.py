"""Rectification records (include/stm_rectify.h): from a camera calibration to the 18 floats an eye is remapped with, and what the
remap leaves of the picture.  numpy only: nothing here needs the library or a GPU.

A record is m00 .. m22 (rectified pixel to camera ray, the inverse of newK * R), fx fy cx cy (the camera matrix of the unrectified
image) and k1 k2 p1 p2 k3 (Brown-Conrady).  host_api.rectify / device_api.d_rectify apply one to an image,
video.FrameStream(rectify=(rec_l, rec_r, border)) one per eye to every frame."""
import numpy as np

RECORD_FLOATS = 18
QMAX = 1048576.0  # |mu|, |mv| beyond it: the pixel is not ok


def record(K, dist, R, newK):
    """The record of one camera: K its 3 x 3 camera matrix, dist its distortion coefficients in OpenCV's order (k1, k2, p1, p2[,
    k3]; None or shorter: zeros), R the 3 x 3 rectifying rotation and newK the 3 x 3 camera matrix of the rectified image (what
    cv2.stereoRectify returns as R1 / R2 and the left 3 x 3 of P1 / P2).  The inverse is taken in float64.  Returns 18 float32."""
    K, R, newK = (np.asarray(a, np.float64).reshape(3, 3) for a in (K, R, newK))
    d = np.zeros(5, np.float64)
    if dist is not None:
        given = np.asarray(dist, np.float64).ravel()
        if given.size > 5:
            raise ValueError("rectify.record: %d distortion coefficients: only k1, k2, p1, p2, k3 are modelled" % given.size)
        d[:given.size] = given
    m = np.linalg.inv(newK @ R)
    rec = np.concatenate([m.ravel(), [K[0, 0], K[1, 1], K[0, 2], K[1, 2]], d]).astype(np.float32)
    if not np.isfinite(rec).all():
        raise ValueError("rectify.record: the record is not finite")
    return rec


def identity():
    """The record that copies: m = I, fx = fy = 1, everything else 0."""
    rec = np.zeros(RECORD_FLOATS, np.float32)
    rec[[0, 4, 8, 9, 10]] = 1.0
    return rec


def check(rec, what="record"):
    """rec as 18 finite float32, or ValueError."""
    rec = np.asarray(rec)
    if rec.shape != (RECORD_FLOATS,) or rec.dtype.kind != "f":
        raise ValueError("rectify: a %s is 18 floats, got %s %s" % (what, rec.dtype, rec.shape))
    rec = rec.astype(np.float32)
    if not np.isfinite(rec).all():
        raise ValueError("rectify: the %s has a float that is not finite" % what)
    return np.ascontiguousarray(rec)


def load_records(path):
    """The (2, 18) float32 array of a .npy file: the left eye's record, then the right eye's.  ValueError for anything else."""
    try:
        a = np.load(path, allow_pickle=False)
    except Exception as e:  # noqa: BLE001 (whatever numpy makes of a malformed file)
        raise ValueError("%s: not a .npy file of records (%s)" % (path, e))
    if a.shape != (2, RECORD_FLOATS) or a.dtype != np.float32:
        raise ValueError("%s: records are a (2, 18) float32 array, got %s %s" % (path, a.dtype, a.shape))
    return check(a[0], "left record"), check(a[1], "right record")


def coords(rec, H, W):
    """Steps A to C of the definition for every pixel of an H x W eye, operation by operation in float32: (qu, qv, ok), int32
    [H][W] each and a bool mask; qu and qv are 0 where not ok."""
    c = check(rec)
    f = np.float32
    with np.errstate(all="ignore"):
        xf = np.broadcast_to(np.arange(W, dtype=f)[None, :], (H, W))
        yf = np.broadcast_to(np.arange(H, dtype=f)[:, None], (H, W))

        def row(a, b, d):
            X = a * xf
            t = b * yf
            X = X + t
            return X + d
        X, Y, Wd = row(c[0], c[1], c[2]), row(c[3], c[4], c[5]), row(c[6], c[7], c[8])
        xn = X / Wd
        yn = Y / Wd
        xx = xn * xn
        yy = yn * yn
        xy = xn * yn
        r2 = xx + yy
        rad = c[17] * r2
        rad = rad + c[14]
        rad = rad * r2
        rad = rad + c[13]
        rad = rad * r2
        rad = rad + f(1)
        a = xy + xy
        a = c[15] * a
        b = xx + xx
        b = r2 + b
        b = c[16] * b
        xd = xn * rad
        xd = xd + a
        xd = xd + b
        a = yy + yy
        a = r2 + a
        a = c[15] * a
        b = xy + xy
        b = c[16] * b
        yd = yn * rad
        yd = yd + a
        yd = yd + b
        u = c[9] * xd
        u = u + c[11]
        v = c[10] * yd
        v = v + c[12]
        mu = np.floor(u * f(32) + f(0.5))
        mv = np.floor(v * f(32) + f(0.5))
        ok = (mu >= -QMAX) & (mu <= QMAX) & (mv >= -QMAX) & (mv <= QMAX)
    assert mu.dtype == np.float32 and mv.dtype == np.float32
    qu = np.where(ok, mu, 0).astype(np.int32)
    qv = np.where(ok, mv, 0).astype(np.int32)
    return qu, qv, ok


def inner_rect(rec, H, W):
    """(top, bottom, left, right): rows [top, bottom), columns [left, right) of the largest axis-aligned rectangle of output pixels
    that are ok and whose four taps all lie inside the H x W eye -- what the remap fills with picture under either border, and what
    a caller hands to FrameStream(active=...).  Computed from the definition; the first of the largest in row-major order of
    (bottom, left).  (0, 0, 0, 0) where no pixel qualifies."""
    qu, qv, ok = coords(rec, H, W)
    x0, y0 = qu >> 5, qv >> 5
    good = ok & (x0 >= 0) & (x0 + 1 <= W - 1) & (y0 >= 0) & (y0 + 1 <= H - 1)
    best, rect = 0, (0, 0, 0, 0)
    height = np.zeros(W, np.int64)
    for y in range(H):
        height = np.where(good[y], height + 1, 0)
        stack = []  # (start column, height): the histogram's largest rectangle
        for x in range(W + 1):
            h = int(height[x]) if x < W else 0
            start = x
            while stack and stack[-1][1] >= h:
                s, sh = stack.pop()
                if sh * (x - s) > best:
                    best, rect = sh * (x - s), (y + 1 - sh, y + 1, s, x)
                start = s
            stack.append((start, h))
    return rect

"""CPU checks of the inputs of the scanline optimisation's path-cost tests (tests/hslo_cases.py): the walk-geometry cases reach every
width and height in every kernel form, the class counter agrees with a scalar restatement, and the images are what they claim."""
import numpy as np

import hslo_cases as hc


def test_the_geometry_cases_cover_every_width_and_height_per_form():
    for form in hc.FORMS:
        assert sorted({W for f, _, W in hc.GEO if f == form}) == hc.GEO_W and sorted({H for f, H, _ in hc.GEO if f == form}) == hc.GEO_H
    assert any(hc.geo_can_cover(H, W) for _, H, W in hc.GEO) and not hc.geo_can_cover(1, 38) and not hc.geo_can_cover(17, 1)


def test_the_geometry_cases_that_can_cover_do():
    for form, H, W in hc.GEO:
        if hc.geo_can_cover(H, W):
            D, zd = hc.GEO_D[form]
            own, other = hc.covering_images(H, W, D, zd, 200 + 7 * H + W)
            for osign in (1, -1):
                hc.assert_all_class_pairs(own, other, D, zd, osign)


def test_class_counts_against_a_scalar_loop():
    H, W, D, zd, T = 4, 7, 5, 1, 15.0
    own, other = hc.palette_image(H, W, 3), hc.palette_image(H, W, 4)
    mo, mt = hc.means(own, other)

    def cls(a, b):
        s = abs(np.float32(a) - np.float32(b))
        return 0 if s < T else 1 if s > T else 2

    for osign in (1, -1):
        want = np.zeros((4, 3, 3), np.int64)
        for k, (dx, dy) in enumerate([(1, 0), (-1, 0), (0, 1), (0, -1)]):
            for y in range(H):
                for x in range(W):
                    px, py = x - dx, y - dy
                    if not (0 <= px < W and 0 <= py < H):
                        continue
                    for d in range(D):
                        o = osign * (d - zd)
                        qx, qpx = min(max(x + o, 0), W - 1), min(max(px + o, 0), W - 1)
                        want[k, cls(mo[y, x], mo[py, px]), cls(mt[y, qx], mt[py, qpx])] += 1
        assert np.array_equal(hc.class_counts(own, other, D, zd, osign, T), want)


def test_the_images_are_what_they_claim():
    img = hc.palette_image(9, 33, 1, elem_sz=4)
    assert set(np.unique(img[..., :3].astype(int).sum(axis=2))) <= set(hc.PALETTE)
    assert (img[..., 0] != img[..., 1]).any() and (img[..., 1] != img[..., 2]).any()  # not grey
    s = hc.unit_step_image(9, 33, 2)[..., :3].astype(int).sum(axis=2)
    assert (np.abs(np.diff(s, axis=0)) == 1).all() and (np.abs(np.diff(s, axis=1)) == 1).all()
    c = hc.cost_volume("planted", 200, 3, 5, 1)
    assert set(np.unique(np.argmin(c, axis=0))) <= {0, 63, 64, 127, 128, 199} and np.isfinite(c).all()

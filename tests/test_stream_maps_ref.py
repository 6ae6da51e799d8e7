"""The depth planes of a frame stream (stm_stream_maps, include/stm_hip.h) on the CPU: plane_ref, the numpy
float32 statement of the definition that tests/test_gpu_stream_maps.py holds the kernel to, against the definition read aloud one
value at a time -- below and above both limits, exact .5 ties, NaN and +-inf, both polarities, both formats."""
import numpy as np
import pytest

MAXCODE = {"u8": 255, "u16": 65535}
DTYPE = {"u8": np.uint8, "u16": np.dtype("<u2")}


def plane_k(fmt, lo, hi):
    """k of the definition: the host's, once per stream"""
    return np.float32(float(MAXCODE[fmt]) / (float(np.float32(hi)) - float(np.float32(lo))))


def plane_ref(disp, fmt, lo, hi):
    """The definition on a whole map, one float32 operation per line.  Returns uint8 or little-endian uint16 codes of disp's shape."""
    f = np.float32
    d = np.ascontiguousarray(disp, dtype=f)
    k = plane_k(fmt, lo, hi)
    with np.errstate(all="ignore"):
        t = (d - f(lo)).astype(f)
        t = (t * k).astype(f)
        t = np.fmax(t, f(0)).astype(f)  # a NaN leaves as 0: fmax returns the other operand
        t = np.fmin(t, f(MAXCODE[fmt])).astype(f)
        t = (t + f(0.5)).astype(f)
    assert t.dtype == f and np.isfinite(t).all()
    return t.astype(np.uint32).astype(DTYPE[fmt])  # truncation of a value in [0.5, maxcode + 0.5]


def plane_loop(disp, fmt, lo, hi):
    """The definition read aloud, one value at a time"""
    f = np.float32
    maxc = f(MAXCODE[fmt])
    k = f(float(MAXCODE[fmt]) / (float(f(hi)) - float(f(lo))))
    out = np.zeros(disp.shape, DTYPE[fmt])
    flat = out.reshape(-1)
    with np.errstate(all="ignore"):
        for n, d in enumerate(np.asarray(disp, f).reshape(-1)):
            t = f(f(d) - f(lo))
            t = f(t * k)
            t = f(0) if (np.isnan(t) or t < f(0)) else t  # fmaxf(t, 0): the other operand for a NaN
            t = maxc if t > maxc else t                   # fminf(t, maxcode)
            flat[n] = int(f(t + f(0.5)))
    return out


def tie_limits(fmt, reverse):
    """lo, hi with hi - lo = maxcode / 2, so that k is exactly 2 (-2 reversed) and every map value lo + (n + 0.5) / 2 lands on a tie"""
    span = MAXCODE[fmt] / 2.0
    return (-3.0 + span, -3.0) if reverse else (-3.0, -3.0 + span)


def plane_case(fmt, lo, hi, seed, shape=(23, 37)):
    """A random map around [lo, hi]: values inside, below and above both limits, the limits themselves, quarter steps (exact ties
    when k is +-2), NaN and +-inf"""
    rng = np.random.RandomState(seed)
    a, b = min(lo, hi), max(lo, hi)
    span = b - a
    d = (a - 0.25 * span + rng.rand(*shape) * 1.5 * span).astype(np.float32)
    flat = d.reshape(-1)
    n = flat.size
    q = rng.permutation(n)
    steps = rng.randint(0, int(4 * span) + 1, size=n // 4)
    flat[q[:n // 4]] = (a + steps / 4.0).astype(np.float32)  # quarter steps: with |k| == 2 every other one is a .5 tie
    flat[q[n // 4:n // 4 + 8]] = [lo, hi, np.nan, np.inf, -np.inf, a - 1000.0, b + 1000.0, -0.0]
    return d


@pytest.mark.parametrize("reverse", [False, True], ids=["lo<hi", "lo>hi"])
@pytest.mark.parametrize("fmt", ["u8", "u16"])
def test_plane_ref_is_the_definition_with_exact_ties(fmt, reverse):
    lo, hi = tie_limits(fmt, reverse)
    assert float(plane_k(fmt, lo, hi)) == (-2.0 if reverse else 2.0)
    d = plane_case(fmt, lo, hi, 11 + reverse)
    got = plane_ref(d, fmt, lo, hi)
    assert got.dtype == DTYPE[fmt] and got.shape == d.shape
    assert np.array_equal(got, plane_loop(d, fmt, lo, hi))
    with np.errstate(all="ignore"):
        t = (d.astype(np.float64) - lo) * float(plane_k(fmt, lo, hi))
        ties = np.isfinite(t) & (t > 0) & (t < MAXCODE[fmt]) & (t - np.floor(t) == 0.5)
    assert ties.sum() > 20  # the case holds exact ties, and each rounds up (t + 0.5 is exact there)
    assert np.array_equal(got[ties].astype(np.int64), (t[ties] + 0.5).astype(np.int64))
    # both clamps fire, and values in between exist
    assert got.min() == 0 and got.max() == MAXCODE[fmt] and ((got > 0) & (got < MAXCODE[fmt])).any()
    assert (d < min(lo, hi)).any() and (d > max(lo, hi)).any()
    # NaN -> 0 whatever the polarity; the infinities go to the ends the polarity gives them
    assert (got[np.isnan(d)] == 0).all() and np.isnan(d).any()
    assert (got[d == np.inf] == (0 if reverse else MAXCODE[fmt])).all() and (got[d == -np.inf] == (MAXCODE[fmt] if reverse else 0)).all()
    assert (got[d == np.float32(lo)] == 0).all() and (got[d == np.float32(hi)] == MAXCODE[fmt]).all()


@pytest.mark.parametrize("fmt", ["u8", "u16"])
@pytest.mark.parametrize("lo, hi", [(0.0, 16.0), (13.25, -2.5), (-4096.0, 4096.0), (1.0, 1.0 + 1.0 / 64.0)], ids=["0..16", "13.25..-2.5", "widest", "narrowest"])
def test_plane_ref_at_ordinary_limits(fmt, lo, hi):
    d = plane_case(fmt, lo, hi, 5)
    got = plane_ref(d, fmt, lo, hi)
    assert np.array_equal(got, plane_loop(d, fmt, lo, hi))
    assert got.min() == 0 and got.max() == MAXCODE[fmt]


def test_u16_codes_are_little_endian():
    got = plane_ref(np.array([[0.0, 1.0, 255.0, 256.0, 65535.0]], np.float32), "u16", 0.0, 65535.0)  # k == 1
    assert got.tobytes() == bytes([0, 0, 1, 0, 255, 0, 0, 1, 255, 255])

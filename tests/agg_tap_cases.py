"""Case builders shared by tests/test_agg_tap_ref.py (CPU oracle alone) and tests/test_gpu_agg_tap.py (the tap of stm_set_agg_tap on
the frame's aggregation chain): content whose arms take every length, volumes for the last horizontal pass whose winner a single
window element decides, and the mutations of an aggregated volume that a comparison of WTA maps has to notice."""
import numpy as np

# the frame calls' defaults: the arms of every case unless it names others
UCD, LCD, USD, LSD = 6.0, 20.0, 34, 17
EPS = 2.0 ** -10  # what a planted hypothesis is lowered by: 4 * 2 * 255 window elements of < 4 + EPS stay exact in 24 bits


def mondrian(H, W, seed):
    """uint8 [H][W][3]: random rectangles of 3 .. 69 pixels a side in random colours over a random ground, later ones over earlier
    ones.  Edges lie anywhere, so arms stop at every length from 1 to usd, and rectangles wider than usd let them run out."""
    rng = np.random.RandomState(seed)
    img = np.empty((H, W, 3), np.uint8)
    img[:] = rng.randint(0, 256, 3)
    for _ in range(max(12, (H * W) // 60)):
        h, w = rng.randint(3, 70, 2)
        y0, x0 = rng.randint(-h + 1, H), rng.randint(-w + 1, W)
        img[max(y0, 0):y0 + h, max(x0, 0):x0 + w] = rng.randint(0, 256, 3)
    return img


def mondrian_pair(H, W, seed=46):
    """(left, right): two mondrians of different seeds -- arms of every length in BOTH views; the pair supplies arms, not matches.
    46 is the first seed at which, at every shape the tests use, both views hold horizontal arms of every length 0 .. usd and (from
    37 rows on) vertical arms 0, lsd and usd; tests/test_agg_tap_ref.py asserts it."""
    return mondrian(H, W, seed), mondrian(H, W, seed + 1000)


def sbs_of(L, R):
    return np.ascontiguousarray(np.concatenate([L, R], axis=1))


def plant_offsets(D, H):
    """offsets `off` such that every d < D is the planted hypothesis (y + off) % D of some row y < H of some volume"""
    return list(range(0, D, H))


def planted_volume(D, H, W, off, seed=7):
    """float32 [D][H][W]: one plane of random integers 1 .. 4 repeated for every hypothesis, and in row y the hypothesis
    (y + off) % D lowered by EPS.  Every window sum is exact in float32; in every row the planted hypothesis wins by n * EPS < 0.07
    (n <= 2 * 255 window elements) and all others tie bit for bit.  off None: nothing planted, a whole volume of ties."""
    plane = np.random.RandomState(seed).randint(1, 5, size=(H, W)).astype(np.float32)
    vol = np.repeat(plane[None], D, axis=0)
    if off is not None:
        y = np.arange(H)
        vol[(y + off) % D, y, :] -= np.float32(EPS)
    return np.ascontiguousarray(vol)


def planted_volumes(D, H, W, seed=7):
    """[(name, volume)]: the planted volumes of all offsets, then the volume of ties"""
    return [("off%d" % off, planted_volume(D, H, W, off, seed)) for off in plant_offsets(D, H)] + [("ties", planted_volume(D, H, W, None, seed))]


def noise_volume(D, H, W, seed=11):
    """float32 [D][H][W] uniform in [1, 2), independent per element: window sums that are not exact, winners by narrow margins"""
    return np.ascontiguousarray(np.random.RandomState(seed).uniform(1.0, 2.0, size=(D, H, W)).astype(np.float32).clip(1.0, np.float32(2.0 - 2.0 ** -23)))


def px_perm(D):
    """pi of the pixel-major volumes as an index array: float L of a record holds hypothesis 16 (L % 4) + L // 4"""
    assert D == 64
    L = np.arange(64)
    return 16 * (L % 4) + L // 4


def window_mutations(D):
    """[(name, f(agg, src) -> mutated agg)] for an aggregated volume agg = agg_hpass(src): one window element dropped (-) or
    counted twice (+) at every column x % 16 == r of one hypothesis, r the first and the last column of a 16-pixel tile"""
    out = []
    for d in range(D):
        for r in (0, 15):
            for sign in (-1.0, 1.0):
                def f(agg, src, d=d, r=r, sign=sign):
                    m = agg.copy()
                    m[d, :, r::16] += np.float32(sign) * src[d, :, r::16]
                    return m
                out.append(("d%d_r%d_%s" % (d, r, "drop" if sign < 0 else "twice"), f))
    return out


def layout_mutations(D):
    """[(name, f(agg, src))]: the last plane takes its neighbour's values (a padding guard one too strict); for D = 64 the volume's
    planes permuted by pi and by pi after pi (a pixel-major record read in the wrong hypothesis order)"""
    def last_plane(agg, src):
        m = agg.copy()
        m[D - 1] = m[D - 2]
        return m
    out = [("plane_D-1_is_D-2", last_plane)]
    if D == 64:
        pi = px_perm(D)
        out += [("px_order_1", lambda agg, src: np.ascontiguousarray(agg[pi])), ("px_order_2", lambda agg, src: np.ascontiguousarray(agg[pi[pi]]))]
    return out


def argmin_blind_mutations():
    """[(name, f(cost, cross, h1, final) -> (h1', final'))]: three faults that WTA maps of ordinary content do not see
    (test_agg_tap_ref.py), applied to the oracle's volume after the first pass (h1' given: the rest of the chain is rerun on it) or
    to the final volume (final' given).  cost: the initial costs; cross: the view's arms [up, down, left, right]."""
    def short_window(cost, cross, h1, final):
        # every hypothesis: the first element of the window [x - armL, x + armR) dropped at the last column of every 16-pixel tile
        m = h1.copy()
        H, W = cost.shape[1:]
        ys, xs = np.meshgrid(np.arange(H), np.arange(15, W, 16), indexing="ij")
        a, n = xs - cross[2][ys, xs].astype(np.int64), cross[2][ys, xs].astype(np.int64) + cross[3][ys, xs]
        m[:, ys, xs] -= np.where(n > 0, cost[:, ys, np.maximum(a, 0)], np.float32(0.0))
        return m, None

    def one_high(cost, cross, h1, final):
        m = h1.copy()
        for d in (0, m.shape[0] // 2, m.shape[0] - 1):
            m[d, :, 95::96] *= np.float32(1.02)
        return m, None

    def lanes_off(cost, cross, h1, final):
        m = final.copy()
        m[3::16, :, 17::64] *= np.float32(1.01)
        return None, m
    return [("short_window", short_window), ("one_hypothesis_high", one_high), ("lanes_off", lanes_off)]

"""Inputs for the region-voting tests (tests/test_gpu_irv_runs.py), and a census of what the column-run vote kernel does with them.

make_case: one view's consistent inputs of dr_irv -- a piecewise-constant disparity with sparse noise, outliers (classes 1 and 2) in
vertical runs of random length, and four random arm planes clamped so that no arm leaves the image (aU <= y, aD <= H - 1 - y,
aL <= x, aR <= W - 1 - x).  With such arms the oracle's clamped reads and the kernel's clamped row segments are the same pixels, so
the two must agree bit for bit.

census: for a single-tile input (H, W <= 64) with thresh_h = 0.0 nothing is pruned, every outlier is listed, and with one view the
list's order is fully determined: column-major (stm_k_irv_compact_cm).  stm_k_irv_vote_cm hands a wave `chl` consecutive entries;
the census walks the list in those chunks and classifies every entry of iteration 0 the way the kernel's `if` does.  It is a
statement about the INPUTS (which branches of the kernel a case reaches), computed without the kernel.
"""
import numpy as np

CLASSES = ("first", "column", "no_overlap", "nd_ge_nrows", "nd_gt_64", "nd_zero", "remove_only", "add_only", "both")


def make_case(H, W, D, zd, seed, vmax=17, hmax=12, density=0.5, run_max=12, block=8, noise=0.05, up_max=None):
    """(disp float32 [H][W], outliers uint8 [H][W], cross uint8 [4][H][W] = up, down, left, right).  vmax / hmax: the longest
    vertical / horizontal arm; up_max: the longest up arm where it differs from vmax; density: the share of outlier pixels;
    run_max: the longest vertical outlier run."""
    rng = np.random.RandomState(seed)
    base = rng.randint(-zd, D - zd, size=(H // block + 1, W // block + 1))
    disp = np.kron(base, np.ones((block, block), np.int64))[:H, :W]
    speck = rng.random_sample((H, W)) < noise
    disp = np.where(speck, rng.randint(-zd, D - zd, size=(H, W)), disp).astype(np.float32)
    outl = np.zeros((H, W), np.uint8)
    gap_max = max(1, int(round(run_max * (1.0 - density) / max(density, 1e-6))))
    for x in range(W):
        y = -int(rng.randint(0, run_max + 1))  # a run may begin above the image: columns do not start in step
        while y < H:
            n = int(rng.randint(1, run_max + 1))
            a, b = min(max(y, 0), H), min(max(y + n, 0), H)
            outl[a:b, x] = rng.randint(1, 3, size=b - a)
            y += n + int(rng.randint(1, gap_max + 1))
    ys, xs = np.mgrid[0:H, 0:W]
    aU = np.minimum(rng.randint(0, (vmax if up_max is None else up_max) + 1, size=(H, W)), ys)
    aD = np.minimum(rng.randint(0, vmax + 1, size=(H, W)), H - 1 - ys)
    aL = np.minimum(rng.randint(0, hmax + 1, size=(H, W)), xs)
    aR = np.minimum(rng.randint(0, hmax + 1, size=(H, W)), W - 1 - xs)
    cross = np.ascontiguousarray(np.stack([aU, aD, aL, aR]).astype(np.uint8))
    return disp, outl, cross


def region_rows(cross, y, x, H, usd):
    """rows t0 .. t1 of the cross region of pixel (y, x): the up arm clamped to usd (d_dr_irv.cu:179-180), both to the image"""
    return y - min(int(cross[0, y, x]), usd, y), y + min(int(cross[1, y, x]), H - 1 - y)


def reliable_in_region(outl, cross, y, x, usd):
    """S0: the reliable pixels of the cross region of (y, x) before the first iteration"""
    H, W = outl.shape
    t0, t1 = region_rows(cross, y, x, H, usd)
    s = 0
    for q in range(t0, t1 + 1):
        a, b = max(x - int(cross[2, q, x]), 0), min(x + int(cross[3, q, x]), W - 1)
        s += int((outl[q, a:b + 1] == 0).sum())
    return s


def census(outl, cross, usd, chl, thresh_s):
    """{class: entries} for iteration 0 of stm_k_irv_vote_cm over a single-tile, unpruned, one-view list walked `chl` entries per
    wave.  "later": entries the first iteration skips (S0 <= thresh_s), which leave the kept histogram as it is; every other
    entry is counted from scratch (first of its chunk, another column, no common row, as many changed rows as the region has,
    more than 64 changed rows) or updates the histogram of the entry before (no row changes, rows only leave, rows only enter,
    both)."""
    H, W = outl.shape
    assert H <= 64 and W <= 64 and 1 <= chl <= 16
    entries = [(y, x) for x in range(W) for y in range(H) if outl[y, x]]
    out = dict.fromkeys(CLASSES + ("later",), 0)
    for i0 in range(0, len(entries), chl):
        have, rx, r0, r1 = False, 0, 0, 0
        for y, x in entries[i0:i0 + chl]:
            if reliable_in_region(outl, cross, y, x, usd) <= thresh_s:
                out["later"] += 1
                continue
            t0, t1 = region_rows(cross, y, x, H, usd)
            nrows = t1 - t0 + 1
            rem_top, add_top = max(min(t0, r1 + 1) - r0, 0), max(min(r0, t1 + 1) - t0, 0)
            rem_bot, add_bot = max(r1 - max(t1, r0 - 1), 0), max(t1 - max(r1, t0 - 1), 0)
            rem, add = rem_top + rem_bot, add_top + add_bot
            nd = rem + add
            if not have:
                k = "first"
            elif x != rx:
                k = "column"
            elif max(t0, r0) > min(t1, r1):
                k = "no_overlap"
            elif nd >= nrows:
                k = "nd_ge_nrows"
            elif nd > 64:
                k = "nd_gt_64"
            elif nd == 0:
                k = "nd_zero"
            elif add == 0:
                k = "remove_only"
            elif rem == 0:
                k = "add_only"
            else:
                k = "both"
            out[k] += 1
            have, rx, r0, r1 = True, x, t0, t1
    out["entries"] = len(entries)
    return out


def wide_rows_in_runs(outl, cross, usd, lo):
    """How many rows wider than `lo` pixels enter, and how many leave, the region between an outlier and the outlier directly
    below it in the same column (the rows an incremental update would add / remove): (entering, leaving)"""
    H, W = outl.shape
    width = np.minimum(cross[2].astype(int), np.arange(W)[None, :]) + np.minimum(cross[3].astype(int), W - 1 - np.arange(W)[None, :]) + 1
    enter = leave = 0
    for x in range(W):
        for y in range(H - 1):
            if outl[y, x] and outl[y + 1, x]:
                a0, a1 = region_rows(cross, y, x, H, usd)
                b0, b1 = region_rows(cross, y + 1, x, H, usd)
                if max(a0, b0) > min(a1, b1):
                    continue
                for q in list(range(a0, min(b0, a1 + 1))) + list(range(max(b1, a0 - 1) + 1, a1 + 1)):
                    leave += int(width[q, x] > lo)
                for q in list(range(b0, min(a0, b1 + 1))) + list(range(max(a1, b0 - 1) + 1, b1 + 1)):
                    enter += int(width[q, x] > lo)
    return enter, leave

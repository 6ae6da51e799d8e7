"""The shot-change detector's numpy statement (steps 1 - 4 of stm_cut_detect in include/stm_hip.h), its properties, and the default
threshold's derivation on the committed images.  No GPU: tests/test_gpu_cut.py compares the kernels with these functions."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

STATE_WORDS = 260
DEFAULT_THRESH = 370  # DESIGN section 25; video.CUT_DEFAULT and CUT_DEFAULT_THRESH of stm_common.h
SINCE_MAX = 1 << 30


def sig_ref(img):
    """step 1: the left eye's signature, 256 counts: sig[cell * 16 + bin] over a 4 x 4 grid of cells and 16 luma bins"""
    img = np.asarray(img)
    H, W = img.shape[:2]
    p = img[:, :, :3].astype(np.int64)
    Y = (p[:, :, 0] + 2 * p[:, :, 1] + p[:, :, 2]) >> 2
    cell = ((4 * np.arange(H, dtype=np.int64)) // H)[:, None] * 4 + ((4 * np.arange(W, dtype=np.int64)) // W)[None, :]
    return np.bincount((cell * 16 + (Y >> 4)).ravel(), minlength=256).astype(np.int64)


def decide_ref(sig, n, state, thresh_permille, min_gap):
    """steps 2 - 3 on a signature: returns the new state (int32, 260) -- state[1] is the cut flag, state[3] the score"""
    state = np.asarray(state, np.int32)
    assert state.shape == (STATE_WORDS,)
    old = state[4:].view(np.uint32).astype(np.int64)
    history = state[0] != 0 and int(old.sum()) == n
    score = (1000 * int(np.abs(sig - old).sum())) // (2 * n) if history else 1000
    since = min(int(state[2]) + 1, SINCE_MAX)
    cut = (not history) or (score >= thresh_permille and since >= min_gap)
    out = np.empty(STATE_WORDS, np.int32)
    out[:4] = (1, int(cut), 0 if cut else since, score)
    out[4:] = sig.astype(np.uint32).view(np.int32)
    return out


def detect_ref(img, state, thresh_permille=DEFAULT_THRESH, min_gap=1):
    """steps 1 - 3 on an image [H][W][>= 3]; None = a zeroed state"""
    img = np.asarray(img)
    st = np.zeros(STATE_WORDS, np.int32) if state is None else state
    return decide_ref(sig_ref(img), img.shape[0] * img.shape[1], st, thresh_permille, min_gap)


def resets_ref(words, cut):
    """step 4: on a cut every given word becomes 0; otherwise they stay"""
    return [0 if cut else w for w in words]


def score_ref(a, b):
    """the score of frame b after frame a"""
    return int(detect_ref(b, detect_ref(a, None))[3])


# ---------------------------------------------------------------- properties
def _noise(H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(H, W, 3)).astype(np.uint8)


@pytest.mark.parametrize("shape", [(4, 4), (5, 7), (16, 17), (37, 61), (67, 130)])
def test_signature_sums_to_n_and_fills_cells(shape):
    H, W = shape
    s = sig_ref(_noise(H, W, 1))
    assert int(s.sum()) == H * W
    assert (s.reshape(16, 16).sum(axis=1) > 0).all()  # H, W >= 4: no cell is empty


def test_signature_bins():
    img = np.zeros((8, 8, 3), np.uint8)
    img[:, :, 0], img[:, :, 1], img[:, :, 2] = 10, 200, 90  # Y = (10 + 400 + 90) >> 2 = 125, bin 7
    s = sig_ref(img).reshape(16, 16)
    assert (s[:, 7] == 4).all() and int(s.sum()) == 64


def test_equal_frames_score_zero():
    img = _noise(37, 61, 2)
    st = detect_ref(img, None)
    assert tuple(st[:4]) == (1, 1, 0, 1000)  # no history: a cut, score 1000
    st = detect_ref(img, st)
    assert tuple(st[:4]) == (1, 0, 1, 0)


def test_state_of_another_size_is_no_history():
    st = detect_ref(_noise(16, 16, 3), None)
    st = detect_ref(_noise(16, 16, 3), st)
    assert st[1] == 0
    st2 = detect_ref(_noise(16, 17, 3), st)
    assert tuple(st2[:4]) == (1, 1, 0, 1000)
    zero = np.zeros(STATE_WORDS, np.int32)
    zero[0] = 1  # valid, but the stored signature sums to 0
    assert tuple(detect_ref(_noise(16, 16, 3), zero)[:4]) == (1, 1, 0, 1000)


def test_since_saturates():
    img = _noise(8, 8, 4)
    st = detect_ref(img, None)
    st[2] = SINCE_MAX - 1
    st = detect_ref(img, st)
    assert st[2] == SINCE_MAX and st[1] == 0
    st = detect_ref(img, st)
    assert st[2] == SINCE_MAX
    st[2] = np.iinfo(np.int32).max  # beyond anything the detector writes: still no overflow
    assert detect_ref(img, st)[2] == SINCE_MAX


def test_min_gap_suppresses_the_flash():
    a = np.full((16, 16, 3), 40, np.uint8)
    flash = np.full((16, 16, 3), 250, np.uint8)
    st = detect_ref(a, None, 300, 3)
    flags = [int(st[1])]
    for img in (a, a, a, flash, a, a):
        st = detect_ref(img, st, 300, 3)
        flags.append(int(st[1]))
    # frame 4 is the flash (a cut: three frames since the first), frame 5 returns to the shot: scored as a cut, suppressed
    assert flags == [1, 0, 0, 0, 1, 0, 0]
    st = detect_ref(a, None, 300, 1)
    flags = [int(st[1])]
    for img in (a, flash, a):
        st = detect_ref(img, st, 300, 1)
        flags.append(int(st[1]))
    assert flags == [1, 0, 1, 1]  # min_gap 1: the flash is two cuts


def test_suppressed_cut_stores_the_signature():
    a = np.full((16, 16, 3), 40, np.uint8)
    b = np.full((16, 16, 3), 250, np.uint8)
    st = detect_ref(b, detect_ref(a, None, 300, 5), 300, 5)
    assert tuple(st[:4]) == (1, 0, 1, 1000)
    assert np.array_equal(st[4:], sig_ref(b).astype(np.int32))


def edge_pair():
    """25 x 40 zeros against the same with 350 pixels at 255: D = 700, score = 700000 // 2000 = 350 exactly"""
    a = np.zeros((25, 40, 3), np.uint8)
    b = a.copy()
    b.reshape(-1, 3)[:350] = 255
    return a, b


def test_threshold_edge():
    a, b = edge_pair()
    assert score_ref(a, b) == 350
    st = detect_ref(a, None)
    assert detect_ref(b, st, 350, 1)[1] == 1
    assert detect_ref(b, st, 351, 1)[1] == 0


def test_resets():
    assert resets_ref([0x3F800000, 1, 7], True) == [0, 0, 0]
    assert resets_ref([0x3F800000, 1, 7], False) == [0x3F800000, 1, 7]


# ---------------------------------------------------------------- the default threshold, on the committed images cut to 360 x 640
_imgs = {}


def image(name):
    if name not in _imgs:
        from stm_amd import bmp_io
        _imgs[name] = np.ascontiguousarray(bmp_io.read_bmp(os.path.join(GOLDEN, name + ".bmp"))[:360, :640])
        assert _imgs[name].shape[:2] == (360, 640)
    return _imgs[name]


def shifted(img, px):
    """the frame panned by px columns: the columns that enter repeat the edge column"""
    return np.concatenate([np.repeat(img[:, :1], px, axis=1), img[:, :-px]], axis=1)


def brightened(img, k):
    return np.clip(img.astype(np.int32) + k, 0, 255).astype(np.uint8)


def noisy(img, a, seed=7):
    n = np.random.RandomState(seed).randint(-a, a + 1, size=img.shape)
    return np.clip(img.astype(np.int32) + n, 0, 255).astype(np.uint8)


def non_cut_scores():
    out = {"bud_2 -> bud_3": score_ref(image("bud_2"), image("bud_3")), "bud_1 -> bud_2": score_ref(image("bud_1"), image("bud_2"))}
    for name in ("bud_2", "fish_1"):
        img = image(name)
        for px in (2, 8, 16, 32):
            out["%s shifted %d px" % (name, px)] = score_ref(img, shifted(img, px))
        for k in (2, 4, 8):
            out["%s +%d levels" % (name, k)] = score_ref(img, brightened(img, k))
        for a in (2, 6):
            out["%s noise +-%d" % (name, a)] = score_ref(img, noisy(img, a))
    return out


def cut_scores():
    return {"bud_2 -> fish_1": score_ref(image("bud_2"), image("fish_1")), "bud_3 -> fish_2": score_ref(image("bud_3"), image("fish_2"))}


def test_default_threshold_separates():
    non, cuts = non_cut_scores(), cut_scores()
    for k, v in list(non.items()) + list(cuts.items()):
        print("%-24s %d" % (k, v))
    assert all(v < DEFAULT_THRESH for v in non.values()), non
    assert all(v > DEFAULT_THRESH for v in cuts.values()), cuts
    # the derivation: the geometric mean of the largest non-cut and the smallest cut score, rounded to a multiple of 10
    gm = (max(non.values()) * min(cuts.values())) ** 0.5
    assert DEFAULT_THRESH == int(gm / 10.0 + 0.5) * 10


def test_default_threshold_is_the_package_default(stm):
    from stm_amd import video
    assert video.CUT_DEFAULT[0] == DEFAULT_THRESH

"""The reduced-resolution frame calls with a temporal history under the input prelude, on the GPU: stm_d_adcensus_stm_2t with all
three history pointers and stm_d_adcensus_stm_2nv12 with all four, under a manual alignment, a given colour balance, both, and an
automatic alignment with a carried device state.  The statement is the full-resolution tests' (test_gpu_align, test_gpu_balance):
the call equals, bit for bit in both maps and the frame, the call with the settings off on the prepared pair.  A BGR call sends
the previous frame through the current field and tables; an NV12 call hands out the prepared split images and takes its history
images as they are passed (they are an earlier call's outputs).  The prepared pair is a BGR frame, so for both entries the
settings-off call is stm_d_adcensus_stm_2t on it -- the reduced BGR call, which test_gpu_reduced_stream pins against the
reference next to the NV12 one; NV12 needs even rows, so its ragged shape is 66 x 130 where the BGR one is 67 x 130."""
import numpy as np
import pytest

import test_gpu_align as ta
import test_gpu_balance as tb
from test_align_ref import align_frame_ref, measure_ref
from test_balance_ref import balance_frame_ref
from test_gpu_reduced_stream import call_2nv12, call_2t
from test_upsample_ref import GUIDED_UP

pytestmark = pytest.mark.gpu

T = 0x2000
WORDS = [3 | T, 3 | T | GUIDED_UP]
SHAPES = {"48x96": (48, 96, 24, 48), "67x130": (67, 130, 33, 65)}
SETTINGS = ["align", "balance", "align+balance", "align-auto"]
CASES = [(f, s, k) for f in ("bgr", "nv12") for s in SETTINGS for k in SHAPES if not (s == "align-auto" and k != "48x96")]


@pytest.fixture(autouse=True)
def _settings_off_afterwards(gpu_ready):
    from stm_amd import device_api as dev
    try:
        yield
    finally:
        dev.set_align_auto(16, 1.0, None)
        dev.set_align(0)
        dev.set_balance(0)


def _prepared(eyes, field, lut):
    """the side-by-side BGR frame the matcher sees: the right eye through the field, then through the tables"""
    l, r = eyes
    W = l.shape[1]
    if field is not None:
        r = np.ascontiguousarray(align_frame_ref(l, r, *field)[:, W:])
    return np.ascontiguousarray(balance_frame_ref(l, r, lut) if lut is not None else np.concatenate([l, r], axis=1))


class _Under:
    """the thread's settings of a case for the duration of a block"""

    def __init__(self, setting, state):
        self.setting, self.state = setting, state

    def __enter__(self):
        from stm_amd import device_api as dev
        if self.setting == "align-auto":
            dev.set_align_auto(5, 0.5, self.state)
            dev.set_align(2)
        if "align" in self.setting.split("+"):
            dev.set_align(1, *ta.FIELD)
        if "balance" in self.setting:
            dev.set_balance(1, tb.GIVEN)

    def __exit__(self, *exc):
        from stm_amd import device_api as dev
        dev.set_align_auto(16, 1.0, None)
        dev.set_align(0)
        dev.set_balance(0)


@pytest.mark.parametrize("fmt,setting,shape", CASES, ids=["%s-%s-%s" % c for c in CASES])
def test_reduced_call_with_history_under_the_prelude(gpu_ready, fmt, setting, shape):
    import torch
    H, W, h, w = SHAPES[shape]
    if fmt == "nv12":
        H &= ~1
    p = ta._params()
    (_, prev_in, _, prev_eyes), (kind, cur_in, _, cur_eyes) = ta._inputs(fmt, *ta._pair(H, W, 0)), ta._inputs(fmt, *ta._pair(H, W, 1))
    lut = tb.GIVEN if "balance" in setting else None
    st0 = st1 = None
    if setting == "align-auto":  # the state carried over from the previous frame at rate 0.5: neither frame's own field
        _, _, st0, _ = measure_ref(prev_eyes[0], prev_eyes[1], 5, state=np.zeros(4, np.float32))
        _, _, st1, _ = measure_ref(cur_eyes[0], cur_eyes[1], 5, state=st0, rate=0.5)
        assert st0[0] == 1.0 and ta._bits(st0) != ta._bits(st1)
        field = tuple(float(v) for v in st1[1:])
    else:
        field = ta.FIELD if "align" in setting else None
    cur_p, prev_p = _prepared(cur_eyes, field, lut), _prepared(prev_eyes, field, lut)
    raw = np.ascontiguousarray(np.concatenate(cur_eyes, axis=1))
    assert not np.array_equal(cur_p, raw)  # the setting changes the pair
    first = call_2t(prev_p, p, h, w, 0.5, 3)
    ql, qr = first[0] + np.float32(0.25), first[1] - np.float32(0.25)
    # BGR: the previous frame prepared with the CURRENT field and tables; NV12: the history images exactly as passed
    prev_raw = np.ascontiguousarray(np.concatenate(prev_eyes, axis=1))
    hist_ref = prev_p if fmt == "bgr" else prev_raw
    for stages in WORDS:
        want = call_2t(cur_p, p, h, w, 0.5, stages, hist=(hist_ref, ql, qr))
        assert not np.array_equal(want[0], call_2t(cur_p, p, h, w, 0.5, stages & ~T)[0])  # the temporal step did something
        if fmt == "nv12":  # ... and a history sent through the field or the tables (the right eye's) would have given another map
            assert not np.array_equal(want[1], call_2t(cur_p, p, h, w, 0.5, stages, hist=(prev_p, ql, qr))[1])
        state = ta._cuda(st0) if st0 is not None else None

        def call():
            if fmt == "bgr":
                return call_2t(cur_in, p, h, w, 0.5, stages, hist=(prev_in, ql, qr))
            return call_2nv12(cur_in[0], cur_in[1], p, h, w, 0.5, stages, hist=(prev_eyes[0], prev_eyes[1], ql, qr))
        with _Under(setting, state):
            got = call()
        for k in range(3):
            assert np.array_equal(got[k], want[k]), (fmt, setting, shape, hex(stages), k)
        assert want[0].any() and want[2].any()
        if fmt == "nv12":  # the split images the call hands out are the prepared eyes
            assert np.array_equal(got[3], cur_p[:, :W]) and np.array_equal(got[4], cur_p[:, W:])
        if state is not None:
            torch.cuda.synchronize()
            assert ta._bits(state.cpu().numpy()) == ta._bits(st1)
        off = call()  # the settings off again: the setting did something to the maps and to the frame
        assert not (np.array_equal(off[0], got[0]) and np.array_equal(off[1], got[1])) and not np.array_equal(off[2], got[2])

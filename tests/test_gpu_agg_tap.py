"""The frame's aggregation chain compared with the CPU oracle on its COST VOLUMES, through stm_set_agg_tap, at every kernel form.

The winner-takes-all maps that every other frame test compares are blind to faults in the aggregated costs (tests/test_agg_tap_ref.py
states how blind).  Here the volume after the first horizontal pass (h1) and after both vertical passes (v2) are read back and
compared byte for byte -- all 2 D H W floats -- and the last pass, fused with WTA, is pinned twice: by its maps on the chain's own
v2, and by its maps on volumes injected in front of it whose winner a single window element decides (agg_tap_cases.py).  Where the
chain keeps the last pass's volume (stage bit 0x100) that is compared as well.

Every case first asks stm_agg_path / stm_first_pass_path / stm_px_order that the form it names is the one that runs, and that the
answers are the same with the tap set."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import agg_tap_cases as tc
from conftest import ROOT

pytestmark = pytest.mark.gpu

HSLO, SUBPIXEL = 0x100, 0x200


# ----------------------------------------------------------------------------- the forms and what the dispatcher must say of them
class Form:
    """variant: stm_set_agg_variant's word.  The rest is what the queries must answer for a frame at stages = 1: on the matrix pipe,
    PX and its order (-1 off PX), stm_k_pq_hc2 (first_pass_path > 0), the waves of stm_k_pq_hc's plan (0: another first pass), the
    register-ring vertical and last-pass kernels.  None = not asserted (the answer depends on the case's D, zd or usd)."""

    def __init__(self, name, variant=0, pipe=True, order=2, hc2=True, waves=12, vregs=True, hregs=True):
        self.name, self.variant, self.pipe, self.order, self.hc2, self.waves, self.vregs, self.hregs = name, variant, pipe, order, hc2, waves, vregs, hregs


DEFAULT = Form("default_hc2_px2")                                                     # stm_k_pq_hc2, stm_k_pq_v12r, stm_k_pq_hsr on PX order 2
SEPARATE_VIEWS = Form("separate_views_hc12", 2000000, hc2=False)                      # stm_k_pq_hc<12, PX>
PX_ORDER_0 = Form("px_order_0", 2000000000, order=0)                                  # 4-byte stores, ascending records
PQ_END_TO_END = Form("pq_end_to_end", 20000000, order=-1, hc2=False)                  # stm_k_pq_hc<12, PQ>, stm_k_pq_v12q, stm_k_pq_hsr on PQ
LDS_VERTICAL = Form("lds_ring_vertical", 10000000, order=-1, hc2=False, vregs=False)  # stm_k_pq_v12t
LDS_LAST = Form("lds_last_pass", 100000000, order=-1, hc2=False, hregs=False)         # stm_k_pq_hs<8, true>
LDS_LAST_SEGMENTS = Form("lds_last_pass_per_segment", 100000010, order=-1, hc2=False, hregs=False)  # stm_k_pq_h<8, true, false>
SEPARATE_COST = Form("separate_cost_kernel", 1000000, order=-1, hc2=False, waves=0)   # stm_k_pq_cost + stm_k_pq_hs<8, false>
SEG_10 = Form("variant_10", 10)            # block-per-segment kernels where a streaming one would run: none does at D 64 by default
SEG_20 = Form("variant_20", 20)            # D > 64 on the block-per-segment kernels (see D100 below); at D 64 the default
SEG_200 = Form("variant_200", 200)         # the renderer's un-fused form: the chain is the default's
SEG_300 = Form("variant_300", 300)         # region voting's older kernels: the chain is the default's
SEG_1000 = Form("variant_1000_h8_cost", 1000, order=-1, hc2=False, waves=0)  # stm_k_pq_h<8, false, true>: 128-pixel segments
SEG_2000 = Form("variant_2000_h12_cost", 2000, order=-1, hc2=False, waves=0)  # stm_k_pq_h<12, false, true>: one block per 192-pixel segment
LEGACY = Form("legacy_vector_alu", 10000, pipe=False)                                 # launch_agg_h2_cost, launch_agg_v, launch_agg_h_wta2
HC8 = Form("hc8_px", 0, hc2=False, waves=8)                                           # stm_k_pq_hc<8, PX> (zero_disp outside 18 .. 45)
OFF_PX = Form("off_px", 0, order=-1, hc2=False, waves=None, vregs=None, hregs=None)   # D outside 49 .. 64, or usd past 36
D100_SEG_20 = Form("D100_variant_20", 20, order=-1, hc2=False, waves=0, vregs=None, hregs=False)  # stm_k_pq_h<.., true> first, stm_k_pq_h<8, true, false> last


def _params(D=64, zd=32, usd=tc.USD, lsd=tc.LSD):
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=D, zero_disp=zd, usd=usd, lsd=lsd)


def _queries(p, H, W, stages):
    from stm_amd import device_api as dev
    a = (p.num_disp, p.zero_disp, H, W, p.usd, stages)
    return dev.agg_path(*a), dev.first_pass_path(*a), dev.px_order(*a)


def assert_form(form, p, H, W, stages=1):
    """under the form's variant the dispatcher answers what the form says (host arithmetic: no GPU needed)"""
    import stm_amd
    from stm_amd import device_api as dev
    stm_amd.lib().stm_set_agg_variant(form.variant)
    try:
        path, fp, order = _queries(p, H, W, stages)
    finally:
        stm_amd.lib().stm_set_agg_variant(0)
    what = "%s at %dx%d D%d zd%d usd%d stages 0x%x: path 0x%x, first pass %d, order %d" % (
        form.name, H, W, p.num_disp, p.zero_disp, p.usd, stages, path, fp, order)
    assert bool(path & dev.AGG_MATRIX_PIPE) == form.pipe, what
    if not form.pipe:
        assert path == 0 and fp == 0 and order == -1, what
        return
    assert order == form.order and bool(path & dev.AGG_PX) == (form.order >= 0), what
    assert (fp > 0) == form.hc2, what
    for want, got in ((form.waves, dev.agg_path_waves(path)), (form.vregs, bool(path & dev.AGG_VREGS)), (form.hregs, bool(path & dev.AGG_HREGS))):
        assert want is None or want == got, what


# ----------------------------------------------------------------------------- content and the oracle's volumes, computed once
_CACHE = {}


def _pair(content, H, W, p):
    """(left, right) uint8 [H][W][3], read only"""
    key = ("pair", content, H, W, p.num_disp, p.zero_disp)
    if key not in _CACHE:
        if content == "synth":
            from stm_amd import synth
            zd = min(max(p.zero_disp, 0), p.num_disp - 1)  # its ground truth is laid out for a zero_disp inside [0, D)
            sbs = synth.sbs_frame(H, W, p.num_disp, zd)[0]
            pair = np.ascontiguousarray(sbs[:, :W]), np.ascontiguousarray(sbs[:, W:])
        else:
            pair = tc.mondrian_pair(H, W)
        for a in pair:
            a.setflags(write=False)
        _CACHE[key] = pair
    return _CACHE[key]


def _pair_key(pair):
    return hashlib.sha1(pair[0].tobytes() + pair[1].tobytes()).hexdigest() + repr(pair[0].shape)


def _arms(orc, pair, p):
    key = ("arms", _pair_key(pair), p.usd, p.lsd, p.ucd, p.lcd)
    if key not in _CACHE:
        _CACHE[key] = [orc.cross_arms(np.array(img), p.ucd, p.lcd, p.usd, p.lsd) for img in pair]
    return _CACHE[key]


def _chain(orc, pair, p):
    """the oracle's chain of both views: {h1, v2, h4: float32 [2][D][H][W], maps: [2][H][W]}, read only"""
    key = ("chain", _pair_key(pair), p.num_disp, p.zero_disp, p.usd, p.lsd, p.ucd, p.lcd, p.ad_coeff, p.census_coeff)
    if key not in _CACHE:
        cross = _arms(orc, pair, p)
        cost = orc.ci_adcensus(np.array(pair[0]), np.array(pair[1]), p.ad_coeff, p.census_coeff, p.num_disp, p.zero_disp)
        h1 = [orc.agg_hpass(cost[v], cross[v]) for v in (0, 1)]
        v2 = [orc.agg_vpass(orc.agg_vpass(h1[v], cross[v]), cross[v]) for v in (0, 1)]
        h4 = [orc.agg_hpass(v2[v], cross[v]) for v in (0, 1)]
        ref = {"h1": np.stack(h1), "v2": np.stack(v2), "h4": np.stack(h4), "maps": np.stack([orc.dc_wta(h4[v], p.zero_disp) for v in (0, 1)])}
        for a in ref.values():
            a.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


# ----------------------------------------------------------------------------- a frame call under the tap
FILL = 0xA5


def _tap_buffer(D, H, W):
    """float32 [2][D][H][W] on the GPU, every byte FILL"""
    import torch
    return torch.full((2 * D * H * W * 4,), FILL, dtype=torch.uint8, device="cuda").view(torch.float32).reshape(2, D, H, W)


def _untouched(t):
    import torch
    return bool((t.reshape(-1).view(torch.uint8) == FILL).all())


def _frame_d(sbs, dl, dr, out, p, stages):
    from stm_amd import device_api as dev
    dev.d_adcensus_stm(sbs, dl, dr, out, p, stages=stages)


def run_tapped(pair, p, stages, variant=0, inject=None, want_h4=False, call=_frame_d, match=None):
    """One frame call with h1, v2 (and h4) tapped and `inject` (float32 [2][D][h][w] or None) written over V2.  The queries must answer
    the same before the tap is set and while it is.  Returns {h1, v2, h4 (or None), maps [2][H][W]} as numpy arrays.  match: the
    match size of a reduced-resolution call (the tap's buffers take it)."""
    import torch
    import stm_amd
    from stm_amd import device_api as dev
    H, W = pair[0].shape[:2]
    h, w = match or (H, W)
    D = p.num_disp
    sbs = torch.from_numpy(tc.sbs_of(np.array(pair[0]), np.array(pair[1]))).cuda()
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    h1, v2 = _tap_buffer(D, h, w), _tap_buffer(D, h, w)
    h4 = _tap_buffer(D, h, w) if want_h4 else None
    d_inject = torch.from_numpy(np.ascontiguousarray(inject)).cuda() if inject is not None else None
    lib = stm_amd.lib()
    lib.stm_set_agg_variant(variant)
    try:
        before = _queries(p, h, w, stages)
        with dev.agg_tap(h1=h1, v2=v2, h4=h4, inject_v2=d_inject):
            assert _queries(p, h, w, stages) == before, "the dispatcher's answers moved with the tap set"
            call(sbs, dl, dr, out, p, stages)
            torch.cuda.synchronize()
        assert _queries(p, h, w, stages) == before
    finally:
        lib.stm_set_agg_variant(0)
    return {"h1": h1.cpu().numpy(), "v2": v2.cpu().numpy(), "h4": h4.cpu().numpy() if want_h4 else None,
            "maps": np.stack([dl.cpu().numpy(), dr.cpu().numpy()])}


def _same_volume(got, want, what):
    """all 2 D H W floats as bytes; on a mismatch the message says where"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        v, d, y, x = bad[0]
        raise AssertionError("%s: %d of %d elements differ, the first at view %d d %d y %d x %d: %r against the oracle's %r; hypotheses %r, "
                             "columns %% 16 %r" % (what, len(bad), got.size, v, d, y, x, got[v, d, y, x], want[v, d, y, x],
                                                  sorted(set(bad[:, 1].tolist()))[:12], sorted(set((bad[:, 3] % 16).tolist()))))


def check_chain(orc, form, content, H, W, p, stages=1):
    """the form runs; then h1, v2 and the maps of one tapped frame against the oracle's chain, as bytes"""
    assert_form(form, p, H, W, stages)
    pair = _pair(content, H, W, p)
    ref = _chain(orc, pair, p)
    got = run_tapped(pair, p, stages, form.variant)
    tag = "%s, %s %dx%d" % (form.name, content, H, W)
    _same_volume(got["h1"], ref["h1"], tag + ", after the first horizontal pass")
    _same_volume(got["v2"], ref["v2"], tag + ", after both vertical passes")
    assert got["maps"].tobytes() == ref["maps"].tobytes(), tag + ", the WTA maps"
    return got, ref


CONTENTS = ["synth", "mondrian"]
BASE = (37, 67)  # below one segment of every kernel, ragged in both directions (H % 16, W % 4 != 0)

# (form, shapes beyond BASE and why)
FORM_SHAPES = [
    (DEFAULT, [(100, 129), (2, 300), (2, 700), (17, 200)]),  # one past a 128-pixel segment, seven row tiles; the ring of 256 wraps; two row parts; one row past a tile
    (SEPARATE_VIEWS, [(2, 300), (100, 129)]),                # two 192-pixel segments; seven row tiles
    (PX_ORDER_0, [(100, 129), (2, 300)]),
    (PQ_END_TO_END, [(100, 129), (17, 200)]),                # stm_k_pq_v12q: one row past a tile
    (LDS_VERTICAL, [(17, 200), (100, 129)]),                 # stm_k_pq_v12t: one row past a tile, two 48-row steps
    (LDS_LAST, [(100, 129)]),                                # stm_k_pq_hs<8, true>: one past a segment
    (LDS_LAST_SEGMENTS, [(100, 129)]),                       # stm_k_pq_h<8, true, false>
    (SEPARATE_COST, [(100, 129), (2, 300)]),                 # stm_k_pq_cost's 128-pixel blocks, stm_k_pq_hs<8, false>'s ring
    (SEG_10, [(100, 129)]), (SEG_20, [(100, 129)]), (SEG_200, [(100, 129)]), (SEG_300, [(100, 129)]),
    (SEG_1000, [(100, 129), (2, 300)]),                      # one past a 128-pixel segment
    (SEG_2000, [(100, 129), (2, 300)]),                      # 2 x 300: one past a 192-pixel segment
    (LEGACY, [(100, 129), (17, 200)]),
]
FORM_CASES = [(f, s) for f, shapes in FORM_SHAPES for s in [BASE] + shapes]


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("form, shape", FORM_CASES, ids=["%s-%dx%d" % (f.name, s[0], s[1]) for f, s in FORM_CASES])
def test_forms(gpu_ready, orc, form, shape, content):
    """D 64, zero_disp 32, usd 34 / lsd 17: every form of the chain that stm_set_agg_variant selects"""
    check_chain(orc, form, content, shape[0], shape[1], _params())


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", [BASE, (100, 129)], ids=["37x67", "100x129"])
@pytest.mark.parametrize("zd", [0, 17, 46, 63, -3, 67])
def test_hc8_over_zero_disp(gpu_ready, orc, zd, shape, content):
    """stm_k_pq_hc<8, PX>: the zero_disp values whose staging does not fit the 12-wave block, the two outside [0, D) included"""
    check_chain(orc, HC8, content, shape[0], shape[1], _params(64, zd))


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", [BASE, (2, 300)], ids=["37x67", "2x300"])
@pytest.mark.parametrize("form", [DEFAULT, SEPARATE_VIEWS], ids=["hc2", "hc12"])
@pytest.mark.parametrize("zd", [18, 45])
def test_hc12_at_its_last_zero_disp(gpu_ready, orc, zd, form, shape, content):
    """zero_disp 18 and 45: the last values with 12 waves -- stm_k_pq_hc2 by default, stm_k_pq_hc<12, PX> with the views separate"""
    check_chain(orc, form, content, shape[0], shape[1], _params(64, zd))


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", [BASE, (100, 129)], ids=["37x67", "100x129"])
@pytest.mark.parametrize("D", [48, 65, 100])
def test_num_disp_off_the_px_range(gpu_ready, orc, D, shape, content):
    """three, five and seven chunks: the PQ layout; D > 64 also leaves the register-ring last pass for stm_k_pq_hs<8, true> and its
    per-pixel minimum across chunk sets"""
    check_chain(orc, OFF_PX, content, shape[0], shape[1], _params(D, D // 2))


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", [BASE, (100, 129)], ids=["37x67", "100x129"])
def test_num_disp_100_per_segment_kernels(gpu_ready, orc, shape, content):
    """variant 20 at D 100: the block-per-segment kernels stm_k_pq_h<.., false, true> and stm_k_pq_h<8, true, false> with seven chunks"""
    check_chain(orc, D100_SEG_20, content, shape[0], shape[1], _params(100, 50))


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", [BASE, (53, 67), (64, 4), (4, 64)], ids=["37x67", "53x67", "64x4", "4x64"])
@pytest.mark.parametrize("form", [DEFAULT, SEPARATE_VIEWS, PQ_END_TO_END, LEGACY], ids=["hc2", "hc12", "pq", "legacy"])
def test_partly_filled_chunk(gpu_ready, orc, form, shape, content):
    """D 49 / zero_disp 20: one real hypothesis in the last chunk of 16 (and in the last quad), fifteen of padding; one group of
    columns and one group of rows"""
    check_chain(orc, form, content, shape[0], shape[1], _params(49, 20))


ARMS = [(29, 14, HC8), (36, 18, HC8), (37, 18, OFF_PX), (60, 30, OFF_PX), (120, 60, LEGACY)]


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", [BASE, (100, 129)], ids=["37x67", "100x129"])
@pytest.mark.parametrize("usd, lsd, form", ARMS, ids=["usd%d" % a[0] for a in ARMS])
def test_arm_lengths(gpu_ready, orc, usd, lsd, form, shape, content):
    """zero_disp 0.  usd 29: the first halo of ten groups; 36: the last on the register rings and PX; 37 and 60: stm_k_pq_v12t and the
    LDS last pass; 120: past what the matrix-pipe kernels hold (aggm_supports), the vector-ALU chain without a variant"""
    check_chain(orc, form, content, shape[0], shape[1], _params(64, 0, usd, lsd))


# ----------------------------------------------------------------------------- stage bits
@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("variant", [0, 10], ids=["streaming", "per_segment"])
@pytest.mark.parametrize("stages", [1 | HSLO, 3 | HSLO], ids=["0x101", "0x103"])
def test_kept_volume(gpu_ready, orc, stages, variant, content):
    """0x100: the chain keeps the last pass's volume for the scanline optimisation: h4 == agg_hpass(v2), on stm_k_pq_hs<8, false>
    and, under variant 10, on stm_k_pq_h<8, false, false>"""
    from stm_amd import device_api as dev
    for H, W in (BASE, (100, 129)):
        p = _params()
        path = dev.agg_path(p.num_disp, p.zero_disp, H, W, p.usd, stages)
        assert path & dev.AGG_MATRIX_PIPE and not path & (dev.AGG_PX | dev.AGG_HREGS), hex(path)
        pair = _pair(content, H, W, p)
        ref = _chain(orc, pair, p)
        got = run_tapped(pair, p, stages, variant, want_h4=True)
        for k in ("h1", "v2", "h4"):
            _same_volume(got[k], ref[k], "stages 0x%x, variant %d, %s %dx%d, %s" % (stages, variant, content, H, W, k))


@pytest.mark.parametrize("variant", [0, 10], ids=["streaming", "per_segment"])
def test_kept_volume_of_an_injected_volume(gpu_ready, orc, variant):
    """0x100 under noise injection: h4 == agg_hpass(inject) -- the last pass's sums themselves, on sums that are not exact"""
    for H, W in (BASE, (100, 129)):
        p = _params()
        pair = _pair("mondrian", H, W, p)
        cross = _arms(orc, pair, p)
        inject = np.stack([tc.noise_volume(64, H, W, 11), tc.noise_volume(64, H, W, 12)])
        got = run_tapped(pair, p, 1 | HSLO, variant, inject=inject, want_h4=True)
        want = np.stack([orc.agg_hpass(inject[v], cross[v]) for v in (0, 1)])
        _same_volume(got["h4"], want, "variant %d, %dx%d, h4 of the injected volume" % (variant, H, W))


def test_wta_chain_writes_no_h4(gpu_ready):
    """without 0x100 no last volume exists: h4 stays as the caller left it"""
    import torch
    from stm_amd import device_api as dev
    H, W = BASE
    p = _params()
    pair = _pair("synth", H, W, p)
    h4 = _tap_buffer(64, H, W)
    with dev.agg_tap(h4=h4):
        _frame_d(torch.from_numpy(tc.sbs_of(*[np.array(a) for a in pair])).cuda(), torch.zeros(H, W, device="cuda"), torch.zeros(H, W, device="cuda"),
                 torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda"), p, 1)
        torch.cuda.synchronize()
    assert _untouched(h4)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("form", [PQ_END_TO_END, LEGACY], ids=["matrix_pipe", "legacy"])
def test_subpixel_rereads_v2(gpu_ready, orc, form, content):
    """0x200: the sub-pixel step reads the last pass's input again, so the chain leaves PX; the v2 it rereads is the oracle's"""
    from stm_amd import device_api as dev
    stages = 1 | SUBPIXEL
    for H, W in (BASE, (100, 129)):
        p = _params()
        variant = form.variant if form is LEGACY else 0
        dev.lib().stm_set_agg_variant(variant)
        try:
            path, fp, order = _queries(p, H, W, stages)
        finally:
            dev.lib().stm_set_agg_variant(0)
        assert bool(path & dev.AGG_MATRIX_PIPE) == form.pipe and order == -1 and fp == 0, hex(path)
        pair = _pair(content, H, W, p)
        ref = _chain(orc, pair, p)
        got = run_tapped(pair, p, stages, variant)
        _same_volume(got["h1"], ref["h1"], "0x201 %s %dx%d h1" % (form.name, H, W))
        _same_volume(got["v2"], ref["v2"], "0x201 %s %dx%d v2" % (form.name, H, W))


# ----------------------------------------------------------------------------- the other frame entries
def test_entry_t(gpu_ready, orc):
    """stm_d_adcensus_stm_t (no history)"""
    from stm_amd import device_api as dev
    H, W = BASE
    p = _params()
    assert_form(DEFAULT, p, H, W, 1)
    pair = _pair("mondrian", H, W, p)
    ref = _chain(orc, pair, p)
    got = run_tapped(pair, p, 1, call=lambda sbs, dl, dr, out, p, stages: dev.d_adcensus_stm_t(sbs, dl, dr, out, p, stages))
    for k in ("h1", "v2"):
        _same_volume(got[k], ref[k], "_t " + k)
    assert got["maps"].tobytes() == ref["maps"].tobytes()


def test_entry_nv12(gpu_ready, orc):
    """stm_d_adcensus_stm_nv12: the chain on the pair the conversion makes"""
    import torch
    from stm_amd import device_api as dev, synth
    from test_nv12_ref import nv12_to_bgr_ref
    H, W = 38, 68  # NV12 needs even sizes
    p = _params()
    assert_form(DEFAULT, p, H, W, 1)
    src = _pair("mondrian", H, W, p)
    y, uv = synth.bgr_to_nv12(tc.sbs_of(np.array(src[0]), np.array(src[1])), 0)
    bgr = nv12_to_bgr_ref(y, uv, 0)
    pair = (np.ascontiguousarray(bgr[:, :W]), np.ascontiguousarray(bgr[:, W:]))
    ref = _chain(orc, pair, p)
    d_y, d_uv = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
    got = run_tapped(pair, p, 1, call=lambda sbs, dl, dr, out, p, stages: dev.d_adcensus_stm_nv12(d_y, d_uv, dl, dr, out, p, stages, 0))
    for k in ("h1", "v2"):
        _same_volume(got[k], ref[k], "_nv12 " + k)
    assert got["maps"].tobytes() == ref["maps"].tobytes()


def test_entry_2s_at_the_match_size(gpu_ready, orc):
    """stm_d_adcensus_stm_2s, 74 x 134 matched at 37 x 67: the tap's volumes have the match size and are the chain of the reduced pair"""
    from stm_amd import device_api as dev
    h, w = BASE
    H, W = 2 * h, 2 * w
    p = _params()
    assert_form(DEFAULT, p, h, w, 3)
    big = _pair("mondrian", H, W, p)
    low = tuple(orc.tx_scale_bilinear(np.array(img), h, w) for img in big)
    ref = _chain(orc, low, p)
    got = run_tapped(big, p, 3, match=(h, w),
                     call=lambda sbs, dl, dr, out, p, stages: dev.d_adcensus_stm_2s(sbs, dl, dr, out, p, h, w, 0.5, stages))
    for k in ("h1", "v2"):
        _same_volume(got[k], ref[k], "_2s " + k)


def test_entry_host_flavour(gpu_ready, orc):
    """stm_adcensus_stm: host buffers in and out, the same body underneath; the tap's buffers stay device memory"""
    import torch
    from stm_amd import device_api as dev, host_api
    H, W = BASE
    p = _params()
    assert_form(DEFAULT, p, H, W, 3)
    pair = _pair("mondrian", H, W, p)
    ref = _chain(orc, pair, p)
    h1, v2 = _tap_buffer(64, H, W), _tap_buffer(64, H, W)
    args = (p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h)
    with dev.agg_tap(h1=h1, v2=v2):
        host_api.adcensus_stm(tc.sbs_of(np.array(pair[0]), np.array(pair[1])), W, H, W, *args)
        torch.cuda.synchronize()
    _same_volume(h1.cpu().numpy(), ref["h1"], "host flavour h1")
    _same_volume(v2.cpu().numpy(), ref["v2"], "host flavour v2")


# ----------------------------------------------------------------------------- injection: the last pass on volumes of our making
LAST_PASS_FORMS = [
    (DEFAULT, 64), (PX_ORDER_0, 64), (PQ_END_TO_END, 64),  # stm_k_pq_hsr on PX order 2, on PX order 0, on PQ
    (LDS_LAST, 64), (OFF_PX, 100),                         # stm_k_pq_hs<8, true> with one chunk set and with two
    (LDS_LAST_SEGMENTS, 64),                               # stm_k_pq_h<8, true, false>
    (LEGACY, 64),                                          # launch_agg_h_wta2
]
INJECT_CASES = [(f, D, s) for f, D in LAST_PASS_FORMS for s in [BASE, (100, 129), (2, 300)]] + \
               [(f, 49, (53, 67)) for f, D in LAST_PASS_FORMS if D == 64]


@pytest.mark.parametrize("form, D, shape", INJECT_CASES, ids=["%s-D%d-%dx%d" % (f.name, D, s[0], s[1]) for f, D, s in INJECT_CASES])
def test_last_pass_on_injected_volumes(gpu_ready, orc, form, D, shape):
    """The mondrian pair supplies the arms; V2 is overwritten with each planted volume (every offset, then the volume of ties) and
    with one noise volume, the views' volumes from different seeds.  The maps must be dc_wta(agg_hpass(inject[v], cross[v])): a
    window one element short or long at any column, a hypothesis read from the wrong float of a record, a padding hypothesis that
    wins (it holds -1.0f; D 49: a winner >= D - zero_disp) or a tie broken the wrong way each change a map (test_agg_tap_ref.py)."""
    H, W = shape
    zd = 20 if D == 49 else D // 2
    p = _params(D, zd)
    assert_form(form, p, H, W, 1)
    pair = _pair("mondrian", H, W, p)
    cross = _arms(orc, pair, p)
    left, right = tc.planted_volumes(D, H, W, 7), tc.planted_volumes(D, H, W, 8)
    volumes = [(a[0], np.stack([a[1], b[1]])) for a, b in zip(left, right)]
    volumes.append(("noise", np.stack([tc.noise_volume(D, H, W, 11), tc.noise_volume(D, H, W, 12)])))
    for name, inject in volumes:
        got = run_tapped(pair, p, 1, form.variant, inject=inject)["maps"]
        want = np.stack([orc.dc_wta(orc.agg_hpass(inject[v], cross[v]), zd) for v in (0, 1)])
        assert got.min() >= -zd and got.max() <= D - 1 - zd, "%s, %s: a winner outside [0, D): %r .. %r" % (form.name, name, got.min(), got.max())
        if got.tobytes() != want.tobytes():
            bad = np.argwhere(got != want)
            v, y, x = bad[0]
            raise AssertionError("%s, volume %s, %dx%d D%d: %d map pixels differ, the first at view %d y %d x %d: d %d against the oracle's %d"
                                 % (form.name, name, H, W, D, len(bad), v, y, x, got[v, y, x] + zd, want[v, y, x] + zd))


def test_subpixel_reads_the_injected_volume(gpu_ready, orc):
    """1 | 0x200 under injection: the parabola is rebuilt from the injected V2, so the maps are those of the per-stage sub-pixel step on
    agg_hpass(inject)"""
    from test_subpixel_ref import subpixel_ref
    H, W, D, zd = 37, 67, 64, 32
    p = _params(D, zd)
    pair = _pair("mondrian", H, W, p)
    cross = _arms(orc, pair, p)
    inject = np.stack([tc.noise_volume(D, H, W, 11), tc.noise_volume(D, H, W, 12)])
    got = run_tapped(pair, p, 1 | SUBPIXEL, inject=inject)["maps"]
    for v in (0, 1):
        agg = orc.agg_hpass(inject[v], cross[v])
        want = subpixel_ref(agg, orc.dc_wta(agg, zd), zd)
        assert got[v].tobytes() == want.astype(np.float32).tobytes(), v


# ----------------------------------------------------------------------------- the stream never sees the tap; taps off is taps never set
def _stream_frames(p, H, W, frames):
    from stm_amd import video
    fs = video.FrameStream(H, W, p)
    try:
        got = []
        for f in frames:
            fs.submit(f)
            got.append(fs.collect())
    finally:
        fs.close()
    return got


def test_frame_stream_never_sees_the_tap(gpu_ready):
    """four frames through a FrameStream (the later ones replay a captured graph) with the thread's tap set, injection included: the
    tap's buffers keep their fill and the stream's outputs are those of a stream without it"""
    import torch
    from stm_amd import device_api as dev, synth
    H, W = 40, 72
    p = _params()
    frames = [synth.sbs_frame(H, W, 64, 32, seed=synth.SEED + k)[0] for k in range(4)]
    plain = _stream_frames(p, H, W, frames)
    bufs = [_tap_buffer(64, H, W) for _ in range(3)]
    inject = torch.from_numpy(np.stack([tc.noise_volume(64, H, W, 11)] * 2)).cuda()
    with dev.agg_tap(bufs[0], bufs[1], bufs[2], inject):
        tapped = _stream_frames(p, H, W, frames)
        torch.cuda.synchronize()
    assert all(_untouched(b) for b in bufs)
    for a, b in zip(plain, tapped):
        assert a[0] == b[0]
        for k in (1, 2, 3):
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()


def off_outputs():
    """digest of a whole frame's outputs on this process's thread settings (test_taps_off_is_a_process_that_never_set_one and its child)"""
    import torch
    from stm_amd import device_api as dev, synth
    H, W = 40, 72
    p = _params()
    sbs = torch.from_numpy(synth.sbs_frame(H, W, 64, 32)[0]).cuda()
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    dev.d_adcensus_stm(sbs, dl, dr, out, p, stages=3)
    torch.cuda.synchronize()
    return hashlib.sha256(dl.cpu().numpy().tobytes() + dr.cpu().numpy().tobytes() + out.cpu().numpy().tobytes()).hexdigest()


def test_taps_off_is_a_process_that_never_set_one(gpu_ready):
    from stm_amd import device_api as dev
    buf = _tap_buffer(64, 40, 72)
    with dev.agg_tap(h1=buf, v2=buf):
        pass
    dev.set_agg_tap(None, None, None, None)
    here = off_outputs()
    assert _untouched(buf)
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_agg_tap as t\n"
            "print('digest', t.off_outputs())\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ("digest " + here) in r.stdout, r.stdout + r.stderr

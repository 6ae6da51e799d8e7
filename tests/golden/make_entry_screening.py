"""Writes tests/golden/entry_screening.json and tests/golden/stream_screening.json: what the stage entries, the thread setters and
the stream setters answer to calls they refuse before they touch the device.

    python tests/golden/make_entry_screening.py             # the stage entries and thread setters: no GPU needed or used
    python tests/golden/make_entry_screening.py --stream    # the stream setters: needs a GPU (stm_stream_create allocates)
    ... --commit HASH                                       # in a tree exported without its history: the commit it was exported from

The companion of make_frame_screening.py, whose runner (call, _convert, apply_settings, refusal, P) it uses.  A case (cases() and
stream_cases() below) is an entry and an argument list, pointers as dummy addresses that a refused call never dereferences (0 =
null); an argument the screen itself reads (a rect, a lut768) is written as a list or "identity" and gets real host memory.  The
files hold, per case, the text of stm_last_error() after its first line (the fail site's file:line, which moves with the code), one
row per label and text with the entries that gave it; their first row names the commit the library was built from.  Run on the
library whose refusals are to be pinned; tests/test_entry_screening.py and tests/test_gpu_stream_screening.py replay the cases
against the files.  A case that is not refused with a message of the entry's own name is an error here, not a table row."""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "entry_screening.json")
OUT_STREAM = os.path.join(HERE, "stream_screening.json")

_spec = importlib.util.spec_from_file_location("make_frame_screening", os.path.join(HERE, "make_frame_screening.py"))
frame = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(frame)
call, _convert, apply_settings, refusal, P = frame.call, frame._convert, frame.apply_settings, frame.refusal, frame.P

NAN, INF = float("nan"), float("inf")
ROWS, COLS = "num_rows=8 num_cols=16", "num_rows=8 num_cols=16 elem_sz=3"
BIG = dict(num_rows=65536, num_cols=32768)    # num_rows * num_cols = 2^31
WIDE = dict(num_rows=40000, num_cols=40000)   # the alignment measurement's 32-bit sums


def spec(text):
    """'a=P b=8 c=0.5' -> the argument names in order and their passing values; P: a dummy address of the argument's own"""
    names, base = [], {}
    for k, tok in enumerate(text.split()):
        n, v = tok.split("=")
        names.append(n)
        base[n] = P(k + 1) if v == "P" else json.loads(v)
    return names, base


# ------------------------------------------------------------------------------------------------- building rules
def dims(ds):
    """the dimension screen (args_ok): every dimension one below its floor, a negative one, and each adjacent pair broken at once"""
    out = [("dim-" + n, {n: lo - 1}) for n, lo in ds] + [("dim-negative", {ds[0][0]: -5})]
    return out + [("dim-%s+%s" % (a, b), {a: la - 1, b: lb - 1}) for (a, la), (b, lb) in zip(ds, ds[1:])]


def chain(rules):
    """rules in the screen's order, each (label, overrides, further single cases {suffix: overrides}): every rule alone, its further
    cases, and each adjacent pair broken at once (label a+b: which one wins is what the table pins)"""
    out = []
    for k, r in enumerate(rules):
        label, over = r[0], r[1]
        out.append((label, over))
        for suffix, o in (r[2] if len(r) > 2 else {}).items():
            out.append((label + "-" + suffix, o))
        if k + 1 < len(rules) and not set(over) & set(rules[k + 1][1]):
            out.append((label + "+" + rules[k + 1][0], dict(over, **rules[k + 1][1])))
    return out


def rng(name, low, high, **more):
    """a range rule on `name`: below it, above it and whatever else (nan=..., inf=...)"""
    extra = {"high": {name: high}}
    extra.update({k: {name: v} for k, v in more.items()})
    return (name, {name: low}, extra)


LENS = lambda mode_bad: [("lens-mode", {"mode": mode_bad[0]}, {"high": {"mode": mode_bad[1]}}),
                         ("pitch", {"pitch": 0.5}, {"nan": {"pitch": NAN}, "inf": {"pitch": INF}}),
                         ("slope", {"slope": NAN}, {"inf": {"slope": -INF}}), ("centre", {"centre": INF}, {"nan": {"centre": NAN}})]
LAYOUT = [rng("tiles_x", 0, 65536), rng("tiles_y", 0, 65536), rng("order", -1, 4)]
OVERLAY = lambda ptr, words: ([("overlay-null", {ptr: 0}), ("overlay-unaligned", {ptr: P(30) + 2})] if words else []) + \
    [rng("ov_rows", 0, 65536), rng("ov_cols", 0, 65536), rng("x0", -65537, 65537), rng("y0", -65537, 65537)]
DEPTH1 = [rng("gain", -0.5, 8.5, nan=NAN), rng("conv", 5000.0, -5000.0, nan=NAN, inf=INF)]
OVERLAY_AUTO = [rng("near_permille", -1, 500), rng("margin", 5000.0, -5000.0, nan=NAN), rng("pad", -1, 4097),
                rng("limit_lo", -5000.0, 5000.0, nan=NAN), rng("limit_hi", 5000.0, -5000.0, inf=INF),
                ("limits-crossed", {"limit_lo": 2.0, "limit_hi": 1.0}), rng("rate_near", 0.0, 1.5, nan=NAN), rng("rate_far", 0.0, 1.5, nan=NAN)]
DEPTH_AUTO = [("budget", {"disp_lo": 2.0, "disp_hi": 2.0}, {"crossed": {"disp_lo": 3.0}, "nan": {"disp_lo": NAN}, "inf": {"disp_hi": INF},
                                                            "far": {"disp_lo": -5000.0}}),
              rng("max_gain", 0.0, 8.5, nan=NAN), rng("clip_permille", -1, 500), rng("rate", 0.0, 1.5, nan=NAN)]
ANTIALIAS = [rng("strength", -1.0, 8.5, nan=NAN), rng("max_radius", 0, 17), rng("gate", -1.0, INF, nan=NAN)]
ALIGN1 = [("a", {"a": NAN}, {"inf": {"a": INF}}), ("b", {"b": INF}, {"nan": {"b": NAN}}), ("c", {"c": -INF}, {"nan": {"c": NAN}})]
ALIGN_AUTO = [rng("radius", 0, 33), rng("rate", 0.0, 2.0, nan=NAN)]
BALANCE_AUTO = [rng("max_shift", -1, 256), rng("rate", 0.0, 2.0, nan=NAN)]
CUT = [rng("thresh_permille", 0, 1001), rng("min_gap", 0, (1 << 20) + 1)]
ACTIVE_AUTO = [rng("thresh_luma", -1, 255), rng("lit_permille", -1, 1000), rng("max_bar_permille", -1, 451), rng("hold", 0, (1 << 20) + 1)]
PACKING = [rng("packing", -1, 4), rng("swap", -1, 2), rng("filter", -1, 2), rng("gap", -1, (1 << 24) + 1),
           ("filter-full", {"filter": 1, "packing": 0}, {"top-bottom": {"filter": 1, "packing": 2}})]
NV12 = lambda cols: [("nv12-rows", {"num_rows": 7}), ("nv12-cols", {cols: 15}), ("nv12-narrow", {"num_cols_sbs": 30}), ("nv12-pitch_y", {"pitch_y": 31}),
                     ("nv12-pitch_uv", {"pitch_uv": 31}), rng("matrix", -1, 4)]
RECT_IN = lambda name: (name, {name: [0, 9, 0, 16]}, {"left": {name: [0, 8, 4, 4]}, "negative": {name: [-1, 8, 0, 16]}, "wide": {name: [0, 8, 0, 17]}})
GEOM = ("angle", {"angle": 0.0}, {"nan": {"angle": NAN}, "steep": {"angle": 89.9}})  # mux_geom_ok speaks as mux_multiview, whoever calls
OVERLAP = lambda out, img, n: ("overlap", {out: P(2) + n - 1}, {"same": {out: P(2)}, "behind": {out: P(2) - n + 1}})


def nulls(*names):
    """the null-pointer rule of `names`: each one null alone, and all of them"""
    return ("null", {n: 0 for n in names}, {n: {n: 0} for n in names} if len(names) > 1 else {})


def stage(name, host, device, rules):
    """one stage in its two flavours: argument specs (None: the flavour does not exist) and rules(d) -> [(label, overrides)], d true
    for the device flavour"""
    out = {}
    for d, text in ((False, host), (True, device)):
        if text is not None:
            seen, kept = {}, []
            for r in rules(d):  # (a chain that starts at the screen before it names that screen's case again)
                if r[0] in seen:
                    assert seen[r[0]] == r[1], (name, r[0])
                    continue
                seen[r[0]] = r[1]
                kept.append(r)
            out["stm_" + ("d_" if d else "") + name] = (spec(text), kept)
    return out


def only_dims(name, host, device, ds):
    return stage(name, host, device, lambda d: dims(ds))


D3 = [("num_disp", 1), ("num_rows", 1), ("num_cols", 1)]
RC = [("num_rows", 1), ("num_cols", 1)]
RCE = RC + [("elem_sz", 3)]
MUX = [("num_views", 2), ("in_rows", 1), ("in_cols", 1), ("out_rows", 1), ("out_cols", 1), ("elem_sz", 3)]
SPLIT = [("num_rows", 1), ("num_cols_sbs", 1), ("num_cols_out", 1), ("elem_sz", 3)]
LOW = [("num_rows", 1), ("num_cols_sbs", 1), ("num_cols", 1), ("num_rows_disp", 1), ("num_cols_disp", 1), ("elem_sz", 3)]
COST = "ad_coeff=10.0 census_coeff=30.0 num_disp=4 zero_disp=2 " + COLS
CROSS = "ucd=20.0 lcd=6.0 usd=5 lsd=3 num_disp=4 " + COLS
DBM = "img_out=P img_in_l=P img_in_r=P disp_l=P disp_r=P occl_l=P occl_r=P mask_l=P mask_r=P shift=0.5 " + COLS
FIT = "disp_l=P disp_r=P " + ROWS + " disp_lo=-2.0 disp_hi=2.0 max_gain=4.0 clip_permille=20 rate=0.5 state=P"
OVFIT = "disp_l=P disp_r=P " + ROWS + " overlay=P ov_rows=2 ov_cols=2 x0=0 y0=0 view_rows=8 view_cols=16 gain=1.0 conv=0.0 near_permille=20 " \
        "margin=1.0 pad=8 limit_lo=-4.0 limit_hi=4.0 rate_near=1.0 rate_far=0.1 restart=0 state=P"
VIEWS = "views=P out=P num_views=8 %sin_rows=8 in_cols=16 out_rows=8 out_cols=16 elem_sz=3"
NV12_IN = "y=P pitch_y=32 uv=P pitch_uv=32 "
SPLIT_ARGS = "num_rows=8 num_cols_sbs=32 num_cols_out=16 elem_sz=3"
LOW_ARGS = "num_rows=8 num_cols_sbs=32 num_cols=16 num_rows_disp=4 num_cols_disp=8 elem_sz=3"
LOW_OUT = "img_l=P img_r=P low_l=P low_r=P census_l=P census_r=P "
IMG = 8 * 16 * 3  # the bytes of the passing image


def depth_fit_rules(rect):
    def rules(d):
        r = [("size", BIG)] + DEPTH_AUTO + ([RECT_IN("rect")] if rect and not d else [])
        return dims(RC) + chain([("dim-num_cols", {"num_cols": 0})] + r)
    return rules


def overlay_fit_rules(rect):
    def rules(d):
        ov = OVERLAY("overlay", d) + ([] if d else [("overlay-null", {"overlay": 0})])  # the host flavour's null check comes after the numbers
        r = [("size", BIG)] + ov + DEPTH1 + OVERLAY_AUTO + ([RECT_IN("rect")] if rect and not d else [])
        return dims(RC + [("view_rows", 1), ("view_cols", 1)]) + chain([("dim-view_cols", {"view_cols": 0})] + r)
    return rules


def overlay_stage_rules(d):
    ov = OVERLAY("overlay", d) + [rng("disparity", 5000.0, -5000.0, nan=NAN)] + ([] if d else [("overlay-null", {"overlay": 0})])
    lens = [("lens-mode", {"lens_mode": -1}, {"high": {"lens_mode": 4}}), ("pitch", {"lens_mode": 1, "pitch": NAN}),
            ("slope", {"lens_mode": 2, "slope": INF}), ("centre", {"lens_mode": 3, "centre": NAN})]
    quilt = [("layout", {"layout": 2}, {"low": {"layout": -1}})] + [(n, dict(o, layout=1), {k: dict(v, layout=1) for k, v in e.items()}) for n, o, e in LAYOUT] + \
        [("tiles", dict(layout=1, tiles_x=256, tiles_y=256, num_views=65536)), ("quilt-lens", dict(layout=1, lens_mode=1)),
         ("quilt-views", dict(layout=1, num_views=7)), ("quilt-no-column", dict(layout=1, out_cols=3)), ("quilt-no-row", dict(layout=1, out_rows=1))]
    out = dims([("num_views", 2), ("out_rows", 1), ("out_cols", 1), ("elem_sz", 3)]) + chain([("dim-elem_sz", {"elem_sz": 2})] + ov + lens) + chain(quilt)
    out += [("lens+layout", dict(lens_mode=4, layout=2)), ("tiles+quilt-lens", dict(layout=1, tiles_x=256, tiles_y=256, num_views=65536, lens_mode=1)),
            ("quilt-lens+views", dict(layout=1, lens_mode=2, num_views=7))]
    return out + [(l, o, "mux_multiview") for l, o in chain([GEOM])]


ENTRIES = {}
for e in (
    only_dims("ci_adcensus", "img_l=P img_r=P cost_l=P cost_r=P " + COST,
              "d_img_l=P d_img_r=P d_cost_l=P d_cost_r=P h_cost_l=P h_cost_r=P mem=P " + COST, D3 + [("elem_sz", 3)]),
    only_dims("ca_cross", "img=P cross=P cost=P acost=P " + CROSS, "d_img=P d_cost=P d_acost=P h_acost=P mem=P d_cross=P " + CROSS,
              D3 + [("elem_sz", 3)]),
    only_dims("dc_wta", *["cost=P disp=P num_disp=4 zero_disp=2 " + ROWS] * 2, D3),
    only_dims("dc_subpixel", *["cost=P disp=P num_disp=4 zero_disp=2 " + ROWS] * 2, D3),
    only_dims("dc_hslo", *["cost=P disp=P img_l=P img_r=P T=15.0 H1=1.0 H2=3.0 num_disp=4 zero_disp=2 " + COLS] * 2, D3 + [("elem_sz", 3)]),
    only_dims("dr_dcc", *["outliers_l=P outliers_r=P disp_l=P disp_r=P " + ROWS] * 2, RC),
    only_dims("dr_irv", *["disp=P outliers=P cross=P thresh_s=20 thresh_h=0.4 " + ROWS + " num_disp=4 zero_disp=2 usd=5 iterations=2"] * 2,
              RC + [("num_disp", 1)]),
    only_dims("dr_interp", *["disp=P outliers=P img=P " + COLS] * 2, RCE),
    only_dims("filter_bilateral_1", *["img=P radius=2 sigma_color=5.0 sigma_spatial=3.0 " + ROWS + " num_disp=4"] * 2,
              [("radius", 0)] + RC + [("num_disp", 1)]),
    only_dims("filter_gaussian_1", *["img=P radius=2 sigma_spatial=3.0 " + ROWS] * 2, [("radius", 0)] + RC),
    only_dims("filter_bleed_1", *["img=P radius=2 " + ROWS] * 2, [("radius", 0)] + RC),
    only_dims("filter_median", *["img=P " + ROWS] * 2, RC),
    only_dims("generate_gaussian_kernel", "kernel=P radius=2 sigma=1.0", None, [("radius", 0)]),
    only_dims("dibr_occl", *["occl_l=P occl_r=P disp_l=P disp_r=P " + ROWS] * 2, RC),
    only_dims("dibr_occl_to_mask", *["mask_l=P mask_r=P occl_l=P occl_r=P " + ROWS] * 2, RC),
    only_dims("dibr_dbm", DBM, DBM, RCE),
    only_dims("dibr_dbm_lin", DBM, DBM, RCE),
    only_dims("dibr_dfm", *["img_out=P img_in_l=P img_in_r=P disp_l=P disp_r=P shift=0.5 " + COLS] * 2, RCE),
    only_dims("demux_sbs", None, "img_l=P img_r=P img_sbs=P " + SPLIT_ARGS, SPLIT),
    only_dims("d_tx_scale", "img_in=P img_out=P in_rows=8 in_cols=16 out_rows=4 out_cols=8 elem_sz=3", None,
              [("in_rows", 1), ("in_cols", 1), ("out_rows", 1), ("out_cols", 1), ("elem_sz", 3)]),  # host pointers despite its name
    stage("disp_upsample", *["disp_out=P disp_low=P img_low=P img=P out_rows=8 out_cols=16 in_rows=4 in_cols=8 elem_sz=3 up=2.0 sigma_color=10.0"] * 2,
          lambda d: dims([("out_rows", 1), ("out_cols", 1), ("in_rows", 1), ("in_cols", 1), ("elem_sz", 3)]) +
          chain([("dim-elem_sz", {"elem_sz": 2}), ("sigma_color", {"sigma_color": 0.0}, {"negative": {"sigma_color": -1.0}, "nan": {"sigma_color": NAN}})])),
    stage("disp_temporal", *["disp=P disp_prev=P img=P img_prev=P " + COLS + " alpha=0.5 thresh_color=30 thresh_disp=1.0"] * 2,
          lambda d: dims(RCE) + chain([("dim-elem_sz", {"elem_sz": 2}), rng("alpha", -0.25, 1.5, nan=NAN), rng("thresh_color", -1, 766),
                                       ("thresh_disp", {"thresh_disp": -1.0}, {"nan": {"thresh_disp": NAN}}),
                                       ("alias", {"disp_prev": P(1)}, {"tail": {"disp_prev": P(1) + 8 * 16 * 4 - 4}, "head": {"disp_prev": P(1) - 8 * 16 * 4 + 4}})])),
    stage("depth_fit", FIT, FIT, depth_fit_rules(False)),
    stage("depth_fit_rect", FIT + " rect=[0,8,0,16]", FIT + " rect=P", depth_fit_rules(True)),
    stage("overlay_fit", OVFIT, OVFIT + " cut_state=0", overlay_fit_rules(False)),
    stage("overlay_fit_rect", OVFIT + " rect=[0,8,0,16]", OVFIT + " cut_state=0 rect=P", overlay_fit_rules(True)),
    stage("align_rows", *["img_out=P img=P " + COLS + " a=0.5 b=0.0 c=0.0"] * 2,
          lambda d: dims(RCE) + chain([("dim-elem_sz", {"elem_sz": 2})] + ALIGN1 + [nulls("img_out", "img"), OVERLAP("img_out", "img", IMG)])),
    stage("align_fit", "img_l=P img_r=P " + COLS + " radius=16 rate=1.0 state=P", "img_l=P img_r=P " + COLS + " radius=16 rate=1.0 state=P valid_blocks=P profiles=0 sad=0",
          lambda d: dims(RCE) + chain([("dim-elem_sz", {"elem_sz": 2}), ("small", {"num_rows": 3}, {"cols": {"num_cols": 7}}), ("sums", WIDE)]) +
          chain([("small", {"num_rows": 3})] + ALIGN_AUTO + [nulls("img_l", "img_r", "state")])),
    stage("balance_fit", "img_l=P img_r=P " + COLS + " max_shift=48 rate=1.0 state=P", "img_l=P img_r=P " + COLS + " max_shift=48 rate=1.0 state=P hist=0",
          lambda d: dims(RCE) + chain([("dim-elem_sz", {"elem_sz": 2}), ("size", BIG)] + BALANCE_AUTO + [nulls("img_l", "img_r", "state")])),
    stage("balance_apply", *["img_out=P img=P " + COLS + " lut768=P state=0"] * 2,
          lambda d: dims(RCE) + chain([("dim-elem_sz", {"elem_sz": 2}), nulls("img_out", "img"),
                                       ("one-of", {"state": P(9)}, {"neither": {"lut768": 0}}), OVERLAP("img_out", "img", IMG)])),
    stage("cut_detect", "img_l=P " + COLS + " thresh_permille=370 min_gap=1 state=P", "img_l=P " + COLS + " thresh_permille=370 min_gap=1 state=P reset0=0 reset1=0 reset2=0 sig=0",
          lambda d: dims([("num_rows", 4), ("num_cols", 4), ("elem_sz", 3)]) + chain([("dim-elem_sz", {"elem_sz": 2}), ("size", BIG)] + CUT + [nulls("img_l", "state")])),
    stage("active_detect", "img_l=P " + COLS + " thresh_luma=24 lit_permille=10 max_bar_permille=300 hold=12 restart=0 state=P",
          "img_l=P " + COLS + " thresh_luma=24 lit_permille=10 max_bar_permille=300 hold=12 restart=0 state=P cut_state=0 counts=0",
          lambda d: dims(RCE) + chain([("dim-elem_sz", {"elem_sz": 2}), ("size", BIG)] + ACTIVE_AUTO + [nulls("img_l", "state")])),
    stage("active_fill", "disp=P " + ROWS + " rect=[0,8,0,16] value=0.0", "disp=P " + ROWS + " rect=P value=0.0",
          lambda d: dims(RC) + chain([("dim-num_cols", {"num_cols": 0}), nulls("disp")] + ([] if d else [RECT_IN("rect")]))),
    stage("view_prefilter", *["img_out=P img=P disp=P " + COLS + " num_views=8 strength=1.0 max_radius=4 gate=0.5 gain=1.0 conv=0.0"] * 2,
          lambda d: dims(RCE + [("num_views", 2)]) + chain([("dim-num_views", {"num_views": 1})] + ANTIALIAS + DEPTH1 +
                                                           [nulls("img_out", "img", "disp"), OVERLAP("img_out", "img", IMG)])),
    stage("mux_multiview", *[VIEWS % "angle=18.43 "] * 2,
          lambda d: dims(MUX) + ([(l, o, "mux_multiview") for l, o in chain([GEOM])] + [("dim-elem_sz+angle", dict(elem_sz=2, angle=0.0))] if d else [])),
    stage("mux_multiview_lens", *[VIEWS % "mode=1 pitch=5.0 slope=0.3 centre=0.0 "] * 2,
          lambda d: dims(MUX) + chain([("dim-elem_sz", {"elem_sz": 2})] + LENS((0, 3)))),
    stage("quilt_multiview", *[VIEWS % "tiles_x=4 tiles_y=2 order=0 filter=0 "] * 2,
          lambda d: dims(MUX) + chain([("dim-elem_sz", {"elem_sz": 2})] + LAYOUT + [rng("filter", -1, 2), ("quilt-views", {"num_views": 7}),
                                      ("quilt-no-column", {"out_cols": 3}), ("quilt-no-row", {"out_rows": 1}),
                                      ("quilt-wide-tile", dict(out_cols=1 << 30, in_cols=1 << 20, tiles_x=1, tiles_y=8)),
                                      ("quilt-tall-tile", dict(out_rows=1 << 30, in_rows=1 << 20, tiles_x=8, tiles_y=1))])),
    stage("mux_overlay", *["frame=P overlay=P ov_rows=2 ov_cols=2 x0=0 y0=0 disparity=0.0 num_views=8 angle=18.43 lens_mode=0 pitch=5.0 slope=0.3 "
                           "centre=0.0 layout=0 tiles_x=4 tiles_y=2 order=0 out_rows=8 out_cols=16 elem_sz=3"] * 2, overlay_stage_rules),
    stage("demux_nv12", *["img_l=P img_r=P " + NV12_IN + SPLIT_ARGS + " matrix=0"] * 2,
          lambda d: dims(SPLIT) + chain([("dim-elem_sz", {"elem_sz": 2})] + NV12("num_cols_out"))),
    stage("mux_nv12", *["y=P pitch_y=16 uv=P pitch_uv=16 img=P " + COLS + " matrix=0"] * 2,
          lambda d: dims([("num_rows", 2), ("num_cols", 2), ("elem_sz", 3)]) +
          chain([("dim-elem_sz", {"elem_sz": 2}), ("odd-rows", {"num_rows": 7}), ("odd-cols", {"num_cols": 15}), ("pitch_y", {"pitch_y": 15}),
                 ("pitch_uv", {"pitch_uv": 15}), rng("matrix", -1, 4)])),
    stage("demux_packed", *["img_l=P img_r=P img=P " + SPLIT_ARGS + " packing=0 swap=0 filter=0 gap=0"] * 2,
          lambda d: dims(SPLIT) + chain([("dim-elem_sz", {"elem_sz": 2})] + PACKING) +
          chain([PACKING[-1][:2], ("odd-cols", dict(packing=1, num_cols_out=15)), ("odd-rows", dict(packing=3, num_rows=7)),
                 ("narrow", dict(swap=1, num_cols_sbs=31), {"gap": dict(gap=5, num_cols_sbs=36), "rows": dict(packing=2, num_cols_sbs=15)})]) +
          [("odd-cols+narrow", dict(packing=1, num_cols_out=15, num_cols_sbs=10))]),
    stage("demux_nv12_packed", *["img_l=P img_r=P " + NV12_IN + SPLIT_ARGS + " matrix=0 packing=0 swap=1 filter=0 gap=0"] * 2,
          lambda d: dims(SPLIT) + chain([("dim-elem_sz", {"elem_sz": 2})] + PACKING) +
          chain([("narrow", dict(num_cols_sbs=31)), ("nv12-rows", dict(num_rows=7), {"rows4": dict(packing=3, num_rows=6)}),
                 ("nv12-cols", dict(num_cols_out=15), {"cols4": dict(packing=1, num_cols_out=18)}), ("nv12-gap", dict(gap=1, num_cols_sbs=34)),
                 ("nv12-pitch_y", dict(pitch_y=31)), ("nv12-pitch_uv", dict(pitch_uv=30)), rng("matrix", -1, 4)])),
    stage("demux_sbs_low", LOW_OUT + "img_sbs=P " + LOW_ARGS, LOW_OUT + "img_sbs=P " + LOW_ARGS,
          lambda d: dims(LOW) + chain([("dim-elem_sz", {"elem_sz": 2}), ("census", {"census_l": 0}, {"right": {"census_r": 0}})])),
    stage("demux_nv12_low", *[LOW_OUT + NV12_IN + LOW_ARGS + " matrix=0"] * 2,
          lambda d: dims(LOW) + chain([("dim-elem_sz", {"elem_sz": 2}), ("census", {"census_l": 0}, {"right": {"census_r": 0}})] + NV12("num_cols"))),
    # ---- the thread setters (their names in the messages: set_lens, ...)
    stage("set_lens", "mode=1 pitch=5.0 slope=0.3 centre=0.0", None, lambda d: chain(LENS((-1, 4)))),
    stage("set_layout", "layout=1 tiles_x=4 tiles_y=2 order=0 filter=0", None,
          lambda d: chain([("layout", {"layout": 2}, {"low": {"layout": -1}})] + LAYOUT + [rng("filter", -1, 2)])),
    stage("set_output", "format=1 matrix=0 pitch=0 uv_row=0", None,
          lambda d: chain([rng("format", -1, 2), rng("matrix", -1, 4), ("pitch", {"pitch": -1}), ("uv_row", {"uv_row": -1})])),
    stage("set_overlay", "mode=1 d_overlay=P ov_rows=2 ov_cols=2 x0=0 y0=0 disparity=0.0", None,
          lambda d: chain([rng("mode", -1, 2)] + OVERLAY("d_overlay", True) + [rng("disparity", 5000.0, -5000.0, nan=NAN, inf=INF)])),
    stage("set_overlay_auto", "mode=1 near_permille=20 margin=1.0 pad=8 limit_lo=-4.0 limit_hi=4.0 rate_near=1.0 rate_far=0.1 d_state=0", None,
          lambda d: chain([rng("mode", -1, 2)] + OVERLAY_AUTO)),
    stage("set_packing", "packing=1 swap=0 filter=0 gap=0", None, lambda d: chain(PACKING)),
    stage("set_depth", "mode=1 gain=1.0 conv=0.0", None,
          lambda d: chain([rng("mode", -1, 3)] + DEPTH1) + [("auto-without-budget", {"mode": 2})]),  # a fresh thread has no budget yet
    stage("set_depth_auto", "disp_lo=-2.0 disp_hi=2.0 max_gain=4.0 clip_permille=20 rate=0.5 d_state=0", None, lambda d: chain(DEPTH_AUTO)),
    stage("set_antialias", "mode=1 strength=1.0 max_radius=4 gate=0.5", None, lambda d: chain([rng("mode", -1, 2)] + ANTIALIAS)),
    stage("set_align", "mode=1 a=0.5 b=0.0 c=0.0", None, lambda d: chain([rng("mode", -1, 3)] + ALIGN1)),
    stage("set_align_auto", "radius=16 rate=1.0 d_state=0", None, lambda d: chain(ALIGN_AUTO)),
    stage("set_balance", 'mode=1 lut768="identity"', None, lambda d: chain([rng("mode", -1, 3), ("lut768", {"lut768": 0})])),
    stage("set_balance_auto", "max_shift=48 rate=1.0 d_state=0", None, lambda d: chain(BALANCE_AUTO)),
    stage("set_cut", "mode=1 thresh_permille=370 min_gap=1 d_state=P", None, lambda d: chain([rng("mode", -1, 2)] + CUT + [("d_state", {"d_state": 0})])),
    stage("set_active", "mode=1 rect=[0,8,0,16] fill=0 fill_disp=0.0", None,
          lambda d: chain([rng("mode", -1, 3), ("rect-null", {"rect": 0}),
                           ("rect", {"rect": [4, 4, 0, 16]}, {"left": {"rect": [0, 8, 9, 3]}, "negative": {"rect": [-1, 8, 0, 16]}}),
                           rng("fill", -1, 2), rng("fill_disp", 5000.0, -5000.0, nan=NAN)]) +
          [("fill-measured", dict(mode=2, rect=0, fill=2)), ("fill_disp-measured", dict(mode=2, rect=0, fill_disp=NAN))]),
    stage("set_active_auto", "thresh_luma=24 lit_permille=10 max_bar_permille=300 hold=12 d_state=0", None, lambda d: chain(ACTIVE_AUTO)),
    stage("set_agg_tap", "d_h1=0 d_v2=0 d_h4=0 d_inject_v2=0", None,
          lambda d: chain([(n, {n: P(k + 1) + 2}) for k, n in enumerate(["d_h1", "d_v2", "d_h4", "d_inject_v2"])])),
    stage("set_irv_chunk", "entries=4", None, lambda d: chain([rng("entries", -1, 17)])),
):
    ENTRIES.update(e)

# the exported entries this table leaves out, each for its reason; tests/test_entry_screening.py holds the rest of _lib.PROTOS against ENTRIES
FRAME_ENTRIES = set(frame.ENTRIES)                          # pinned by frame_screening.json
STREAM_PREFIX = "stm_stream_"                               # need a stream, so a device: stream_screening.json
NO_SCREEN = {
    "stm_version", "stm_set_stream", "stm_get_stream", "stm_set_error_mode", "stm_last_error", "stm_release_workspace",  # refuse nothing
    "stm_prof_enable", "stm_prof_reset", "stm_prof_read",                                                               # clamp or count
    "stm_set_agg_variant", "stm_set_irv_paper_ratio", "stm_set_ref_quirks", "stm_set_quilt_lds_limit",                  # take any int
    "stm_agg_path", "stm_first_pass_path", "stm_px_order", "stm_irv_path",                                              # answer 0 / -1, no error
    "stm_get_layout", "stm_get_output", "stm_get_overlay", "stm_get_overlay_auto", "stm_get_packing", "stm_get_antialias", "stm_get_align",
    "stm_get_balance", "stm_get_cut", "stm_get_active",                                                                  # getters
    "stm_bmp_read", "stm_bmp_write", "stm_bmp_free",                                                                     # file helpers, no fail()
}


def cases():
    out = []
    for name, ((names, base), rules) in ENTRIES.items():
        for r in rules:
            label, over = r[0], r[1]
            vals = dict(base, **over)
            assert set(over) <= set(base), (name, label, set(over) - set(base))
            out.append(dict(entry=name, label=label, settings=[], args=[vals[n] for n in names], says=r[2] if len(r) > 2 else name[4:]))
    return out


# ------------------------------------------------------------------------------------------------- running a case (the tests' too)
# every thread setting back to its default: the frame table's list and the settings it does not use
RESET = frame.RESET + [["stm_set_depth", [0, 0.0, 0.0]], ["stm_set_antialias", [0, 0.0, 0, 0.0]], ["stm_set_active", [0, 0, 0, 0.0]],
                       ["stm_set_overlay_auto", [0, 0, 0.0, 0, 0.0, 0.0, 0.0, 0.0, 0]], ["stm_set_agg_tap", [0, 0, 0, 0]], ["stm_set_irv_chunk", [0]]]


def materialise(args):
    """an argument written as a list becomes an int array in host memory (the screen reads it); returns the arguments and what keeps
    the arrays alive"""
    keep = [(ctypes.c_int * len(a))(*a) for a in args if isinstance(a, list)]
    it = iter(keep)
    return [ctypes.addressof(next(it)) if isinstance(a, list) else a for a in args], keep


def run(lib, protos, case):
    """the case's call (error mode 1, set by the caller): stm_last_error() after its first line; every setting reset behind it"""
    args, keep = materialise(case["args"])
    try:
        return refusal(lib, protos, dict(case, args=args))
    finally:
        apply_settings(lib, protos, RESET)
        del keep


def in_fresh_thread(fn):
    """fn() on a thread of its own, whose settings are the defaults whatever the caller's thread has set (a depth budget cannot be
    taken back, and set_depth's mode 2 is refused only without one)"""
    box = {}

    def body():
        try:
            box["value"] = fn()
        except BaseException as e:  # noqa: B902 -- handed to the caller's thread
            box["error"] = e
    t = threading.Thread(target=body)
    t.start()
    t.join()
    if "error" in box:
        raise box["error"]
    return box["value"]


def load_table(path=OUT):
    """({(entry, label): text}, the commit in the header).  A row is [label, text, entries]: the entries (without stm_, space-separated)
    whose case `label` is refused with "<name>: " + text, <name> being the case's `says`"""
    rows = json.load(open(path))
    assert rows[0][0] == "#commit"
    return {("stm_" + e, label): text for label, text, entries in rows[1:] for e in entries.split()}, rows[0][1]


def record(lib, protos, all_cases, runner):
    rows = {}  # (label, text) -> entries, in the order of first appearance
    for c in all_cases:
        assert len(c["args"]) + ("before" in c) == len(protos[c["entry"]][0]), c["entry"]  # (a stream case: the handle comes first)
        msg = runner(lib, protos, c)
        assert msg.startswith(c["says"] + ": "), (c["entry"], c["label"], msg)  # refused by the entry's own screen, or not a row
        rows.setdefault((c["label"], msg[len(c["says"]) + 2:]), []).append(c["entry"][4:])
    return rows


def write(path, rows, n):
    if "--commit" in sys.argv:  # a tree exported without its history: the caller names the commit it was exported from
        commit = sys.argv[sys.argv.index("--commit") + 1]
    else:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"]).decode().strip()
        dirty = subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain", "--", "stereo-to-multiview-cuda_amd/csrc", "include"]).decode().strip()
        assert not dirty, "the library's sources differ from the commit the table would name:\n" + dirty
    head = ["#commit", commit, "the library these refusals were recorded from was built at this commit"]
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in [head] + [[label, text, " ".join(e)] for (label, text), e in rows.items()]) + "\n]\n")
    print("%d cases in %d rows, %d distinct texts, longest %d bytes -> %s" % (n, len(rows), len({t for _, t in rows}),
                                                                             max(len(t) for _, t in rows), path))


# ------------------------------------------------------------------------------------------------- the stream setters (GPU)
# one stream of a small frame; the setters refuse on the host, before the first submit and, after one submit / collect, with "only
# before the first submit".  stm_stream_create itself has no screen: it is not a row
STREAM = dict(num_rows=40, num_cols_sbs=128, num_cols=64, num_rows_out=40, num_cols_out=64, elem_sz=3, num_views=8, angle=18.43, num_disp=16,
              zero_disp=8, ad_coeff=10.0, census_coeff=30.0, ucd=20.0, lcd=6.0, usd=17, lsd=8, thresh_s=20, thresh_h=0.4)
NARROW = dict(STREAM, num_cols_sbs=127)   # no room for two views side by side, and odd
# (a stream of 2^31 pixels cannot be created: the *_size_ok rules of the stream setters are pinned through the stages that share them)

# setter -> (argument spec without the handle: a call a fresh stream accepts; the rules a fresh stream's screen can fire)
STREAM_SETTERS = {
    "stm_stream_set_stages": ("stages=3", [("stages-guided", {"stages": 3 | 0x1000}), ("stages-hslo", {"stages": 3 | 0x100}), ("stages-2", {"stages": 2}),
                                           ("stages-guided+hslo", {"stages": 3 | 0x1000 | 0x100})]),
    "stm_stream_set_match_size": ("num_rows_disp=20 num_cols_disp=32 disp_scale=0.5",
                                  chain([("size", {"num_rows_disp": 0}, {"cols": {"num_cols_disp": -1}}),
                                         ("disp_scale", {"disp_scale": 0.0}, {"nan": {"disp_scale": NAN}, "inf": {"disp_scale": INF}})])),
    "stm_stream_set_temporal": ("alpha=0.5 thresh_color=24 thresh_disp=1.5",
                                chain([rng("alpha", -0.25, 1.5, nan=NAN), rng("thresh_color", -1, 766), ("thresh_disp", {"thresh_disp": -1.0}, {"nan": {"thresh_disp": NAN}})])),
    "stm_stream_set_input": ("format=1 matrix=0", chain([rng("format", -1, 2), rng("matrix", -1, 4)])),
    "stm_stream_set_packing": ("packing=0 swap=1 filter=0 gap=0", chain(PACKING) + [("narrow", dict(gap=2))]),
    "stm_stream_set_lens": ("mode=1 pitch=5.0 slope=0.3 centre=0.0", chain(LENS((-1, 4)))),
    "stm_stream_set_layout": ("layout=1 tiles_x=4 tiles_y=2 order=0 filter=0", chain([("layout", {"layout": 2})] + LAYOUT + [rng("filter", -1, 2)])),
    "stm_stream_set_output": ("format=0 matrix=0", chain([rng("format", -1, 2)]) + [("matrix", dict(format=1, matrix=4)), ("no-quilt", dict(format=1))]),
    "stm_stream_set_overlay": ("max_rows=4 max_cols=4", [("size", {"max_rows": 0}), ("size-high", {"max_cols": 65536}), ("size-negative", {"max_rows": -1})]),
    "stm_stream_overlay": ("overlay=P ov_rows=2 ov_cols=2 x0=0 y0=0 disparity=0.0", [("no-overlay", {})]),
    "stm_stream_set_overlay_auto": ("mode=1 near_permille=20 margin=1.0 pad=8 limit_lo=-4.0 limit_hi=4.0 rate_near=1.0 rate_far=0.1",
                                    chain([rng("mode", -1, 2)] + OVERLAY_AUTO) + [("no-overlay", {})]),
    "stm_stream_set_depth": ("mode=1 gain=1.0 conv=0.0", chain([rng("mode", -1, 3)] + DEPTH1) + [("auto-without-budget", {"mode": 2})]),
    "stm_stream_set_depth_auto": ("disp_lo=-2.0 disp_hi=2.0 max_gain=4.0 clip_permille=20 rate=0.5", chain(DEPTH_AUTO)),
    "stm_stream_set_antialias": ("mode=1 strength=1.0 max_radius=4 gate=0.5", chain([rng("mode", -1, 2)] + ANTIALIAS)),
    "stm_stream_set_align": ("mode=1 a=0.5 b=0.0 c=0.0", chain([rng("mode", -1, 3)] + ALIGN1)),
    "stm_stream_set_align_auto": ("radius=16 rate=1.0", chain(ALIGN_AUTO)),
    "stm_stream_set_balance": ('mode=1 lut768="identity"', chain([rng("mode", -1, 3), ("lut768", {"lut768": 0})])),
    "stm_stream_set_balance_auto": ("max_shift=48 rate=1.0", chain(BALANCE_AUTO)),
    "stm_stream_set_cut": ("mode=1 thresh_permille=370 min_gap=1", chain([rng("mode", -1, 2)] + CUT)),
    "stm_stream_set_active": ("mode=1 rect=[0,40,0,64] fill=0 fill_disp=0.0 thresh_luma=24 lit_permille=10 max_bar_permille=300 hold=12",
                              chain([rng("mode", -1, 3), ("rect-null", {"rect": 0}), ("rect", {"rect": [4, 4, 0, 64]}), rng("fill", -1, 2),
                                     rng("fill_disp", 5000.0, -5000.0, nan=NAN), ("rect-outside", {"rect": [0, 41, 0, 64]}, {"wide": {"rect": [0, 40, 0, 65]}})]) +
                              chain([(n, dict(o, mode=2), {k: dict(v, mode=2) for k, v in e.items()}) for n, o, e in ACTIVE_AUTO])),
}
# what the stream is given before the case's call: the rules that depend on the stream's own state
STREAM_STATES = [
    # (label, setter, overrides, the calls that come first, the stream's geometry)
    ("guided-without-size-off", "stm_stream_set_match_size", dict(num_rows_disp=0, num_cols_disp=0),
     [["stm_stream_set_match_size", [20, 32, 0.5]], ["stm_stream_set_stages", [3 | 0x1000]]], STREAM),
    ("stages-reduced", "stm_stream_set_stages", dict(stages=3 | 0x100), [["stm_stream_set_match_size", [20, 32, 0.5]]], STREAM),
    ("packed", "stm_stream_set_match_size", {}, [["stm_stream_set_packing", [0, 1, 0, 0]]], STREAM),
    ("match-size", "stm_stream_set_packing", {}, [["stm_stream_set_match_size", [20, 32, 0.5]]], STREAM),
    ("nv12-odd", "stm_stream_set_input", {}, [], NARROW),
    ("nv12-packed-gap", "stm_stream_set_input", {}, [["stm_stream_set_packing", [1, 0, 0, 1]]], STREAM),
    ("nv12-gap", "stm_stream_set_packing", dict(packing=1, swap=0, gap=1), [["stm_stream_set_input", [1, 0]]], STREAM),
    ("narrow-stream", "stm_stream_set_packing", {}, [], NARROW),
    ("layout-0-under-nv12", "stm_stream_set_layout", dict(layout=0), [["stm_stream_set_layout", [1, 4, 2, 0, 0]], ["stm_stream_set_output", [1, 0]]], STREAM),
    ("nv12-with-overlay", "stm_stream_set_output", dict(format=1), [["stm_stream_set_layout", [1, 4, 2, 0, 0]], ["stm_stream_set_overlay", [4, 4]]], STREAM),
    ("overlay-under-nv12", "stm_stream_set_overlay", {}, [["stm_stream_set_layout", [1, 4, 2, 0, 0]], ["stm_stream_set_output", [1, 0]]], STREAM),
    ("too-large", "stm_stream_overlay", dict(overlay=[0] * 20, ov_rows=5, ov_cols=4), [["stm_stream_set_overlay", [4, 4]]], STREAM),
    ("too-wide", "stm_stream_overlay", dict(overlay=[0] * 20, ov_rows=4, ov_cols=5), [["stm_stream_set_overlay", [4, 4]]], STREAM),
    ("ov_rows", "stm_stream_overlay", dict(overlay=[0] * 4, ov_rows=-1), [["stm_stream_set_overlay", [4, 4]]], STREAM),
    ("ov_cols", "stm_stream_overlay", dict(overlay=[0] * 4, ov_cols=65536), [["stm_stream_set_overlay", [4, 4]]], STREAM),
    ("x0", "stm_stream_overlay", dict(overlay=[0] * 4, x0=65537), [["stm_stream_set_overlay", [4, 4]]], STREAM),
    ("y0", "stm_stream_overlay", dict(overlay=[0] * 4, y0=-65537), [["stm_stream_set_overlay", [4, 4]]], STREAM),
    ("disparity", "stm_stream_overlay", dict(overlay=[0] * 4, disparity=NAN), [["stm_stream_set_overlay", [4, 4]]], STREAM),
    ("ov_rows+too-large", "stm_stream_overlay", dict(overlay=[0] * 4, ov_rows=65536, ov_cols=5), [["stm_stream_set_overlay", [4, 4]]], STREAM),
    ("narrow", "stm_stream_set_align", {}, [], NARROW),
    ("narrow-auto", "stm_stream_set_align", dict(mode=2), [], NARROW),
    ("narrow", "stm_stream_set_balance", {}, [], NARROW),
    ("narrow-auto", "stm_stream_set_balance", dict(mode=2), [], NARROW),
    ("a+narrow", "stm_stream_set_align", dict(a=NAN), [], NARROW),
    ("mode+narrow", "stm_stream_set_balance", dict(mode=3), [], NARROW),
]
# a call every setter accepts on a fresh stream is refused after the first submit; stm_stream_overlay has no such rule
AFTER_SUBMIT = {name: {} for name in STREAM_SETTERS if name != "stm_stream_overlay"}
AFTER_SUBMIT["stm_stream_set_input"] = dict(format=0)         # (format 1 would allocate)
AFTER_SUBMIT["stm_stream_set_overlay"] = dict(max_rows=0, max_cols=0)
AFTER_SUBMIT["stm_stream_set_overlay_auto"] = dict(mode=0)
AFTER_SUBMIT["stm_stream_set_depth"] = dict(mode=0)
AFTER_SUBMIT["stm_stream_set_align"] = dict(mode=0)
AFTER_SUBMIT["stm_stream_set_balance"] = dict(mode=0)
AFTER_SUBMIT["stm_stream_set_cut"] = dict(mode=0)
AFTER_SUBMIT["stm_stream_set_active"] = dict(mode=0, rect=0)
# ... and, each broken argument rule coming first, the cases where both are broken: the argument's message wins
AFTER_SUBMIT_BROKEN = {"stm_stream_set_stages": dict(stages=2), "stm_stream_set_temporal": dict(alpha=NAN), "stm_stream_set_lens": dict(mode=4),
                       "stm_stream_set_layout": dict(layout=2), "stm_stream_set_output": dict(format=2), "stm_stream_set_packing": dict(packing=4),
                       "stm_stream_set_depth_auto": dict(rate=NAN), "stm_stream_set_antialias": dict(mode=2), "stm_stream_set_cut": dict(mode=2),
                       "stm_stream_set_align_auto": dict(radius=0), "stm_stream_set_balance_auto": dict(max_shift=256),
                       "stm_stream_set_match_size": dict(disp_scale=NAN), "stm_stream_set_input": dict(format=2),
                       "stm_stream_set_overlay": dict(max_rows=65536), "stm_stream_set_overlay_auto": dict(mode=2),
                       "stm_stream_set_depth": dict(mode=3), "stm_stream_set_align": dict(mode=3), "stm_stream_set_balance": dict(mode=3),
                       "stm_stream_set_active": dict(mode=3)}


def stream_cases():
    """every case: entry, label, args (without the handle), `before` (the setter calls that prepare the stream), `geometry`, `submitted`"""
    out = []

    def add(name, label, over, before=(), geometry=STREAM, submitted=False):
        names, base = spec(STREAM_SETTERS[name][0])
        assert set(over) <= set(base), (name, label)
        vals = dict(base, **over)
        out.append(dict(entry=name, label=label, args=[vals[n] for n in names], before=[list(b) for b in before], geometry=geometry,
                        submitted=submitted, says=name[4:]))
    for name, (_, rules) in STREAM_SETTERS.items():
        for r in rules:
            add(name, r[0], r[1])
    for label, name, over, before, geometry in STREAM_STATES:
        add(name, label, over, before, geometry)
    for name, over in AFTER_SUBMIT.items():
        add(name, "after-submit", over, submitted=True)
    for name, over in AFTER_SUBMIT_BROKEN.items():
        add(name, "broken+after-submit", over, submitted=True)
    return out


class Streams:
    """the streams the cases run on: one per (geometry, submitted) that no case has changed yet -- a refused setter leaves the stream as
    it was, so a stream serves case after case; one prepared by `before` calls serves that case alone"""

    def __init__(self, lib, protos):
        self.lib, self.protos, self.clean = lib, protos, {}

    def create(self, geometry, submitted):
        import numpy as np
        lib = self.lib
        h = lib.stm_stream_create(*[geometry[n] for n in STREAM])
        assert h
        if submitted:  # one frame through: any picture will do
            frame_in = np.random.RandomState(5).randint(0, 256, size=(geometry["num_rows"], geometry["num_cols_sbs"], 3)).astype(np.uint8)
            assert lib.stm_stream_submit(h, frame_in.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))) == 0, lib.stm_last_error()
            assert lib.stm_stream_collect(h, None, None, None) == 0, lib.stm_last_error()
        return h

    def run(self, case):
        """the case's call on its stream: (the setter's return value, stm_last_error() after its first line)"""
        lib, key = self.lib, (json.dumps(case["geometry"], sort_keys=True), case["submitted"])
        own = bool(case["before"])
        if own or key not in self.clean:
            h = self.create(case["geometry"], case["submitted"])
            if not own:
                self.clean[key] = h
        else:
            h = self.clean[key]
        try:
            for setter, a in case["before"]:
                assert call(lib, self.protos, setter, [h] + a) == 0, (setter, a, lib.stm_last_error())
            args, keep = materialise(case["args"])
            lib.stm_d_filter_median(None, 0, 0)  # plant a known message: a call that records nothing shows this one
            rc = call(lib, self.protos, case["entry"], [h] + args)
            del keep
            return rc, lib.stm_last_error().decode().split("\n", 1)[1]
        finally:
            if own:
                lib.stm_stream_destroy(h)

    def close(self):
        for h in self.clean.values():
            self.lib.stm_stream_destroy(h)
        self.clean = {}


def main():
    sys.path.insert(0, ROOT)
    import stm_amd
    from stm_amd import _lib
    lib = stm_amd.lib()
    lib.stm_set_error_mode(1)
    try:
        if "--stream" in sys.argv[1:]:
            streams = Streams(lib, _lib.PROTOS)

            def runner(lib, protos, c):
                rc, msg = streams.run(c)
                assert rc == -1, (c["entry"], c["label"], rc)
                return msg
            try:
                all_cases = stream_cases()
                write(OUT_STREAM, record(lib, _lib.PROTOS, all_cases, runner), len(all_cases))
            finally:
                streams.close()
        else:
            all_cases = cases()
            write(OUT, in_fresh_thread(lambda: record(lib, _lib.PROTOS, all_cases, run)), len(all_cases))
    finally:
        lib.stm_set_error_mode(0)


if __name__ == "__main__":
    main()

"""Writes tests/golden/frame_screening.json: what the ten frame entries answer to calls they refuse before they touch the device.

    python tests/golden/make_frame_screening.py

A case (cases() below) is an entry, the thread settings to apply (setter calls) and the argument list (pointers as dummy addresses,
never dereferenced: 0 = null); cases() builds them from the rules, the same list every time.  The file holds what was recorded for
them: the text of stm_last_error() after its first line (the file:line of the fail site, which moves with the code), one row per
case label and text with the entries that gave it, since most rules read the same for every entry but for its name.  Run on the
library whose refusals are to be pinned; tests/test_frame_screening.py replays the cases against the file.  No GPU is needed or
used: a case that is not refused with a message of the entry's own name is an error here, not a table row."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "frame_screening.json")

FULL = ["img_sbs", "disp_l", "disp_r", "interlaced", "num_rows", "num_cols_sbs", "num_cols", "num_rows_out", "num_cols_out", "elem_sz",
        "num_views", "angle", "num_disp", "zero_disp", "ad_coeff", "census_coeff", "ucd", "lcd", "usd", "lsd", "thresh_s", "thresh_h"]
RED = FULL[:9] + ["num_rows_disp", "num_cols_disp", "elem_sz", "disp_scale"] + FULL[10:]
NV12_HEAD = ["y", "pitch_y", "uv", "pitch_uv", "matrix", "disp_l", "disp_r", "interlaced"]
HIST3 = ["prev_sbs", "prev_disp_l", "prev_disp_r", "alpha", "thresh_color", "thresh_disp"]
HIST4 = ["prev_img_l", "prev_img_r", "prev_disp_l", "prev_disp_r", "alpha", "thresh_color", "thresh_disp", "img_l", "img_r"]
# entry -> (argument names in order, reduced, host, NV12, history form, takes `stages`)
ENTRIES = {
    "stm_d_adcensus_stm": (FULL + ["stages"], False, False, False, 0, True),
    "stm_d_adcensus_stm_t": (FULL + ["stages"] + HIST3, False, False, False, 3, True),
    "stm_d_adcensus_stm_nv12": (NV12_HEAD + FULL[4:] + ["stages"] + HIST4, False, False, True, 4, True),
    "stm_d_adcensus_stm_2": (RED, True, False, False, 0, False),
    "stm_d_adcensus_stm_2s": (RED + ["stages"], True, False, False, 0, True),
    "stm_d_adcensus_stm_2t": (RED + ["stages"] + HIST3, True, False, False, 3, True),
    "stm_d_adcensus_stm_2nv12": (NV12_HEAD + RED[4:] + ["stages"] + HIST4, True, False, True, 4, True),
    "stm_adcensus_stm": (FULL, False, True, False, 0, False),
    "stm_adcensus_stm_2": (RED, True, True, False, 0, False),
    "stm_adcensus_stm_2s": (RED + ["stages"], True, True, False, 0, True),
}


def P(k):
    """a dummy address: far apart, so that no two buffers of any case's size overlap unless the case says so"""
    return k << 44


BASE = dict(img_sbs=P(1), disp_l=P(2), disp_r=P(3), interlaced=P(4), y=P(5), uv=P(6), img_l=P(7), img_r=P(8), prev_sbs=0, prev_img_l=0,
            prev_img_r=0, prev_disp_l=0, prev_disp_r=0, num_rows=8, num_cols_sbs=32, num_cols=16, num_rows_out=8, num_cols_out=16,
            num_rows_disp=4, num_cols_disp=8, elem_sz=3, disp_scale=0.5, num_views=8, angle=18.43, num_disp=4, zero_disp=2, ad_coeff=10.0,
            census_coeff=30.0, ucd=20.0, lcd=6.0, usd=5, lsd=3, thresh_s=20, thresh_h=0.4, stages=3, pitch_y=32, pitch_uv=32, matrix=0,
            alpha=0.5, thresh_color=30, thresh_disp=1.0)
T = 0x2000
ALL3 = dict(prev_sbs=P(9), prev_disp_l=P(10), prev_disp_r=P(11))
ALL4 = dict(prev_img_l=P(9), prev_img_r=P(12), prev_disp_l=P(10), prev_disp_r=P(11))


def geom(H, Wsbs, W, **more):
    """a frame geometry, the NV12 pitches following the frame's width and the output the view"""
    return dict(num_rows=H, num_cols_sbs=Wsbs, num_cols=W, pitch_y=Wsbs, pitch_uv=2 * ((Wsbs + 1) // 2), **more)


# settings: a list of setter calls; "identity" stands for the 768-byte identity table, an integer in a pointer's place for a dummy
# address (a state or an overlay, never read by a refused call)
PACK = lambda *a: ["stm_set_packing", list(a)]
ALIGN1 = [["stm_set_align", [1, 0.5, 0.0, 0.0]]]
ALIGN2 = [["stm_set_align_auto", [16, 1.0, 0]], ["stm_set_align", [2, 0.0, 0.0, 0.0]]]
BAL1 = [["stm_set_balance", [1, "identity"]]]
BAL2 = [["stm_set_balance_auto", [48, 1.0, 0]], ["stm_set_balance", [2, 0]]]
CUT = [["stm_set_cut", [1, 370, 1, P(13)]]]
QUILT = lambda tx, ty: [["stm_set_layout", [1, tx, ty, 0, 0]]]
NV12OUT = lambda pitch=0, uv_row=0: [["stm_set_output", [1, 0, pitch, uv_row]]]
OVERLAY = [["stm_set_overlay", [1, P(14), 2, 2, 0, 0, 0.0]]]
LENS = [["stm_set_lens", [1, 5.0, 0.3, 0.0]]]
BIG = geom(65536, 65536, 32768, num_rows_out=8, num_cols_out=16)  # num_rows * num_cols = 2^31
WIDE = geom(40000, 80000, 40000)                                     # the alignment measurement's 32-bit sums


def rules(name):
    """(label, argument overrides, settings) of every refusal this entry can give before it touches the device, each rule alone and,
    where two screens are adjacent, both broken at once (labels with a +: the first named wins)"""
    _, reduced, host, nv12, hist, has_stages = ENTRIES[name]
    out = []

    def add(label, over=None, settings=()):
        out.append((label, dict(over or {}), [list(s) for s in settings]))
    # ---- dimensions and elem_sz
    dims = ["num_rows", "num_cols_sbs", "num_cols", "num_rows_out", "num_cols_out"] + (["num_rows_disp", "num_cols_disp"] if reduced else []) + \
           ["elem_sz", "num_views", "num_disp"]
    lows = dict(elem_sz=2, num_views=1)
    for d in dims:
        add("dim-" + d, {d: lows.get(d, 0)})
    add("dim-negative", dict(num_rows=-5))
    for a, b in zip(dims, dims[1:]):
        add("dim-%s+%s" % (a, b), {a: lows.get(a, 0), b: lows.get(b, 0)})
    # ---- packing
    if reduced or host:
        add("packing-unsupported", {}, [PACK(1, 0, 0, 0)])
        add("dim-num_disp+packing", dict(num_disp=0), [PACK(1, 0, 0, 0)])
        if has_stages:
            add("packing+stages", dict(stages=2), [PACK(0, 1, 0, 0)])
    else:
        add("packing-odd-cols", geom(8, 32, 15), [PACK(1, 0, 0, 0)])
        add("packing-odd-rows", geom(7, 32, 16), [PACK(3, 0, 0, 0)])
        add("packing-narrow", geom(8, 31, 16), [PACK(0, 1, 0, 0)])
        add("packing-narrow-gap", geom(8, 20, 16), [PACK(1, 0, 0, 5)])
        add("packing-narrow-rows", geom(8, 15, 16), [PACK(2, 0, 0, 0)])
        add("dim-num_disp+packing", geom(8, 32, 15, num_disp=0), [PACK(1, 0, 0, 0)])
        add("packing-odd-cols+narrow", geom(8, 10, 15), [PACK(1, 0, 0, 0)])
        if nv12:
            add("packing-nv12-rows", geom(7, 32, 16), [PACK(0, 1, 0, 0)])
            add("packing-nv12-rows4", geom(6, 32, 16), [PACK(3, 0, 0, 0)])
            add("packing-nv12-cols", geom(8, 32, 15), [PACK(0, 1, 0, 0)])
            add("packing-nv12-cols4", geom(8, 32, 18), [PACK(1, 0, 0, 0)])
            add("packing-nv12-gap", geom(8, 34, 16), [PACK(0, 0, 0, 1)])
            add("packing-nv12-pitch_y", dict(pitch_y=31), [PACK(0, 1, 0, 0)])
            add("packing-nv12-pitch_uv", dict(pitch_uv=30), [PACK(0, 1, 0, 0)])
            add("packing-nv12-matrix", dict(matrix=4), [PACK(0, 1, 0, 0)])
            add("packing-nv12-gap+pitch_y", dict(geom(8, 34, 16), pitch_y=8), [PACK(0, 0, 0, 1)])
            add("packing-nv12+pair", dict(matrix=-1, img_r=0), [PACK(0, 1, 0, 0)])
        else:
            add("packing+history" if hist else "packing+0x2000", geom(8, 32, 15, stages=3 | T, alpha=2.0), [PACK(1, 0, 0, 0)])
    # ---- the NV12 frame and the image pair
    if nv12:
        add("nv12-rows", geom(7, 32, 16))
        add("nv12-cols", geom(8, 32, 15))
        add("nv12-narrow", geom(8, 30, 16))
        add("nv12-pitch_y", dict(pitch_y=31))
        add("nv12-pitch_uv", dict(pitch_uv=31))
        add("nv12-matrix", dict(matrix=4))
        add("nv12-rows+cols", geom(7, 32, 15))
        add("nv12-pitch_y+matrix", dict(pitch_y=0, matrix=-1))
        add("dim-num_disp+nv12", geom(7, 32, 16, num_disp=0))
        add("pair-left-only", dict(img_r=0))
        add("pair-right-only", dict(img_l=0))
        add("nv12-matrix+pair", dict(matrix=9, img_l=0))
        add("pair+history", dict(img_r=0, stages=3 | T, alpha=-1.0))
        if reduced:
            add("stages+nv12", geom(7, 32, 16, stages=2))
    # ---- the `stages` word of the reduced calls
    if reduced and has_stages:
        for s in (2, 1, 0, 3 | 0x4000, 3 | 0x8000, 0x1003 | 0x10000) + (() if hist else (3 | T,)):
            add("stages-0x%x" % s, dict(stages=s))
        add("stages-hslo-subpix", dict(stages=3 | 0x300))
        add("stages-0x2+hslo-subpix", dict(stages=2 | 0x300))
        add("dim-num_disp+stages", dict(num_disp=0, stages=2))
    # ---- bit 0x2000
    if name == "stm_d_adcensus_stm":
        add("0x2000-no-history", dict(stages=3 | T))
        add("0x2000+hslo-subpix", dict(stages=3 | T | 0x300))
    if hist:
        full = ALL3 if hist == 3 else ALL4
        some = dict(full, prev_disp_r=0)
        add("history-alpha", dict(stages=3 | T, alpha=1.5))
        add("history-alpha-negative", dict(full, stages=3 | T, alpha=-0.25))
        add("history-thresh_color", dict(stages=3 | T, thresh_color=766))
        add("history-thresh_color-negative", dict(stages=3 | T, thresh_color=-1))
        add("history-thresh_disp", dict(full, stages=3 | T, thresh_disp=-1.0))
        add("history-alpha+thresh_color", dict(stages=3 | T, alpha=1.5, thresh_color=-1))
        add("history-thresh_color+thresh_disp", dict(stages=3 | T, thresh_color=999, thresh_disp=-1.0))
        add("history-partial", dict(some, stages=3 | T))
        add("history-one-pointer", dict(prev_disp_l=P(10), stages=3 | T))
        add("history-thresh_disp+partial", dict(some, stages=3 | T, thresh_disp=-2.0))
        for k, (a, b) in enumerate([("prev_disp_l", "disp_l"), ("prev_disp_l", "disp_r"), ("prev_disp_r", "disp_l"), ("prev_disp_r", "disp_r")]):
            add("history-alias-%d" % k, dict(full, stages=3 | T, **{a: BASE[b]}))
        add("history-alias-tail", dict(full, stages=3 | T, prev_disp_l=BASE["disp_r"] + 8 * 16 * 4 - 4))
        if not reduced:
            add("history-stage-1", dict(stages=1 | T))
            add("history-thresh_disp+stage-1", dict(stages=1 | T, thresh_disp=-1.0))
            add("history-stage-1+partial", dict(some, stages=1 | T))
            add("history-stage-1+stages", dict(stages=1 | T | 0x400))
        if reduced:  # the reduced calls screen the whole `stages` word ahead of the history, the full-resolution ones after it
            add("stages-hslo-subpix+history", dict(some, stages=3 | T | 0x300, alpha=7.0))
        else:
            add("history-partial+stages", dict(some, stages=3 | T | 0x300))
            add("history-alias+stages", dict(full, stages=3 | T | 0x300, prev_disp_r=BASE["disp_r"]))
        if hist == 3:
            add("history-narrow", dict(full, **geom(8, 31, 16, stages=3 | T)))
            add("history-narrow+alias", dict(full, **geom(8, 31, 16, stages=3 | T, prev_disp_l=BASE["disp_l"])))
            add("history-narrow-no-pointers+align", geom(8, 31, 16, stages=3 | T), ALIGN1)
        else:
            add("history-no-images", dict(stages=3 | T, img_l=0, img_r=0))
            add("history-no-images+partial", dict(some, stages=3 | T, img_l=0, img_r=0))
            if not reduced:
                add("history-stage-1+no-images", dict(stages=1 | T, img_l=0, img_r=0))
            for k, (a, b) in enumerate([("prev_img_l", "img_l"), ("prev_img_l", "img_r"), ("prev_img_r", "img_l"), ("prev_img_r", "img_r"),
                                        ("prev_img_l", "disp_l"), ("prev_disp_r", "img_r")]):
                add("history-alias-image-%d" % k, dict(full, stages=3 | T, **{a: BASE[b]}))
            add("history-alias-image-tail", dict(full, stages=3 | T, prev_img_r=BASE["img_l"] + 8 * 16 * 3 - 1))
        add("history-alias+layout", dict(full, stages=3 | T, prev_disp_l=BASE["disp_l"]), NV12OUT())
    # ---- the `stages` rules the full-resolution bodies share
    if not reduced and not host:
        add("stages-hslo-subpix", dict(stages=3 | 0x300))
        add("stages-interp-stage-1", dict(stages=1 | 0x400))
        add("stages-linear-stage-2", dict(stages=2 | 0x800))
        add("stages-linear-stage-1", dict(stages=1 | 0x800))
        add("stages-guided", dict(stages=3 | 0x1000))
        add("stages-hslo-subpix+interp", dict(stages=1 | 0x300 | 0x400))
        add("stages-interp+linear", dict(stages=1 | 0x400 | 0x800))
        add("stages-linear+guided", dict(stages=2 | 0x800 | 0x1000))
        add("stages-guided+layout", dict(stages=3 | 0x1000), NV12OUT())
    elif reduced and has_stages:
        add("stages-hslo-subpix+layout", dict(stages=3 | 0x300), NV12OUT())
    # ---- layout, lens, overlay and output format against a rendering call
    add("output-no-quilt", {}, NV12OUT())
    add("overlay-nv12", dict(num_views=8), QUILT(4, 2) + NV12OUT() + OVERLAY)
    add("overlay-nv12+no-quilt", {}, NV12OUT() + OVERLAY)
    add("overlay-tiles", dict(num_views=65536), QUILT(256, 256) + OVERLAY)
    add("overlay-tiles+quilt-views", dict(num_views=65537), QUILT(256, 256) + OVERLAY)
    add("quilt-lens", {}, QUILT(4, 2) + LENS)
    add("quilt-lens+views", dict(num_views=7), QUILT(4, 2) + LENS)
    add("quilt-views", dict(num_views=7), QUILT(4, 2))
    add("quilt-no-column", dict(num_cols_out=3), QUILT(4, 2))
    add("quilt-no-row", dict(num_rows_out=1), QUILT(4, 2))
    add("quilt-wide-tile", dict(num_cols_out=1 << 30, num_views=2), QUILT(1, 2))
    add("quilt-tall-tile", dict(num_rows_out=1 << 30, num_views=2), QUILT(2, 1))
    add("quilt-views+no-column", dict(num_views=7, num_cols_out=3), QUILT(4, 2))
    add("quilt-no-column+no-row", dict(num_cols_out=3, num_rows_out=1), QUILT(4, 2))
    add("quilt-no-row+output", dict(num_rows_out=1), QUILT(4, 2) + NV12OUT())
    add("output-odd-rows", dict(num_rows_out=9), QUILT(4, 2) + NV12OUT())
    add("output-odd-cols", dict(num_cols_out=17), QUILT(4, 2) + NV12OUT())
    add("output-odd-tile-width", dict(num_cols_out=12), QUILT(4, 2) + NV12OUT())
    add("output-odd-tile-height", dict(num_rows_out=6), QUILT(4, 2) + NV12OUT())
    add("output-pitch", {}, QUILT(4, 2) + NV12OUT(pitch=15))
    add("output-uv_row", {}, QUILT(4, 2) + NV12OUT(uv_row=7))
    add("output-odd-rows+odd-cols", dict(num_rows_out=9, num_cols_out=17), QUILT(4, 2) + NV12OUT())
    add("output-pitch+uv_row", {}, QUILT(4, 2) + NV12OUT(pitch=15, uv_row=7))
    if not nv12:
        add("layout+align", geom(8, 31, 16), NV12OUT() + ALIGN1)
    add("layout+cut", geom(2, 32, 16, num_rows_disp=1, num_cols_disp=2), NV12OUT() + CUT)
    # ---- alignment, balance, shot changes: the settings screen
    if not nv12:
        add("align-narrow", geom(8, 31, 16), ALIGN1)
        add("align-narrow-auto", geom(8, 31, 16), ALIGN2)
        add("balance-narrow", geom(8, 31, 16), BAL1)
        add("balance-narrow-auto", geom(8, 31, 16), BAL2)
        add("align-narrow+balance-narrow", geom(8, 31, 16), ALIGN1 + BAL1)
        add("balance-narrow+cut", geom(3, 5, 3), BAL1 + CUT)
    small = dict(num_rows_disp=1, num_cols_disp=2)
    add("align-small-rows", geom(2, 32, 16, **small), ALIGN2)
    add("align-small-cols", geom(8, 12, 6, **small), ALIGN2)
    add("align-sums", WIDE, ALIGN2)
    add("align-small+balance", geom(2, 32, 16, **small), ALIGN2 + BAL2)
    add("align-small+cut", geom(2, 32, 16, **small), ALIGN2 + CUT)
    add("balance-size", BIG, BAL2)
    add("align-sums+balance-size", BIG, ALIGN2 + BAL2)
    add("balance-size+cut", BIG, BAL2 + CUT)
    add("cut-small-rows", geom(2, 32, 16, **small), CUT)
    add("cut-small-cols", geom(8, 4, 2, **small), CUT)
    add("cut-size", BIG, CUT)
    add("cut-small-under-align-1-balance-1", geom(2, 32, 16, **small), ALIGN1 + BAL1 + CUT)
    return out


def cases():
    out = []
    for name, (names, _, _, _, _, _) in ENTRIES.items():
        for label, over, settings in rules(name):
            vals = dict(BASE, **over)
            out.append(dict(entry=name, label=label, settings=settings, args=[vals[n] for n in names]))
    return out


# ------------------------------------------------------------------------------------------------- running a case (the test's too)
RESET = [["stm_set_packing", [0, 0, 0, 0]], ["stm_set_align", [0, 0.0, 0.0, 0.0]], ["stm_set_balance", [0, 0]], ["stm_set_cut", [0, 0, 0, 0]],
         ["stm_set_layout", [0, 1, 1, 0, 0]], ["stm_set_output", [0, 0, 0, 0]], ["stm_set_overlay", [0, 0, 0, 0, 0, 0, 0.0]],
         ["stm_set_lens", [0, 0.0, 0.0, 0.0]]]


def _convert(argtype, v):
    import ctypes
    if v == "identity":
        return (ctypes.c_uint8 * 768)(*[k & 255 for k in range(768)])
    if argtype in (ctypes.c_int, ctypes.c_float, ctypes.c_double):
        return v
    if v == 0:
        return None
    return v if argtype is ctypes.c_void_p else ctypes.cast(ctypes.c_void_p(v), argtype)


def call(lib, protos, name, args):
    return getattr(lib, name)(*[_convert(t, v) for t, v in zip(protos[name][0], args)])


def apply_settings(lib, protos, settings):
    for setter, args in settings:
        assert call(lib, protos, setter, args) == 0, (setter, args, lib.stm_last_error())


def refusal(lib, protos, case):
    """the case's call under its settings (error mode 1, set by the caller): stm_last_error() after its first line"""
    try:
        apply_settings(lib, protos, case["settings"])
        lib.stm_d_filter_median(None, 0, 0)  # plant a known message: a call that records nothing shows this one
        call(lib, protos, case["entry"], case["args"])
        return lib.stm_last_error().decode().split("\n", 1)[1]
    finally:
        apply_settings(lib, protos, RESET)


def load_table():
    """{(entry, label): message} from the file.  A row is [label, text, entries]: the entries (by their names in the messages,
    space-separated) whose case `label` is refused with "<name>: " + text"""
    rows = json.load(open(OUT))
    return {("stm_" + e, label): e + ": " + text for label, text, entries in rows for e in entries.split()}


def main():
    sys.path.insert(0, ROOT)
    import stm_amd
    from stm_amd import _lib
    lib = stm_amd.lib()
    lib.stm_set_error_mode(1)
    rows = {}  # (label, text) -> entries, in the order of first appearance
    n = 0
    try:
        for c in cases():
            name = c["entry"][4:]
            msg = refusal(lib, _lib.PROTOS, c)
            assert len(c["args"]) == len(_lib.PROTOS[c["entry"]][0]), c["entry"]
            assert msg.startswith(name + ": "), (c["entry"], c["label"], msg)  # refused by the entry's own screen, or not a row
            rows.setdefault((c["label"], msg[len(name) + 2:]), []).append(name)
            n += 1
    finally:
        lib.stm_set_error_mode(0)
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps([label, text, " ".join(e)]) for (label, text), e in rows.items()) + "\n]\n")
    print("%d cases in %d rows, %d distinct texts -> %s" % (n, len(rows), len({t for _, t in rows}), OUT))


if __name__ == "__main__":
    main()

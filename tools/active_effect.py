"""What the active picture area buys, measured on the CPU oracle's maps and the numpy statement (no GPU): the committed bud pair
(tests/golden/bud_2 + bud_3), 640 x 384, D = 32, zero_disp 16 (the parameters of tests/golden/make_golden_c1.py), with bars painted
over the picture.

  - letterbox_noise: 49 rows top and bottom at levels 0 .. 3, independent in the two eyes (codec noise in black bars);
    pillarbox_black: 80 black columns each side.  Per case the rectangle tests/test_active_ref.py's detect_ref measures at the
    defaults, and the gain depth mode 2 fits (budget -4 .. 4, max_gain 1, clip 20) under that rectangle, on the whole maps, and on
    the unbarred pair's maps over the same rectangle.
  - overlay_in_bottom_bar: a 24-row subtitle strip wholly inside the bottom bar of a pure black letterbox, placed (near 20, margin
    1, pad 0, limits -8 .. 10) without the rectangle, with it, and -- the yardstick -- on the unbarred pair with the strip slid onto
    the last picture rows.
usage: python tools/active_effect.py [--out FILE.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import stm_amd  # noqa: F401
    from oracle import pyoracle as orc
    import test_active_ref as ref
    orc.build()
    res = {"params": ref.P, "budget": ref.BUDGET, "detector": ref.DEFAULTS}
    res.update(ref.effect(orc))
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Record tests/golden/qwen_smart_resize.json from the installed transformers' own smart_resize (Qwen2-VL image processor, Pillow
backend): rows [h, w, min_pixels, max_pixels, H, W], with H = W = null where the library refuses the aspect ratio.

  python tests/golden/make_qwen_image_golden.py

The rows cover the three branches (plain rounding, over max_pixels, under min_pixels), the 200 : 1 refusal on either side of the bound, sizes
whose rounded side is an odd number of 28-pixel units, ties of round() (half-way sizes such as 42 and 70), and the processor's default
bounds as well as the small bounds of the reference's video route (max_pixels = 128 * 128).
"""
import json
import os
import random

from transformers.models.qwen2_vl.image_processing_pil_qwen2_vl import smart_resize

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT = (56 * 56, 28 * 28 * 1280)
BOUNDS = [DEFAULT, (56 * 56, 128 * 128), (4 * 28 * 28, 16384 * 28 * 28), (256 * 28 * 28, 1280 * 28 * 28), (28 * 28, 28 * 28)]


def main():
    rng = random.Random(20250)
    cases = []
    fixed = [(128, 128), (90, 200), (61, 37), (480, 640), (28, 28), (30, 1000), (140, 140), (3000, 4000), (42, 42), (70, 70), (14, 14), (13, 13),
             (1, 1), (1, 200), (1, 201), (201, 1), (5, 1000), (5, 1001), (1000, 5), (41, 43), (98, 98), (99, 154), (1080, 1920), (2160, 3840),
             (8, 8), (55, 57), (56, 56), (57, 55), (10, 2000), (27, 29), (84, 28), (28, 84), (6000, 8000), (65535, 400), (400, 65535)]
    for hw in fixed:
        for b in BOUNDS:
            cases.append(hw + b)
    while len(cases) < 215:
        kind = rng.randrange(4)
        if kind == 0:
            h, w = rng.randint(1, 120), rng.randint(1, 120)              # mostly under min_pixels
        elif kind == 1:
            h, w = rng.randint(100, 1200), rng.randint(100, 1200)        # mostly plain rounding
        elif kind == 2:
            h, w = rng.randint(900, 9000), rng.randint(900, 9000)        # over max_pixels
        else:
            h = rng.randint(1, 40)
            w = h * rng.randint(150, 230)                                # around the 200 : 1 bound
            if rng.random() < 0.5:
                h, w = w, h
        cases.append((h, w) + rng.choice(BOUNDS))
    rows = []
    for h, w, lo, hi in cases:
        try:
            H, W = smart_resize(h, w, 28, lo, hi)
        except ValueError:
            H = W = None
        rows.append([h, w, lo, hi, H, W])
    with open(os.path.join(HERE, "qwen_smart_resize.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("%d rows, %d refused" % (len(rows), sum(r[4] is None for r in rows)))


if __name__ == "__main__":
    main()

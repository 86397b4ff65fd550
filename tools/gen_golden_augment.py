"""Fixture tests/golden/augment_boxes.json for tests/test_augment_host.py, recorded from the reference (dev container only: it
imports the reference's dataloaders/transforms.py, with ``torchvision`` stubbed in sys.modules - the module only needs
``torchvision.transforms.InterpolationMode`` at import time, and the sampler itself uses ``random`` alone).

For every seed s and every (W, H, n_px) below, after ``random.seed(s)``, what the training loader's
``TensorMultiScaleCrop(n_px, [1, .875, .75, .66])`` followed by ``TensorRandomHorizontalFlip()`` draws for 8 clips in a row:

  cases[i] = {"seed": s, "W": W, "H": H, "n_px": n_px, "flip": false,
              "boxes": [[crop_w, crop_h, off_w, off_h] x 8]}           8 calls of _sample_crop_size((W, H)), nothing between
  cases[j] = {..., "flip": true, "boxes": [...], "flips": [0 / 1 x 8]}  per clip _sample_crop_size, then random.random() < 0.5
                                                                        (the draw TensorRandomHorizontalFlip.__call__ makes)
and the same with the constructor's other settings, under "variants": more_fix_crop=False, fix_crop=False, max_distort=0.

Only these numbers are committed.

    python tools/gen_golden_augment.py [--reference DIR]
"""
import argparse
import json
import os
import random
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "augment_boxes.json")

SEEDS = (0, 1, 7, 2024)
SIZES = ((320, 240, 224), (640, 360, 224), (226, 300, 224), (224, 224, 224), (60, 45, 32))      # (W, H, n_px)
CLIPS = 8
VARIANTS = {"five_offsets": dict(more_fix_crop=False), "free_offsets": dict(fix_crop=False), "no_distort": dict(max_distort=0)}


def import_transforms(reference):
    if "torchvision" not in sys.modules:
        tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")

        class InterpolationMode:
            BILINEAR, BICUBIC = "bilinear", "bicubic"
        tr.InterpolationMode = InterpolationMode
        tv.transforms = tr
        sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    sys.dont_write_bytecode = True
    sys.path.insert(0, reference)
    try:
        import dataloaders.transforms as rt
    finally:
        sys.path.remove(reference)
    return rt


def record(rt, seed, W, H, n_px, flip, **kw):
    crop = rt.TensorMultiScaleCrop(n_px, [1, .875, .75, .66], **kw)
    random.seed(seed)
    boxes, flips = [], []
    for _ in range(CLIPS):
        boxes.append([int(v) for v in crop._sample_crop_size((W, H))])
        if flip:
            flips.append(int(random.random() < 0.5))
    case = dict(seed=seed, W=W, H=H, n_px=n_px, flip=flip, boxes=boxes)
    if flip:
        case["flips"] = flips
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="the reference's checkout (default: where oracle/ looks for it)")
    a = ap.parse_args()
    if a.reference is None:
        from oracle.gen_golden_clip import REF
        a.reference = REF
    rt = import_transforms(a.reference)
    doc = dict(scales=[1, .875, .75, .66], clips=CLIPS, cases=[], variants={})
    for seed in SEEDS:
        for (W, H, n_px) in SIZES:
            for flip in (False, True):
                doc["cases"].append(record(rt, seed, W, H, n_px, flip))
    for name, kw in VARIANTS.items():
        doc["variants"][name] = dict(kwargs=kw, cases=[record(rt, seed, W, H, n_px, True, **kw)
                                                       for seed in SEEDS[:2] for (W, H, n_px) in SIZES])
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d cases, %d bytes" % (OUT, len(doc["cases"]) + sum(len(v["cases"]) for v in doc["variants"].values()),
                                            os.path.getsize(OUT)))


if __name__ == "__main__":
    main()

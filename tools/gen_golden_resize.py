"""Record tests/golden/resize_golden.npz from Pillow: the inputs of tests/resize_ref.cases() and what
``Image.resize(BICUBIC)`` + the centre crop give for them at n_px = 32 (the transform of dataloaders/rawvideo_util.py:16-23;
the resized size and the crop offsets follow torchvision's Resize / CenterCrop as tests/resize_ref.py states them).

    python tools/gen_golden_resize.py
"""
import os
import sys

import numpy as np
from PIL import Image
import PIL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resize_ref as R  # noqa: E402

N_PX = 32


def pillow_transform(frame, n_px):
    H, W = frame.shape[:2]
    oh, ow = R.resized_size(H, W, n_px)
    img = Image.fromarray(frame)
    if (oh, ow) != (H, W):
        img = img.resize((ow, oh), Image.BICUBIC)
    top, left = R.crop_offset(oh, n_px), R.crop_offset(ow, n_px)
    return np.asarray(img)[top:top + n_px, left:left + n_px]


def main():
    out = {"n_px": np.int32(N_PX), "pillow_version": np.array(PIL.__version__)}
    for name, (H, W, kind) in R.cases().items():
        x = R.make_input(H, W, kind, seed=len(name))
        out["in/" + name] = x
        out["out/" + name] = np.stack([pillow_transform(f, N_PX) for f in x], 0)
    path = os.path.join(ROOT, "tests", "golden", "resize_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()

"""Fixture of the device loader's RGB path: an RGB8 image and PIL's convert('L') of it (what the reference's loaders do to
every image they read, data_load_val.py:110-117), so that the GPU test needs no PIL.

    python tests/golden/make_frontend_golden.py        # writes tests/golden/frontend_rgb_l.npz (needs Pillow)

The image: random pixels, with the 8 corners of the colour cube, the grays and the single-channel ramps (every value of each
channel alone: the rounding of each coefficient) in its first rows."""
import os

import numpy as np

H, W = 200, 240


def make_rgb():
    rng = np.random.default_rng(20240611)
    rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    ext = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]
    ext += [(v, v, v) for v in range(256)]
    for c in range(3):
        for v in range(256):
            p = [0, 0, 0]
            p[c] = v
            ext.append(tuple(p))
    flat = rgb.reshape(-1, 3)
    flat[:len(ext)] = np.array(ext, np.uint8)
    return rgb


def main():
    from PIL import Image
    import PIL
    rgb = make_rgb()
    lum = np.asarray(Image.fromarray(rgb, "RGB").convert("L"))
    assert lum.shape == (H, W) and lum.dtype == np.uint8
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "frontend_rgb_l.npz")
    np.savez(out, rgb=rgb, l=lum, pil_version=np.array(PIL.__version__))
    print(out, os.path.getsize(out), "bytes; PIL", PIL.__version__)


if __name__ == "__main__":
    main()

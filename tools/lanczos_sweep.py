"""Measurement, not a test (DESIGN.md §3 pil_resize): LANCZOS through mhip_pil_resize_rgb_host against Pillow on uniform noise
over 76 shape pairs, and BILINEAR / BICUBIC on every eighth of them.  Run from the repository root on a GPU:
``PYTHONPATH=. python tools/lanczos_sweep.py``."""
import numpy as np
from PIL import Image

from marie_icr_amd._lib import Context
from marie_icr_amd.dit import pil_resize_rgb

ctx = Context(0)
rng = np.random.default_rng(12345)
pairs = [((3300, 2550), (224, 224)), ((2200, 1700), (224, 224)), ((1100, 850), (224, 224)), ((3, 2), (224, 224)),
         ((224, 224), (3, 5)), ((1, 1), (7, 9))]
for _ in range(70):
    pairs.append(((int(rng.integers(1, 900)), int(rng.integers(1, 900))), (int(rng.integers(1, 300)), int(rng.integers(1, 300)))))
bad = 0
coeffs = 0
for k, (src, dst) in enumerate(pairs):
    a = rng.integers(0, 256, (src[0], src[1], 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(a).resize((dst[1], dst[0]), Image.LANCZOS))
    got = pil_resize_rgb(ctx, a, dst, filter=1)
    d = int((got != want).sum())
    coeffs += dst[0] * (int(np.ceil(3 * max(src[0] / dst[0], 1))) * 2 + 1) + dst[1] * (int(np.ceil(3 * max(src[1] / dst[1], 1))) * 2 + 1)
    if d:
        bad += 1
        print(f"DIFF {src} -> {dst}: {d} of {got.size} bytes, max |d| = {int(np.abs(got.astype(int) - want.astype(int)).max())}")
    # the two older filters stay Pillow's too
    for f, pf in ((2, Image.BILINEAR), (3, Image.BICUBIC)):
        if k % 8 == 0:
            w2 = np.asarray(Image.fromarray(a).resize((dst[1], dst[0]), pf))
            if not np.array_equal(pil_resize_rgb(ctx, a, dst, filter=f), w2):
                print(f"DIFF filter {f} {src} -> {dst}")
                bad += 1
print(f"sweep: {len(pairs)} shape pairs, about {coeffs} coefficient slots, {bad} with a difference")
ctx.close()

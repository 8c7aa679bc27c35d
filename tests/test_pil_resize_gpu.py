"""The batched Pillow-exact resizer (csrc/pil_resize.hip: pil_coeffs_batch / pil_hpass_batch / pil_vpass_batch kernels, what TrOCR
and LayoutLMv3 run) at kernel level through mhip_pil_resize_fragments_host: byte-equal with Pillow's Image.resize per fragment
and with the single-image kernels.

Fragments (h x w) 1x1, 3x7, 50x5, 17x40 and 64x200 lie in one byte buffer at non-zero offsets with rows wider than 3 w: one-tap
windows, strong down-scaling in one axis with up-scaling in the other, and a tap count (kmax) that a fragment other than the
first sets.  The entry hands back exactly n images, so there are no bytes behind them to guard."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAG_HW = ((1, 1), (3, 7), (50, 5), (17, 40), (64, 200))
OUT_HW = ((32, 32), (8, 24))
FILTERS = (1, 2, 3)   # PIL.Image.LANCZOS, BILINEAR, BICUBIC


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def packed():
    """(base, frags, images): the byte buffer, (src_offset, h, w, row_stride) per fragment, and the fragments as arrays"""
    rng = np.random.default_rng(7)
    frags, images, off = [], [], 13
    for i, (h, w) in enumerate(FRAG_HW):
        stride = 3 * w + 5 + 3 * i
        frags.append((off, h, w, stride))
        images.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        off += h * stride + 7
    base = rng.integers(0, 256, off, dtype=np.uint8)     # noise between the rows too: a wrong stride or offset reads it
    for (o, h, w, stride), img in zip(frags, images):
        for y in range(h):
            base[o + y * stride: o + y * stride + 3 * w] = img[y].reshape(-1)
    base.setflags(write=False)
    return base, frags, images


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("out_hw", OUT_HW)
def test_fragments_match_pillow(ctx, packed, out_hw, filt):
    from PIL import Image

    from marie_icr_amd.dit import pil_resize_fragments

    base, frags, images = packed
    got = pil_resize_fragments(ctx, base, frags, out_hw, filt)
    assert got.shape == (len(frags), out_hw[0], out_hw[1], 3)
    for i, img in enumerate(images):
        ref = np.asarray(Image.fromarray(img).resize((out_hw[1], out_hw[0]), filt))
        assert np.array_equal(got[i], ref), (FRAG_HW[i], out_hw, filt, int(np.abs(got[i].astype(int) - ref).max()))


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("out_hw", OUT_HW)
def test_single_fragment_equals_single_image_kernels(ctx, packed, out_hw, filt):
    from marie_icr_amd.dit import pil_resize_fragments, pil_resize_rgb

    for img in packed[2]:
        h, w = img.shape[:2]
        got = pil_resize_fragments(ctx, img, [(0, h, w, 3 * w)], out_hw, filt)
        assert np.array_equal(got[0], pil_resize_rgb(ctx, img, out_hw, filter=filt)), ((h, w), out_hw, filt)


def test_fragment_outside_the_buffer_is_refused(ctx, packed):
    from marie_icr_amd._lib import MarieHipError
    from marie_icr_amd.dit import pil_resize_fragments

    base, frags, _ = packed
    o, h, w, stride = frags[-1]
    for bad in ((o, h + 1, w, stride), (o, h, w, 3 * w - 1), (base.size - 2, 1, 1, 3)):
        with pytest.raises(MarieHipError):
            pil_resize_fragments(ctx, base, [frags[0], bad], (8, 8), 3)

"""Writes tests/golden/jpeg/: a dozen small pictures encoded by Pillow (libjpeg), each with Pillow's OWN decode of it (draft "YCbCr": the luma plane,
and for 4:4:4 pictures the chroma planes) -- the pin of the MJPEG decode to an implementation outside this repository.  Needs Pillow; the tests only
read the files it wrote.

While writing, it asserts the pin for the restatement tests/jpeg_ref.py (JPEG leaves the IDCT open, so +-1 is as exact as two decoders get):
  luma vs Pillow: max |d| <= 1 and at most 5 % of the samples differ;  4:4:4 chroma after the 2x2 box, fully covered cells: max |d| <= 1.

    python tests/golden/make_golden_jpeg.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_ref  # noqa: E402

OUT = os.path.join(HERE, "jpeg")

# name: (mode, width, height, save options)
FIXTURES = {
    "c420_16x16": ("YCbCr", 16, 16, dict(quality=75, subsampling=2)),            # default tables: also the source of the Annex K tables for jpeg_ref
    "g_8x8": ("L", 8, 8, dict(quality=75)),
    "c420_53x37": ("YCbCr", 53, 37, dict(quality=50, subsampling=2)),
    "c420_72x40_rst3": ("YCbCr", 72, 40, dict(quality=60, subsampling=2, restart_marker_blocks=3)),
    "c422_48x32": ("YCbCr", 48, 32, dict(quality=70, subsampling=1)),
    "c444_40x24": ("YCbCr", 40, 24, dict(quality=80, subsampling=0)),
    "c444_53x37": ("YCbCr", 53, 37, dict(quality=30, subsampling=0)),
    "c420_64x48_opt": ("YCbCr", 64, 48, dict(quality=65, subsampling=2, optimize=True)),
    "c420_32x32_q1": ("YCbCr", 32, 32, dict(quality=1, subsampling=2)),
    "g_37x21": ("L", 37, 21, dict(quality=40)),
    # refused features
    "prog_32x32": ("YCbCr", 32, 32, dict(quality=75, subsampling=2, progressive=True)),
    "cmyk_16x16": ("CMYK", 16, 16, dict(quality=75)),
}
REFUSED = ("prog_32x32", "cmyk_16x16")


def content(rng, mode, w, h):
    nc = {"L": 1, "YCbCr": 3, "CMYK": 4}[mode]
    yy, xx = np.mgrid[0:h, 0:w]
    planes = []
    for c in range(nc):
        g = 128 + 70 * np.sin(xx / (5.0 + 3 * c) + c) * np.cos(yy / (7.0 - c)) + rng.normal(0, 18, (h, w))
        planes.append(np.clip(g, 0, 255).astype(np.uint8))
    a = planes[0] if nc == 1 else np.stack(planes, axis=-1)
    return Image.fromarray(a, mode)


def pillow_planes(data):
    im = Image.open(io.BytesIO(data))
    im.draft("YCbCr", im.size)
    im.load()
    a = np.asarray(im)
    return [a] if a.ndim == 2 else [a[:, :, c] for c in range(3)]


def check_pin(name, data, planes):
    """The two conditions; returns the share of luma samples that differ."""
    f, dw, dh, _ = jpeg_ref.RefDecoder().decode_picture(data)
    h, w = planes[0].shape
    d = np.abs(f[:h, :w].astype(int) - planes[0].astype(int))
    share = float((d != 0).mean())
    assert d.max() <= 1 and share <= 0.05, (name, int(d.max()), share)
    if name.startswith("c444"):
        for c in (0, 1):
            p = planes[1 + c].astype(int)
            hh, ww = h // 2, w // 2
            box = (p[0:2 * hh:2, 0:2 * ww:2] + p[0:2 * hh:2, 1:2 * ww:2] + p[1:2 * hh:2, 0:2 * ww:2] + p[1:2 * hh:2, 1:2 * ww:2] + 2) >> 2
            dc = np.abs(f[dh:dh + hh, c:2 * ww:2].astype(int) - box)
            assert dc.max() <= 1, (name, c, int(dc.max()))
    return share


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(0x4A504547)
    for name, (mode, w, h, opts) in FIXTURES.items():
        buf = io.BytesIO()
        content(rng, mode, w, h).save(buf, "JPEG", **opts)
        data = buf.getvalue()
        assert len(data) < 16384, (name, len(data))
        open(os.path.join(OUT, name + ".jpg"), "wb").write(data)
        if name in REFUSED:
            print(f"{name}: {len(data)} bytes (for refusal)")
            continue
        planes = pillow_planes(data)
        np.save(os.path.join(OUT, name + ".y.npy"), planes[0])
        if name.startswith("c444"):
            np.save(os.path.join(OUT, name + ".cb.npy"), planes[1])
            np.save(os.path.join(OUT, name + ".cr.npy"), planes[2])
        share = check_pin(name, data, planes)
        print(f"{name}: {len(data)} bytes, luma max |d| <= 1, {100 * share:.2f} % of samples differ")


if __name__ == "__main__":
    main()

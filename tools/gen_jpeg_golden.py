#!/usr/bin/env python
"""Writes tests/golden/jpeg_pillow.npz: what a real codec of the libjpeg family makes of a few small frames, for K12's distance-to-a-codec
tests (tests/test_jpeg_host.py, tests/test_gpu_jpeg.py). Needs Pillow; run it by hand when the fixture has to be regenerated:

    python tools/gen_jpeg_golden.py [--out tests/golden/jpeg_pillow.npz]

Recorded: the input frames, Pillow's save(format="JPEG", quality=q, subsampling=2) + load round trip at each quality, the quantisation
tables Pillow reports for each quality (natural order), and the Pillow / libjpeg version strings."""
import argparse
import io
import os

import numpy as np

QUALITIES = (95, 75, 50, 100)


def frames():
    rng = np.random.default_rng(20240612)
    H, W = 48, 64
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.stack([xx * 255 // (W - 1), yy * 255 // (H - 1), (xx + yy) * 255 // (H + W - 2)], axis=-1)
    noise = rng.integers(0, 256, (H, W, 3))
    sines = np.stack([127.5 + 90 * np.sin(xx / 3.0 + c) * np.cos(yy / (4.0 + c)) for c in range(3)], axis=-1) + rng.normal(0, 12, (H, W, 3))
    out = {
        "ramp": ramp, "noise": noise, "sines": np.clip(np.rint(sines), 0, 255),
        "odd24x40": rng.integers(0, 256, (24, 40, 3)) // 2 + np.stack([np.mgrid[0:24, 0:40][1] * 3] * 3, axis=-1),
        "odd17x33": rng.integers(0, 256, (17, 33, 3)),
        "mcu16": rng.integers(0, 256, (16, 16, 3)),
        "flat": np.full((32, 32, 3), (200, 30, 90)),
        "checker": np.stack([((np.mgrid[0:32, 0:48][0] + np.mgrid[0:32, 0:48][1]) % 2) * 255] * 3, axis=-1),
    }
    return {k: np.ascontiguousarray(v).astype(np.uint8) for k, v in out.items()}


def pillow_roundtrip(frame, quality):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(frame, "RGB").save(buf, format="JPEG", quality=quality, subsampling=2)
    im = Image.open(io.BytesIO(buf.getvalue()))
    q = im.quantization
    out = np.asarray(im.convert("RGB"))
    return out, np.array([list(q[0]), list(q[1])], dtype=np.uint16)


def main():
    import PIL
    from PIL import features

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "jpeg_pillow.npz"))
    args = ap.parse_args()
    rec = {"names": np.array(list(frames())), "qualities": np.array(QUALITIES, dtype=np.int32),
           "pillow_version": np.array(PIL.__version__),
           "libjpeg_version": np.array("%s %s" % ("libjpeg-turbo" if features.check_feature("libjpeg_turbo") else "libjpeg",
                                                   features.version_feature("libjpeg_turbo") or features.version_codec("jpg")))}
    for name, f in frames().items():
        rec["in_" + name] = f
        for q in QUALITIES:
            out, qt = pillow_roundtrip(f, q)
            rec["out_%s_q%d" % (name, q)] = out
            rec["qt_q%d" % q] = qt
    np.savez_compressed(args.out, **rec)
    print("wrote %s (%d bytes), %s / %s" % (args.out, os.path.getsize(args.out), rec["pillow_version"], rec["libjpeg_version"]))


if __name__ == "__main__":
    main()

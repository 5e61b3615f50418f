"""The cases of the SIFT extraction tests: small synthetic images from a seeded generator, the options of each case, and
the loader of tests/golden/sift_vlfeat.npz (what VLFeat itself gave for them, see tests/golden/sift_vlfeat.md).

The tests read the images from the fixture, not from the generator: the generator is the record of how they were made
(numpy's exp may differ in the last bit between versions; the committed bytes may not)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_vlfeat.npz")

DEFAULTS = dict(max_num_features=8192, first_octave=-1, num_octaves=4, octave_resolution=3, peak_threshold=0.02 / 3.0,
                edge_threshold=10.0, max_num_orientations=2, upright=0, normalization=0)


def blob_image(w, h, n, seed, smin=1.0, smax=5.0, border=False, extra=()):
    """A sum of n anisotropic Gaussian blobs of random sign around mid-grey, quantised to uint8. border: every centre
    within 3 px of an edge. extra: (cx, cy, sigma, amplitude) blobs placed on purpose."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    im = np.zeros((h, w))
    for i in range(n):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        if border:
            side = rng.randint(4)
            d = rng.uniform(0, 3)
            if side == 0:
                cx = d
            elif side == 1:
                cx = w - 1 - d
            elif side == 2:
                cy = d
            else:
                cy = h - 1 - d
        sx, sy = rng.uniform(smin, smax, 2)
        th = rng.uniform(0, np.pi)
        a = rng.uniform(0.08, 0.35) * (1 if rng.randint(2) else -1)
        u = np.cos(th) * (xx - cx) + np.sin(th) * (yy - cy)
        v = -np.sin(th) * (xx - cx) + np.cos(th) * (yy - cy)
        im += a * np.exp(-(u * u / (2 * sx * sx) + v * v / (2 * sy * sy)))
    for cx, cy, s, a in extra:
        im += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return np.clip(np.floor((0.5 + im) * 255 + 0.5), 0, 255).astype(np.uint8)


def _case(image, **options):
    o = dict(DEFAULTS)
    o.update(options)
    return dict(image=image, options=o)


def make_cases():
    """name -> dict(image, options). The generator side: used to make the fixture."""
    base = blob_image(96, 80, 60, 2)
    return {
        # 160 x 120: octave -1 is 320 x 240, several tiles of both convolution passes in each direction
        "blobs160": _case(blob_image(160, 120, 150, 1)),
        "blobs96": _case(base),
        # odd halves 33 x 22, 16 x 11; 134 x 90 at octave -1 is a multiple of no tile dimension
        "odd67": _case(blob_image(67, 45, 40, 3)),
        "constant": _case(np.full((30, 40), 128, np.uint8)),
        # refinement's border guards, one-sided gradients, windows cut by the edge
        "border": _case(blob_image(64, 48, 40, 4, smin=1.0, smax=3.0, border=True)),
        # coarse blobs: detections in the last octave
        "coarse": _case(blob_image(128, 96, 12, 5, smin=7.0, smax=13.0)),
        # a blob centred on the corner of four column-pass tiles of octave -1 (64, 32) and one on a row-pass seam (128, 8)
        "seam": _case(blob_image(96, 80, 20, 6, extra=((32.0, 16.0, 2.0, 0.3), (64.0, 4.0, 1.5, -0.3)))),
        "first0": _case(base, first_octave=0),
        "res2": _case(base, octave_resolution=2),
        "upright": _case(base, upright=1),
        "l2": _case(base, normalization=1),
        "cut": _case(base, max_num_features=25),
        "one_orientation": _case(base, max_num_orientations=1),
    }


_fixture = None


def fixture():
    """name -> dict(image, options, octaves=[dict(o, w, h, det_i [n][4] = o ix iy is, det_f [n][4] = x y s sigma, counts [n],
    angles [n][4], float_desc [rows][128])], level_num_features, level_num_rows, keypoints [all rows][4], descriptors
    [all rows][128] uint8 UBC, skip, num_out): VLFeat's own results. The final result is rows skip .. skip + num_out."""
    global _fixture
    if _fixture is None:
        z = np.load(GOLDEN)
        meta = json.loads(bytes(z["meta"]).decode())
        out = {}
        for name, m in meta["cases"].items():
            c = dict(image=z[name + "/image"], options=m["options"], octaves=[], bounds=meta.get("bounds", {}))
            for k in range(m["num_octaves"]):
                p = "%s/oct%d/" % (name, k)
                o, w, h = (int(v) for v in z[p + "info"])
                c["octaves"].append(dict(o=o, w=w, h=h, det_i=z[p + "det_i"], det_f=z[p + "det_f"], counts=z[p + "counts"],
                                         angles=z[p + "angles"], float_desc=z[p + "float_desc"]))
            for key in ("level_num_features", "level_num_rows", "keypoints", "descriptors"):
                c[key] = z[name + "/" + key]
            c["skip"], c["num_out"] = int(m["skip"]), int(m["num_out"])
            out[name] = c
        _fixture = out
    return _fixture


def case_names():
    return sorted(fixture())

"""Golden fixtures for the reference's src/RDE.py, run as its own program (the
unmodified file) under /opt/conda/bin/python3.9 (numpy 1.26, PIL 8.4, skimage)
on three small image pairs this script writes itself.  Build container only:

    python tests/golden/make_golden_rde.py

Each tests/golden/rde_<name>.npz holds the two PNG files as bytes, their pixel
arrays, the names and lengths of the code-stream files (their contents do not
matter to RDE.py: zeros of the same length stand in) and the lines RDE.py
printed, with the working directory replaced by the placeholder {D}.

RDE.py takes its mean of squares in float32; vcf_amd/codec/rde.py divides the
exact integer sum in float64.  The two agree to about 1e-7 relative, so the
`:.2f` values are equal away from a rounding boundary: every pair here has its
exact RMSE * 100 at least 0.01 away from a half-integer (asserted below; a pair
that fails wants another seed).
"""
import io
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import PY39, REF_SRC  # noqa: E402

# name, shape, seed, noise amplitude, code-stream files (name, length), the -c argument
CASES = [
    ("rgb_37x53", (37, 53, 3), 101, 6, [("encoded.tif", 2917)], "encoded*"),
    ("grey_16x16", (16, 16), 102, 3, [("encoded.tif", 311)], "encoded.tif"),
    ("rgb_64x96_two", (64, 96, 3), 103, 11, [("encoded.tif", 7001), ("encoded_shape.bin", 12)], "encoded"),
]


def pair(shape, seed, amp):
    rng = np.random.Generator(np.random.PCG64(seed))
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    noise = rng.integers(-amp, amp + 1, shape)
    b = np.clip(a.astype(np.int64) + noise, 0, 255).astype(np.uint8)
    return a, b


def exact_rmse(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return math.sqrt(int((d * d).sum()) / d.size)


def png_bytes(a):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="PNG")
    return buf.getvalue()


def do_case(name, shape, seed, amp, files, cflag):
    a, b = pair(shape, seed, amp)
    rmse = exact_rmse(a, b)
    frac = (rmse * 100) % 1.0
    assert abs(frac - 0.5) >= 0.01, f"{name}: RMSE * 100 = {rmse * 100!r} is too near a rounding boundary: change the seed"
    opng, dpng = png_bytes(a), png_bytes(b)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "original.png"), "wb") as f:
            f.write(opng)
        with open(os.path.join(d, "decoded.png"), "wb") as f:
            f.write(dpng)
        for fn, n in files:
            with open(os.path.join(d, fn), "wb") as f:
                f.write(bytes(n))
        cmd = [PY39, "-W", "ignore", os.path.join(REF_SRC, "RDE.py"), "-o", os.path.join(d, "original.png"),
               "-c", os.path.join(d, cflag), "-d", os.path.join(d, "decoded.png")]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=d)
        if r.returncode != 0:
            raise RuntimeError(f"reference run failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
        lines = [ln.replace(d, "{D}") for ln in r.stdout.splitlines()]
    np.savez_compressed(os.path.join(HERE, f"rde_{name}.npz"), original=a, decoded=b,
                        original_png=np.frombuffer(opng, np.uint8), decoded_png=np.frombuffer(dpng, np.uint8),
                        cs_names=np.array([fn for fn, _ in files]), cs_lengths=np.array([n for _, n in files], np.int64),
                        cflag=np.array(cflag), lines=np.array(lines))
    return dict(name=name, shape=list(shape), seed=seed, amp=amp, files=[list(f) for f in files], cflag=cflag,
                exact_rmse=rmse, source="src/RDE.py run as a program", lines=lines)


def main():
    if not os.path.exists(PY39) or not os.path.isdir(REF_SRC):
        sys.exit("needs /opt/conda/bin/python3.9 and /root/reference (build container only)")
    manifest = dict(generator="tests/golden/make_golden_rde.py", reference="src/RDE.py (unmodified, run as a program)",
                    cases=[do_case(*c) for c in CASES])
    with open(os.path.join(HERE, "manifest_rde.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    for c in manifest["cases"]:
        print(c["name"], c["exact_rmse"], *c["lines"], sep="\n  ")


if __name__ == "__main__":
    main()

"""Generate the 2D-MDCT fixtures under tests/golden/ from the reference itself.

Run in the build container only (python3.9 and the reference are not on the
GPU box):

    python tests/golden/make_golden_mdct.py

Drives the reference's unmodified src/2D-MDCT.py encode_fn/decode_fn through
_run_ref.py, with the shims of make_golden.py (no new shim: -p at B = 8 hits
the shim's identity cv2.resize).  The input is copied to /tmp/original.png
before each decode, which the reference's rate/distortion log reads.

Writes mdct_<case>.npz (rgb, the indices read from the reference's .tif, the
.tif bytes, _shape.bin, the decoded frame) and manifest_mdct.json.

Robust by construction: the reference sums in float64 through BLAS, in an
order nobody controls, so every case is also computed with
tests/mdct_restated.py in two accumulation orders; both must give exactly the
reference's indices and pixels, and the manifest records how far the case
stays from every quantizer and truncation threshold.  A case that fails gets
another seed.
"""
import json
import os
import shutil
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402
import mdct_restated as M  # noqa: E402

CASES = [
    # name, kind, H, W, seed, reference CLI flags (shared by encode/decode)
    ("rand_1x1", "rand", 1, 1, 13, []),
    ("rand_3x17_q3", "rand", 3, 17, 14, ["-q", "3"]),
    ("smooth_37x45", "smooth", 37, 45, 1, []),
    ("smooth_37x45_b12", "smooth", 37, 45, 1, ["-B", "12"]),
    ("rand_40x48_x", "rand", 40, 48, 7, ["-x"]),
    ("smooth_64x64_p", "smooth", 64, 64, 9, ["-p"]),
    ("flat_48x56_b32", "flat", 48, 56, 2, ["-B", "32"]),
    ("smooth_33x35_b4", "smooth", 33, 35, 21, ["-B", "4"]),
    ("extreme_32x40_q1", "extreme", 32, 40, 3, ["-q", "1"]),
    ("rand_24x24_b64_q7", "rand", 24, 24, 15, ["-B", "64", "-q", "7"]),
    ("rand_10x14_b2", "rand", 10, 14, 16, ["-B", "2"]),
]


def options(flags):
    B, Q, fl = 8, 32, 0
    it = iter(flags)
    for f in it:
        if f == "-B":
            B = int(next(it))
        elif f == "-q":
            Q = int(next(it))
        elif f == "-x":
            fl |= M.NO_SUBBANDS
        elif f == "-p":
            fl |= M.PERCEPTUAL
    return B, Q, fl


def run_ref(sub, in_fn, out_fn, flags):
    import subprocess
    env = dict(os.environ)
    env["PYTHONPATH"] = os.path.join(HERE, "shims") + os.pathsep + G.REF_SRC
    env["VCF_GOLDEN_HIDE_IMAGECODECS"] = "1"
    env["OMP_NUM_THREADS"] = "1"
    cmd = [G.PY39, "-W", "ignore", os.path.join(HERE, "_run_ref.py"), "2D-MDCT", sub, in_fn, out_fn] + flags
    r = subprocess.run(cmd, env=env, cwd=G.REF_SRC, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"reference run failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    return int([l for l in r.stdout.splitlines() if l.startswith("RESULT_BYTES")][0].split()[1])


def do_case(tmp, name, kind, H, W, seed, flags):
    B, Q, fl = options(flags)
    for attempt in range(8):
        rgb = G.synth(kind, H, W, seed + 1000 * attempt)
        in_fn = os.path.join(tmp, f"{name}.png")
        Image.fromarray(rgb).save(in_fn)
        enc = os.path.join(tmp, f"{name}_enc")
        dec = os.path.join(tmp, f"{name}_dec.png")
        nbytes = run_ref("encode", in_fn, enc, flags)
        tif = open(enc + ".tif", "rb").read()
        shape_bin = open(enc + "_shape.bin", "rb").read()
        k = G.tiff_pixels(enc + ".tif")
        shutil.copyfile(in_fn, "/tmp/original.png")
        run_ref("decode", enc, dec, flags)
        decoded = np.array(Image.open(dec))
        ok = shape_bin == M.shape_bin(H, W, B)
        margins = []
        for order in ("fwd", "rev"):
            e = M.encode(rgb, B, Q, fl, order)
            d = M.decode(k, H, W, B, Q, fl, order)
            ok = ok and np.array_equal(e["k"], k) and np.array_equal(d["rgb"], decoded)
            margins.append((float(M.index_margin(e["pre"], Q).min()), float(M.pixel_margin(d["pre"]).min())))
        if ok:
            break
        print(f"{name}: seed {seed + 1000 * attempt} is not robust, trying another", flush=True)
    else:
        raise RuntimeError(f"{name}: no robust seed")
    clipped = int(np.count_nonzero((k == 0) | (k == 255)))
    if kind == "extreme":
        # the clip at 0 and 255 (not the DCT path's wrap) must be exercised: some coefficient's
        # k + 128 has to fall outside [0, 255]
        raw = (M.encode(rgb, B, Q, fl)["coef32"] / np.float32(Q)).astype(np.int32) + 128
        assert np.count_nonzero(raw < 0) and np.count_nonzero(raw > 255), "extreme case without clipped indices"
    meta = dict(name=name, kind=kind, H=H, W=W, seed=seed + 1000 * attempt, flags=flags, B=B, Q=Q,
                encode_bytes=nbytes, k_shape=list(k.shape), indices_at_0_or_255=clipped,
                min_index_margin=min(m[0] for m in margins), min_pixel_margin=min(m[1] for m in margins),
                sha256=dict(rgb=G.sha(rgb.tobytes()), k=G.sha(k.tobytes()), tif=G.sha(tif),
                            decoded=G.sha(decoded.tobytes())))
    np.savez_compressed(os.path.join(HERE, f"mdct_{name}.npz"), rgb=rgb, k=k, decoded=decoded,
                        tif=np.frombuffer(tif, np.uint8), shape_bin=np.frombuffer(shape_bin, np.uint8))
    return meta


def main():
    if not os.path.exists(G.PY39) or not os.path.isdir(G.REF_SRC):
        sys.exit("needs /opt/conda/bin/python3.9 and /root/reference (build container only)")
    manifest = dict(
        generator="tests/golden/make_golden_mdct.py",
        reference="Sistemas-Multimedia/VCF src/2D-MDCT.py encode_fn/decode_fn (unmodified glue)",
        python="/opt/conda/bin/python3.9, tifffile stdlib-zlib path (imagecodecs hidden)",
        robustness="every case equals tests/mdct_restated.py in both accumulation orders; min_index_margin = "
                   "least distance of coefficient / Q to a nonzero integer, min_pixel_margin = least distance "
                   "of a pixel value before truncation to 1..255 (float64, over both orders)",
        cases=[])
    with tempfile.TemporaryDirectory() as tmp:
        for c in CASES:
            manifest["cases"].append(do_case(tmp, *c))
            print("done", c[0], manifest["cases"][-1]["min_index_margin"], manifest["cases"][-1]["min_pixel_margin"],
                  flush=True)
    with open(os.path.join(HERE, "manifest_mdct.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()

"""Generate the 2D-KLT fixtures under tests/golden/ from the reference itself.

Run in the build container only (python3.9 and the reference are not on the
GPU box):

    python tests/golden/make_golden_klt.py

Drives the reference's unmodified src/2D-KLT.py encode_fn/decode_fn through
_run_ref_klt.py, with the shims of make_golden.py.  The runner records the
float64 weights the encoder transformed with; float32 of them must equal the
reference's {out}_weights.npz.

Writes klt_<case>.npz (rgb, weights64, the indices read from the reference's
.tif, the .tif bytes, _shape.bin, the decoded frame) and manifest_klt.json.
No case at B = 16: the float64 weights alone are 1.5 MB there.

Robust by construction: the reference multiplies through BLAS, in an order
nobody controls, and decodes in float32.  Every case is also computed with
tests/klt_restated.py: the indices, given weights64, in two accumulation
orders, and the decoded frame in float64 (two orders) and float32 (two
orders); all must give exactly the reference's output and stay at least 1e-9
away from every quantizer and truncation threshold (the one-colour frame
excepted, whose weights are unit vectors and whose arithmetic is exact); the
manifest records the distances.  A case that fails gets another seed.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402
import klt_restated as K  # noqa: E402

CASES = [
    # name, kind, H, W, seed, reference CLI flags (shared by encode/decode)
    ("smooth_61x77", "smooth", 61, 77, 1, []),
    ("rand_40x48_b4_q8", "rand", 40, 48, 1, ["-B", "4", "-q", "8"]),
    ("rand_64x72_q1", "rand", 64, 72, 1, ["-q", "1"]),
    ("flat_48x56", "const", 48, 56, 2, []),
    ("rand_40x48_x", "rand", 40, 48, 7, ["-x"]),
    ("smooth_37x45_b12", "smooth", 37, 45, 1, ["-B", "12"]),
    ("rand_17x9_b2", "rand", 17, 9, 16, ["-B", "2"]),
    ("smooth_9x9_b8", "smooth", 9, 9, 21, []),
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
            fl |= K.NO_SUBBANDS
    return B, Q, fl


def synth(kind, H, W, seed):
    """make_golden.py's inputs, and "const": one colour all over, so that C = 0 exactly (its
    "flat" is constant per 8 x 8 block only, which leaves a covariance of rank one)."""
    if kind == "const":
        rng = np.random.Generator(np.random.PCG64(seed))
        return np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (H, W, 3)).copy()
    return G.synth(kind, H, W, seed)


def run_ref(sub, in_fn, out_fn, flags):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.path.join(HERE, "shims") + os.pathsep + G.REF_SRC
    env["VCF_GOLDEN_HIDE_IMAGECODECS"] = "1"
    env["OMP_NUM_THREADS"] = "1"
    cmd = [G.PY39, "-W", "ignore", os.path.join(HERE, "_run_ref_klt.py"), sub, in_fn, out_fn] + flags
    r = subprocess.run(cmd, env=env, cwd=G.REF_SRC, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"reference run failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    return int([l for l in r.stdout.splitlines() if l.startswith("RESULT_BYTES")][0].split()[1])


def do_case(tmp, name, kind, H, W, seed, flags):
    B, Q, fl = options(flags)
    D = B * B
    for attempt in range(8):
        rgb = synth(kind, H, W, seed + 1000 * attempt)
        in_fn = os.path.join(tmp, f"{name}.png")
        Image.fromarray(rgb).save(in_fn)
        enc = os.path.join(tmp, f"{name}_enc")
        dec = os.path.join(tmp, f"{name}_dec.png")
        nbytes = run_ref("encode", in_fn, enc, flags)
        tif = open(enc + ".tif", "rb").read()
        shape_bin = open(enc + "_shape.bin", "rb").read()
        w64 = np.load(enc + "_weights64.npy")
        w32 = np.load(enc + "_weights.npz")["weights"]
        assert w64.dtype == np.float64 and w64.shape == (3, D, D)
        assert w32.dtype == np.float32 and np.array_equal(w64.astype(np.float32), w32), "weights file"
        k = G.tiff_pixels(enc + ".tif")
        run_ref("decode", enc, dec, flags)
        decoded = np.array(Image.open(dec))
        ok = shape_bin == K.shape_bin(H, W)
        margins = []
        for order in ("fwd", "rev"):
            e = K.encode(rgb, w64, B, Q, fl, order)
            d = K.decode(k, H, W, w32, B, Q, fl, order, np.float64)
            d32 = K.decode(k, H, W, w32, B, Q, fl, order, np.float32)
            ok = (ok and np.array_equal(e["k"], k) and np.array_equal(d["rgb"], decoded)
                  and np.array_equal(d32["rgb"], decoded))
            margins.append((float(K.index_margin(e["pre"], Q).min()), float(K.pixel_margin(d["pre"]).min())))
        if kind == "const":
            # C = 0: eigh returns a permutation of the unit vectors, every product and sum is exact
            # in any order, so values that sit exactly on a threshold are safe
            assert np.all((w64 == 0) | (np.abs(w64) == 1)) and np.all(np.abs(w64).sum(2) == 1)
        else:
            ok = ok and min(m[0] for m in margins) >= 1e-9 and min(m[1] for m in margins) >= 1e-9
        if ok:
            break
        print(f"{name}: seed {seed + 1000 * attempt} is not robust, trying another", flush=True)
    else:
        raise RuntimeError(f"{name}: no robust seed")
    k32 = K.encode(rgb, w64, B, Q, fl)["k32"]
    wrapped = int(np.count_nonzero((k32 < 0) | (k32 > 255)))
    if name == "rand_64x72_q1":
        assert wrapped, "the wrap to u8 must be exercised"
    meta = dict(name=name, kind=kind, H=H, W=W, seed=seed + 1000 * attempt, flags=flags, B=B, Q=Q,
                encode_bytes=nbytes, k_shape=list(k.shape), n_blocks=K.n_blocks(H, W, B), wrapped_indices=wrapped,
                min_index_margin=min(m[0] for m in margins), min_pixel_margin=min(m[1] for m in margins),
                sha256=dict(rgb=G.sha(rgb.tobytes()), weights64=G.sha(w64.tobytes()), k=G.sha(k.tobytes()),
                            tif=G.sha(tif), decoded=G.sha(decoded.tobytes())))
    np.savez_compressed(os.path.join(HERE, f"klt_{name}.npz"), rgb=rgb, weights64=w64, k=k, decoded=decoded,
                        tif=np.frombuffer(tif, np.uint8), shape_bin=np.frombuffer(shape_bin, np.uint8))
    return meta


def main():
    if not os.path.exists(G.PY39) or not os.path.isdir(G.REF_SRC):
        sys.exit("needs /opt/conda/bin/python3.9 and /root/reference (build container only)")
    manifest = dict(
        generator="tests/golden/make_golden_klt.py",
        reference="Sistemas-Multimedia/VCF src/2D-KLT.py encode_fn/decode_fn (unmodified glue)",
        python="/opt/conda/bin/python3.9, tifffile stdlib-zlib path (imagecodecs hidden)",
        robustness="every case equals tests/klt_restated.py: indices given weights64 in both accumulation "
                   "orders, pixels in float64 and in float32, both orders each; min_index_margin = least "
                   "distance of coefficient / Q to a nonzero integer, min_pixel_margin = least distance of a "
                   "pixel value before truncation to 1..255 (float64, over both orders)",
        cases=[])
    with tempfile.TemporaryDirectory() as tmp:
        for c in CASES:
            manifest["cases"].append(do_case(tmp, *c))
            print("done", c[0], manifest["cases"][-1]["min_index_margin"], manifest["cases"][-1]["min_pixel_margin"],
                  manifest["cases"][-1]["wrapped_indices"], flush=True)
    with open(os.path.join(HERE, "manifest_klt.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()

"""Generate the 2D-LBT fixtures under tests/golden/ from the reference itself.

Run on the CPU, where the reference is (it is not on the GPU machine):

    python tests/golden/make_golden_lbt.py

Runs the reference's unmodified src/2D-LBT.py as a program (encode, then
decode) under this interpreter through _run_ref_lbt.py -> _run_ref_main.py,
with -c z_lib (the entropy codec whose imports exist here), the shims of
make_golden.py and tests/golden/shims_lbt/ (skimage.io over PIL, cv2 with
imwrite).  The runner seeds torch and records the initial weights the
reference draws.

Writes lbt_<case>.npz (the image, the initial We and Wd, the reference's .pth
bytes, its trained encoder matrix, its decoder matrix and mean, its index array, its code-stream and
_shape.bin, its decoded pixels) and manifest_lbt.json.  Every case is also
computed with tests/lbt_restated.py from the same initial weights, in float64;
the manifest records
  d_ref       the largest absolute difference between the reference's float32
              matrices (encoder and decoder) and the restatement's,
  spread      the relative difference of the float64 loss at the two,
  index_boundary / pixel_boundary / *_disagree
              the share of values in the boundary sets (tests/lbt_restated.py)
              and the share of them on which reference and restatement differ.
A case whose boundary sets hold more than 1 % of its values, or on which the
reference differs from the restatement off them, gets another image seed.
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
import lbt_restated as R  # noqa: E402

REF_SRC = G.REF_SRC
TORCH_SEED = 0

CASES = [
    # name, H, W, image seed, reference CLI flags (shared by encode and decode), encode-only flags
    ("rand_37x45", 37, 45, 1, [], ["--epochs", "20"]),
    ("rand_16x24_b4_q8", 16, 24, 1, ["-B", "4", "-q", "8"], ["--epochs", "20"]),
    ("rand_9x9", 9, 9, 1, [], ["--epochs", "20"]),
    ("rand_15x21_b3", 15, 21, 1, ["-B", "3"], ["--epochs", "20"]),
    ("rand_40x48_x", 40, 48, 1, ["-x"], ["--epochs", "20"]),
    ("rand_40x48_p", 40, 48, 1, ["-p"], ["--epochs", "20"]),
    ("rand_32x32_b4_q1", 32, 32, 1, ["-B", "4", "-q", "1"], ["--epochs", "20"]),
    ("rand_24x32_b4_full", 24, 32, 1, ["-B", "4"], []),
]


def options(flags):
    o = dict(B=8, Q=32, flags=0, epochs=1000)
    it = iter(flags)
    for f in it:
        if f == "-B":
            o["B"] = int(next(it))
        elif f == "-q":
            o["Q"] = int(next(it))
        elif f == "--epochs":
            o["epochs"] = int(next(it))
        elif f == "-x":
            o["flags"] |= R.NO_SUBBANDS
        elif f == "-p":
            o["flags"] |= R.PERCEPTUAL
    return o


def run_ref(sub, record, flags):
    """`python 2D-LBT.py <sub> -c z_lib <flags>`: /tmp/original.png -> /tmp/encoded* -> /tmp/decoded.png
    (the reference's encode() and decode() ignore -o, -e and -d, 2D-LBT.py:465-466, 566-567)."""
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(HERE, "shims_lbt"), os.path.join(HERE, "shims"), REF_SRC])
    env["OMP_NUM_THREADS"] = "1"
    cmd = [sys.executable, "-W", "ignore", os.path.join(HERE, "_run_ref_lbt.py"), str(TORCH_SEED), record, "2D-LBT",
           sub, "-c", "z_lib"] + flags
    r = subprocess.run(cmd, env=env, cwd=REF_SRC, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"reference run failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")


def do_case(tmp, name, H, W, seed, flags, enc_flags):
    import torch
    o = options(flags + enc_flags)
    B, Q, fl, epochs = o["B"], o["Q"], o["flags"], o["epochs"]
    D = B * B
    for attempt in range(16):
        img_seed = seed + 1000 * attempt
        rgb = R.synth_frame(H, W, img_seed)
        for f in ("/tmp/encoded.npz", "/tmp/encoded_shape.bin", "/tmp/encoded.weights.pth", "/tmp/decoded.png"):
            if os.path.exists(f):
                os.remove(f)
        Image.fromarray(rgb).save("/tmp/original.png")
        record = os.path.join(tmp, f"{name}_init.npz")
        run_ref("encode", record, flags + enc_flags)
        init = np.load(record)
        we0, wd0, we_ref = init["we0"], init["wd0"], init["we"]
        assert we0.shape == (D, D) and wd0.shape == (D, D) and we0.dtype == np.float32 and int(init["draws"]) == 4
        pth = open("/tmp/encoded.weights.pth", "rb").read()
        npz = open("/tmp/encoded.npz", "rb").read()
        shape_bin = open("/tmp/encoded_shape.bin", "rb").read()
        ck = torch.load("/tmp/encoded.weights.pth", weights_only=True)
        wd_ref = ck["decoder_state"]["weight"].numpy().copy()
        mean_ref = float(ck["mean_val"])
        k = np.load("/tmp/encoded.npz")["a"]
        run_ref("decode", os.path.join(tmp, "unused.npz"), flags)
        decoded = np.array(Image.open("/tmp/decoded.png"))
        assert shape_bin == R.shape_bin(H, W) and wd_ref.dtype == np.float32 and wd_ref.shape == (D, D)

        # the restatement, float64, from the same initial weights
        X = R.centred(rgb, B, mean_ref).astype(np.float64)
        we, wd = R.train(X, we0, wd0, epochs)
        d_ref = float(np.max(np.abs(wd - wd_ref)))
        d_ref = max(d_ref, float(np.max(np.abs(we - we_ref))))
        loss_ref = float(R.loss_terms(X, we_ref.astype(np.float64), wd_ref.astype(np.float64))[0])
        loss_rest = float(R.loss_terms(X, we, wd)[0])
        e = R.encode(rgb, we_ref, mean_ref, B, Q, fl)
        d = R.decode(k, H, W, wd_ref, mean_ref, B, Q, fl)
        ib, pb = R.index_boundary(e["pre"], e["mag"], D), R.pixel_boundary(d["pre"], d["mag"], D)
        i_bad, p_bad = e["k"] != k, d["rgb"] != decoded
        ok = (ib.mean() <= 0.01 and pb.mean() <= 0.01 and not np.any(i_bad & ~ib) and not np.any(p_bad & ~pb)
              and np.all(np.abs(e["k"].astype(int) - k) <= 1) and np.all(np.abs(d["rgb"].astype(int) - decoded) <= 1)
              and abs(float(R.mean_of(rgb, B)) - mean_ref) <= 2.0 ** -17)
        if ok:
            break
        print(f"{name}: image seed {img_seed} rejected (index boundary {ib.mean():.4f}, off-boundary index "
              f"differences {int(np.sum(i_bad & ~ib))}, pixel boundary {pb.mean():.4f}, off-boundary pixel "
              f"differences {int(np.sum(p_bad & ~pb))})", flush=True)
    else:
        raise RuntimeError(f"{name}: no image seed passes")
    meta = dict(name=name, H=H, W=W, image_seed=img_seed, torch_seed=TORCH_SEED, flags=flags, encode_flags=enc_flags,
                B=B, Q=Q, epochs=epochs, k_shape=list(k.shape), rows=int(X.shape[0]), d_ref=d_ref,
                spread=abs(loss_ref - loss_rest) / abs(loss_rest), loss_restated=loss_rest,
                loss_reference=loss_ref,
                index_boundary=float(ib.mean()), index_boundary_disagree=float((i_bad & ib).sum() / max(1, ib.sum())),
                pixel_boundary=float(pb.mean()), pixel_boundary_disagree=float((p_bad & pb).sum() / max(1, pb.sum())))
    np.savez_compressed(os.path.join(HERE, f"lbt_{name}.npz"), rgb=rgb, we0=we0, wd0=wd0, we_ref=we_ref, wd_ref=wd_ref,
                        mean_ref=np.float64(mean_ref), k=k, decoded=decoded, pth=np.frombuffer(pth, np.uint8),
                        npz=np.frombuffer(npz, np.uint8), shape_bin=np.frombuffer(shape_bin, np.uint8))
    return meta


def main():
    if not os.path.isdir(REF_SRC):
        sys.exit("needs the reference's sources")
    manifest = dict(generator="tests/golden/make_golden_lbt.py",
                    reference="Sistemas-Multimedia/VCF src/2D-LBT.py run as a program, -c z_lib", cases=[])
    with tempfile.TemporaryDirectory() as tmp:
        for c in CASES:
            manifest["cases"].append(do_case(tmp, *c))
            m = manifest["cases"][-1]
            print("done", c[0], "d_ref", m["d_ref"], "spread", m["spread"], "boundary", m["index_boundary"],
                  m["pixel_boundary"], flush=True)
    with open(os.path.join(HERE, "manifest_lbt.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()

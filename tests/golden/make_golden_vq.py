"""Golden fixtures for the vector quantizer (tests/golden/vq_*.npz).

    python tests/golden/make_golden_vq.py

k-means fixtures (vq_<name>.npz), made with this interpreter's scikit-learn:
the image, an explicit initial codebook (K data vectors, drawn by a seeded
generator), what sklearn.cluster.KMeans(init=<that array>, n_init=1,
algorithm="lloyd") returned for the image's blocks (labels, centres, n_iter_,
inertia) and sklearn's inertias for init="k-means++", random_state 0..7.
Every fixture is checked for robustness before it is written: in the
restatement (tests/vq_restated.py) the gap between the best and the
second-best distance of every vector in every iteration, from the fixture's
codebook and from the restated k-means++ (seed 0), must exceed
gamma = 4 * D * 2^-52 * (255^2 * D), the rounding bound of a D-term dot
product of u8 data; else the image seed moves on.  The restated fit must also
reproduce sklearn's labels and n_iter_, and reach an inertia no greater than
the worst of sklearn's eight.

Reference pairs (vq_ref_VQ.npz, vq_ref_color-VQ.npz): src/VQ.py and
src/color-VQ.py run unmodified as programs (tests/golden/_run_ref_main.py)
under /opt/conda/bin/python3.9 (scikit-learn 0.24.2, tifffile 2021.7.2) with
the shims of tests/golden/shims (cv2; information_theory.information, A14):
the label file's bytes and pixels, the codebook file's bytes and array, the
decoded image.  The reference does not seed its k-means, so another run gives
another codebook; the pair pins the decoder and the file layout.
"""
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import vq_restated as R  # noqa: E402
from make_golden import PY39, REF_SRC, synth, tiff_pixels  # noqa: E402

# name, kind, H, W, BS, K
CASES = [
    ("smooth_32x48_b4_k16", "smooth", 32, 48, 4, 16),
    ("rand_32x48_b4_k16", "rand", 32, 48, 4, 16),
    ("rand_24x40_b2_k32", "rand", 24, 40, 2, 32),
    ("rand_16x16_b1_k8", "rand", 16, 16, 1, 8),
    ("smooth_64x96_b4_k256", "smooth", 64, 96, 4, 256),
    ("smooth_128x160_b8_k300", "smooth", 128, 160, 8, 300),
]
REF_CASES = [("VQ", ["-b", "4", "-q", "16"], 71), ("color-VQ", ["-q", "8"], 72)]


def image(kind, H, W, seed):
    if kind == "smooth":
        # make_golden's smooth field is nearly flat at these sizes: a steeper one, so that K clusters exist
        rng = np.random.Generator(np.random.PCG64(seed))
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        ch = [128 + 70 * np.sin(x / 9 + c) + 45 * np.cos(y / 7 - c) + rng.normal(0, 6, (H, W)) for c in range(3)]
        return np.clip(np.rint(np.stack(ch, -1)), 0, 255).astype(np.uint8)
    return synth(kind, H, W, seed)


def try_case(kind, H, W, BS, K, seed):
    from sklearn.cluster import KMeans
    img = image(kind, H, W, seed)
    X = R.blocks(img, BS)
    N, D = X.shape
    g = R.gamma(D)
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    init = X[np.sort(rng.choice(N, K, replace=False))]
    if len(np.unique(init, axis=0)) != K:
        return None, "duplicate initial centroids"
    gaps = []
    cent, labels, rep = R.fit(X, K, init=init, gaps=gaps)
    if min(gaps) <= g:
        return None, f"gap {min(gaps):.3g} <= gamma {g:.3g} (explicit init)"
    gaps = []
    _, _, own = R.fit(X, K, seed=0, gaps=gaps)
    if min(gaps) <= g:
        return None, f"gap {min(gaps):.3g} <= gamma {g:.3g} (k-means++ seed 0)"
    km = KMeans(n_clusters=K, init=init.astype(np.float64), n_init=1, algorithm="lloyd").fit(X.astype(int))
    assert np.array_equal(km.labels_, labels), "the restatement's labels differ from sklearn's"
    assert km.n_iter_ == rep["n_iter"], (km.n_iter_, rep["n_iter"])
    assert np.abs(km.cluster_centers_ - cent).max() <= 1e-10
    pp = np.array([KMeans(n_clusters=K, init="k-means++", n_init=1, algorithm="lloyd", random_state=s)
                   .fit(X.astype(int)).inertia_ for s in range(8)])
    assert own["inertia"] <= pp.max(), f"restated k-means++ fit {own['inertia']} above sklearn's worst {pp.max()}"
    arrays = dict(img=img, BS=np.int32(BS), K=np.int32(K), init=init.astype(np.uint8),
                  sk_labels=km.labels_.astype(np.uint16), sk_centers=km.cluster_centers_,
                  sk_n_iter=np.int32(km.n_iter_), sk_inertia=np.float64(km.inertia_), sk_pp_inertias=pp)
    info = dict(seed=seed, n_iter=int(km.n_iter_), stop=rep["stop_reason"], own_inertia=own["inertia"],
                own_over_median=own["inertia"] / float(np.median(pp)), own_n_iter=own["n_iter"],
                own_stop=own["stop_reason"])
    return arrays, info


def ref_pair(module, flags, seed):
    from make_golden_standalone import _run
    for fn in ("/tmp/original.png", "/tmp/decoded.png", "/tmp/encoded.tif", "/tmp/encoded_centroids.npz"):
        if os.path.exists(fn):
            os.remove(fn)
    rgb = image("smooth", 32, 48, seed)
    Image.fromarray(rgb).save("/tmp/original.png")
    _run(module, ["encode"] + flags)
    arrays = dict(rgb=rgb, enc=np.frombuffer(open("/tmp/encoded.tif", "rb").read(), np.uint8),
                  labels=tiff_pixels("/tmp/encoded.tif"),
                  codebook_file=np.frombuffer(open("/tmp/encoded_centroids.npz", "rb").read(), np.uint8),
                  codebook=np.load("/tmp/encoded_centroids.npz")["a"])
    _run(module, ["decode"] + flags)
    arrays["decoded"] = np.array(Image.open("/tmp/decoded.png"))
    np.savez_compressed(os.path.join(HERE, f"vq_ref_{module}.npz"), **arrays)
    return dict(module=module, flags=flags, seed=seed, labels_dtype=str(arrays["labels"].dtype),
                labels_shape=list(arrays["labels"].shape), codebook_dtype=str(arrays["codebook"].dtype),
                codebook_shape=list(arrays["codebook"].shape))


def main():
    manifest = dict(generator="tests/golden/make_golden_vq.py", cases=[], reference=[])
    for i, (name, kind, H, W, BS, K) in enumerate(CASES):
        for attempt in range(20):
            seed = 100 * (i + 1) + attempt
            arrays, info = try_case(kind, H, W, BS, K, seed)
            if arrays is not None:
                break
            print("retry", name, info, flush=True)
        else:
            sys.exit(f"no robust image for {name}")
        np.savez_compressed(os.path.join(HERE, f"vq_{name}.npz"), **arrays)
        manifest["cases"].append(dict(name=name, kind=kind, H=H, W=W, BS=BS, K=K, **info))
        print("done", name, info, flush=True)
    if os.path.exists(PY39) and os.path.isdir(REF_SRC):
        for module, flags, seed in REF_CASES:
            manifest["reference"].append(ref_pair(module, flags, seed))
            print("done", module, flush=True)
    else:
        sys.exit("the reference pairs need /opt/conda/bin/python3.9 and /root/reference (build container only)")
    with open(os.path.join(HERE, "manifest_vq.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()

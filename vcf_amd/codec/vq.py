"""The vector-quantization codecs, drop-ins for src/VQ.py's and
src/color-VQ.py's CoDec classes.

VQ.py clusters the BS x BS x C blocks of the image with k-means, sends the
block labels (H/BS x W/BS uint16) through the -c entropy codec and writes the
codebook next to the code-stream ({encoded}_centroids.npz, array `a`);
color-VQ.py does the same with one pixel per vector.  k-means runs on the GPU
(vcf_amd.vq: sklearn's Lloyd iteration, started by a seeded k-means++; the
reference does not seed its own, so its codebooks differ from run to run and
from these).  encode()/decode() keep the reference's hard-wired
/tmp/original.png, /tmp/encoded<ext> and /tmp/decoded.png, with the codebook
named after -e as VQ.py:110 does; encode_fn/decode_fn take explicit names and
put the codebook beside the code-stream they name.
"""
from __future__ import annotations

import logging
import os

import numpy as np

from .. import vq as VQ
from .pixel import _PixelCoDec

DEFAULT_BLOCK_SIZE = 4          # VQ.py:15
DEFAULT_N_CLUSTERS = 256        # VQ.py:17
DEFAULT_N_COLOR_CLUSTERS = 32   # color-VQ.py:14
SEED = 0                        # the CLIs have no seed flag


def energy(x) -> float:
    """information_theory.information.energy (un-vendored; A14, unpinned): the sum of squares in float64."""
    x = np.asarray(x, np.float64)
    return np.sum(x * x)


def sort_by_energy(centroids: np.ndarray, labels: np.ndarray):
    """VQ.py:87-100: codebook rows in ascending energy, labels renamed to match."""
    N_clusters = centroids.shape[0]
    centroids_energy = np.empty(N_clusters)
    for counter, i in enumerate(centroids):
        centroids_energy[counter] = energy(i)
    argsort_centroids = np.argsort(centroids_energy)
    lut = np.empty_like(argsort_centroids, dtype=np.int16)
    lut[argsort_centroids] = np.arange(N_clusters)
    labels = lut[labels]
    _centroids = np.empty_like(centroids)
    for i in range(N_clusters):
        _centroids[lut[i]] = centroids[i]
    return _centroids, labels


class _VQBase(_PixelCoDec):
    BS = 1

    def __init__(self, args, min_index_val=0, max_index_val=255):
        super().__init__(args)
        self.seed = SEED
        self.report = None        # vcf_amd.vq.FitReport of the last quantize()

    def _codebook_fn(self, prefix):
        return f"{prefix}_centroids.npz"

    def _check(self, img):
        if img.ndim != 3 or img.dtype != np.uint8 or not 1 <= img.shape[2] <= 4:
            raise NotImplementedError(f"{img.dtype} {img.shape} images: the HIP path takes u8 H x W x C, C <= 4")

    def _fit(self, img):
        H, W, _ = img.shape
        if H % self.BS or W % self.BS:
            # VQ.py:72: np.reshape of a clipped block raises
            raise ValueError(f"cannot reshape: {H} x {W} is not a whole number of {self.BS} x {self.BS} blocks")
        n_blocks = (H // self.BS) * (W // self.BS)
        if n_blocks < self.N_clusters:
            logging.warning('\033[91m' + "Warning: Must reduce number of clusters. Image not big enough | too much "
                            "pixel reducction" + '\033[0m')
            self.N_clusters = n_blocks
        if self.N_clusters > VQ.MAX_K:
            raise NotImplementedError(f"{self.N_clusters} clusters: the HIP path takes up to {VQ.MAX_K}")
        centroids, labels, self.report = VQ.fit(img, self.BS, self.N_clusters, seed=self.seed)
        logging.info(f"k-means: {self.report}")
        return centroids, labels

    def encode(self):
        return self._encode("/tmp/original.png", "/tmp/encoded", self._codebook_fn(self.args.encoded))

    def decode(self):
        return self._decode("/tmp/encoded", "/tmp/decoded.png", self._codebook_fn(self.args.encoded))

    def encode_fn(self, in_fn, out_fn):
        return self._encode(in_fn, out_fn, self._codebook_fn(out_fn))

    def decode_fn(self, in_fn, out_fn):
        return self._decode(in_fn, out_fn, self._codebook_fn(in_fn))

    def _save_codebook(self, fn, centroids):
        np.savez_compressed(file=fn, a=centroids)
        self.total_output_size += os.path.getsize(fn)

    def _load_codebook(self, fn):
        self.total_input_size += os.path.getsize(fn)
        return np.load(file=fn)["a"]

    def _labels(self, k):
        k = np.asarray(k)
        if k.ndim != 2:
            raise ValueError(f"label array of shape {k.shape}: expected two dimensions")
        return np.ascontiguousarray(k, dtype=np.uint16)


class VQCoDec(_VQBase):
    """VQ.CoDec (src/VQ.py:34-137)."""

    def __init__(self, args, min_index_val=0, max_index_val=255):
        super().__init__(args)
        self.BS = int(getattr(args, "block_size_VQ", DEFAULT_BLOCK_SIZE))
        self.N_clusters = int(getattr(args, "N_clusters", DEFAULT_N_CLUSTERS))
        if self.BS < 1 or self.BS > 16:
            raise NotImplementedError(f"block size {self.BS}: the HIP path takes 1..16")

    def quantize(self, img, codebook_fn=None):
        """:66-113: labels (H/BS x W/BS uint16); the codebook (K, BS*BS, C) float64 goes to its file."""
        centroids, labels = self._fit(img)
        centroids, labels = sort_by_energy(centroids, labels)
        labels = labels.reshape((img.shape[0] // self.BS, img.shape[1] // self.BS)).astype(np.uint16)
        centroids = centroids.reshape(centroids.shape[0], self.BS * self.BS, img.shape[2])
        self._save_codebook(codebook_fn or self._codebook_fn(self.args.encoded), centroids)
        return labels

    def dequantize(self, labels, codebook_fn=None):
        """:117-137 and decode's .astype(np.uint8): the u8 image."""
        centroids = self._load_codebook(codebook_fn or self._codebook_fn(self.args.encoded))
        if centroids.ndim != 3 or centroids.shape[1] != self.BS * self.BS:
            raise ValueError(f"cannot reshape a codebook of shape {centroids.shape} into {self.BS} x {self.BS} blocks")
        return VQ.decode(self._labels(labels), centroids, self.BS, centroids.shape[2])

    def _encode(self, in_fn, out_fn, codebook_fn):
        img = self.encode_read_fn(in_fn)
        self._check(img)
        k = self.quantize(img, codebook_fn)
        return self.encode_write_fn(self.compress(k), out_fn)

    def _decode(self, in_fn, out_fn, codebook_fn):
        k = self.decompress(self.decode_read_fn(in_fn))
        y = self.dequantize(k, codebook_fn)
        return self.decode_write_fn(self.filter(y), out_fn)


class ColorVQCoDec(_VQBase):
    """color-VQ.CoDec (src/color-VQ.py:29-90): one pixel per vector, a uint8 codebook, labels unsorted."""

    def __init__(self, args, min_index_val=0, max_index_val=255):
        super().__init__(args)
        self.N_clusters = int(getattr(args, "N_color_clusters", DEFAULT_N_COLOR_CLUSTERS))

    def quantize(self, img):
        """:65-79: (labels H x W uint16, centroids (K, 3) uint8)."""
        if img.shape[2] != 3:
            raise ValueError(f"cannot reshape array of shape {img.shape} into RGB triplets")   # :70
        if img.shape[0] * img.shape[1] < self.N_clusters:
            # KMeans.fit: n_samples should be >= n_clusters
            raise ValueError(f"n_samples={img.shape[0] * img.shape[1]} should be >= n_clusters={self.N_clusters}.")
        centroids, labels = self._fit(img)
        return labels.reshape(img.shape[:2]).astype(np.uint16), centroids.astype(np.uint8)

    def dequantize(self, labels, centroids):
        """:81-90: centroids[labels] as uint8."""
        centroids = np.asarray(centroids)
        if centroids.ndim != 2 or centroids.shape[1] != 3:
            raise ValueError(f"cannot reshape a codebook of shape {centroids.shape} into RGB triplets")
        return VQ.decode(self._labels(labels), centroids.astype(np.float64), 1, 3)

    def _encode(self, in_fn, out_fn, codebook_fn):
        img = self.encode_read_fn(in_fn)
        self._check(img)
        labels, centroids = self.quantize(img)
        output_size = self.encode_write_fn(self.compress(labels), out_fn)
        self._save_codebook(codebook_fn, centroids)      # :45-47: after the code-stream
        return output_size

    def _decode(self, in_fn, out_fn, codebook_fn):
        labels = self.decompress(self.decode_read_fn(in_fn))
        centroids = self._load_codebook(codebook_fn)
        img = self.dequantize(labels, centroids)
        return self.decode_write_fn(self.filter(img), out_fn)

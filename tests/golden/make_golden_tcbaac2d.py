"""Regenerates tests/golden/tcbaac2d.npz: the symbols of some of the
version-4 test frames (tests/tcbaac2d_cases.py) and the containers the host
coder (HostTiledCBAACCodec, vcf_cbaac2d_*) writes for them.

    python tests/golden/make_golden_tcbaac2d.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tcbaac2d_cases import cases  # noqa: E402
from vcf_amd import tcbaac as T  # noqa: E402

NAMES = ("one_tile", "cropped_3ch", "one_symbol", "one_row", "one_column", "tiles_16x32", "two_dims", "all_128")


def main():
    out = {}
    for name in NAMES:
        img, tile, nclass = cases()[name]
        data = T.HostTiledCBAACCodec(nclass=nclass, ctx2d=True, tile=tile).compress(img).getvalue()
        out[f"sym_{name}"] = img
        out[f"bytes_{name}"] = np.frombuffer(data, np.uint8)
    np.savez_compressed(os.path.join(HERE, "tcbaac2d.npz"), **out)


if __name__ == "__main__":
    main()

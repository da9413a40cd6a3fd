#!/usr/bin/env python3
"""Drop-in for `python 2D-LBT.py [-g] {encode,decode} ...` (src/2D-LBT.py):
YCoCg + a learned B x B block transform (a linear autoencoder trained per image) + deadzone +
TIFF, the hot span on the GPU."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from vcf_amd.codec import parser as P  # noqa: E402
from vcf_amd.codec.main import main  # noqa: E402
from vcf_amd.codec.lbt2d import CoDec  # noqa: E402

if __name__ == "__main__":
    main(P.lbt_parser(entropy=P.entropy_of(sys.argv[1:]), filter=P.filter_of(sys.argv[1:])), CoDec)

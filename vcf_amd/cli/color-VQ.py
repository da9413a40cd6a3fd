#!/usr/bin/env python3
"""Drop-in for `python color-VQ.py [-g] {encode,decode} ...` (src/color-VQ.py):
colour quantization by clustering the RGB triplets, k-means on the GPU."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from vcf_amd.codec import parser as P  # noqa: E402
from vcf_amd.codec.main import main  # noqa: E402
from vcf_amd.codec.vq import ColorVQCoDec  # noqa: E402

if __name__ == "__main__":
    main(P.build_color_vq_parser(entropy=P.entropy_of(sys.argv[1:])), ColorVQCoDec)

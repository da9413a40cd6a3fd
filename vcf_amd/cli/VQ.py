#!/usr/bin/env python3
"""Drop-in for `python VQ.py [-g] {encode,decode} ...` (src/VQ.py):
vector quantization of the image's pixel blocks, k-means on the GPU."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from vcf_amd.codec import parser as P  # noqa: E402
from vcf_amd.codec.main import main  # noqa: E402
from vcf_amd.codec.vq import VQCoDec  # noqa: E402

if __name__ == "__main__":
    main(P.build_vq_parser(entropy=P.entropy_of(sys.argv[1:])), VQCoDec)

#!/usr/bin/env python3
"""Drop-in for `python RDE.py [-o original] [-c codestream] [-d decoded]` (src/RDE.py): sizes, bits
per pixel, RMSE and J = R + D, the distortion measured on the GPU; -N evaluates a frame sequence, --ssim
adds one `RDE: SSIM: x.xxxx` line."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from vcf_amd.codec.rde import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())

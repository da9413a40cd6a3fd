#!/usr/bin/env python3
"""`python RD-curve.py -o image -q 8,16,32 [-N n] [-B b] [-p] [-x] [--ssim] [--json]`: bytes, bits per
pixel, RMSE, PSNR and J (with --ssim, the SSIM too) of the default 2D-DCT chain for every -q value, the frames
resident on the GPU.
No counterpart in the reference (there: a loop of 2D-DCT.py encode, decode and RDE.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from vcf_amd.codec.rde import curve_main  # noqa: E402

if __name__ == "__main__":
    sys.exit(curve_main())

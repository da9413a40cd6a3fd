#!/usr/bin/env python3
"""`python rate-control.py encode -o img.png -e out --target_bpp B | --target_bytes N [--rate estimate|coded]`
plus 2D-DCT.py's flags: the files of `2D-DCT.py encode -q <chosen>` and out_q.txt with the chosen
integer.  `decode --q_from_files` decodes at it (vcf_amd/codec/ratecontrol.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from vcf_amd.codec import parser as P  # noqa: E402
from vcf_amd.codec.main import main  # noqa: E402
from vcf_amd.codec.ratecontrol import CoDec  # noqa: E402

if __name__ == "__main__":
    main(P.rate_control_parser(entropy=P.entropy_of(sys.argv[1:])), CoDec)

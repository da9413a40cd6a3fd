"""tests/golden/shims/cv2.py plus imwrite (BGR in, as OpenCV), over PIL."""
import importlib.util
import os

import numpy as np
from PIL import Image

_spec = importlib.util.spec_from_file_location(
    "_vcf_cv2_shim", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "shims", "cv2.py"))
_base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_base)
globals().update({k: v for k, v in vars(_base).items() if not k.startswith("_")})


def imwrite(fn, img):
    Image.fromarray(np.asarray(img)[..., ::-1]).save(fn)
    return True

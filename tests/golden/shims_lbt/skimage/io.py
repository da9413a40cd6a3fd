"""skimage.io.imread / imsave for 8-bit RGB files, over PIL (lossless)."""
import numpy as np
from PIL import Image


def imread(fn):
    return np.array(Image.open(fn))


def imsave(fn, img, **kwargs):
    Image.fromarray(np.asarray(img)).save(fn)

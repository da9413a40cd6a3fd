"""The entropy-codec registry behind -c (no_filter.py:14-21): what every
codec of this package hands its index arrays to."""
from __future__ import annotations

from .tiff import TIFFCodec


def _cbaac(args=None):
    from ..cbaac import CBAACCodec
    return CBAACCodec(getattr(args, "order", 0) if args is not None else 0)


def _cbahc(args=None):
    from ..cbahc import CBAHCCodec
    return CBAHCCodec(getattr(args, "order", 0) if args is not None else 0)


def _tcbaac(args=None):
    from ..tcbaac import DEFAULT_SEG, TiledCBAACCodec
    return TiledCBAACCodec(getattr(args, "order", 0) if args is not None else 0,
                           getattr(args, "segment_symbols", DEFAULT_SEG) if args is not None else DEFAULT_SEG)


def _tcbaac_prior(args=None):
    from ..tcbaac import CLASS_SEG, PRIOR_CLASSES, TiledCBAACCodec
    return TiledCBAACCodec(getattr(args, "order", 0) if args is not None else 0,
                           getattr(args, "segment_symbols", CLASS_SEG) if args is not None else CLASS_SEG, prior=True,
                           nclass=PRIOR_CLASSES)


def _tcbaac_2d(args=None):
    from ..tcbaac import PRIOR_CLASSES, TILE_2D, TiledCBAACCodec
    return TiledCBAACCodec(0, prior=True, nclass=PRIOR_CLASSES, ctx2d=True, tile=TILE_2D)


class ZlibCodec:
    """z_lib.py:12-29: the index array as np.savez_compressed(a=...), on the host."""
    file_extension = ".npz"

    def compress(self, img):
        import io

        import numpy as np
        out = io.BytesIO()
        np.savez_compressed(file=out, a=img)
        return out

    def decompress(self, codestream):
        import io

        import numpy as np
        data = codestream.read() if hasattr(codestream, "read") else codestream
        with np.load(io.BytesIO(data)) as z:
            return z["a"]


# TCBAAC: CBAAC in independent segments on the GPU (vcf_amd/tcbaac.py, a new container);
# TCBAACP: the same with every segment's models seeded by a prior row of the frame: 8 rows, one per run of
# segments (about one subband row each), 4096-symbol segments (container version 3);
# TCBAAC2D: every channel plane in 64 x 64 tiles, each symbol's model chosen by the magnitudes of its left and
# upper neighbours in the tile (16 contexts), seeded per prior class and context (container version 4)
ENTROPY_CODECS = {"TIFF": TIFFCodec, "z_lib": ZlibCodec, "CBAAC": _cbaac, "CBAHC": _cbahc, "TCBAAC": _tcbaac, "TCBAACP": _tcbaac_prior,
                  "TCBAAC2D": _tcbaac_2d}


def register_entropy_codec(name, cls):
    ENTROPY_CODECS[name] = cls


def make_entropy(args):
    """The entropy codec named by -c (no_filter.py:14-21)."""
    ec_name = getattr(args, "entropy_image_codec", "TIFF")
    if ec_name not in ENTROPY_CODECS:
        raise NotImplementedError(f"entropy codec {ec_name!r} (have: {sorted(ENTROPY_CODECS)})")
    maker = ENTROPY_CODECS[ec_name]
    return maker(args) if maker in (_cbaac, _cbahc, _tcbaac, _tcbaac_prior, _tcbaac_2d) else maker()

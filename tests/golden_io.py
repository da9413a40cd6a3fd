"""Loading fixtures of tests/golden/ that are stored in pieces.

No committed file may exceed 1 MiB, so an .npz above that is kept as its bytes
cut into consecutive pieces NAME.npz.part00, NAME.npz.part01, ... (each at
most PART_BYTES; `python tests/golden_io.py NAME.npz` cuts a freshly made
file and removes it).  load_npz() reads either form."""
import glob
import io
import os
import sys

import numpy as np

PART_BYTES = 900 * 1024


def load_npz(path: str, **kw):
    """np.load(path, **kw) of a whole file, or of its pieces joined in order."""
    if os.path.exists(path):
        return np.load(path, **kw)
    parts = sorted(glob.glob(glob.escape(path) + ".part[0-9][0-9]"))
    if not parts:
        raise FileNotFoundError(path)
    data = bytearray()
    for p in parts:
        with open(p, "rb") as f:
            data += f.read()
    return np.load(io.BytesIO(bytes(data)), **kw)


def split_npz(path: str) -> list:
    """Cut `path` into pieces of at most PART_BYTES and remove it."""
    with open(path, "rb") as f:
        data = f.read()
    for old in glob.glob(glob.escape(path) + ".part[0-9][0-9]"):
        os.remove(old)
    names = []
    for i in range(0, len(data), PART_BYTES):
        names.append(f"{path}.part{i // PART_BYTES:02d}")
        with open(names[-1], "wb") as f:
            f.write(data[i:i + PART_BYTES])
    os.remove(path)
    return names


if __name__ == "__main__":
    for fn in sys.argv[1:]:
        print(fn, "->", len(split_npz(fn)), "pieces")

"""The 2D-LBT side file {out}.weights.pth without torch.

2D-LBT.py:133-136 stores torch.save({'decoder_state': {'weight': float32 (D, D)},
'mean_val': float}).  torch.save writes an uncompressed zip: <prefix>/data.pkl
(a protocol-2 pickle in which the tensor is a call of
torch._utils._rebuild_tensor_v2 on a persistent id ('storage',
torch.FloatStorage, '0', 'cpu', numel)), <prefix>/data/0 (the little-endian
float32 values, 64-byte aligned in the file), and the small records version,
byteorder, .format_version and .storage_alignment.  This module writes exactly
that payload, byte for byte the same on every run, and reads it back with an
unpickler that admits those globals and nothing else: a .pth file is a pickle,
and a pickle from elsewhere can name any callable.
"""
from __future__ import annotations

import collections
import io
import pickle
import struct
import zipfile

import numpy as np

__all__ = ["save", "load", "dumps", "loads"]

PREFIX = "archive"
_ALIGN = 64


# ---- writer -----------------------------------------------------------------
def _uni(s: str) -> bytes:
    b = s.encode()
    return b"X" + struct.pack("<I", len(b)) + b


def _int(n: int) -> bytes:
    if n < 0x100:
        return b"K" + bytes([n])
    if n < 0x10000:
        return b"M" + struct.pack("<H", n)
    return b"J" + struct.pack("<i", n)


def _pickle(D: int, mean: float) -> bytes:
    """data.pkl as torch.save writes it for this payload (memo indices included)."""
    memo = iter(range(256))

    def put():
        return b"q" + bytes([next(memo)])

    p = b"\x80\x02}" + put() + b"("
    p += _uni("decoder_state") + put() + b"ccollections\nOrderedDict\n" + put() + b")R" + put()
    p += _uni("weight") + put() + b"ctorch._utils\n_rebuild_tensor_v2\n" + put() + b"(("
    p += _uni("storage") + put() + b"ctorch\nFloatStorage\n" + put() + _uni("0") + put() + _uni("cpu") + put()
    p += _int(D * D) + b"t" + put() + b"Q" + _int(0) + _int(D) + _int(D) + b"\x86" + put()
    p += _int(D) + _int(1) + b"\x86" + put() + b"\x89h\x02)R" + put() + b"t" + put() + b"R" + put() + b"s"
    # the state_dict's _metadata attribute: OrderedDict({'': {'version': 1}})
    p += b"}" + put() + _uni("_metadata") + put() + b"h\x02)R" + put() + _uni("") + put() + b"}" + put()
    p += _uni("version") + put() + _int(1) + b"sssb"
    p += _uni("mean_val") + put() + b"G" + struct.pack(">d", mean) + b"u."
    return p


def dumps(weight: np.ndarray, mean: float) -> bytes:
    """The bytes of the .pth file for a float32 (D, D) decoder matrix and the scalar mean."""
    w = np.asarray(weight)
    if w.dtype != np.float32 or w.ndim != 2 or w.shape[0] != w.shape[1]:
        raise ValueError(f"decoder weights {w.dtype} {w.shape} are not float32 (D, D)")
    w = np.ascontiguousarray(w).astype("<f4", copy=False)
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        def record(name, data, align=False):
            info = zipfile.ZipInfo(f"{PREFIX}/{name}", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_STORED
            if align:   # pad the local header with an extra field so the data starts on 64 bytes
                start = buf.tell() + 30 + len(info.filename.encode()) + 4
                pad = -start % _ALIGN
                info.extra = b"FB" + struct.pack("<H", pad) + b"Z" * pad
            z.writestr(info, data)

        record("data.pkl", _pickle(w.shape[0], float(mean)))
        record(".format_version", b"1")
        record(".storage_alignment", b"64")
        record("byteorder", b"little")
        record("data/0", w.tobytes(), align=True)
        record("version", b"3\n")
    return buf.getvalue()


def save(path: str, weight: np.ndarray, mean: float) -> None:
    data = dumps(weight, mean)
    with open(path, "wb") as f:
        f.write(data)


# ---- reader -----------------------------------------------------------------
class _FloatStorage:
    """Stands for torch.FloatStorage in the persistent id."""


def _rebuild_tensor_v2(storage, offset, size, stride, requires_grad=False, backward_hooks=None, metadata=None):
    return dict(storage=storage, offset=offset, size=tuple(size), stride=tuple(stride))


_ADMITTED = {
    ("collections", "OrderedDict"): collections.OrderedDict,
    ("torch._utils", "_rebuild_tensor_v2"): _rebuild_tensor_v2,
    ("torch", "FloatStorage"): _FloatStorage,
}


class _Unpickler(pickle.Unpickler):
    def find_class(self, module, name):
        try:
            return _ADMITTED[(module, name)]
        except KeyError:
            pass
        if module == "torch" and name.endswith("Storage"):
            raise ValueError(f"{module}.{name}: the decoder weights are not float32")
        raise pickle.UnpicklingError(f"global {module}.{name} is not part of a 2D-LBT weights file")

    def persistent_load(self, pid):
        if (not isinstance(pid, tuple) or len(pid) != 5 or pid[0] != "storage" or pid[1] is not _FloatStorage
                or not isinstance(pid[2], str) or not isinstance(pid[4], int)):
            raise pickle.UnpicklingError(f"persistent id {pid!r} is not a float32 storage")
        return pid[2], pid[4]


def loads(data: bytes, D: int | None = None):
    """-> (decoder weights float32 (D, D), mean as a Python float).  ValueError when the matrix is
    not float32 (D, D) (any square D when D is None); pickle.UnpicklingError for a pickle that
    names anything but the payload's own globals."""
    with zipfile.ZipFile(io.BytesIO(data)) as z:
        pkl = [n for n in z.namelist() if n.endswith("/data.pkl") or n == "data.pkl"]
        if len(pkl) != 1:
            raise ValueError("not a torch.save archive: no data.pkl")
        prefix = pkl[0][:-len("data.pkl")]
        obj = _Unpickler(io.BytesIO(z.read(pkl[0]))).load()
        try:
            t = obj["decoder_state"]["weight"]
            mean = obj["mean_val"]
            (key, numel), size, stride, offset = t["storage"], t["size"], t["stride"], t["offset"]
        except (KeyError, TypeError, ValueError) as e:
            raise ValueError("not a 2D-LBT weights file: decoder_state.weight / mean_val missing") from e
        if isinstance(mean, bool) or not isinstance(mean, (int, float)):
            raise ValueError(f"mean_val {mean!r} is not a number")
        if len(size) != 2 or size[0] != size[1] or (D is not None and size[0] != D):
            want = "(D, D)" if D is None else f"({D}, {D})"
            raise ValueError(f"decoder weights {size} are not float32 {want}")
        n = size[0]
        if stride != (n, 1) or offset != 0 or numel != n * n or not key.isdigit():
            raise ValueError("decoder weights are not one contiguous float32 storage")
        raw = z.read(f"{prefix}data/{key}")
        if len(raw) != 4 * n * n:
            raise ValueError(f"storage of {len(raw)} bytes does not hold float32 ({n}, {n})")
    return np.frombuffer(raw, "<f4").reshape(n, n).astype(np.float32), float(mean)


def load(path: str, D: int | None = None):
    with open(path, "rb") as f:
        return loads(f.read(), D)

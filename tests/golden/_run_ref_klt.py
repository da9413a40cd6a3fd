"""Runs ONE reference 2D-KLT encode_fn/decode_fn in-process under python3.9.

Invoked by make_golden_klt.py as
    PYTHONPATH=tests/golden/shims:/root/reference/src python3.9 _run_ref_klt.py \
        <encode|decode> <in_fn> <out_fn> [reference CLI flags...]
The reference module is imported unmodified, as _run_ref.py does.  On encode
LBT_Autoencoder.train is wrapped, only to record the float64 weights the
encoder transforms with (the file it writes holds them rounded to float32):
they go to <out_fn>_weights64.npy, one (D, D) matrix per channel in the order
of the calls.
"""
import importlib
import os
import sys

if os.environ.get("VCF_GOLDEN_HIDE_IMAGECODECS") == "1":
    sys.modules["imagecodecs"] = None
import warnings

warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402

sub, in_fn, out_fn = sys.argv[1:4]
flags = sys.argv[4:]
sys.argv = ["2D-KLT.py", sub] + flags
mod = importlib.import_module("2D-KLT")
import parser as ref_parser  # noqa: E402  (the reference's src/parser.py)

recorded = []
_train = mod.LBT_Autoencoder.train


def train(self, patches):
    r = _train(self, patches)
    recorded.append(np.array(self.weights, dtype=np.float64, copy=True))
    assert self.weights.dtype == np.float64
    return r


mod.LBT_Autoencoder.train = train

args = ref_parser.parser.parse_known_args()[0]
codec = mod.CoDec(args)
fn = codec.encode_fn if sub == "encode" else codec.decode_fn
n = fn(in_fn, out_fn)
if sub == "encode":
    assert len(recorded) == 3
    np.save(out_fn + "_weights64.npy", np.stack(recorded))
print(f"RESULT_BYTES {n}")
print(f"RESULT_BLOCK_SIZE {getattr(codec, 'block_size', None)}")

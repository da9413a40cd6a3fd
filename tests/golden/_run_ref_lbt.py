"""Runs the reference's src/2D-LBT.py as its own program through _run_ref_main.py, with two things
done from outside first: torch.manual_seed(<seed>), and torch.nn.init.normal_ wrapped to record
what it draws.  LBTModel.reset_weights (2D-LBT.py:67-69) draws the encoder matrix, then the
decoder matrix; it runs once at construction and once more when encode_image starts, so the last
two draws are the initial weights of the training.  torch.nn.Module.eval is wrapped too:
encode_image calls it on the model right after the last Adam step (:139), which is where the
trained encoder matrix, which no file holds, is recorded.  All go to <record>.npz (we0, wd0, we).

    PYTHONPATH=<shims_lbt>:<shims>:<reference src> python _run_ref_lbt.py <seed> <record> \\
        2D-LBT [reference CLI flags...]
"""
import os
import runpy
import sys

import numpy as np
import torch

seed, record = int(sys.argv[1]), sys.argv[2]
torch.manual_seed(seed)
torch.set_num_threads(1)
drawn = []
_normal = torch.nn.init.normal_


def normal_(tensor, *args, **kwargs):
    r = _normal(tensor, *args, **kwargs)
    drawn.append(tensor.detach().clone().numpy())
    return r


torch.nn.init.normal_ = normal_
trained = {}
_eval = torch.nn.Module.eval


def eval_(self):
    if hasattr(self, "encoder") and hasattr(self, "decoder"):
        trained["we"] = self.encoder.weight.detach().clone().numpy()
    return _eval(self)


torch.nn.Module.eval = eval_
sys.argv = [sys.argv[0]] + sys.argv[3:]
try:
    runpy.run_path(os.path.join(os.path.dirname(os.path.abspath(__file__)), "_run_ref_main.py"), run_name="__main__")
finally:
    if len(drawn) >= 2:
        np.savez(record, we0=drawn[-2], wd0=drawn[-1], draws=len(drawn), **trained)

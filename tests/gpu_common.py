"""What the GPU tests of the evaluation family (test_gpu_evaluate.py, test_gpu_evaluate_grad.py, test_gpu_certify.py) share: the
built library, a solver for a case group, the group's arguments as device tensors, bit-identity of two result dicts, a synthetic group."""
import numpy as np
import pytest

from tests import eval_cases as ec
from tests import util


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def solver(g, path=0, max_batch=None):
    import biped_mpc_py_amd as bm
    return bm.BatchSolver(cparams=ec.cparams_of(g, path), max_batch=max_batch or max(16, g["x_fb"].shape[0]))


def dev_args(a):
    """kernel_args as CUDA tensors of the dtypes the device entries take."""
    import torch
    dt = dict(x_fb=np.float32, foot=np.float32, contact=np.uint8, phase=np.int32, controls=np.float32, x_cmd=np.float32, mu=np.float32,
              x_ref=np.float32, foot_ref=np.float32)
    return {k: None if v is None else torch.from_numpy(np.ascontiguousarray(np.asarray(v).astype(dt[k]))).cuda() for k, v in a.items()}


def identical(x, y, where="", *, keys):
    for k in keys:
        assert np.array_equal(x[k], y[k], equal_nan=True), (where, k)


def synth_group(B, h, gait, seed):
    s = util.synth_batch(B, h, seed, gait=gait)
    return ec._group(h, s["half"], None, s["x_fb"], s["foot"], s["contact"], s["phase"], s["x_cmd"], np.zeros((B, h, 12)))

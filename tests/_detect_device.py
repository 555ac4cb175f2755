"""What test_gpu_detect_kernels.py and test_gpu_detect_edges.py share on the device (imported, never collected)."""
import numpy as np
import torch


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def run_tail(ops, case):
    """ops.mask_head_tail into an output pre-filled with NaN; a second call must return the same bits."""
    x, wd, bd, wm, bm, ids = case
    out = torch.full((x.shape[0], 2 * x.shape[1], 2 * x.shape[1]), float("nan"), device="cuda")
    args = (dev(x), dev(wd), dev(bd), dev(np.ascontiguousarray(wm.T)), dev(bm), dev(ids, torch.int32))
    got = ops.mask_head_tail(*args, out=out)
    assert got is out
    first = out.cpu().numpy().copy()
    again = ops.mask_head_tail(*args).cpu().numpy()
    assert np.array_equal(first.view(np.int32), again.view(np.int32)), "two calls differ"
    return first

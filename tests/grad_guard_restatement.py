"""fp64 restatement of the gradient guard's record (include/genesis_hip.h, gx_grad_guard), written from the formulas of the header
with numpy, shared by tests/test_grad_guard_cpu.py (which pins the coefficient to torch.nn.utils.clip_grad_norm_) and
tests/test_grad_guard_gpu.py (which holds the kernels to it).  It imports nothing from genesis_amd."""
import math

import numpy as np


def sum_squares(arrays):
    """sum over all elements of (double)g * (double)g, numpy's pairwise fp64 sum per array."""
    return float(sum(np.sum(np.asarray(a).astype(np.float64) ** 2) for a in arrays))


def coef64(norm, max_norm):
    """clamp(max_norm / (norm + 1e-6), max=1) in fp64, a NaN staying a NaN (torch.clamp); max_norm None: 1."""
    if max_norm is None:
        return 1.0
    c = float(max_norm) / (float(norm) + 1e-6)
    return c if (c < 1.0 or c != c) else 1.0


def record_ref(S, gscale, max_norm):
    """-> (norm64, norm32, coef64, coef32) of the header's formulas from S (fp64) and the fp32 value gscale."""
    with np.errstate(all='ignore'):
        norm = float(np.float32(gscale)) * math.sqrt(S) if S == S and S >= 0 else float('nan')
        c = coef64(norm, max_norm)
        return norm, np.float32(norm), c, np.float32(c)


def ulps32(got, want):
    """Distance of two fp32 values in units of the spacing at `want` (0 for equal values, NaNs included)."""
    got, want = np.float32(got), np.float32(want)
    if (got != got and want != want) or got == want:
        return 0.0
    return abs(float(got) - float(want)) / float(np.spacing(np.abs(want)))

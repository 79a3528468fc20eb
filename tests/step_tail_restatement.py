"""fp64 restatements of the tail of a training step, written from the formulas in the kernel comments of
genesis_amd/csrc/gx_optim.hip and gx_latent.hip with plain torch / numpy ops, plus the inputs and the measured float32 bounds
that tests/test_step_tail_cpu.py (which pins all of this to torch.optim and to the recorded GECO series) and
tests/test_step_tail_gpu.py (which holds the kernels to it) share.  It imports nothing from genesis_amd.

Every restatement works in float64 ON THE VALUES its float32 / float64 inputs hold: one step from the state the code under test
started that step from, so the figure compared is the error of ONE update and not what a trajectory makes of it.

How the float32 bounds are formed.  An error relative to |m'| alone has no bound: m' = m + (g - m)(1 - b1) cancels (m = 0.1,
g = -0.9 leaves the rounding of its operands in a result a thousand times smaller -- a group of ONE element shows it at once),
and p' - p = -step_size m' / denom inherits that from m'.  What a float32 evaluation can promise is an error relative to the
magnitudes that ENTER the sum, mag = max(|m'|, |m|, |grad_scale g|); v' is a sum of non-negative terms and has no such
problem.  Each figure is a worst case PER ELEMENT, every element against its own scale, so one wrong element or a wrong
moment shows whatever the rest of the tensor holds:
    m:  max_i |m_i - ref_i| / mag_i                         v:  max_i |v_i - ref_i| / |ref_i|
    p:  max_i (|p_i - ref_i| - ulp32(ref_i))+ / (step_size mag_i / denom_i)
        (the update an uncancelled moment would make; the final rounding of p is the one ulp)
An element whose scale is 0 (a zero gradient on zero moments) must be exact.
A float32 result below the smallest normal number may be flushed (g = 1e-25: g * g = 1e-50), so m and v get 2^-126 on top."""
import math

import numpy as np
import torch

F64 = torch.float64
F32_TINY = float(np.finfo(np.float32).tiny)


def f32(x):
    """The float32-rounded value of x as a Python float: what a `float` parameter of the C ABI receives."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------- optimisers
LR, BETA1, BETA2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-8
RMS_ALPHA, RMS_EPS, SGD_MOMENTUM = 0.99, 1e-8, 0.9
# (n32, n64): one element; one short of / one past a 1024-element block with a single / a 33-element fp64 group; the old test's
# size; one past BOTH grid caps (2048 fp32 blocks, 256 fp64 blocks: every thread takes a strided second trip); more fp64 blocks
# than fp32 blocks
PAIR_SIZES = ((1, 0), (1023, 1), (1025, 33), (10007, 0), (2048 * 1024 + 1027, 256 * 1024 + 5), (5, 3 * 1024))
GRAD_SCALES = (1.0, 0.5, 0.125, f32(1.0 / 3.0))
GUARD = 64

# Worst one-step error of torch.optim.Adam in float32 on the CPU against adam_ref over PAIR_SIZES x GRAD_SCALES, five steps
# each (measured by tests/test_step_tail_cpu.py::test_float32_adam_stays_inside_the_bound, which prints them; the figures
# below are the measured maxima, all three at n32 = 2098179, with the fourth digit rounded up).  The kernels get
# ADAM_GPU_MARGIN times these: a different but legal float32 evaluation order (contraction into fma, the lerp written either
# way) and the rounding of sqrt and division.
ADAM_F32_ERR = {'p': 2.211e-7, 'm': 6.354e-8, 'v': 2.610e-7}
ADAM_GPU_MARGIN = 4.0


def adam_scalars(t, lr=LR, b1=BETA1, b2=BETA2):
    """(step_size, sqrt(bias_correction2)) in double from the step counter t >= 1, as adam_body forms them."""
    bc1 = 1.0 - math.pow(b1, float(t))
    bc2 = 1.0 - math.pow(b2, float(t))
    return lr / bc1, math.sqrt(bc2)


def adam_ref(p, g, m, v, t, grad_scale=1.0, lr=LR, b1=BETA1, b2=BETA2, eps=ADAM_EPS):
    """torch.optim.Adam (no weight decay, no amsgrad), one step: -> (p', m', v') in float64.  grad_scale: the float the ABI
    carries (already float32-rounded), widened; it multiplies the gradient first."""
    p, g, m, v = (x.detach().to(F64) for x in (p, g, m, v))
    step_size, bc2_sqrt = adam_scalars(t, lr, b1, b2)
    gi = g * float(grad_scale)
    m2 = m + (gi - m) * (1.0 - b1)                         # exp_avg.lerp_(grad, 1 - beta1)
    v2 = v * b2 + gi * gi * (1.0 - b2)                     # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    denom = v2.sqrt() / bc2_sqrt + eps
    return p - step_size * (m2 / denom), m2, v2


def adam_scales(p, g, m, v, t, grad_scale=1.0, lr=LR, b1=BETA1, b2=BETA2, eps=ADAM_EPS):
    """The scales of the module docstring for the same step: -> {'p': step_size mag / denom, 'm': mag, 'v': |v'|} (float64)."""
    _, m2, v2 = adam_ref(p, g, m, v, t, grad_scale, lr, b1, b2, eps)
    step_size, bc2_sqrt = adam_scalars(t, lr, b1, b2)
    mag = torch.maximum(torch.maximum(m2.abs(), m.detach().to(F64).abs()), (g.detach().to(F64) * float(grad_scale)).abs())
    return {'p': step_size * mag / (v2.sqrt() / bc2_sqrt + eps), 'm': mag, 'v': v2.abs()}


def rmsprop_ref(p, g, sq, grad_scale=1.0, lr=LR, alpha=RMS_ALPHA, eps=RMS_EPS):
    """torch.optim.RMSprop(lr) (no momentum, not centred), one step: -> (p', square_avg') in float64."""
    p, g, sq = (x.detach().to(F64) for x in (p, g, sq))
    gi = g * float(grad_scale)
    sq2 = sq * alpha + gi * gi * (1.0 - alpha)
    return p - lr * (gi / (sq2.sqrt() + eps)), sq2


def sgd_ref(p, g, buf, grad_scale=1.0, lr=LR, momentum=SGD_MOMENTUM):
    """torch.optim.SGD(lr, momentum), one step from a zero-initialised buffer (0.9 * 0 + g is torch's buf = grad at the first
    step): -> (p', buf') in float64."""
    p, g, buf = (x.detach().to(F64) for x in (p, g, buf))
    buf2 = buf * momentum + g * float(grad_scale)
    return p - lr * buf2, buf2


def optimiser_inputs(n32, n64, steps, seed=0):
    """-> p32 [n32], p64 [n64], grads: `steps` pairs (g32, g64) drawn N(0, (0.1 + it)^2) as test_adam_kernel_matches_torch draws
    them.  Seeded per size: the CPU measurement and the GPU test see the same numbers."""
    gen = torch.Generator().manual_seed(1000 * seed + n32 % 997 + n64 % 991)
    p32 = torch.randn(n32, generator=gen)
    p64 = torch.randn(n64, generator=gen, dtype=F64)
    grads = [(torch.randn(n32, generator=gen) * (0.1 + it), torch.randn(n64, generator=gen, dtype=F64) * (0.1 + it))
             for it in range(steps)]
    return p32, p64, grads


class GuardedBuffers(object):
    """k buffers of n elements of one dtype inside ONE tensor, as the trainer's bucket holds its gradients with a tail behind
    them: GUARD elements before and after every buffer, filled (like the buffers) with seeded normal numbers.  snapshot() /
    guards_unchanged(snapshot) compare the guard elements bit for bit."""

    def __init__(self, n, dtype, k, device, seed=0):
        stride = n + 2 * GUARD
        self.n, self.bits = n, (torch.int32 if dtype == torch.float32 else torch.int64)
        self.whole = torch.randn(k * stride, generator=torch.Generator().manual_seed(seed), dtype=dtype).to(device)
        self.views = [self.whole[i * stride + GUARD:i * stride + GUARD + n] for i in range(k)]
        self.guard = torch.ones(k * stride, dtype=torch.bool, device=device)
        for i in range(k):
            self.guard[i * stride + GUARD:i * stride + GUARD + n] = False
        assert int(self.guard.sum()) == 2 * GUARD * k

    def snapshot(self):
        return self.whole.clone()

    def guards_unchanged(self, snapshot):
        return torch.equal(self.whole.view(self.bits)[self.guard], snapshot.view(self.bits)[self.guard])


def same_bits(a, b):
    """a and b (same floating dtype and shape) hold the same bit patterns."""
    bits = torch.int32 if a.dtype == torch.float32 else torch.int64
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


def ulp32(x):
    """Spacing of float32 at the (float64) values of x."""
    a = np.abs(x.detach().cpu().numpy()).astype(np.float32)
    return torch.from_numpy(np.spacing(a).astype(np.float64))


def _worst(err, scale):
    """max_i err_i / scale_i; where scale_i = 0 the error must be 0."""
    zero = scale == 0
    assert bool((err[zero] == 0).all()), 'an error where the reference scale is 0'
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / scale[~zero]).max())


def adam_f32_ratios(got, ref, scales):
    """got = (p, m, v) in float32, ref = adam_ref's float64 values and scales = adam_scales' for the same inputs.
    -> the three per-element figures of the module docstring (dimensionless)."""
    gp, gm, gv = (x.detach().cpu().to(F64) for x in got)
    rp, rm, rv = (x.detach().cpu() for x in ref)
    if gp.numel() == 0:
        return {'p': 0.0, 'm': 0.0, 'v': 0.0}
    return {'p': _worst(((gp - rp).abs() - ulp32(rp)).clamp_min(0), scales['p']),
            'm': _worst(((gm - rm).abs() - F32_TINY).clamp_min(0), scales['m']),
            'v': _worst(((gv - rv).abs() - F32_TINY).clamp_min(0), scales['v'])}


# ------------------------------------------------------------------------------------------------- GECO
GECO_BETA_MIN, GECO_BETA_MAX = 1e-10, 1e10
# Largest relative distance, over the 300 steps of the recorded series, of a float32 torch transcription of the update from
# geco_ref run in float64 on the same series, for beta and for the moving average, per speedup setting (measured by
# tests/test_step_tail_cpu.py::test_float32_geco_drift_on_the_series; the measured figures, the fourth digit rounded up).  beta is a running product of exponentials: an ulp of expf per step compounds, so the kernel
# gets GECO_GPU_MARGIN times this over the whole curve.
GECO_F32_DRIFT = {'main_su10': {'beta': 2.399e-5, 'ema': 4.576e-7}, 'main_none': {'beta': 7.090e-6, 'ema': 4.576e-7}}
GECO_GPU_MARGIN = 4.0
GECO_SINGLE_RTOL = 1e-6                                # one update: two float32 roundings and one expf


def geco_ref(beta, ema, err, goal, step_size, alpha, speedup, beta_min=GECO_BETA_MIN, beta_max=GECO_BETA_MAX):
    """One GECO update in float64.  ema None: the first call (the moving average becomes the error itself).
    -> (beta', ema')."""
    err = float(err)
    ema = err if ema is None else (1.0 - alpha) * err + alpha * float(ema)
    c = goal - ema
    arg = speedup * step_size * c if (speedup is not None and c > 0) else step_size * c
    try:
        factor = math.exp(arg)
    except OverflowError:
        factor = math.inf
    return min(max(factor * float(beta), beta_min), beta_max), ema


def geco_ref_series(errs, goal, step_size, alpha, speedup, beta_init=1.0, ema=None):
    """geco_ref over a series -> float64 arrays (beta [T], ema [T]) after each update."""
    beta, betas, emas = float(beta_init), [], []
    for e in np.asarray(errs, dtype=np.float64):
        beta, ema = geco_ref(beta, ema, e, goal, step_size, alpha, speedup)
        betas.append(beta); emas.append(ema)
    return np.array(betas), np.array(emas)


def geco_f32_series(errs, goal, step_size, alpha, speedup, beta_init=1.0):
    """The same update transcribed with float32 torch scalars (what a float32 implementation computes) -> float64 arrays."""
    t = lambda x: torch.tensor(x, dtype=torch.float32)        # noqa: E731
    beta, ema, betas, emas = t(beta_init), None, [], []
    for e in np.asarray(errs, dtype=np.float32):
        e = t(float(e))
        ema = e if ema is None else (1.0 - alpha) * e + alpha * ema
        c = goal - ema
        factor = torch.exp(speedup * step_size * c) if (speedup is not None and float(c) > 0) else torch.exp(step_size * c)
        beta = (factor * beta).clamp(t(GECO_BETA_MIN), t(GECO_BETA_MAX))
        betas.append(float(beta)); emas.append(float(ema))
    return np.array(betas), np.array(emas)


def rel_dist(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


# ------------------------------------------------------------------------------------------------- the small launches
def beta_warmup_ref(beta, step, warm_iters):
    """clamp(beta * step / warm_iters, 0, beta) in float64 (Python ints and floats)."""
    return min(max(beta * float(step) / warm_iters, 0.0), beta)


def elbo_ref(err, kl, beta):
    """err [B], kl [R, B] or None, beta: a float -> (out[5] = (err + beta kl, err + kl, err, kl, beta), d_err, d_kl) with err, kl
    the float64 batch means (kl: summed over its rows); d_err = 1 / B, d_kl = beta / B as float32 values."""
    B = err.numel()
    e = float(err.detach().cpu().to(F64).mean())
    k = float(kl.detach().cpu().to(F64).mean(1).sum()) if kl is not None and kl.numel() else 0.0
    out = torch.tensor([e + beta * k, e + k, e, k, beta], dtype=F64)
    return out, np.float32(1.0) / np.float32(B), np.float32(beta) / np.float32(B)


def mse_rmse_ref(x, r):
    """x, r [B, n] -> (mean_b mse_b, mean_b sqrt(mse_b)), mse_b the mean over n of (x - r)^2, in float64."""
    mse = ((x.detach().cpu().to(F64) - r.detach().cpu().to(F64)) ** 2).flatten(1).mean(1)
    return float(mse.mean()), float(mse.sqrt().mean())

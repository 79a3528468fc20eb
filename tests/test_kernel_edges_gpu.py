"""The per-pixel kernels off the beaten path: ragged planes, odd counts, unaligned operands, refusals, dynamic-K masks and
saturated inputs.  Every value is compared with the same operation in plain torch on the CPU in float64 (autograd for the
gradients), at the rtol / atol tests/test_kernels_gpu.py applies to that output; which branch a case reaches is read off the
host dispatch code.

What each case would catch (one-line mistakes in the branch it reaches; argued from the code, never run):

  maskpool_fwd_kernel, scalar loop (HW & 3 != 0)      a loop that starts at threadIdx.x * 4 or strides by 4 * blockDim.x (pixels
                                                      skipped: S and msum too small), `p <= HW` (reads the next plane)
  maskpool_fwd_kernel, C % 4 != 0                     a missing `c0 + c < C` on the load (reads the next image's planes into the
                                                      sums) or on the store (S rows of the next slot overwritten: value check)
  maskpool_bwd_kernel (scalar; dead to the old suite) any indexing slip at all: `p > HW`, gsh indexed [c * K + k], df stride C
  maskpool_bwd_vec_kernel, C % 4 != 0, C < 4          cend = cbeg + cper unclamped (waves 1..3 walk past channel C: df of the next
                                                      image written, a[] polluted), ared summed over waves that never wrote
  gated statistics / apply, scalar path               `i < (HW >> 2)` kept in the scalar loop (HW = 1: nothing summed, rstd = inf),
                                                      a plane offset computed in float4 units
  gated statistics, nchunk that does not divide N     `nb` not clamped to n0 + nc (the short last chunk reads image N: the next
                                                      tensor), `per` rounded down (the last images never counted)
  plane_sum_kernel / bias_act_bwd_kernel tails        HW / 4 iterations in the scalar loop, `i <= HW`
  gx_categorical_kl_fwd, HW % block != 0, 1023/1025   `p < HW` dropped from the stride loop (the next image's masks summed in),
                                                      the 1024-thread kernel reducing only 4 of its 16 waves, a bucket that
                                                      loads q[k] for k >= K from slot k (out of range at K = 5, 9) instead of 0
  mixture / scan / log-softmax / KL-bwd / row_sum     `p > HW` or a missing guard in the last workgroup (writes into the next
                                                      image or tensor: value check of the neighbour, sentinel check where the
                                                      caller owns the destination), err_part indexed without gridDim.y, row_sum
                                                      reading `cols` from the wrong row, its second 64-thread block unguarded
  K = 5 / K = 16 / K = 1                              a K-specialised instantiation wired to the wrong constant (K == 5 -> <7>),
                                                      `k <= K`, an LDS / register array sized KMAX - 1, se = 0 at K = 1
  unaligned operands                                  a 16-byte access chosen on HW & 3 alone
  refusals                                            a GX_CHECK_ARG that stopped refusing (the kernels behind them index with
                                                      the refused quantity: LDS arrays of KMAX, power-of-two masks, grid.y limits)
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

hip = pytest.importorskip('genesis_amd.hip_ops')
from genesis_amd._lib import GenesisHipError  # noqa: E402

DEV = 'cuda'
F64 = torch.float64


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def close(a, b, rtol=1e-4, atol=1e-4, msg=''):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert err <= atol + rtol * ref, '%s max err %.3e (ref max %.3e)' % (msg, err, ref)


def finite(*ts):
    for t in ts:
        if t is not None:
            assert bool(torch.isfinite(t).all()), 'non-finite values'


def to(t):
    return None if t is None else t.to(DEV)


def leaf(t, dtype=F64):
    return t.detach().to(dtype).clone().requires_grad_(True)


def offset_view(t, off):
    """A contiguous device copy of `t` that starts `off` elements into a 16-byte aligned buffer."""
    buf = torch.zeros(t.numel() + 8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * off) % 16
    return v


# ------------------------------------------------------------------------------------------------- references (any dtype)
def maskpool_ref(f, log_m, gS, gms):
    """-> S [B,K,C], msum [B,K], df, dlog_m (f, log_m: leaves)."""
    m = log_m.exp()                                          # [K,B,1,H,W]
    S = (m.unsqueeze(3) * f.unsqueeze(0).unsqueeze(2)).sum((2, 4, 5)).transpose(0, 1)      # [K,B,1,C,H,W] -> [B,K,C]
    ms = m.sum((2, 3, 4)).transpose(0, 1)
    df, dlm = torch.autograd.grad((S * gS.to(S.dtype)).sum() + (ms * gms.to(S.dtype)).sum(), (f, log_m))
    return S, ms, df, dlm


def mixture_ref(x, dec, log_w, K, std1, std2, pixel_bound, g):
    """Genesis.x_loss (no log-sum-exp trick) -> err [B], recon, x_r [K,B,3,H,W], log-weights [K,B,1,H,W], s, (ddec, dlog_w)."""
    B, _, H, W = x.shape
    d = dec.view(K, B, dec.shape[1], H, W)
    mu = torch.sigmoid(d[:, :, :3]) if pixel_bound else d[:, :, :3]
    lm = F.log_softmax(d[:, :, 3:4], 0) if log_w is None else log_w
    std = torch.tensor([std1] + [std2] * (K - 1), dtype=dec.dtype).view(K, 1, 1, 1, 1)
    logn = -((x.unsqueeze(0) - mu) ** 2) / (2 * std ** 2) - std.log() - math.log(math.sqrt(2 * math.pi))
    s = (lm + logn).exp().sum(0)
    err = -(s.log()).sum((1, 2, 3))
    recon = (lm.exp() * mu).sum(0)
    wrt = (dec,) if log_w is None else (dec, log_w)
    grads = torch.autograd.grad((err * g.to(err.dtype)).sum(), wrt)
    return err, recon, mu, lm, s, grads


def scan_ref(l, s0, last):
    T = l.shape[0]
    s = torch.zeros_like(l[0]) if s0 is None else s0
    ms, ss = [], []
    for t in range(T):
        ms.append(s if (last and t == T - 1) else s + F.logsigmoid(l[t]))
        s = s + F.logsigmoid(-l[t])
        ss.append(s)
    return torch.stack(ms), torch.stack(ss)


def kl_ref(lm, lr):
    """MONet.kl_m_loss as torch.distributions writes it (Categorical renormalises the clamped masks)."""
    from torch.distributions.categorical import Categorical
    from torch.distributions.kl import kl_divergence
    K, B = lm.shape[:2]
    floor = torch.tensor(1e-5, dtype=lm.dtype)
    m = torch.max(torch.stack(list(lm), 4).exp(), floor)
    r = torch.max(torch.stack(list(lr), 4).exp(), floor)
    return kl_divergence(Categorical(m.view(-1, K)), Categorical(r.view(-1, K))).view(B, -1).sum(1)


def off_the_clamp(lm):
    """Moves every mask whose exp lies within a relative 2e-3 of the 1e-5 clamp 1 % down (the clamp's gradient is discontinuous)
    and asserts that none is left within 1e-3."""
    lm = lm.clone()
    near = (lm.double().exp() / 1e-5 - 1).abs() < 2e-3
    lm[near] -= 0.01
    assert float((lm.double().exp() / 1e-5 - 1).abs().min()) > 1e-3
    return lm


def dyn_masks(K, B, H, W, nsteps, seed):
    """log-softmax over the first n_b slots of image b, exactly -1e10 in the slots after it (gx_icsbp_fwd_dyn's padding)."""
    lm = torch.empty(K, B, 1, H, W)
    for b, n in enumerate(nsteps):
        lm[:n, b] = F.log_softmax(rnd(n, 1, H, W, seed=seed + b, scale=3.0), 0)
        lm[n:, b] = -1e10
    return lm


def gated_ref(y, bias, norm, prm, eps=1e-5):
    """norm_h(h) * sigmoid(norm_g(g)) with the statistics written out (F.instance_norm refuses a 1 x 1 plane)."""
    h, gt = (y + bias.view(1, -1, 1, 1)).chunk(2, 1)

    def nrm(t, gamma, beta):
        dims = (0, 2, 3) if norm == 'bn' else (2, 3)
        mean = t.mean(dims, keepdim=True)
        var = ((t - mean) ** 2).mean(dims, keepdim=True)
        return (t - mean) / torch.sqrt(var + eps) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)

    if norm:
        h, gt = nrm(h, prm[0], prm[1]), nrm(gt, prm[2], prm[3])
    return h * torch.sigmoid(gt)


def latent_ref(zh, eps, lin, all_w):
    """models/genesisv2_config.py:154-160, genesis_config.py:288-343 -> (z, mu, sigma, log_q, log_p), (dzh, dlin)."""
    from torch.distributions import Normal
    mu, sp = zh.chunk(2, dim=-1)
    sigma = F.softplus(sp + 0.5) + 1e-8
    mu, sigma = mu.transpose(0, 1), sigma.transpose(0, 1)
    z = mu + sigma * eps.to(zh.dtype)
    log_q = Normal(mu, sigma).log_prob(z).sum(2)
    if lin is not None:
        mr, sr = lin.chunk(2, dim=2)
        lp = Normal(torch.tanh(mr), torch.sigmoid(sr + 4.0) + 1e-4).log_prob(z[1:]).sum(2)
        log_p = torch.cat((Normal(0., 1.).log_prob(z[:1]).sum(2), lp), 0)
    else:
        log_p = Normal(0., 1.).log_prob(z).sum(2)
    outs = (z, mu, sigma, log_q, log_p)
    loss = sum((o * w.to(zh.dtype)).sum() for o, w in zip(outs, all_w))
    grads = torch.autograd.grad(loss, (zh,) if lin is None else (zh, lin))
    return outs, grads


# ------------------------------------------------------------------------------------------------- 1. ragged planes, odd counts
def run_maskpool(f, log_m, fd=None, lmd=None, seed=24):
    B, C = f.shape[:2]
    K = log_m.shape[0]
    gS, gms = rnd(B, K, C, seed=seed), rnd(B, K, seed=seed + 1)
    S_ref, ms_ref, df_ref, dlm_ref = maskpool_ref(leaf(f), leaf(log_m), gS, gms)
    fd = to(f) if fd is None else fd
    lmd = to(log_m) if lmd is None else lmd
    Sd, msd = hip.maskpool_fwd(fd, lmd)
    df, dlm = hip.maskpool_bwd(fd, lmd, to(gS), to(gms))
    finite(Sd, msd, df, dlm)
    close(Sd, S_ref, 1e-5, 1e-5, 'S')
    close(msd, ms_ref, 1e-5, 1e-5, 'msum')
    close(df, df_ref, 1e-5, 1e-5, 'df')
    close(dlm, dlm_ref, 1e-5, 1e-5, 'dlog_m')


@pytest.mark.parametrize('B,C,H,W,K', [(2, 6, 5, 7, 3), (1, 5, 17, 17, 5), (2, 10, 8, 8, 16), (1, 3, 8, 8, 1), (2, 4, 1, 1, 2)])
def test_maskpool_ragged(B, C, H, W, K):
    """(2,6,5,7,3):   maskpool_fwd_kernel's scalar loop over p; C % 4 = 2 (last channel block half empty); gx_maskpool_bwd ->
                      maskpool_bwd_kernel (the scalar kernel), one partly filled workgroup.
    (1,5,17,17,5):    HW = 289: scalar loops with a second trip / a second workgroup of 33 pixels (`p >= HW` tail);
                      the K == 5 instantiations of both kernels' dispatch (the scalar backward has none: run-time K).
    (2,10,8,8,16):    (HW & 3) == 0: 16-byte loads; C % 4 != 0 forward, maskpool_bwd_vec_kernel with cper = 3: waves get
                      3 / 3 / 3 / 1 channels; K = KMAX = 16 on the run-time-K instantiation.
    (1,3,8,8,1):      C < 4: cper = 1, wave 3 of the vector backward has cbeg = 3 = C (nothing to do) yet its ared row is summed;
                      K = 1.
    (2,4,1,1,2):      HW = 1: one active thread per workgroup, the block reduction over 255 zeros."""
    f = rnd(B, C, H, W, seed=22).relu()
    log_m = torch.log_softmax(rnd(K, B, 1, H, W, seed=23, scale=3.0), 0)
    run_maskpool(f, log_m)


def run_mixture(form, pixel_bound, x, dec, log_w, K, std1=0.7, std2=0.7, seed=28):
    B = x.shape[0]
    g = rnd(B, seed=seed) + 1.5
    dr = leaf(dec)
    lr = None if log_w is None else leaf(log_w)
    err_ref, recon_ref, xr_ref, lm_ref, s_ref, grads = mixture_ref(x.double(), dr, lr, K, std1, std2, pixel_bound, g)
    assert float(s_ref.detach().min()) > 1e-30          # (the reference has no log-sum-exp trick: stay out of its underflow regime)
    xd, dd = to(x), to(dec)
    if form == 'plain':
        err, recon, x_r, log_m_r = hip.mixture_fwd(xd, dd, K, std2, pixel_bound)
        ddec = hip.mixture_bwd(xd, dd, to(g), K, std2, pixel_bound)
        finite(log_m_r)
        close(log_m_r, lm_ref, 1e-5, 1e-5, 'log_m_r')
    else:
        err, recon, x_r = hip.mixture_w_fwd(xd, dd, to(log_w), K, std1, std2, pixel_bound)
        ddec, dlw = hip.mixture_w_bwd(xd, dd, to(log_w), to(g), K, std1, std2, pixel_bound)
        finite(dlw)
        close(dlw, grads[1], 1e-4, 1e-5, 'dlog_w')
    finite(err, recon, x_r, ddec)
    close(err, err_ref, 2e-6, 1e-3, 'err')
    close(recon, recon_ref, 1e-5, 1e-5, 'recon')
    close(x_r, xr_ref, 1e-5, 1e-5, 'x_r')
    close(ddec, grads[0], 1e-4, 1e-5, 'ddec')


MIX_SHAPES = [(2, 5, 7, 5), (1, 17, 17, 16), (2, 1, 257, 1)]          # B, H, W, K


@pytest.mark.parametrize('pixel_bound', [True, False])
@pytest.mark.parametrize('form', ['plain', 'w4', 'w3'])
@pytest.mark.parametrize('B,H,W,K', MIX_SHAPES + [(65, 1, 257, 5)])
def test_mixture_ragged(form, pixel_bound, B, H, W, K):
    """mixture_kernel<false / true, KT> in its three forms (plain: log-softmax of the logit channel; w4 / w3: external
    log-weights with DC = 4 / DC = 3, the first slot on its own std), both pixel_bound values.
    (2,5,7,5):      HW = 35: one workgroup, 221 threads behind `p < HW` that still take part in block_sum_dd; K == 5 instantiation.
    (1,17,17,16):   HW = 289: `p >= HW` tail in the second workgroup, err_part [B][2]; K = KMAX on the run-time-K instantiation.
    (2,1,257,1):    HW = 257: ONE pixel in the second workgroup; row_sum_kernel over nb = 2 partials; K = 1 (lse = 0).
    (65,1,257,5):   B = 65: row_sum_kernel's second 64-thread block has one row (`r >= rows`)."""
    DC = 3 if form == 'w3' else 4
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(26))
    dec = rnd(K * B, DC, H, W, seed=27, scale=2.0)
    log_w = None if form == 'plain' else torch.log_softmax(rnd(K, B, 1, H, W, seed=73, scale=3.0), 0)
    run_mixture(form, pixel_bound, x, dec, log_w, K, std1=0.7 if form == 'plain' else 0.5)


def run_scan(l, s0, last, gm, gs):
    lr_ = leaf(l)
    s0r = None if s0 is None else leaf(s0)
    ref_m, ref_s = scan_ref(lr_, s0r, last)
    ld, s0d = to(l), to(s0)
    got_m, got_s = hip.sbp_scan_fwd(ld, s0d, last)
    finite(got_m, got_s)
    close(got_m, ref_m, 1e-5, 1e-5, 'log_m')
    close(got_s, ref_s, 1e-5, 1e-5, 'log_s')
    for which in ('m', 's', 'both'):
        a, b = (gm if which != 's' else None), (gs if which != 'm' else None)
        loss = (0 if a is None else (ref_m * a.double()).sum()) + (0 if b is None else (ref_s * b.double()).sum())
        wrt = (lr_,) if s0r is None else (lr_, s0r)
        if last and l.shape[0] == 1 and which == 'm' and s0r is None:
            ref_g = (torch.zeros_like(lr_),)                     # log_m = the initial scope: no path to the logits
        else:
            ref_g = torch.autograd.grad(loss, wrt, retain_graph=True, allow_unused=True)
        g_l, g_s0 = hip.sbp_scan_bwd(ld, to(a), to(b), last, s0 is not None)
        finite(g_l, g_s0)
        close(g_l, torch.zeros_like(lr_) if ref_g[0] is None else ref_g[0], 1e-5, 1e-5, 'g_logits (%s)' % which)
        if s0 is not None:
            close(g_s0, ref_g[1], 1e-5, 1e-5, 'g_log_s0 (%s)' % which)


@pytest.mark.parametrize('with_s0', [False, True])
@pytest.mark.parametrize('last', [False, True])
@pytest.mark.parametrize('T', [1, 2, 17])
@pytest.mark.parametrize('P', [1, 255, 257])
def test_stick_breaking_scan_ragged(P, T, last, with_s0):
    """sbp_scan_fwd_kernel / sbp_scan_bwd_kernel: P = 1 and 255 leave the only workgroup partly filled, P = 257 puts one pixel
    into the second (`p >= P` tail); T = 1 (the last-scope step is also the first), 2, 17; log_s0 null / given; the backward with
    g_log_m only, g_log_s only (null pointers) and both."""
    l = rnd(T, 1, 1, 1, P, seed=80) * 4
    s0 = -rnd(1, 1, 1, P, seed=81).abs() if with_s0 else None
    run_scan(l, s0, last, rnd(T, 1, 1, 1, P, seed=82), rnd(T, 1, 1, 1, P, seed=83))


def run_kl(lm, lr, through_r, seed=86):
    B = lm.shape[1]
    g = rnd(B, seed=seed)
    a, b = leaf(lm), leaf(lr)
    ref = kl_ref(a, b)
    ga, gb = torch.autograd.grad((ref * g.double()).sum(), (a, b), allow_unused=True)
    lmd, lrd = to(lm), to(lr)
    got = hip.categorical_kl_fwd(lmd, lrd)
    g_m, g_r = hip.categorical_kl_bwd(lmd, lrd, to(g), through_r)
    finite(got, g_m, g_r)
    close(got, ref, 2e-5, 1e-4, 'kl_m')
    close(g_m, torch.zeros_like(a) if ga is None else ga, 1e-4, 1e-6, 'g_log_m')
    if through_r:
        close(g_r, torch.zeros_like(b) if gb is None else gb, 1e-4, 1e-6, 'g_log_m_r')
    else:
        assert g_r is None


@pytest.mark.parametrize('through_r', [False, True])
@pytest.mark.parametrize('K', [1, 4, 5, 8, 9, 16, 17])
@pytest.mark.parametrize('H,W', [(5, 7), (33, 31), (25, 41)])
def test_categorical_mask_kl_ragged(H, W, K, through_r):
    """gx_categorical_kl_fwd: HW = 35 and 1023 run 256 threads (one partial stride / three strides and 255 pixels), HW = 1025 runs
    1024 threads with ONE pixel in the second stride; K = 1, 4 | 5, 8 | 9, 16 | 17 are the edges of categorical_kl_fwd_kernel
    <4> / <8> / <16> / <0>.  categorical_kl_bwd_kernel: B * HW is no multiple of 256 (`idx >= B * HW` tail); gradient to log_m
    only (g_log_m_r null) and to both."""
    B = 2
    lm = off_the_clamp(F.log_softmax(rnd(K, B, 1, H, W, seed=84) * 6, 0))
    lr = off_the_clamp(F.log_softmax(rnd(K, B, 1, H, W, seed=85) * 6, 0))
    run_kl(lm, lr, through_r)


def run_logsoftmax(dec, K, seed=6):
    KB, C, H, W = dec.shape
    B = KB // K
    g = rnd(K, B, 1, H, W, seed=seed)
    dr = leaf(dec)
    ref = F.log_softmax(dr[:, C - 1:].reshape(K, B, 1, H, W), dim=0)
    ref_g, = torch.autograd.grad((ref * g.double()).sum(), dr)
    out = hip.logsoftmax_k_fwd(to(dec), K)
    g_dec = hip.logsoftmax_k_bwd(out, to(g), C)
    finite(out, g_dec)
    close(out, ref, 2e-6, 2e-6, 'fwd')
    close(g_dec, ref_g, 2e-6, 2e-6, 'bwd')


@pytest.mark.parametrize('K', [1, 5])
@pytest.mark.parametrize('C', [1, 4])
@pytest.mark.parametrize('H,W', [(5, 7), (1, 257)])
def test_log_softmax_over_the_slots_ragged(H, W, C, K):
    """logsoftmax_k_fwd_kernel / logsoftmax_k_bwd_kernel: B * HW = 70 (one partly filled workgroup) and 514 (two pixels in the
    third: `idx >= B * HW` tail); C = 1: the logit channel is the only one, g_dec has no zero-filled colour planes; K = 1."""
    run_logsoftmax(rnd(K * 2, C, H, W, seed=5, scale=4.0), K)


def run_gated(norm, y, bias, prm, g, yd=None):
    N, C2 = y.shape[:2]
    yr, br = leaf(y), leaf(bias)
    pr = [leaf(t) for t in prm]
    ref = gated_ref(yr, br, norm, pr)
    grads = torch.autograd.grad((ref * g.double()).sum(), [yr, br] + (pr if norm else []))
    args = [to(t) for t in prm] if norm else [None] * 4
    yd = to(y) if yd is None else yd
    out, stats = hip.gated_norm_fwd(yd, to(bias), norm, *args)
    res = hip.gated_norm_bwd(yd, to(bias), norm, *args, stats, to(g))
    finite(out, *res)
    close(out, ref, 1e-5, 1e-5, 'fwd')
    close(res[0], grads[0], 1e-4, 1e-5, 'dy')
    if norm:
        for got, r, nm in zip(res[1:5], grads[2:], ('dgamma_h', 'dbeta_h', 'dgamma_g', 'dbeta_g')):
            close(got, r, 1e-4, 1e-4, nm)
    close(res[5], grads[1], 1e-4, 1e-3 if norm else 1e-4, 'dbias')


def gated_operands(N, C, H, W):
    y = rnd(N, 2 * C, H, W, seed=91, scale=2.0)
    bias = rnd(2 * C, seed=92, scale=0.5)
    prm = [1 + 0.3 * rnd(C, seed=93), 0.2 * rnd(C, seed=94), 1 + 0.3 * rnd(C, seed=95), 0.2 * rnd(C, seed=96)]
    return y, bias, prm, rnd(N, C, H, W, seed=97)


@pytest.mark.parametrize('norm', ['bn', 'in', None])
@pytest.mark.parametrize('N,C,H,W', [(3, 5, 1, 1), (2, 6, 5, 7), (2, 4, 3, 3), (4, 3, 17, 17), (3, 342, 1, 1), (3, 342, 2, 2),
                                     (5, 256, 1, 3)])
def test_gated_norm_ragged(norm, N, C, H, W):
    """gated_stats_partial_kernel, gated_bwd_sums_kernel, gated_apply_kernel, gated_bwd_apply_kernel on their scalar paths
    (HW & 3 != 0):
    (3,5,1,1):     the Sylvester VAE's last gated unit: one value per plane ('in': zero variance, rstd = 1 / sqrt(eps)).
    (2,6,5,7), (2,4,3,3), (4,3,17,17): HW = 35, 9, 289 (a second trip of the 256-thread loops).
    (3,342,1,1), (3,342,2,2): 'bn' and None: nchunks = min(N, 2048 / (2 C)) = 2 does not divide N = 3 -- the smallest N with a
                   short last chunk (per = 2: images {0,1}, {2}); scalar and 16-byte paths.
    (5,256,1,3):   nchunks = 4, per = 2: chunks {0,1}, {2,3}, {4} and an EMPTY fourth chunk (na = 6 > nb = 5)."""
    run_gated(norm, *gated_operands(N, C, H, W))


@pytest.mark.parametrize('act', ['relu', 'elu', None])
@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('C', [1, 5])
@pytest.mark.parametrize('H,W', [(1, 1), (5, 7), (1, 257)])
def test_bias_act_bwd_ragged(H, W, C, N, act):
    """bias_act_bwd_kernel (one workgroup per plane: HW = 1, 35 leave it partly filled, 257 gives thread 0 a second trip) and
    chan_sum_kernel over N = 1 / 3 partials (64 threads).  plane_sum_kernel's scalar path (gx_chan_sums_launch) has no caller
    that accepts such a plane: gx_conv1x1_bwd_act needs H W % 64 == 0 and the conv3x3 callers their own tile sizes, so through
    hip_ops only its 16-byte path runs (test_conv1x1_bwd_destinations covers an odd channel count on it)."""
    pre = rnd(N, C, H, W, seed=5)
    out = F.relu(pre) if act == 'relu' else (F.elu(pre) if act == 'elu' else pre)
    g = rnd(N, C, H, W, seed=6)
    pr = leaf(pre)
    o64 = F.relu(pr) if act == 'relu' else (F.elu(pr) if act == 'elu' else pr * 1.0)
    ref, = torch.autograd.grad((o64 * g.double()).sum(), pr)
    dy, db = hip.bias_act_bwd(to(out), to(g), act)
    finite(dy, db)
    close(dy, ref, 1e-5, 1e-5, 'dy')
    close(db, ref.sum((0, 2, 3)), 1e-4, 1e-4, 'dbias')


def run_latent(zh, eps, lin, tol=None):
    """PosteriorFn + PriorLogPFn against latent_ref; tol: {name: (rtol, atol)} overrides of test_kernels_gpu's figures."""
    from genesis_amd import functions as fn
    tol = tol or {}
    B, K, D2 = zh.shape
    D = D2 // 2
    w = [rnd(K, B, D, seed=4), rnd(K, B, D, seed=5), rnd(K, B, D, seed=6), rnd(K, B, seed=7), rnd(K, B, seed=8)]
    outs_ref, grads_ref = latent_ref(leaf(zh), eps, None if lin is None else leaf(lin), w)
    zg = to(zh).requires_grad_()
    lg = to(lin).requires_grad_() if lin is not None else None
    z, mu, sigma, log_q = fn.PosteriorFn.apply(zg, to(eps))
    log_p = fn.PriorLogPFn.apply(z, lg)
    kl = fn.PriorLogPFn.apply(z.detach(), None if lg is None else lg.detach(), log_q.detach())
    outs = (z, mu, sigma, log_q, log_p)
    sum((o * to(wi)).sum() for o, wi in zip(outs, w)).backward()
    finite(kl, zg.grad, None if lg is None else lg.grad, *outs)
    close(kl, outs_ref[3] - outs_ref[4], *tol.get('kl', (1e-5, 1e-4)), msg='kl = log_q - log_p')
    for o, r, name in zip(outs, outs_ref, ('z', 'mu', 'sigma', 'log_q', 'log_p')):
        close(o, r, *tol.get(name, (1e-5, 1e-5)), msg=name)
    close(zg.grad, grads_ref[0], *tol.get('dzh', (1e-4, 1e-5)), msg='dzh')
    if lin is not None:
        close(lg.grad, grads_ref[1], *tol.get('dlin', (1e-4, 1e-5)), msg='dlin')


@pytest.mark.parametrize('K', [1, 2])
@pytest.mark.parametrize('D', [1, 3, 65])
def test_latent_nodes_short_rows(D, K):
    """posterior_fwd / _bwd, prior_logp_fwd / _bwd kernels (one wave per (slot, image) row, `d = lane; d < D; d += 64`): D = 1 and
    3 leave 63 / 61 lanes of the wave reduction idle, D = 65 gives lane 0 a second trip; B = 1, K = 1 (one row: three idle waves
    in the workgroup, no conditional prior) and K = 2 (a lin of ONE row)."""
    B = 1
    zh = rnd(B, K, 2 * D, seed=1, scale=2.0)
    eps = torch.randn(K, B, D, generator=torch.Generator().manual_seed(2))
    lin = rnd(K - 1, B, 2 * D, seed=3, scale=2.0) if K > 1 else None
    run_latent(zh, eps, lin)


@pytest.mark.parametrize('B,R', [(1, 1), (1, 65), (65, 1), (1, 0)])
def test_elbo_one_image(B, R):
    """gx_elbo_fwd / gx_elbo_bwd at B = 1 (the mean over one image) and R / B one past a wave (65); R = 0: no KL term."""
    from genesis_amd import functions as fn
    err = (rnd(B, seed=1) * 100 + 500).to(DEV).requires_grad_()
    kl = (rnd(R, B, seed=2) * 10).to(DEV).requires_grad_() if R else None
    beta = torch.tensor([0.37], device=DEV)
    tail = torch.zeros(2, device=DEV)
    loss, out = fn.ElboFn.apply(err, kl, beta, tail)
    e = err.detach().cpu().double().mean()
    k = kl.detach().cpu().double().mean(1).sum() if R else torch.zeros((), dtype=F64)
    finite(loss, out, tail)
    close(out, torch.stack((e + 0.37 * k, e + k, e, k, torch.tensor(0.37, dtype=F64))), rtol=1e-6, atol=1e-6)
    close(tail, torch.stack((e, k)), rtol=1e-6, atol=1e-6)
    assert float(loss.detach()) == float(out[0])
    loss.backward()
    close(err.grad, torch.full((B,), 1.0 / B), rtol=1e-6, atol=0)
    if R:
        close(kl.grad, torch.full((R, B), 0.37 / B), rtol=1e-6, atol=0)


@pytest.mark.parametrize('R,C', [(1, 65), (65, 1), (1, 1), (65, 65), (1, 3)])
def test_pooled_head_one_row(R, C):
    """gx_pooled_head_fwd / _bwd with one row (B = 1, K = 1), one channel (LayerNorm of a single value: y = beta, no gradient to
    the row) and 65 = one past a wave in either direction."""
    from genesis_amd import functions as fn
    lin, msum = rnd(R, C, seed=1, scale=30.0), rnd(R, seed=2).abs() * 50 + 0.01
    fb, ga, be, g = rnd(C, seed=3), rnd(C, seed=4) + 1.5, rnd(C, seed=5), rnd(R, C, seed=6)
    ref = [leaf(t) for t in (lin, msum, fb, ga, be)]
    obj = (ref[0] + ref[1].unsqueeze(-1) * ref[2]) / (ref[1].unsqueeze(-1) + 1e-5)
    yr = F.layer_norm(obj, (C,), ref[3], ref[4], 1e-5)
    (yr * g.double()).sum().backward()
    dev = [t.to(DEV).requires_grad_() for t in (lin, msum, fb, ga, be)]
    y = fn.PooledHeadFn.apply(*dev, 1e-5)
    close(y, yr, rtol=1e-5, atol=1e-5, msg='y')
    (y * g.to(DEV)).sum().backward()
    for a, b, n in zip(dev, ref, ('dlin', 'dmsum', 'dfbias', 'dgamma', 'dbeta')):
        finite(a.grad)
        # C = 1: dlin is analytically zero and what is left is the rounding of x - mean times rstd = 1 / sqrt(eps) = 316; fp32
        # torch's own layer_norm backward is 1.373e-5 from fp64 at (65, 1), past the 1e-5 of test_pooled_head: x 4 of that
        atol = 4 * 1.373e-5 if (C == 1 and n == 'dlin') else 1e-5
        close(a.grad, b.grad, rtol=1e-4, atol=atol, msg=n)


# ------------------------------------------------------------------------------------------------- 2. out-of-range writes
SENTINEL = 0x7FC5A5A5          # a quiet NaN with a payload no kernel produces


class Arena(object):
    """One flat fp32 buffer pre-filled with SENTINEL; take(n) hands out contiguous slices `gap` elements apart; untouched()
    asserts that every element outside the slices still holds the sentinel's bits."""

    def __init__(self, total, gap=5, start=3):
        self.buf = torch.full((total,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
        self.pos, self.gap, self.taken = start, gap, []

    def take(self, *shape):
        n = int(torch.Size(shape).numel())
        assert self.pos + n + self.gap <= self.buf.numel()
        v = self.buf[self.pos:self.pos + n].view(shape)
        self.taken.append((self.pos, self.pos + n))
        self.pos += n + self.gap
        return v

    def untouched(self, inside=None):
        """inside: optional bool mask [total] of elements the call may write (default: the slices handed out)."""
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEV)
        if inside is None:
            for a, b in self.taken:
                keep[a:b] = False
        else:
            keep &= ~inside
        bits = self.buf.view(torch.int32)
        assert bool((bits[keep] == SENTINEL).all()), 'a kernel wrote outside its destination'
        if inside is None:
            for a, b in self.taken:
                assert bool((bits[a:b] != SENTINEL).all()), 'a destination element was never written'


@pytest.mark.parametrize('norm', ['bn', 'in', None])
@pytest.mark.parametrize('N,C,H,W', [(2, 6, 5, 7), (2, 4, 4, 4)])
def test_gated_norm_bwd_destinations(norm, N, C, H, W):
    """gated_norm_bwd(out=): the five parameter-gradient destinations as slices of one sentinel-filled buffer, at a ragged (HW = 35)
    and an aligned (HW = 16) plane: nothing outside them changes, and they hold what the call without `out` returns."""
    y, bias, prm, g = gated_operands(N, C, H, W)
    args = [to(t) for t in prm] if norm else [None] * 4
    yd, bd, gd = to(y), to(bias), to(g)
    _, stats = hip.gated_norm_fwd(yd, bd, norm, *args)
    plain = hip.gated_norm_bwd(yd, bd, norm, *args, stats, gd)
    ar = Arena(8 * C + 64)
    dst = ([ar.take(C) for _ in range(4)] if norm else [None] * 4) + [ar.take(2 * C)]
    res = hip.gated_norm_bwd(yd, bd, norm, *args, stats, gd, out=tuple(dst))
    ar.untouched()
    assert torch.equal(res[0], plain[0])
    for d, r, p in zip(dst, res[1:], plain[1:]):
        if d is not None:
            assert r.data_ptr() == d.data_ptr() and torch.equal(d, p)


@pytest.mark.parametrize('N,Cin,Cout,H,W,gated', [(2, 5, 3, 8, 8, True), (2, 16, 8, 16, 16, False)])
def test_conv1x1_bwd_destinations(N, Cin, Cout, H, W, gated):
    """conv1x1_bwd(out=(dw, db, dgate)) into slices of one sentinel-filled buffer.  (2,5,3,8,8): the smallest plane the entry point
    takes (H W = 64: conv1x1_wgrad_mfma_kernel, one chunk per image) with odd channel counts and a gate (conv1x1_finalize_kernel);
    (2,16,8,16,16): H W = 256, conv1x1_wgrad_lds_kernel, col_sum2_kernel writes dw / db itself.  Values against fp64 autograd; the
    first shape also runs conv1x1_bwd_act, whose bias gradient comes from plane_sum_kernel's 16-byte path over Cin = 5 planes."""
    x, w, b = rnd(N, Cin, H, W, seed=29), rnd(Cout, Cin, 1, 1, seed=30, scale=0.2), rnd(Cout, seed=31)
    gate = torch.tensor(0.35) if gated else None
    dy = rnd(N, Cout, H, W, seed=33)
    xr, wr, br = leaf(x), leaf(w), leaf(b)
    gr = leaf(gate) if gated else None
    y_ref = F.conv2d(xr, wr, br)
    y_ref = gr * y_ref if gated else y_ref
    grads = torch.autograd.grad((y_ref * dy.double()).sum(), [xr, wr, br] + ([gr] if gated else []))
    ar = Arena(Cout * Cin + Cout + 64)
    dst = (ar.take(Cout, Cin), ar.take(Cout), ar.take(1).view(()) if gated else None)
    dx, dw, db, dgate = hip.conv1x1_bwd(to(x), to(dy), to(w), to(b), to(gate), out=dst)
    ar.untouched()
    close(dx, grads[0], 1e-5, 1e-5, 'dx')
    close(dst[0], grads[1].view(Cout, Cin), 1e-4, 1e-4, 'dw')
    close(dst[1], grads[2], 1e-4, 1e-4, 'db')
    if gated:
        close(dst[2], grads[3], 1e-4, 1e-3, 'dgate')
        xa = F.relu(x)
        dxa, _, _, dbx = hip.conv1x1_bwd_act(to(xa), to(dy), to(w), to(b), 'relu')
        close(dbx, dxa.double().sum((0, 2, 3)), rtol=1e-6, atol=1e-6, msg='dbx')


def gn_operands(N, C, H, W):
    y = rnd(N, C, H, W, seed=8, scale=2.0) + 0.3
    return y, 1 + 0.3 * rnd(C, seed=9), 0.2 * rnd(C, seed=10), rnd(N, C, H, W, seed=11)


@pytest.mark.parametrize('N,C,H,W,groups', [(3, 6, 2, 2, 3), (2, 16, 8, 8, 8)])
def test_gn_relu_bwd_destinations(N, C, H, W, groups):
    """gn_relu_bwd(out=(dgamma, dbeta, dbias)) into slices of one sentinel-filled buffer: GroupNorm's smallest plane (H = W = 2:
    the scalar loops, W % 4 != 0) and an aligned one; values against fp64 autograd."""
    y, gamma, beta, g = gn_operands(N, C, H, W)
    yr, gr, br = leaf(y), leaf(gamma), leaf(beta)
    ref = F.relu(F.group_norm(yr, groups, gr, br, 1e-5))
    grads = torch.autograd.grad((ref * g.double()).sum(), (yr, gr, br))
    yd, gd, bd = to(y), to(gamma), to(beta)
    out = torch.empty(N, C, H, W, device=DEV)
    mean, rstd = hip.gn_relu_fwd(yd, gd, bd, groups, 1e-5, (out, 0, 0))
    close(out, ref, 1e-5, 1e-5, 'fwd')
    ar = Arena(3 * C + 64)
    dst = (ar.take(C), ar.take(C), ar.take(C))
    dy, _, _, _ = hip.gn_relu_bwd(yd, gd, bd, mean, rstd, groups, (to(g), 0, 0), None, True, out=dst)
    ar.untouched()
    close(dy, grads[0], 1e-4, 1e-5, 'dy')
    close(dst[0], grads[1], 1e-4, 1e-4, 'dgamma')
    close(dst[1], grads[2], 1e-4, 1e-4, 'dbeta')
    close(dst[2], grads[0].sum((0, 2, 3)), 1e-4, 1e-4, 'dbias')


@pytest.mark.parametrize('N,C,H,W,groups,mode1', [(3, 6, 2, 2, 3, 1), (2, 16, 8, 8, 8, 2)])
def test_gn_relu_fwd_destination_views(N, C, H, W, groups, mode1):
    """gn_relu_fwd's dst0 / dst1 views inside one sentinel-filled buffer: dst0 is the channel slice [2, 2 + C) of a concat buffer
    of C + 3 channels, dst1 the 2 x up-sampled (H = W = 2, the smallest plane: scalar stores) or 2 x down-sampled (8 x 8: 16-byte
    stores) copy in channels [1, 1 + C) of a second one.  The other channels of both buffers and everything around them keep the
    sentinel.  (The views start 16 bytes apart from an aligned base: the GroupNorm kernels pick their 16-byte stores on W % 4
    alone, see the summary of the change that added this file.)"""
    y, gamma, beta, _ = gn_operands(N, C, H, W)
    ref = F.relu(F.group_norm(y.double(), groups, gamma.double(), beta.double(), 1e-5))
    H1, W1 = (2 * H, 2 * W) if mode1 == 1 else (H // 2, W // 2)
    ref1 = F.interpolate(ref, scale_factor=2.0 if mode1 == 1 else 0.5, mode='nearest')
    ar = Arena(N * (C + 3) * H * W + N * (C + 2) * H1 * W1 + 64, gap=8, start=4)
    cat, other = ar.take(N, C + 3, H, W), ar.take(N, C + 2, H1, W1)
    hip.gn_relu_fwd(to(y), to(gamma), to(beta), groups, 1e-5, (cat, 2, 0), (other, 1, mode1))
    inside = torch.zeros(ar.buf.numel(), dtype=torch.bool, device=DEV)
    (a0, b0), (a1, b1) = ar.taken
    inside[a0:b0].view(N, C + 3, H, W)[:, 2:2 + C] = True
    inside[a1:b1].view(N, C + 2, H1, W1)[:, 1:1 + C] = True
    ar.untouched(inside)
    close(cat[:, 2:2 + C], ref, 1e-5, 1e-5, 'dst0')
    close(other[:, 1:1 + C], ref1, 1e-5, 1e-5, 'dst1')


@pytest.mark.parametrize('R,C', [(5, 7), (64, 64)])
def test_pooled_head_bwd_destinations(R, C):
    """pooled_head_bwd(out=(dfbias, dgamma, dbeta)) into slices of one sentinel-filled buffer, ragged (5 rows of 7) and aligned."""
    lin, msum = rnd(R, C, seed=1, scale=30.0), rnd(R, seed=2).abs() * 50 + 0.01
    fb, ga, be, g = rnd(C, seed=3), rnd(C, seed=4) + 1.5, rnd(C, seed=5), rnd(R, C, seed=6)
    ref = [leaf(t) for t in (lin, msum, fb, ga, be)]
    obj = (ref[0] + ref[1].unsqueeze(-1) * ref[2]) / (ref[1].unsqueeze(-1) + 1e-5)
    (F.layer_norm(obj, (C,), ref[3], ref[4], 1e-5) * g.double()).sum().backward()
    d = [to(t) for t in (lin, msum, fb, ga, be)]
    _, stats = hip.pooled_head_fwd(*d, 1e-5)
    ar = Arena(3 * C + 64)
    dst = (ar.take(C), ar.take(C), ar.take(C))
    dlin, dmsum, _, _, _ = hip.pooled_head_bwd(d[0], d[1], d[2], d[3], stats, to(g), out=dst)
    ar.untouched()
    for got, r, n in zip((dlin, dmsum) + dst, ref, ('dlin', 'dmsum', 'dfbias', 'dgamma', 'dbeta')):
        close(got, r.grad, rtol=1e-4, atol=1e-5, msg=n)


# ------------------------------------------------------------------------------------------------- 3. unaligned operands
@pytest.mark.parametrize('off', [1, 2, 3])
@pytest.mark.parametrize('which', ['f', 'log_m', 'both'])
def test_maskpool_unaligned(which, off):
    """f and / or log_m as contiguous slices `off` elements into an aligned buffer, H W % 4 == 0: gx_vec4_ok sends the forward to
    maskpool_fwd_kernel's scalar loop and the backward to maskpool_bwd_kernel instead of 16-byte accesses at a 4-byte aligned
    address."""
    B, C, H, W, K = 2, 6, 4, 6, 3
    f = rnd(B, C, H, W, seed=22).relu()
    log_m = torch.log_softmax(rnd(K, B, 1, H, W, seed=23, scale=3.0), 0)
    fd = offset_view(f, off) if which != 'log_m' else to(f)
    lmd = offset_view(log_m, off) if which != 'f' else to(log_m)
    run_maskpool(f, log_m, fd, lmd)


@pytest.mark.parametrize('off', [1, 2, 3])
@pytest.mark.parametrize('norm', ['bn', 'in', None])
def test_gated_norm_unaligned(norm, off):
    """y as a contiguous slice `off` elements into an aligned buffer, H W % 4 == 0: gated_stats_partial_kernel and
    gated_bwd_sums_kernel follow the apply kernels onto the scalar path (one predicate, gx_vec4_ok)."""
    y, bias, prm, g = gated_operands(3, 5, 2, 6)
    run_gated(norm, y, bias, prm, g, offset_view(y, off))


# ------------------------------------------------------------------------------------------------- 4. refusals
def _z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def _icsbp(B, C, H, W, K):
    return lambda: hip.icsbp_fwd(_z(B, C, H, W), _z((), dtype=F64), _z(B, 1, H, W), K)


def _icsbp_bwd(B, C, H, W, K):
    return lambda: hip.icsbp_bwd(_z(B, C, H, W), _z((), dtype=F64), _z(max(K - 1, 0), B, C),
                                 _z(max(K - 1, 0), B, dtype=torch.int64), _z(K, B, 1, H, W))


def _icsbp_raw(entry, kernel_type=0, min_mass=None, nsteps=True, short=0):
    """The IC-SBP C entry points with explicit pointers (B = 2, C = 8, 8 x 8, K = 3; zeros of the right sizes): what the wrappers
    cannot express -- a kernel number outside 0..2, min_mass = 0 or a null nsteps on the dynamic-K entries, a workspace `short`
    bytes below gx_icsbp_bwd_ws_bytes.  Every one is refused by a GX_CHECK_ARG ahead of the first launch."""
    import ctypes
    from genesis_amd import _lib
    B, C, H, W, K = 2, 8, 8, 8, 3

    def call():
        p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
        colour, ls, rand, g = _z(B, C, H, W), _z((), dtype=F64), _z(B, 1, H, W), _z(K, B, 1, H, W)
        log_m, log_s, seeds, idx = _z(K, B, 1, H, W), _z(K, B, 1, H, W), _z(K - 1, B, C), _z(K - 1, B, dtype=torch.int64)
        ns = p(_z(B, dtype=torch.int32)) if nsteps else None
        if entry.startswith('gx_icsbp_fwd'):
            head = (p(colour), p(ls), p(rand), None, B, C, H, W, K, kernel_type)
            outs = (p(log_m), p(log_s), p(seeds), p(idx))
            if entry == 'gx_icsbp_fwd_dyn':
                _lib.call(entry, *head, float(min_mass), *outs, ns, hip._stream())
            else:
                _lib.call(entry, *head, *outs, hip._stream())
            return
        nb = _lib.query('gx_icsbp_bwd_ws_bytes', B, H, W, K)
        ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
        head = (p(colour), p(ls), p(seeds), p(idx), p(g))
        tail = (B, C, H, W, K, kernel_type, p(_z(B, C, H, W)), p(_z((), dtype=F64)), p(ws), nb - short, hip._stream())
        if entry == 'gx_icsbp_bwd_dyn':
            _lib.call(entry, *head, ns, *tail)
        else:
            _lib.call(entry, *head, *tail)
    return call


def _mix(K, std=0.7, B=2, S=4):
    return lambda: hip.mixture_fwd(_z(B, 3, S, S), _z(K * B, 4, S, S), K, std)


def _mix_bwd(K, std=0.7, B=2, S=4):
    return lambda: hip.mixture_bwd(_z(B, 3, S, S), _z(K * B, 4, S, S), _z(B), K, std)


def _mixw(K, std=0.7, B=2, S=4):
    return lambda: hip.mixture_w_fwd(_z(B, 3, S, S), _z(K * B, 3, S, S), _z(K, B, 1, S, S), K, std, std)


def _mixw_bwd(K, std=0.7, B=2, S=4):
    return lambda: hip.mixture_w_bwd(_z(B, 3, S, S), _z(K * B, 3, S, S), _z(K, B, 1, S, S), _z(B), K, std, std)


def _gn_fwd(H, W, C=8, groups=4):
    return lambda: hip.gn_relu_fwd(_z(2, C, H, W), _z(C), _z(C), groups, 1e-5, (_z(2, C, H, W), 0, 0))


def _gn_bwd(H, W, C=8, groups=4):
    return lambda: hip.gn_relu_bwd(_z(2, C, H, W), _z(C), _z(C), _z(2 * groups), _z(2 * groups), groups, (_z(2, C, H, W), 0, 0))


def _lstm(H):
    return lambda: hip.lstm_step_fwd(_z(2, 4 * H), None, None, _z(4 * H, H), _z(4 * H), _z(2, 4 * H), _z(2, H), _z(2, H))


REFUSALS = {      # id -> (call, the C entry point its message must name)
    'maskpool_fwd K=17': (lambda: hip.maskpool_fwd(_z(2, 4, 4, 4), _z(17, 2, 1, 4, 4)), 'gx_maskpool_fwd'),
    'maskpool_bwd K=17': (lambda: hip.maskpool_bwd(_z(2, 4, 4, 4), _z(17, 2, 1, 4, 4), _z(2, 17, 4), _z(2, 17)), 'gx_maskpool_bwd'),
    'mixture_fwd K=17': (_mix(17), 'gx_mixture_fwd'),
    'mixture_bwd K=17': (_mix_bwd(17), 'gx_mixture_bwd'),
    'mixture_w_fwd K=17': (_mixw(17), 'gx_mixture_fwd'),
    'mixture_w_bwd K=17': (_mixw_bwd(17), 'gx_mixture_bwd'),
    'mixture_fwd pixel_std=0': (_mix(3, 0.0), 'gx_mixture_fwd'),
    'mixture_bwd pixel_std=0': (_mix_bwd(3, 0.0), 'gx_mixture_bwd'),
    'mixture_w_fwd pixel_std=0': (_mixw(3, 0.0), 'gx_mixture_fwd'),
    'mixture_w_bwd pixel_std=0': (_mixw_bwd(3, 0.0), 'gx_mixture_bwd'),
    'icsbp_fwd K=18': (_icsbp(2, 8, 8, 8, 18), 'gx_icsbp_fwd'),
    'icsbp_fwd C=9': (_icsbp(2, 9, 8, 8, 3), 'gx_icsbp_fwd'),
    'icsbp_fwd HW=32': (_icsbp(2, 8, 4, 8, 3), 'gx_icsbp_fwd'),
    'icsbp_fwd HW=96': (_icsbp(2, 8, 8, 12, 3), 'gx_icsbp_fwd'),
    'icsbp_fwd HW=32768': (_icsbp(1, 8, 128, 256, 3), 'gx_icsbp_fwd'),
    'icsbp_bwd K=18': (_icsbp_bwd(2, 8, 8, 8, 18), 'gx_icsbp_bwd'),
    'icsbp_bwd C=9': (_icsbp_bwd(2, 9, 8, 8, 3), 'gx_icsbp_bwd'),
    'icsbp_bwd HW=96': (_icsbp_bwd(2, 8, 8, 12, 3), 'gx_icsbp_bwd'),
    'icsbp_fwd_dyn min_mass=0': (_icsbp_raw('gx_icsbp_fwd_dyn', min_mass=0.0), 'gx_icsbp_fwd_dyn'),
    'icsbp_fwd_dyn nsteps=null': (_icsbp_raw('gx_icsbp_fwd_dyn', min_mass=3.0, nsteps=False), 'gx_icsbp_fwd_dyn'),
    'icsbp_bwd_dyn nsteps=null': (_icsbp_raw('gx_icsbp_bwd_dyn', nsteps=False), 'gx_icsbp_bwd_dyn'),
    'icsbp_bwd workspace one byte short': (_icsbp_raw('gx_icsbp_bwd', short=1), 'gx_icsbp_bwd'),
    'icsbp_fwd kernel_type=3': (_icsbp_raw('gx_icsbp_fwd', kernel_type=3), 'gx_icsbp_fwd'),
    'icsbp_bwd kernel_type=3': (_icsbp_raw('gx_icsbp_bwd', kernel_type=3), 'gx_icsbp_bwd'),
    'gn_relu_fwd W=6': (_gn_fwd(8, 6), 'gx_gn_relu_fwd'),
    'gn_relu_fwd H=1': (_gn_fwd(1, 8), 'gx_gn_relu_fwd'),
    'gn_relu_fwd C%groups': (_gn_fwd(8, 8, C=6, groups=4), 'gx_gn_relu_fwd'),
    'gn_relu_fwd view slice': (lambda: hip.gn_relu_fwd(_z(2, 8, 4, 4), _z(8), _z(8), 4, 1e-5, (_z(2, 9, 4, 4), 2, 0)), 'gx_gn_relu_fwd'),
    'gn_relu_bwd W=6': (_gn_bwd(8, 6), 'gx_gn_relu_bwd'),
    'gn_relu_bwd H=1': (_gn_bwd(1, 8), 'gx_gn_relu_bwd'),
    'gn_relu_bwd C%groups': (_gn_bwd(8, 8, C=6, groups=4), 'gx_gn_relu_bwd'),
    'conv1x1_fwd Cout=9': (lambda: hip.conv1x1_fwd(_z(2, 4, 8, 8), _z(9, 4, 1, 1), _z(9)), 'gx_conv1x1_fwd'),
    'conv1x1_bwd HW=35': (lambda: hip.conv1x1_bwd(_z(2, 4, 5, 7), _z(2, 3, 5, 7), _z(3, 4, 1, 1), _z(3)), 'gx_conv1x1_bwd'),
    'conv1x1_bwd Cin=129': (lambda: hip.conv1x1_bwd(_z(1, 129, 8, 8), _z(1, 3, 8, 8), _z(3, 129, 1, 1), _z(3)), 'gx_conv1x1_bwd'),
    'conv1x1_bwd_act HW=35': (lambda: hip.conv1x1_bwd_act(_z(2, 4, 5, 7), _z(2, 3, 5, 7), _z(3, 4, 1, 1), _z(3), 'relu'), 'gx_conv1x1_bwd'),
    'conv1x1_bwd_act act=None': (lambda: hip.conv1x1_bwd_act(_z(2, 4, 8, 8), _z(2, 3, 8, 8), _z(3, 4, 1, 1), _z(3), None), 'gx_conv1x1_bwd_act'),
    'conv1x1_gn_fwd HW=9': (lambda: hip.conv1x1_gn_fwd(_z(2, 8, 3, 3), _z(8), _z(8), _z(8), _z(8), 4, _z(3, 8), _z(3)), 'gx_conv1x1_gn_fwd'),
    'conv1x1_gn_fwd Cout=9': (lambda: hip.conv1x1_gn_fwd(_z(2, 8, 4, 4), _z(8), _z(8), _z(8), _z(8), 4, _z(9, 8), _z(9)), 'gx_conv1x1_gn_fwd'),
    'conv1x1_gn_fwd Cin%groups': (lambda: hip.conv1x1_gn_fwd(_z(2, 6, 4, 4), _z(8), _z(8), _z(6), _z(6), 4, _z(3, 6), _z(3)), 'gx_conv1x1_gn_fwd'),
    'conv1x1_gn_wgrad HW=64': (lambda: hip.conv1x1_gn_wgrad(_z(2, 8, 8, 8), _z(8), _z(8), _z(8), _z(8), 4, _z(2, 3, 8, 8)), 'gx_conv1x1_gn_wgrad'),
    'conv1x1_gn_wgrad Cin=65': (lambda: hip.conv1x1_gn_wgrad(_z(1, 65, 16, 16), _z(5), _z(5), _z(65), _z(65), 5, _z(1, 3, 16, 16)),
                                'gx_conv1x1_gn_wgrad'),
    'gn_relu_bwd_proj Cout=9': (lambda: hip.gn_relu_bwd_proj(_z(2, 8, 4, 4), _z(8), _z(8), _z(8), _z(8), 4, _z(2, 9, 4, 4), _z(9, 8)),
                                'gx_gn_relu_bwd_proj'),
    'gn_relu_bwd_proj W=2': (lambda: hip.gn_relu_bwd_proj(_z(2, 8, 2, 2), _z(8), _z(8), _z(8), _z(8), 4, _z(2, 3, 2, 2), _z(3, 8)),
                             'gx_gn_relu_bwd_proj'),
    'mask_image_stack HW=35': (lambda: hip.mask_image_stack(_z(2, 2, 1, 5, 7), _z(2, 3, 5, 7)), 'gx_mask_image_stack'),
    'mask_image_stack planes=65536': (lambda: hip.mask_image_stack(_z(16, 1024, 1, 2, 2), _z(1024, 3, 2, 2)), 'gx_mask_image_stack'),
    'matmul_nn_fwd N=6': (lambda: hip.matmul_nn_fwd(_z(2, 4), _z(4, 6)), 'gx_matmul_nn_fwd'),
    'matmul_nn_bwd N=6': (lambda: hip.matmul_nn_bwd(_z(2, 4), _z(4, 6), _z(2, 6)), 'gx_matmul_nn_bwd'),
    'lstm_step_fwd H=24': (_lstm(24), 'gx_lstm_step_fwd'),
    'lstm_step_bwd H=24': (lambda: hip.lstm_step_bwd(_z(2, 24), None, _z(96, 24), _z(2, 96), _z(2, 24), None, None, _z(2, 96), _z(2, 24)),
                           'gx_lstm_step_bwd'),
    'bcast_conv3x3_fwd d=6': (lambda: hip.bcast_conv3x3_fwd(_z(2, 3), _z(4, 5, 3, 3), _z(4), _z(6), _z(6), 'relu'), 'gx_bcast_conv3x3_fwd'),
    'bcast_conv3x3_bwd d=6': (lambda: hip.bcast_conv3x3_bwd(_z(2, 4, 6, 6), _z(2, 4, 6, 6), _z(2, 3), _z(4, 5, 3, 3), _z(6), _z(6), 'relu'),
                              'gx_bcast_conv3x3_bwd'),
}


@pytest.mark.parametrize('case', sorted(REFUSALS))
def test_refused_shapes(case):
    """Every shape the C side refuses is refused by its GX_CHECK_ARG -- GX_EINVAL (-1), before any launch (each check stands ahead
    of the first hipLaunchKernelGGL of its entry point; a failed launch would be GX_ELAUNCH, -2) -- with a message that names the
    entry point.  The operands are zeros of the refused shape: had a refusal gone, nothing here would be out of range for the
    allocation, only wrong."""
    call, entry = REFUSALS[case]
    with pytest.raises(GenesisHipError) as e:
        call()
    msg = str(e.value)
    assert 'failed (-1)' in msg and (entry + ':') in msg.split('failed (-1)', 1)[1], msg


def _short_ws(monkeypatch):
    from genesis_amd import _lib
    real = _lib.query
    seen = []

    def query(name, *a):
        n = real(name, *a)
        if name.endswith('_ws_bytes'):
            assert n > 32, (name, n)          # (so that half of it is short even after _ws's 16-byte minimum)
            seen.append(name)
            return n // 2
        return n
    monkeypatch.setattr(_lib, 'query', query)
    return seen


WORKSPACES = {
    'mixture_fwd': (lambda: hip.mixture_fwd(_z(16, 3, 4, 4), _z(32, 4, 4, 4), 2, 0.7), 'gx_mixture_fwd'),
    'mixture_w_fwd': (lambda: hip.mixture_w_fwd(_z(16, 3, 4, 4), _z(32, 3, 4, 4), _z(2, 16, 1, 4, 4), 2, 0.7, 0.7), 'gx_mixture_fwd'),
    'conv1x1_bwd': (lambda: hip.conv1x1_bwd(_z(2, 4, 8, 8), _z(2, 3, 8, 8), _z(3, 4, 1, 1), _z(3)), 'gx_conv1x1_bwd'),
    'conv1x1_bwd_act': (lambda: hip.conv1x1_bwd_act(_z(2, 4, 8, 8), _z(2, 3, 8, 8), _z(3, 4, 1, 1), _z(3), 'relu'), 'gx_conv1x1_bwd_act'),
    'bias_act_bwd': (lambda: hip.bias_act_bwd(_z(4, 4, 2, 2), _z(4, 4, 2, 2), 'relu'), 'gx_bias_act_bwd'),
    'gated_norm_bwd': (lambda: hip.gated_norm_bwd(_z(2, 8, 2, 2), _z(8), 'bn', _z(4), _z(4), _z(4), _z(4), _z(256), _z(2, 4, 2, 2)),
                       'gx_gated_norm_bwd'),
    'pooled_head_bwd': (lambda: hip.pooled_head_bwd(_z(8, 8), _z(8), _z(8), _z(8), _z(8, 2), _z(8, 8)), 'gx_pooled_head_bwd'),
    'gn_relu_bwd': (_gn_bwd(4, 4), 'gx_gn_relu_bwd'),
    'icsbp_bwd': (_icsbp_bwd(2, 8, 8, 8, 3), 'gx_icsbp_bwd'),
    'bcast_conv3x3_bwd': (lambda: hip.bcast_conv3x3_bwd(_z(4, 4, 8, 8), _z(4, 4, 8, 8), _z(4, 3), _z(4, 5, 3, 3), _z(8), _z(8), 'relu'),
                          'gx_bcast_conv3x3_bwd'),
}


@pytest.mark.parametrize('case', sorted(WORKSPACES))
def test_refused_workspaces(case, monkeypatch):
    """A workspace half the size the entry point's own *_ws_bytes query asks for (the wrappers size theirs by that query: it
    answers half here) is refused by the argument check, before any launch."""
    seen = _short_ws(monkeypatch)
    call, entry = WORKSPACES[case]
    with pytest.raises(GenesisHipError) as e:
        call()
    msg = str(e.value)
    assert seen and 'failed (-1)' in msg and entry + ':' in msg and 'workspace too small' in msg, msg


# ------------------------------------------------------------------------------------------------- 5. dynamic-K masks, saturation
@pytest.mark.parametrize('H,W', [(6, 6), (5, 7)])
def test_dynamic_k_masks_into_their_consumers(H, W):
    """Masks as gx_icsbp_fwd_dyn leaves them -- image b stops after n_b of K = 5 steps, n_b = 1, K - 1, K in one batch, the slots
    after it hold exactly -1e10 -- fed to maskpool, the mixture with external weights and the categorical KL (as log_m and as
    log_m_r), forward and backward, on the 16-byte (6 x 6) and scalar (5 x 7) paths: exp(-1e10) = 0 must come out as a weight of
    zero and a gradient of zero, never as inf - inf or 0 / 0."""
    K, B, n = 5, 3, (1, 4, 5)
    lm = off_the_clamp(dyn_masks(K, B, H, W, n, seed=40))
    assert all(bool((lm[k:, b] == -1e10).all()) for b, k in enumerate(n))
    run_maskpool(rnd(B, 6, H, W, seed=22).relu(), lm)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(26))
    for DC in (4, 3):
        run_mixture('w', True, x, rnd(K * B, DC, H, W, seed=27, scale=2.0), lm, K, std1=0.5)
    lr = off_the_clamp(dyn_masks(K, B, H, W, n, seed=50))
    full = off_the_clamp(F.log_softmax(rnd(K, B, 1, H, W, seed=85) * 6, 0))
    run_kl(lm, lr, True)
    run_kl(lm, full, True)
    run_kl(full, lr, True)


def saturated_scan_inputs():
    T, P = 7, 300
    vals = torch.tensor([-90., -30., -5., 0., 5., 30., 90.])
    g = torch.Generator().manual_seed(60)
    l = vals[torch.randint(0, 7, (T, 1, 1, 1, P), generator=g)]
    l[:, 0, 0, 0, :7] = vals.view(1, 7).expand(T, 7)             # every value at every step, whatever the draw
    return l, -rnd(1, 1, 1, P, seed=81).abs()


@pytest.mark.parametrize('last', [False, True])
def test_stick_breaking_scan_saturated(last):
    """Logits from {-90, -30, -5, 0, 5, 30, 90} over T = 7 steps: logsigmoid_f at large |x| (expf(-|x|) underflows, log1pf(0)),
    sigmoid_f(-90) = 1 / (1 + inf) = 0, scopes down to -630.  (fp32 torch against fp64 torch on these inputs: inside 1e-5 / 1e-5 on
    every output, so the project's figures stand.)"""
    l, s0 = saturated_scan_inputs()
    run_scan(l, s0, last, rnd(*l.shape, seed=82), rnd(*l.shape, seed=83))


def saturated_logsoftmax_inputs():
    K, B, C, H, W = 5, 2, 4, 5, 7
    dec = rnd(K * B, C, H, W, seed=5, scale=4.0)
    dec[:, C - 1] = rnd(K * B, H, W, seed=61, scale=80.0)
    dec[:K, C - 1, 0, 0] = torch.tensor([80., -80., 0., 79.5, -80.])      # the full spread inside one pixel
    return dec, K


def test_log_softmax_over_the_slots_saturated():
    """Mask logits spread over +-80 across the slots: expf(x - mx) underflows to 0 for the far slots, log_m_r down to -160 and
    exp(log_m_r) = 0 in the backward.  (fp32 torch against fp64 torch: inside 2e-6 / 2e-6.)"""
    run_logsoftmax(*saturated_logsoftmax_inputs())


def saturated_latent_inputs():
    B, K, D = 2, 2, 10
    args = torch.tensor([-30., -5., 19.9, 20.1, 60.])
    zh = rnd(B, K, 2 * D, seed=1, scale=2.0)
    pick = torch.arange(B * K * D).view(B, K, D) % 5
    zh[..., D:] = args[pick] - 0.5
    # softplus(-30) + 1e-8 = 1e-8: z - mu = sigma eps is far below one ulp of a mean of order 1, in the reference's own fp32
    # evaluation as in the kernel's (both form z first and subtract mu again); those latents get mu = 0, where the subtraction is exact
    zh[..., :D][pick == 0] = 0.0
    eps = torch.randn(K, B, D, generator=torch.Generator().manual_seed(2))
    lin = rnd(K - 1, B, 2 * D, seed=3, scale=2.0)
    idx = torch.arange(0, 2 * D, 3)                                   # tanh / sigmoid arguments of +-30 on every third column
    lin[..., idx] = torch.where(idx % 2 == 0, 30.0, -30.0)
    lin[..., idx[idx >= D]] -= 4.0                                    # (to_prior_sigma adds 4 to its argument)
    return zh, eps, lin


def test_latent_nodes_saturated():
    """softplus_t / softplus_grad_t on both sides of the threshold (sp + 0.5 = 19.9, 20.1, 60), far below it (-5, and -30 where
    sigma = 1e-8 is the floor) and the prior's tanhf / sigmoid_t at +-30 (tanh' = 0, sigma = 1e-4).  fp32 torch against fp64 torch
    on these inputs, as a fraction of the figures of test_latent_posterior_and_prior in close()'s measure: z 0.005, sigma < 0.001,
    log_q 0.017, log_p 0.015, kl 0.016, dzh 0.001, dlin 0.003 -- plain fp32 meets them all, so they stand unchanged."""
    run_latent(*saturated_latent_inputs())


def saturated_kl_inputs():
    K, B, H, W = 4, 2, 9, 9
    lm = off_the_clamp(F.log_softmax(rnd(K, B, 1, H, W, seed=84) * 12, 0))
    lr = off_the_clamp(F.log_softmax(rnd(K, B, 1, H, W, seed=85) * 12, 0))
    for t in (lm, lr):
        below = float((t.exp() < 1e-5).float().mean())
        assert 0.05 < below < 0.95, below                # masks on both sides of the clamp
    return lm, lr


def test_categorical_mask_kl_saturated():
    """Masks on both sides of the 1e-5 clamp (logits spread over +-12), none within a relative 1e-3 of it (asserted by
    off_the_clamp): the `a > 1e-5f` branches of categorical_kl_bwd_kernel, both ways, for both arguments."""
    run_kl(*saturated_kl_inputs(), True)


def saturated_mixture_inputs(K=5, B=2, H=5, W=7):
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(26))
    dec = rnd(K * B, 4, H, W, seed=27, scale=5.0)
    dec[:, 3] = rnd(K * B, H, W, seed=62, scale=40.0)
    return x, dec, K


@pytest.mark.parametrize('pixel_bound', [True, False])
def test_mixture_saturated(pixel_bound):
    """Mask logits spread over +-40 (expf(logit - mx) underflows in the slot softmax, log_m_r down to -80) and colour
    pre-activations up to +-5 (sigmoid saturates; unbounded: (x - mu)^2 / (2 std^2) up to 37) -- inside the regime where the fp64
    reference's s = sum_k exp(log_m_k + log N_k) stays above 1e-30 (asserted in run_mixture): the reference has no log-sum-exp
    trick and neither has the kernel."""
    x, dec, K = saturated_mixture_inputs()
    run_mixture('plain', pixel_bound, x, dec, None, K)

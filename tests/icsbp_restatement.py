"""InstanceColouringSBP.forward (modules/attention.py:162-226) restated image by image in float64 torch on the CPU, with the
dynamic-K stop as gx_icsbp_fwd_dyn documents it (include/genesis_hip.h, genesis_amd/csrc/gx_attention.hip) and the margins
by which its three discontinuities are missed.  Written from the paper's recursion and the entry point's contract, not from
oracle/v2_oracle.py: tests/test_icsbp_cpu.py holds the two against each other.

    scope_0 = 1;  step t = 0 .. K-2 of image b:
        i_t     = first argmax_p rand_p scope_t,p            (or the forced seed_idx[t, b])
        seed_t  = colour[:, i_t]                             (the gradient flows through the gather)
        d_p     = sum_c (colour_c,p - seed_t,c)^2
        alpha_p = exp(-d / sigma) | exp(-sqrt(st(d, 1e-10, 1e10)) / sigma) | max(1 - d / sigma, 0),   sigma = exp(log_sigma)
        a_p     = st(alpha_p, 0.01, 0.99)                    st(x, lo, hi) = x + (clamp(x) - x).detach()
        log_m_t = log scope_t + log a;   mass_t = sum_p exp(log_m_t)
        min_mass > 0 and mass_t < min_mass:  the image stops, n_b = t (the seed of step t was drawn and stays)
        log scope_t+1 = log scope_t + log(1 - a)
    log_m[n_b] = log scope_{n_b};  log_m[t > n_b] = -1e10 exactly (a constant);  log_s[t > n_b] = log scope_{n_b};
    seeds[t > n_b] = 0, idx[t > n_b] = 0;  n_b = K - 1 for an image that never stops.
"""
import torch

F64 = torch.float64
PAD = -1e10


def st_clamp(x, lo, hi):
    return x + (x.clamp(lo, hi) - x).detach()


def first_argmax(v):
    return int((v == v.max()).nonzero()[0, 0])


def icsbp(colour, log_sigma, rand_pixel, K, kernel='gaussian', seed_idx=None, min_mass=0.0, g_log_m=None):
    """colour [B,C,H,W], log_sigma 0-dim, rand_pixel [B,1,H,W], optional forced seed_idx [K-1,B] (long), min_mass (0: off),
    optional g_log_m [K,B,1,H,W].  -> dict: log_m, log_s [K,B,1,H,W], seeds [K-1,B,C], idx [K-1,B] (long), nsteps [B] (long),
    dcolour [B,C,H,W] and dlog_sigma (0-dim) where g_log_m is given, and the margins

      gap   [K-1,B]  (largest - second largest) / largest of rand * scope at every step whose seed was drawn (inf elsewhere)
      mass  [K-1,B]  the mask mass of every step evaluated (nan elsewhere);  margin_b = min |mass / min_mass - 1| (inf when off)
      margin_a = min gap;  margin_c = min |1 - d / sigma| over pixels and evaluated steps (inf unless epanechnikov)."""
    assert kernel in ('gaussian', 'laplacian', 'epanechnikov'), kernel
    B, C, H, W = colour.shape
    HW = H * W
    col = colour.detach().to(F64).clone().requires_grad_(True)
    lsg = log_sigma.detach().to(F64).clone().requires_grad_(True)
    sigma = lsg.exp()
    rnd = rand_pixel.detach().to(F64).reshape(B, HW)
    log_m = [[None] * B for _ in range(K)]
    log_s = [[None] * B for _ in range(K)]
    seeds = torch.zeros(max(K - 1, 0), B, C, dtype=F64)
    idx = torch.zeros(max(K - 1, 0), B, dtype=torch.int64)
    nsteps = torch.full((B,), K - 1, dtype=torch.int64)
    gap = torch.full((max(K - 1, 0), B), float('inf'), dtype=F64)
    mass = torch.full((max(K - 1, 0), B), float('nan'), dtype=F64)
    margin_c = float('inf')
    for b in range(B):
        c = col[b].reshape(C, HW)
        ls = torch.zeros(HW, dtype=F64)
        log_s[0][b] = ls
        n = K - 1
        for t in range(K - 1):
            v = rnd[b] * ls.detach().exp()
            top = torch.topk(v, 2).values
            gap[t, b] = (top[0] - top[1]) / top[0]
            i = first_argmax(v) if seed_idx is None else int(seed_idx[t, b])
            idx[t, b] = i
            seed = c[:, i]
            seeds[t, b] = seed.detach()
            d = ((c - seed.unsqueeze(1)) ** 2).sum(0)
            if kernel == 'gaussian':
                alpha = torch.exp(-d / sigma)
            elif kernel == 'laplacian':
                alpha = torch.exp(-st_clamp(d, 1e-10, 1e10).sqrt() / sigma)
            else:
                alpha = (1 - d / sigma).clamp(min=0)
                margin_c = min(margin_c, float((1 - d / sigma).detach().abs().min()))
            a = st_clamp(alpha, 0.01, 0.99)
            lm = ls + a.log()
            mass[t, b] = lm.detach().exp().sum()
            if min_mass > 0 and float(mass[t, b]) < min_mass:
                n = t
                break
            log_m[t][b] = lm
            ls = ls + (1 - a).log()
            log_s[t + 1][b] = ls
        nsteps[b] = n
        log_m[n][b] = ls
        for t in range(n + 1, K):
            log_m[t][b] = torch.full((HW,), PAD, dtype=F64)
            log_s[t][b] = ls
    lm_all = torch.stack([torch.stack(r) for r in log_m]).view(K, B, 1, H, W)
    out = dict(log_m=lm_all.detach(), log_s=torch.stack([torch.stack(r) for r in log_s]).detach().view(K, B, 1, H, W),
               seeds=seeds, idx=idx, nsteps=nsteps, gap=gap, mass=mass, margin_c=margin_c,
               margin_a=float(gap.min()) if gap.numel() else float('inf'),
               margin_b=float((mass[~mass.isnan()] / min_mass - 1).abs().min()) if min_mass > 0 and K > 1 else float('inf'))
    if g_log_m is not None:
        loss = (lm_all * g_log_m.detach().to(F64)).sum()
        if loss.requires_grad:
            dc, dl = torch.autograd.grad(loss, (col, lsg), allow_unused=True)
        else:                   # K = 1, or every image stopped at step 0: the masks do not depend on the inputs
            dc = dl = None
        out['dcolour'] = dc if dc is not None else torch.zeros_like(col)
        out['dlog_sigma'] = dl if dl is not None else torch.zeros((), dtype=F64)
    return out


def padded(nsteps, K, H, W):
    """[K,B,1,H,W] bool: the slots gx_icsbp_fwd_dyn pads (t > nsteps[b])."""
    t = torch.arange(K).view(K, 1)
    return (t > nsteps.view(1, -1).to(torch.int64)).view(K, -1, 1, 1, 1).expand(K, nsteps.numel(), 1, H, W)

"""IC-SBP (genesis_amd/csrc/gx_attention.hip: gx_icsbp_fwd[_dyn], gx_icsbp_bwd[_dyn]) at every dispatch its host code can pick,
at every channel count the kernels guard for, at K = 1, 2 and 17, with forced seed collisions and at every dynamic-K stop.
The forward dispatch is a pure function of HW (threads_for: T = min(HW, 1024); ppt = HW / T picks icsbp_fwd_kernel<1 | 2 | 4> or
the generic <0>); the backward runs T = min(HW, 256) threads on nch = HW / T chunks, and icsbp_bwd_finalize_kernel's chunk loop
adds two chunks per round (nch >= 8) and has a tail statement (nch <= 4).  One table per group of cases; every row DECLARES the
dispatch it reaches, and tests/test_icsbp_cpu.py holds the declaration against the formulas.  Every case

  1. builds its inputs on the CPU so that the float64 restatement (tests/icsbp_restatement.py) misses every discontinuity by a
     stated margin: the top two of rand * scope differ by MARGIN_A relative at every step (so seed_idx must equal the
     reference's EXACTLY -- there is no replay with the reference's seeds in this file), every mask mass is MARGIN_B away from
     min_mass, and for the Epanechnikov kernel no pixel lies within MARGIN_C of the kink at d = sigma,
  2. puts every operand in the middle of a NaN buffer and every output in the middle of a sentinel-filled buffer (the output
     itself starts as NaN, the integer outputs as a sentinel integer), the backward's workspace -- sized by
     gx_icsbp_bwd_ws_bytes -- between two guard bands and filled with NaN, and calls the C entry points through _lib.call,
  3. asserts bit-identical guard bands, finite outputs, the values at tests/test_kernels_gpu.py::test_icsbp's bounds in its
     close() measure (log_m, log_s 1e-5 / 2e-5; seeds exact; dcolour 2e-4 / 2e-4; dlog_sigma 2e-4 / 1e-5: no bound here is new)
     and that a second run gives the same bits.

What each row would catch (one-line mistakes in the code it reaches; argued from the code, never run):

  32 x 64, 64 x 32 (ppt = 2)          `ppt == 2` launched as <4>: slots 2 and 3 index pixels >= HW -- the next image's colours (the
                                      NaN band behind the last image), log_s of the next image and the band behind it written;
                                      a <2> path that reads ls[p], the LDS scope only the generic kernel initialises
  <2> / <4>, argmax in every slot     a register slot never considered (`q = 1`, `q < NR - 1`): the reference argmax of some
                                      (image, step) lies in each slot q, so seed_idx differs
  8 x 8, 8 x 16, 16 x 16, 16 x 32     red_v[w] / red_i[w] merged over 16 waves when nw = 1, 2, 4, 8: LDS nobody wrote takes part
  (argmax outside wave 0)             in the argmax and in the dynamic-K mass; a merge that keeps wave 0 (`w < nw - 1`, lane 0
                                      storing before the shuffle finished) loses the candidate of the other waves
  C = 1, 2, 3, 5, 7                   `tid < C` replaced by MAXC on the seed load (reads channel planes C..7: the next image, the NaN
                                      band behind the last) or on the seed store (row (t B + b) C + tid runs into the next
                                      image's seed and the band behind seeds); cv[q][c] / col[c] not zeroed for c >= C together
                                      with a distance loop over MAXC; dcolour stored for c >= C (the next image's gradient)
  K = 17                              seed_sh or sums sized K - 2 (15 rows): step 15 lands on the LDS behind it
  K = 2, K = 1                        a step loop that assumes K - 1 >= 2; at K = 1 nothing runs: log_m[0] = log_s[0] = 0, zero
                                      gradients, and the workspace query must not return 0 partial rows
  nch = 1, 2 (and 4)                  the finalize tail statement dropped (these have no loop round: every seed gradient and
                                      d log_sigma would be 0); nch = 2: the tail runs in thread quarters 0 and 1 only
  nch = 4, 8, 16, 32                  the loop bound `ch + 4 <= nchunks` (nch = 4: quarter 0 adds chunk 4, the next image's
                                      partials or NaN workspace); `ch += 4`; quarters combined before all four were written
  HW = 64, 128 backward               block_sum_multi with one or two waves summing red rows of waves that do not exist
  forced seeds                        a second draw of the same seed pixel overwriting instead of adding (compared over the seed
                                      pixels alone); the scatter at pixel 0, HW - 1, and on both sides of the first chunk boundary
  dynamic K: nsteps exact             n_exec off by one; the mass reduced over waves that do not exist; `tot <= min_mass`
  dynamic K: mask n_b, padding        padding written from n_exec instead of n_exec + 1 (mask n_b must be the remaining scope);
                                      seeds / indices of the steps never run left as they were (NaN / the sentinel)
  dynamic K: NaN workspace            the `t >= n` branch of icsbp_bwd_kernel not writing its zero partials: the finalize kernel
                                      sums what the last user of the workspace left (NaN here: a non-finite gradient)
  dynamic K: padded gradients         `gs` started from g_m[K - 1] for a stopped image, g_m[t] read for t > n: g = 1e30 in the
                                      padded slots must give the same bits as random values there
  ICSBPFn with min_mass > 0           the node not handing nsteps to its backward (the stopped images' padded masks differentiated)
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from tests import icsbp_restatement as R

gpu = pytest.mark.gpu

DEV = 'cuda'
F64 = torch.float64
GUARD = 4096              # elements on each side of every operand and output
WS_GUARD = 16384          # bytes on each side of the workspace
SENTINEL = 1.2345e30      # float guard bands (finite, so that torch.equal can compare them)
ISENT, IFILL = 0x5A5A5A5A, -7777      # integer guard bands / what an integer output starts as
MARGIN_A, MARGIN_B, MARGIN_C = 1e-4, 0.05, 1e-4
ALL = ('gaussian', 'laplacian', 'epanechnikov')
G = ('gaussian',)


# ===================================================================================================== the case tables
def row(rid, H, W, K, C, B, kernels, fT, inst, bT, nch, rounds, tail, **more):
    """fT / inst: forward threads and icsbp_fwd_kernel's template argument (0: generic); bT / nch: backward threads and chunks;
    rounds / tail: loop rounds of the finalize kernel's chunk loop and the thread quarters whose tail statement runs."""
    return dict(dict(id=rid, H=H, W=W, K=K, C=C, B=B, kernels=kernels, fT=fT, inst=inst, bT=bT, nch=nch, rounds=rounds, tail=tail),
                **more)


VALUE_ROWS = [
    row('8x8-k17-c8', 8, 8, 17, 8, 3, ALL, 64, 1, 64, 1, 0, (0,)),
    row('8x16-k2-c3', 8, 16, 2, 3, 3, ALL, 128, 1, 128, 1, 0, (0,)),
    row('16x32-k5-c8', 16, 32, 5, 8, 2, G, 512, 1, 256, 2, 0, (0, 1)),
    row('16x64-k3-c8', 16, 64, 3, 8, 2, G, 1024, 1, 256, 4, 0, (0, 1, 2, 3)),
    row('32x64-k5-c8', 32, 64, 5, 8, 2, ALL, 1024, 2, 256, 8, 1, ()),
    row('64x32-k3-c1', 64, 32, 3, 1, 3, G, 1024, 2, 256, 8, 1, ()),
    row('32x128-k4-c5', 32, 128, 4, 5, 3, G, 1024, 4, 256, 16, 2, ()),
    row('64x128-k4-c8', 64, 128, 4, 8, 2, ALL, 1024, 0, 256, 32, 4, ()),
    row('16x16-k1-c8', 16, 16, 1, 8, 2, G, 256, 1, 256, 1, 0, (0,)),
    row('16x16-k7-c2', 16, 16, 7, 2, 3, ('laplacian',), 256, 1, 256, 1, 0, (0,)),
    row('16x16-k7-c7', 16, 16, 7, 7, 3, ('laplacian',), 256, 1, 256, 1, 0, (0,)),
]
IMAGES = ('ramp', 'regions')
VALUE_CASES = [(r, k, im) for r in VALUE_ROWS for k in r['kernels'] for im in IMAGES]

FORCED_ROWS = [
    row('forced-16x32', 16, 32, 4, 8, 2, G, 512, 1, 256, 2, 0, (0, 1)),
    row('forced-32x64', 32, 64, 4, 8, 2, G, 1024, 2, 256, 8, 1, ()),
]
FORCED_CASES = [(r, im) for r in FORCED_ROWS for im in IMAGES]


def forced_seeds(r):
    """[K-1, B]: image 0 draws pixel 0 twice and pixel HW - 1; image 1 draws 255 twice and 256 (both sides of the boundary of the
    backward's first 256-pixel chunk)."""
    HW = r['H'] * r['W']
    return torch.tensor([[0, 255], [HW - 1, 256], [0, 255]], dtype=torch.int64)


# dynamic K.  images: (regions, fraction of the plane they cover); the rest is "scatter" (every pixel its own widely spaced colour).
SCATTER, HALF, TWO, FULL = (0, 0.0), (1, 0.5), (2, 0.5), (5, 1.0)
DYN_ROWS = [
    row('dyn-8x8', 8, 8, 5, 8, 3, G, 64, 1, 64, 1, 0, (0,), images=(SCATTER, HALF, FULL), min_mass=3.2, nsteps=(0, 1, 4)),
    row('dyn-16x16', 16, 16, 5, 8, 3, ALL, 256, 1, 256, 1, 0, (0,), images=(HALF, FULL, SCATTER), min_mass=12.8, nsteps=(1, 4, 0)),
    row('dyn-16x16-b1', 16, 16, 5, 8, 1, ALL, 256, 1, 256, 1, 0, (0,), images=(HALF,), min_mass=12.8, nsteps=(1,)),
    row('dyn-32x64', 32, 64, 5, 8, 3, G, 1024, 2, 256, 8, 1, (), images=(FULL, SCATTER, HALF), min_mass=102.4, nsteps=(4, 0, 1)),
    # the model's own threshold (20): the clamp floor alone gives a mask 0.01 HW + 0.98 = 21.46 pixels here, so no image can stop
    # at step 0; the batch stops at 1, 2 and never
    row('dyn-32x64-mass20', 32, 64, 5, 8, 3, G, 1024, 2, 256, 8, 1, (), images=(HALF, TWO, FULL), min_mass=20.0, nsteps=(1, 2, 4)),
    row('dyn-64x128', 64, 128, 5, 8, 3, G, 1024, 0, 256, 32, 4, (), images=(SCATTER, HALF, FULL), min_mass=409.6, nsteps=(0, 1, 4)),
]
DYN_CASES = [(r, k, mode) for r in DYN_ROWS for k in r['kernels'] for mode in ('forced', 'free')]
FN_ROW = row('fn-16x16', 16, 16, 5, 8, 3, G, 256, 1, 256, 1, 0, (0,), images=(FULL, SCATTER, HALF), min_mass=12.8, nsteps=(4, 0, 1))
ALL_ROWS = VALUE_ROWS + FORCED_ROWS + DYN_ROWS + [FN_ROW]


# ===================================================================================================== inputs (CPU)
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def close(a, b, rtol, atol, msg=''):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, '%s shape %s, the reference %s' % (msg, tuple(a.shape), tuple(b.shape))
    if b.numel() == 0:          # (seeds at K = 1)
        return
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= atol + rtol * ref, '%s max err %.3e (ref max %.3e)' % (msg, err, ref)


def log_sigma_of(K):
    return torch.tensor(1.0 / (K * math.log(2)), dtype=F64).log()       # the model's initial bandwidth, as test_icsbp


def ramp_image(B, C, H, W):
    """The generator of tests/test_kernels_gpu.py::test_icsbp: uniform colours scaled by 0.7 plus the coordinate ramp in the last
    min(2, C) channels."""
    colour = rnd(B, C, H, W, seed=18, scale=0.7)
    uv = torch.stack(torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing='ij'))
    n = min(2, C)
    colour[:, C - n:] += uv[2 - n:]
    return colour


def regions_image(B, C, H, W):
    """2 x 3 blocks of one colour each (per image) plus noise of 0.01: inside the seed's block alpha sits on the upper clamp bound,
    in the other blocks on the lower one."""
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    rid = (y * 2 // H) * 3 + x * 3 // W
    base = rnd(B, 6, C, seed=41, scale=0.8)
    colour = base[:, rid].permute(0, 3, 1, 2).contiguous()
    return colour + rnd(B, C, H, W, seed=42, scale=0.01)


def scatter_code(p):
    """[8, n]: pixel index -> a point of a grid with spacing 1.5 (two bits in each of channels 0..5, one in 6 and 7: 14 bits)."""
    ch = [((p >> (2 * c)) & 3) for c in range(6)] + [(p >> 12) & 1, (p >> 13) & 1]
    return 1.5 * torch.stack(ch).float()


def dyn_image(spec, H, W, seed):
    """One [8, H, W] image: `nreg` equal regions of one colour each (noise 0.01) in the LAST `frac` of the pixels, scatter before them.
    Any two scatter pixels, any two regions and any region and scatter pixel are at squared distance >= 2.25 (alpha below the
    clamp floor for all three kernels at K = 5).  -> colour, region id per pixel (-1: scatter)."""
    nreg, frac = spec
    HW = H * W
    p = torch.arange(HW)
    colour = scatter_code(p)
    nR = int(round(frac * HW))
    rid = torch.full((HW,), -1, dtype=torch.int64)
    if nreg:
        q = p[HW - nR:] - (HW - nR)
        rid[HW - nR:] = q * nreg // nR
        rc = scatter_code(rid[HW - nR:])
        rc[7] = -3.0
        colour[:, HW - nR:] = rc + rnd(8, nR, seed=seed, scale=0.01)
    return colour.view(8, H, W), rid


def dyn_batch(r):
    ims = [dyn_image(spec, r['H'], r['W'], 60 + b) for b, spec in enumerate(r['images'])]
    return torch.stack([c for c, _ in ims]), [rid for _, rid in ims]


def dyn_forced_seeds(r, rids):
    """Step t of image b: the middle pixel of region t while there is one, then distinct scatter pixels."""
    K, B = r['K'], r['B']
    idx = torch.zeros(K - 1, B, dtype=torch.int64)
    for b, rid in enumerate(rids):
        nreg = int(rid.max()) + 1
        scat = (rid < 0).nonzero().flatten()
        for t in range(K - 1):
            if t < nreg:
                px = (rid == t).nonzero().flatten()
                idx[t, b] = px[len(px) // 2]
            else:
                idx[t, b] = scat[(3 + 11 * t) % len(scat)]
    return idx


def argmax_placement(r, idx):
    """What the row requires of the reference's free argmax: a seed in every register slot of <2> / <4>, one beyond the first T pixels
    of the generic kernel, one outside wave 0 of a workgroup of two or more waves."""
    idx = idx.flatten()
    if idx.numel() == 0:
        return True
    fT = r['fT']
    ok = bool((((idx % fT) >> 6) != 0).any()) if fT > 64 else True
    if r['inst'] in (2, 4):
        ok = ok and {int(i) // fT for i in idx} == set(range(r['inst']))
    if r['inst'] == 0:
        ok = ok and bool((idx >= fT).any())
    return ok


_INPUTS = {}
MAX_TRIES, MAX_PASSES = 60, 6


def _search(colour, ls, K, kernel, make_rand, accept, min_mass=0.0, seed_idx=None, g=None, need_a=None):
    """Tries rand_pixel seeds 19, 20, ... until the float64 restatement meets the margins (and `accept`).  For the Epanechnikov
    kernel the pixels within 2 MARGIN_C of the kink are scaled by 1.003 first (at most MAX_PASSES times)."""
    need_a = seed_idx is None if need_a is None else need_a
    for s in range(19, 19 + MAX_TRIES):
        rand = make_rand(s)
        col = colour.clone()
        moved = 0
        for _ in range(MAX_PASSES):
            ref = R.icsbp(col, ls, rand, K, kernel, seed_idx, min_mass, g)
            if ref['margin_c'] >= MARGIN_C:
                break
            sigma = float(ls.exp())
            for b in range(col.shape[0]):
                near = torch.zeros(col.shape[2:], dtype=torch.bool)
                for t in range(K - 1):
                    d = ((col[b].double() - ref['seeds'][t, b].view(-1, 1, 1)) ** 2).sum(0)
                    near |= (1 - d / sigma).abs() < 2 * MARGIN_C
                for t in range(K - 1):
                    near.view(-1)[int(ref['idx'][t, b])] = False        # (a seed is at d = 0 of its own step: leave the seeds alone)
                col[b][:, near] *= 1.003
                moved += int(near.sum())
        else:
            continue
        if (need_a and ref['margin_a'] < MARGIN_A) or ref['margin_b'] < MARGIN_B or not accept(ref):
            continue
        return dict(colour=col, rand=rand, log_sigma=ls, ref=ref, rand_seed=s, moved=moved, g=g, seed_idx=seed_idx)
    raise AssertionError('no rand_pixel seed in %d meets the margins' % MAX_TRIES)


def value_inputs(r, kernel, image):
    key = ('value', r['id'], kernel, image)
    if key not in _INPUTS:
        B, C, H, W, K = r['B'], r['C'], r['H'], r['W'], r['K']
        colour = ramp_image(B, C, H, W) if image == 'ramp' else regions_image(B, C, H, W)
        g = rnd(K, B, 1, H, W, seed=20)
        _INPUTS[key] = _search(colour, log_sigma_of(K), K, kernel,
                               lambda s: torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(s)),
                               lambda ref: argmax_placement(r, ref['idx']), g=g)
    return _INPUTS[key]


def forced_inputs(r, image):
    key = ('forced', r['id'], image)
    if key not in _INPUTS:
        B, C, H, W, K = r['B'], r['C'], r['H'], r['W'], r['K']
        colour = ramp_image(B, C, H, W) if image == 'ramp' else regions_image(B, C, H, W)
        _INPUTS[key] = _search(colour, log_sigma_of(K), K, 'gaussian',
                               lambda s: torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(s)),
                               lambda ref: True, seed_idx=forced_seeds(r), g=rnd(K, B, 1, H, W, seed=20))
    return _INPUTS[key]


def dyn_inputs(r, kernel, mode):
    """mode 'forced': the seeds of dyn_forced_seeds; 'free': rand_pixel in [0.5, 1) inside the regions and [0, 0.5) in the scatter,
    so that the free argmax visits the regions first (a region just visited has scope 0.01)."""
    key = ('dyn', r['id'], kernel, mode)
    if key not in _INPUTS:
        B, H, W, K = r['B'], r['H'], r['W'], r['K']
        colour, rids = dyn_batch(r)
        inreg = torch.stack([rid >= 0 for rid in rids]).view(B, 1, H, W)

        def make_rand(s):
            # (u ** 16: the scope of a plane of equal regions is all but flat, so the top two of rand * scope are the top two of
            #  rand; of thousands of uniform draws they are 1 / HW apart, of their 16th powers 16 / HW)
            u = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(s)) ** 16
            return torch.where(inreg, 0.5 + 0.5 * u, 0.5 * u)
        _INPUTS[key] = _search(colour, log_sigma_of(K), K, kernel, make_rand, lambda ref: True, min_mass=r['min_mass'],
                               seed_idx=dyn_forced_seeds(r, rids) if mode == 'forced' else None, g=rnd(K, B, 1, H, W, seed=20),
                               need_a=True)
        _INPUTS[key]['rids'] = rids
    return _INPUTS[key]


# ===================================================================================================== the guarded launch
def _guarded_in(t):
    """t in the middle of a NaN buffer -> (the buffer, the view)."""
    buf = torch.full((t.numel() + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _guarded_out(shape, dtype=torch.float32):
    n = 1
    for s in shape:
        n *= s
    if dtype in (torch.float32, torch.float64):
        buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
        buf[GUARD:GUARD + n] = float('nan')
    else:
        buf = torch.full((n + 2 * GUARD,), ISENT, dtype=dtype, device=DEV)
        buf[GUARD:GUARD + n] = IFILL
    # (the address is taken from the buffer: an empty view -- seeds and seed_idx at K = 1 -- has none of its own)
    return buf, buf[GUARD:GUARD + n].view(shape), ctypes.c_void_p(buf.data_ptr() + GUARD * buf.element_size())


def _bands_intact(buf, n, what):
    s = torch.full((GUARD,), SENTINEL if buf.is_floating_point() else ISENT, dtype=buf.dtype, device=DEV)
    assert torch.equal(buf[:GUARD], s), '%s: the guard band in FRONT of it was written' % what
    assert torch.equal(buf[GUARD + n:], s), '%s: the guard band BEHIND it was written' % what


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def run_forward(inp, kernel, K, seed_idx=None, min_mass=0.0):
    """gx_icsbp_fwd / gx_icsbp_fwd_dyn on guarded buffers -> {name: device view} (nsteps only with min_mass > 0)."""
    from genesis_amd import _lib, hip_ops as hip
    B, C, H, W = inp['colour'].shape
    keep = dict(colour=_guarded_in(inp['colour']), rand=_guarded_in(inp['rand']))
    ls = inp['log_sigma'].to(DEV)
    sidx = seed_idx.to(DEV) if seed_idx is not None else None
    outs = dict(log_m=_guarded_out((K, B, 1, H, W)), log_s=_guarded_out((K, B, 1, H, W)), seeds=_guarded_out((K - 1, B, C)),
                idx=_guarded_out((K - 1, B), torch.int64))
    head = (_ptr(keep['colour'][1]), _ptr(ls), _ptr(keep['rand'][1]), _ptr(sidx) if sidx is not None else None, B, C, H, W, K,
            hip.KERNELS[kernel])
    tail = tuple(outs[k][2] for k in ('log_m', 'log_s', 'seeds', 'idx'))
    if min_mass > 0:
        outs['nsteps'] = _guarded_out((B,), torch.int32)
        _lib.call('gx_icsbp_fwd_dyn', *head, float(min_mass), *tail, outs['nsteps'][2], hip._stream())
    else:
        _lib.call('gx_icsbp_fwd', *head, *tail, hip._stream())
    torch.cuda.synchronize()
    for name, (buf, view, _) in outs.items():
        _bands_intact(buf, view.numel(), 'forward ' + name)
        if view.is_floating_point():
            assert bool(torch.isfinite(view).all()), 'forward %s: non-finite values (an element nobody wrote, or a NaN guard read)' % name
        else:
            assert not bool((view == IFILL).any()), 'forward %s: an element nobody wrote' % name
    for k, (buf, view) in keep.items():
        assert torch.equal(view.cpu(), inp[k]), 'forward: operand %s was modified' % k
    return dict({k: v[1] for k, v in outs.items()}, _keep=outs)


def run_backward(inp, kernel, K, fwd, g, nsteps=None):
    """gx_icsbp_bwd / gx_icsbp_bwd_dyn with the forward's own seeds and indices, the workspace NaN between two guard bands."""
    from genesis_amd import _lib, hip_ops as hip
    B, C, H, W = inp['colour'].shape
    keep = dict(colour=_guarded_in(inp['colour']), g=_guarded_in(g))
    ls = inp['log_sigma'].to(DEV)
    outs = dict(dcolour=_guarded_out((B, C, H, W)), dlog_sigma=_guarded_out((1,), F64))
    nb = _lib.query('gx_icsbp_bwd_ws_bytes', B, H, W, K)
    assert nb >= 8 * (B * (H * W // min(H * W, 256)) * max(K - 1, 1) * 9 + B)
    wsbuf = torch.full((nb + 2 * WS_GUARD,), 0xFF, dtype=torch.uint8, device=DEV)        # (0xFF bytes read as doubles: NaN)
    wsbuf[:WS_GUARD] = 0xA5
    wsbuf[WS_GUARD + nb:] = 0xA5
    ws = ctypes.c_void_p(wsbuf.data_ptr() + WS_GUARD)
    head = (_ptr(keep['colour'][1]), _ptr(ls), fwd['_keep']['seeds'][2], fwd['_keep']['idx'][2], _ptr(keep['g'][1]))
    dims = (B, C, H, W, K, hip.KERNELS[kernel], outs['dcolour'][2], outs['dlog_sigma'][2], ws, nb, hip._stream())
    if nsteps is not None:
        _lib.call('gx_icsbp_bwd_dyn', *head, _ptr(nsteps), *dims)
    else:
        _lib.call('gx_icsbp_bwd', *head, *dims)
    torch.cuda.synchronize()
    for name, (buf, view, _) in outs.items():
        _bands_intact(buf, view.numel(), 'backward ' + name)
        assert bool(torch.isfinite(view).all()), ('backward %s: non-finite values (an element or a partial sum nobody wrote: the '
                                                  'workspace started as NaN)' % name)
    band = torch.full((WS_GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    assert torch.equal(wsbuf[:WS_GUARD], band), 'the bytes in front of the workspace were written'
    assert torch.equal(wsbuf[WS_GUARD + nb:], band), 'the bytes behind the workspace (%d bytes) were written' % nb
    return outs['dcolour'][1], outs['dlog_sigma'][1][0]


def same_bits(a, b, what):
    for k in [k for k in a if not k.startswith('_')]:
        assert torch.equal(a[k], b[k]), '%s: %s differs between two runs' % (what, k)


# ===================================================================================================== the conditions (no GPU)
def test_icsbp_table_meets_its_conditions():
    """What the GPU tests rely on, asserted on the float64 reference: margins (a), (b), (c) of every case, the argmax placement
    of every value row, the stop points of every dynamic-K row, and that the tables reach every class the issue names."""
    for r, kernel, image in VALUE_CASES:
        inp = value_inputs(r, kernel, image)
        ref = inp['ref']
        assert ref['margin_a'] >= MARGIN_A and ref['margin_c'] >= MARGIN_C, (r['id'], kernel, image)
        assert argmax_placement(r, ref['idx']), (r['id'], kernel, image)
        assert inp['moved'] <= 1e-3 * inp['colour'].numel() + 8, (r['id'], kernel, image, inp['moved'])
        assert inp['colour'].dtype == inp['rand'].dtype == torch.float32
    for r, image in FORCED_CASES:
        idx = forced_inputs(r, image)['seed_idx']
        HW = r['H'] * r['W']
        assert {0, HW - 1, 255, 256} == set(idx.flatten().tolist())
        assert all(len(set(idx[:, b].tolist())) < r['K'] - 1 for b in range(r['B']))        # a pixel drawn twice in every image
    for r, kernel, mode in DYN_CASES:
        inp = dyn_inputs(r, kernel, mode)
        ref = inp['ref']
        assert ref['margin_b'] >= MARGIN_B and ref['margin_c'] >= MARGIN_C, (r['id'], kernel, mode, ref['margin_b'])
        assert ref['margin_a'] >= MARGIN_A              # (forced runs too: the issue puts both under margin (a))
        assert tuple(ref['nsteps'].tolist()) == r['nsteps'], (r['id'], kernel, mode, ref['nsteps'])
    # coverage
    fwd = {(r['inst'], r['fT'] // 64) for r in VALUE_ROWS}
    assert {(1, 1), (1, 2), (1, 8), (1, 16), (2, 16), (4, 16), (0, 16)} <= fwd
    assert any(r['inst'] == 0 and r['H'] * r['W'] // r['fT'] == 8 for r in VALUE_ROWS)
    assert {1, 2, 4, 8, 16, 32} <= {r['nch'] for r in VALUE_ROWS}
    assert {64, 128, 256} <= {r['bT'] for r in VALUE_ROWS}
    assert {1, 2, 3, 5, 7, 8} <= {r['C'] for r in VALUE_ROWS} and {1, 2, 17} <= {r['K'] for r in VALUE_ROWS}
    assert any(r['H'] != r['W'] for r in VALUE_ROWS)
    for inst in (1, 2, 0):
        rows = [r for r in DYN_ROWS if r['inst'] == inst and r['B'] == 3]
        assert rows and all(0 in r['nsteps'] or r['min_mass'] == 20.0 for r in rows)
        assert all(r['K'] - 1 in r['nsteps'] and any(0 < n < r['K'] - 1 for n in r['nsteps']) for r in rows)
    assert any(r['B'] == 1 for r in DYN_ROWS) and any(r['fT'] == 64 for r in DYN_ROWS)
    assert all(abs(r['min_mass'] - 0.05 * r['H'] * r['W']) < 1e-9 or r['min_mass'] == 20.0 for r in DYN_ROWS)


# ===================================================================================================== the GPU tests
def check_forward(fwd, ref, what):
    assert torch.equal(fwd['idx'].cpu(), ref['idx']), '%s: seed_idx %s, the reference %s (its smallest top-two gap: %.2e)' % (
        what, fwd['idx'].cpu().tolist(), ref['idx'].tolist(), ref['margin_a'])
    close(fwd['seeds'], ref['seeds'], 0, 0, what + ' seeds')


@gpu
@pytest.mark.parametrize('r,kernel,image', VALUE_CASES, ids=['%s-%s-%s' % (r['id'], k, im) for r, k, im in VALUE_CASES])
def test_icsbp_value_row(r, kernel, image):
    inp = value_inputs(r, kernel, image)
    ref, K = inp['ref'], r['K']
    assert ref['margin_a'] >= MARGIN_A and argmax_placement(r, ref['idx'])
    fwd = run_forward(inp, kernel, K)
    check_forward(fwd, ref, r['id'])
    dcol, dls = run_backward(inp, kernel, K, fwd, inp['g'])
    print('%-16s %-12s %-7s rand seed %d  log_m err %.2e (max %.2e)  dcolour err %.2e (max %.2e)  dlog_sigma %.6e (ref %.6e)' % (
        r['id'], kernel, image, inp['rand_seed'], float((fwd['log_m'].cpu().double() - ref['log_m']).abs().max()),
        float(ref['log_m'].abs().max()), float((dcol.cpu().double() - ref['dcolour']).abs().max()), float(ref['dcolour'].abs().max()),
        float(dls), float(ref['dlog_sigma'])))
    close(fwd['log_m'], ref['log_m'], 1e-5, 2e-5, 'log_m')
    close(fwd['log_s'], ref['log_s'], 1e-5, 2e-5, 'log_s')
    assert float((fwd['log_m'].exp().sum(0) - 1).abs().max()) < 1e-3        # the reference's own invariant (utils/misc.py:258-270)
    close(dcol, ref['dcolour'], 2e-4, 2e-4, 'dcolour')
    close(dls, ref['dlog_sigma'], 2e-4, 1e-5, 'dlog_sigma')
    if K == 1:      # no step: the one mask is the whole scope -- and the same through the wrappers, whose seeds are empty tensors
        assert not bool(fwd['log_m'].any()) and not bool(fwd['log_s'].any()) and not bool(dcol.any()) and float(dls) == 0.0
        from genesis_amd import hip_ops as hip
        cd, ld = inp['colour'].to(DEV), inp['log_sigma'].to(DEV)
        lm, lsd, sd, idx = hip.icsbp_fwd(cd, ld, inp['rand'].to(DEV), 1, kernel)
        assert sd.shape == (0, r['B'], r['C']) and idx.shape == (0, r['B']) and not bool(lm.any()) and not bool(lsd.any())
        dc, dl = hip.icsbp_bwd(cd, ld, sd, idx, inp['g'].to(DEV), kernel)
        assert not bool(dc.any()) and float(dl) == 0.0
    fwd2 = run_forward(inp, kernel, K)
    same_bits(fwd, fwd2, r['id'] + ' forward')
    dcol2, dls2 = run_backward(inp, kernel, K, fwd2, inp['g'])
    assert torch.equal(dcol, dcol2) and torch.equal(dls, dls2), r['id'] + ': the backward differs between two runs'


@gpu
@pytest.mark.parametrize('r,image', FORCED_CASES, ids=['%s-%s' % (r['id'], im) for r, im in FORCED_CASES])
def test_icsbp_forced_seed_collisions(r, image):
    """The same pixel drawn in two steps, seeds at pixel 0, HW - 1, 255 and 256: the finalize kernel's scatter-add must land twice;
    dcolour at the seed pixels is compared on its own, so that a lost add cannot hide under the plane's maximum."""
    inp = forced_inputs(r, image)
    ref, K, sidx = inp['ref'], r['K'], inp['seed_idx']
    fwd = run_forward(inp, 'gaussian', K, seed_idx=sidx)
    check_forward(fwd, ref, r['id'])
    close(fwd['log_m'], ref['log_m'], 1e-5, 2e-5, 'log_m')
    close(fwd['log_s'], ref['log_s'], 1e-5, 2e-5, 'log_s')
    dcol, dls = run_backward(inp, 'gaussian', K, fwd, inp['g'])
    close(dcol, ref['dcolour'], 2e-4, 2e-4, 'dcolour')
    close(dls, ref['dlog_sigma'], 2e-4, 1e-5, 'dlog_sigma')
    B, C = r['B'], r['C']
    at = lambda t: torch.stack([t.cpu().flatten(2)[b][:, sorted(set(sidx[:, b].tolist()))] for b in range(B)])      # noqa: E731
    print('%s %s: dcolour at the seed pixels: max |err| %.3e, max |ref| %.3e (plane max %.3e)' % (
        r['id'], image, float((at(dcol).double() - at(ref['dcolour'])).abs().max()), float(at(ref['dcolour']).abs().max()),
        float(ref['dcolour'].abs().max())))
    close(at(dcol), at(ref['dcolour']), 2e-4, 2e-4, 'dcolour at the seed pixels')
    dcol2, dls2 = run_backward(inp, 'gaussian', K, fwd, inp['g'])
    assert torch.equal(dcol, dcol2) and torch.equal(dls, dls2)


def check_dynamic_forward(fwd, ref, r, what):
    K, B, H, W = r['K'], r['B'], r['H'], r['W']
    n = ref['nsteps']
    assert fwd['nsteps'].cpu().tolist() == n.tolist(), '%s: nsteps %s, the reference %s (masses %s, min_mass %g)' % (
        what, fwd['nsteps'].cpu().tolist(), n.tolist(), ref['mass'].t().tolist(), r['min_mass'])
    check_forward(fwd, ref, what)
    pad = R.padded(n, K, H, W)
    lm, lsd = fwd['log_m'].cpu(), fwd['log_s'].cpu()
    assert bool((lm[pad] == -1e10).all()), what + ': a padded mask is not exactly -1e10'
    for b in range(B):
        nb = int(n[b])
        assert not bool(fwd['seeds'][nb + 1:, b].any()) and not bool(fwd['idx'][nb + 1:, b].any()), what + ': a seed of a step never run'
        for t in range(nb + 1, K):      # log_s after the stop: the remaining scope
            assert torch.equal(lsd[t, b], lm[nb, b]), what + ': log_s after the stop'
        if nb == 0:
            assert not bool(lm[0, b].any()), what + ': stopped at step 0, the first mask must be all zeros'
    close(lm[~pad], ref['log_m'][~pad], 1e-5, 2e-5, what + ' log_m (unpadded entries)')
    close(lsd, ref['log_s'], 1e-5, 2e-5, what + ' log_s')
    return pad


@gpu
@pytest.mark.parametrize('r,kernel,mode', DYN_CASES, ids=['%s-%s-%s' % (r['id'], k, m) for r, k, m in DYN_CASES])
def test_icsbp_dynamic_k(r, kernel, mode):
    inp = dyn_inputs(r, kernel, mode)
    ref, K = inp['ref'], r['K']
    assert ref['margin_b'] >= MARGIN_B and ref['margin_a'] >= MARGIN_A
    assert tuple(ref['nsteps'].tolist()) == r['nsteps']
    fwd = run_forward(inp, kernel, K, seed_idx=inp['seed_idx'], min_mass=r['min_mass'])
    what = '%s %s %s' % (r['id'], kernel, mode)
    pad = check_dynamic_forward(fwd, ref, r, what)
    g = inp['g']
    dcol, dls = run_backward(inp, kernel, K, fwd, g, fwd['nsteps'])
    print('%-28s nsteps %s  dcolour err %.2e (max %.2e)  dlog_sigma %.6e (ref %.6e)' % (
        what, fwd['nsteps'].cpu().tolist(), float((dcol.cpu().double() - ref['dcolour']).abs().max()), float(ref['dcolour'].abs().max()),
        float(dls), float(ref['dlog_sigma'])))
    close(dcol, ref['dcolour'], 2e-4, 2e-4, 'dcolour')
    close(dls, ref['dlog_sigma'], 2e-4, 1e-5, 'dlog_sigma')
    g2 = g.clone()
    g2[pad] = 1e30          # gradients that arrive in padded slots do nothing
    assert bool(pad.any()) and torch.equal(g2[~pad], g[~pad])
    dcol2, dls2 = run_backward(inp, kernel, K, fwd, g2, fwd['nsteps'])
    assert torch.equal(dcol, dcol2) and torch.equal(dls, dls2), what + ': a gradient in a padded slot reached dcolour or dlog_sigma'
    fwd2 = run_forward(inp, kernel, K, seed_idx=inp['seed_idx'], min_mass=r['min_mass'])
    same_bits(fwd, fwd2, what)


@gpu
def test_icsbp_function_hands_nsteps_to_its_backward():
    """functions.ICSBPFn with min_mass > 0 on a plain 1 x 1 colour head against autograd of the restatement composed with F.conv2d
    (float64).  The head's weight is a signed permutation: colour is feat permuted plus the bias and d feat is d colour permuted,
    exactly, so d feat carries dcolour's bound (2e-4 / 2e-4) and d log_sigma its own (2e-4 / 1e-5); the head's parameter gradients
    are compared with the float64 sums over the node's own d colour at test_conv1x1's 1e-4 / 1e-4."""
    from genesis_amd import functions as fn
    r = FN_ROW
    B, C, H, W, K = r['B'], r['C'], r['H'], r['W'], r['K']
    inp = dyn_inputs(r, 'gaussian', 'free')
    perm = torch.tensor([3, 0, 6, 1, 7, 2, 5, 4])
    sign = torch.tensor([1., -1., 1., 1., -1., 1., -1., -1.])
    w = torch.zeros(C, C)
    w[torch.arange(C), perm] = sign
    bias = rnd(C, seed=31, scale=0.5)
    feat = (sign.view(1, C, 1, 1) * (inp['colour'] - bias.view(1, C, 1, 1)))[:, torch.argsort(perm)]
    ls, g = inp['log_sigma'], inp['g']
    # the reference
    fr, wr, br = [t.double().requires_grad_() for t in (feat, w, bias)]
    col_ref = F.conv2d(fr, wr.view(C, C, 1, 1), br)
    assert float((col_ref.detach() - inp['colour'].double()).abs().max()) < 1e-6
    ref = R.icsbp(col_ref, ls, inp['rand'], K, 'gaussian', None, r['min_mass'], g)
    assert tuple(ref['nsteps'].tolist()) == r['nsteps'] and ref['margin_a'] >= MARGIN_A and ref['margin_b'] >= MARGIN_B
    dfeat_ref, = torch.autograd.grad(col_ref, fr, ref['dcolour'])
    # the node
    fd, wd, bd = [t.to(DEV).requires_grad_() for t in (feat, w.view(C, C, 1, 1), bias)]
    ld = ls.to(DEV).requires_grad_()
    log_m, log_s, colour, seeds, idx, nsteps = fn.ICSBPFn.apply(fd, wd, bd, None, None, ld, inp['rand'].to(DEV), K, 'gaussian', None,
                                                                r['min_mass'])
    assert nsteps.cpu().tolist() == ref['nsteps'].tolist() and torch.equal(idx.cpu(), ref['idx'])
    pad = R.padded(ref['nsteps'], K, H, W)
    assert bool((log_m.cpu()[pad] == -1e10).all())
    close(log_m.cpu()[~pad], ref['log_m'][~pad], 1e-5, 2e-5, 'log_m (unpadded entries)')
    g2 = g.clone()
    g2[pad] = 1e30
    dfeat, dw, db, dls = torch.autograd.grad((log_m * g2.to(DEV)).sum(), (fd, wd, bd, ld))
    assert all(bool(torch.isfinite(t).all()) for t in (dfeat, dw, db, dls))
    close(dfeat, dfeat_ref, 2e-4, 2e-4, 'dfeat')
    close(dls, ref['dlog_sigma'], 2e-4, 1e-5, 'dlog_sigma')
    dcol = torch.einsum('oc,bchw->bohw', w.double(), dfeat.cpu().double())          # W W^T = 1: d colour = W d feat
    close(db, dcol.sum((0, 2, 3)), 1e-4, 1e-4, 'db')
    close(dw.view(C, C), torch.einsum('bohw,bchw->oc', dcol, feat.double()), 1e-4, 1e-4, 'dw')

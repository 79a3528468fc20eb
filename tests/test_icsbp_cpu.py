"""Without a GPU: the float64 restatement of IC-SBP (tests/icsbp_restatement.py) against oracle/v2_oracle.py's ic_sbp, the
conditions tests/test_icsbp_plans_gpu.py puts on its inputs, and the dispatch every row of its tables declares against the
host code's formulas restated here (threads_for, the ppt switch, icsbp_bwd_threads and icsbp_bwd_finalize_kernel's chunk loop
in genesis_amd/csrc/gx_attention.hip), so that a typo in a table is found here and not on the GPU."""
import pytest
import torch

from oracle import v2_oracle as O
from tests import icsbp_restatement as R
from tests import test_icsbp_plans_gpu as T

F64 = torch.float64
KERNELS = ('gaussian', 'laplacian', 'epanechnikov')


# ---- the restatement against the oracle
def operands(B, C, H, W, K, seed=0):
    colour = T.ramp_image(B, C, H, W).double() + T.rnd(B, C, H, W, seed=seed + 1, scale=0.05).double()
    rand = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(seed + 2), dtype=F64)
    g = T.rnd(K, B, 1, H, W, seed=seed + 3).double()
    return colour, T.log_sigma_of(K), rand, g


@pytest.mark.parametrize('forced', [False, True])
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('B,C,H,W,K', [(3, 8, 8, 16, 6), (2, 3, 16, 8, 2), (1, 5, 8, 8, 4)])
def test_restatement_equals_the_oracle(B, C, H, W, K, kernel, forced):
    colour, ls, rand, g = operands(B, C, H, W, K)
    sidx = torch.randint(0, H * W, (K - 1, B), generator=torch.Generator().manual_seed(7)) if forced else None
    if forced:
        sidx[-1] = sidx[0]          # the same pixel drawn twice
    cr, lr = colour.clone().requires_grad_(), ls.clone().requires_grad_()
    log_m, log_s, seeds, idxs = O.ic_sbp(cr, lr, K - 1, rand, kernel, list(sidx) if forced else None)
    (torch.stack(log_m) * g).sum().backward()
    got = R.icsbp(colour, ls, rand, K, kernel, sidx, 0.0, g)
    assert torch.equal(got['idx'], torch.stack(idxs)) and torch.equal(got['seeds'], torch.stack(seeds).detach())
    assert got['nsteps'].tolist() == [K - 1] * B and got['margin_b'] == float('inf')
    assert (got['margin_c'] < float('inf')) == (kernel == 'epanechnikov')
    for name, mine, ref in (('log_m', got['log_m'], torch.stack(log_m)), ('log_s', got['log_s'], torch.stack(log_s)),
                            ('dcolour', got['dcolour'], cr.grad), ('dlog_sigma', got['dlog_sigma'], lr.grad)):
        assert mine.dtype == F64 and ref.dtype == F64
        err = float((mine - ref.detach()).abs().max())
        assert err <= 1e-12 * (1 + float(ref.detach().abs().max())), (name, err)
    # margin (a): the gap of the top two of rand * scope, recomputed from the oracle's scopes
    if not forced:
        for t in range(K - 1):
            v = (rand * log_s[t].detach().exp()).flatten(1)
            top = v.topk(2, dim=1).values
            assert torch.allclose(got['gap'][t], (top[:, 0] - top[:, 1]) / top[:, 0], rtol=1e-9, atol=0)


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('spec,n', [(T.HALF, 1), (T.TWO, 2), (T.FULL, 4)])
def test_restatement_equals_the_oracle_with_dynamic_k(spec, n, kernel):
    """dynamic_K=True (one image per call, min_mass = 20 as modules/attention.py:218-219 hard-codes): the oracle returns the n + 1
    masks of the steps that ran and the remaining scope; the restatement pads to K with -1e10."""
    K, H, W = 5, 32, 64
    colour, rid = T.dyn_image(spec, H, W, 60)
    colour = colour.unsqueeze(0).double()
    ls = T.log_sigma_of(K)
    inreg = (rid >= 0).view(1, 1, H, W)
    u = torch.rand(1, 1, H, W, generator=torch.Generator().manual_seed(3), dtype=F64)
    rand = torch.where(inreg, 0.5 + 0.5 * u, 0.5 * u)
    g = T.rnd(K, 1, 1, H, W, seed=4).double()
    cr, lr = colour.clone().requires_grad_(), ls.clone().requires_grad_()
    log_m, log_s, seeds, idxs = O.ic_sbp(cr, lr, K - 1, rand, kernel, None, dynamic_K=True)
    got = R.icsbp(colour, ls, rand, K, kernel, None, 20.0, g)
    nrun = len(log_m) - 1
    assert got['nsteps'].tolist() == [nrun] and nrun == n
    pad = R.padded(got['nsteps'], K, H, W)
    assert bool((got['log_m'][pad] == -1e10).all()) and int(pad.sum()) == (K - 1 - nrun) * H * W
    assert float((got['log_m'][:nrun + 1] - torch.stack(log_m).detach()).abs().max()) <= 1e-12 * (1 + float(torch.stack(log_m).abs().max()))
    assert float((got['log_s'][:nrun + 1] - torch.stack(log_s).detach()).abs().max()) <= 1e-10
    assert all(torch.equal(got['log_s'][t], got['log_m'][nrun]) for t in range(nrun + 1, K))
    nseed = len(idxs)           # (the oracle draws the seed of the step that stops, as the kernel does)
    assert nseed == min(nrun + 1, K - 1) and torch.equal(got['idx'][:nseed], torch.stack(idxs))
    assert not bool(got['idx'][nseed:].any()) and not bool(got['seeds'][nseed:].any())
    (torch.stack(log_m) * g[:nrun + 1]).sum().backward()
    assert float((got['dcolour'] - cr.grad).abs().max()) <= 1e-12 * (1 + float(cr.grad.abs().max()))
    assert abs(float(got['dlog_sigma'] - lr.grad)) <= 1e-12 * (1 + abs(float(lr.grad)))


def test_restatement_stops_per_image_and_at_k_1():
    """A batch stops image by image (the oracle cannot: it asserts B == 1), and K = 1 is one mask of zeros with zero gradients."""
    r = T.DYN_ROWS[1]
    inp = T.dyn_inputs(r, 'gaussian', 'free')
    for b in range(r['B']):
        one = R.icsbp(inp['colour'][b:b + 1], inp['log_sigma'], inp['rand'][b:b + 1], r['K'], 'gaussian', None, r['min_mass'], inp['g'][:, b:b + 1])
        assert one['nsteps'].tolist() == [r['nsteps'][b]]
        assert torch.equal(one['log_m'][:, 0], inp['ref']['log_m'][:, b]) and torch.equal(one['dcolour'][0], inp['ref']['dcolour'][b])
    colour, ls, rand, g = operands(2, 8, 8, 8, 1)
    got = R.icsbp(colour, ls, rand, 1, 'gaussian', None, 0.0, g)
    assert got['log_m'].shape == (1, 2, 1, 8, 8) and not bool(got['log_m'].any()) and not bool(got['log_s'].any())
    assert not bool(got['dcolour'].any()) and float(got['dlog_sigma']) == 0.0 and got['seeds'].shape == (0, 2, 8)
    assert got['margin_a'] == got['margin_b'] == got['margin_c'] == float('inf')


# ---- the GPU file's tables
def test_icsbp_table_meets_its_conditions():
    T.test_icsbp_table_meets_its_conditions()


def mirror_threads_for(HW):
    return max(min(HW, 1024), 64)


def mirror_forward(HW):
    """-> (T, ppt, the template argument GX_ICSBP_LAUNCH picks)."""
    t = mirror_threads_for(HW)
    ppt = HW // t if HW % t == 0 else 0
    return t, ppt, ppt if ppt in (1, 2, 4) else 0


def mirror_backward(HW):
    t = HW if HW < 256 else 256
    return t, -(-HW // t)


def mirror_finalize(nch):
    """The chunk loop of icsbp_bwd_finalize_kernel for each of the four thread quarters -> (loop rounds, quarters whose tail runs)."""
    rounds, tail = set(), []
    for q in range(4):
        ch, n = q, 0
        while ch + 4 < nch:
            ch += 8
            n += 1
        rounds.add(n)
        if ch < nch:
            tail.append(q)
    assert len(rounds) == 1          # (every power-of-two chunk count gives all four quarters the same number of rounds)
    return rounds.pop(), tuple(tail)


@pytest.mark.parametrize('r', T.ALL_ROWS, ids=lambda r: r['id'])
def test_declared_dispatch_is_what_the_host_code_derives(r):
    HW = r['H'] * r['W']
    assert HW & (HW - 1) == 0 and 64 <= HW <= 16384 and 1 <= r['C'] <= 8 and 1 <= r['K'] <= 17 and r['B'] in (1, 2, 3)
    fT, ppt, inst = mirror_forward(HW)
    assert (r['fT'], r['inst']) == (fT, inst) and ppt == HW // fT
    assert (r['bT'], r['nch']) == mirror_backward(HW)
    assert (r['rounds'], r['tail']) == mirror_finalize(r['nch'])
    assert r['B'] * r['C'] * HW * 4 <= 1 << 20


def test_ids_are_unique_and_no_row_was_removed():
    ids = [r['id'] for r in T.ALL_ROWS]
    assert len(ids) == len(set(ids))
    assert (len(T.VALUE_ROWS), len(T.VALUE_CASES), len(T.FORCED_CASES), len(T.DYN_ROWS), len(T.DYN_CASES)) == (11, 38, 4, 6, 20)
    assert (T.MARGIN_A, T.MARGIN_B, T.MARGIN_C) == (1e-4, 0.05, 1e-4)

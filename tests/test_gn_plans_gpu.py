"""GroupNorm + ReLU (genesis_amd/csrc/gx_norm.hip) plan by plan: every kernel family, register plan, thread class and view mode
the host dispatch (gn_plan_fwd, gn_plan_bwd, plan_reg, small_threads, proj_split_ok) can pick, reached by the smallest
shape that reaches it.  One table per entry point; every row DECLARES the plan it is meant to reach and the test asserts that
hip_ops.gn_last_plan() -- the record the launcher writes just before it launches -- equals the declaration, so a row that
drifts to another kernel fails the TABLE, and equals what the plan query (hip_ops.gn_fwd_plan / gn_bwd_plan) answers for the
arguments of that launch.  tests/test_gn_plans_cpu.py holds the written enumeration these tables must cover.

Every case
  1. calls the C ABI through _lib.call on buffers the test owns,
  2. fills every output with NaN beforehand (dy, dgamma / dbeta / dbias, mean, rstd, both destination buffers, y_sum, wpart,
     bpart, the workspace): an element no workgroup wrote fails the comparison, whatever the allocator handed out,
  3. makes destination buffers wider than the view: their other channels must still be NaN afterwards,
  4. compares with F.relu(F.group_norm(...)) and autograd in float64 on the CPU (views: F.interpolate(mode='nearest') and channel
     slices of a torch.cat buffer; the projected backward: the 1x1 conv as F.conv2d), PER (image, group) SLAB for tensors and per
     group's channel block for the [C] gradients, so that a wrong slab of small values cannot hide behind another slab's maximum.

Inputs: y = rnd * 2 + 0.3 as tests/test_kernel_edges_gpu.py's gn_operands.  A ReLU decision that differs between fp32 and fp64
changes dy by a whole term, so wherever the fp64 pre-activation xhat * gamma + beta lies within MARGIN = 1e-4 of zero that element
of y is moved by NUDGE = 0.01 away from zero and everything is recomputed (build_inputs); at most 3 passes, at most 1e-3 of the
elements (asserted per row, on the CPU too).

Bounds (none derived from the kernels):
  mean      |mean - ref| <= 2^-23 |ref| + 1e-9 max|y|        (fp64 accumulation, one rounding)
  rstd      relative error <= 2^-23 + m 2^-52 E[y^2] / var    (the share of the one-pass fp64 variance; the rows with
                                                               y = 1000 + 0.5 rnd are there for this formula)
  forward   1e-5 / 1e-5, dy 1e-4 / 1e-5, dgamma / dbeta / dbias 1e-4 / 1e-4, wpart / bpart 1e-4 / 1e-4 (rtol / atol: the project's
            bars, tests/test_kernels_gpu.py), applied per slab.  Where torch's own fp32 CPU autograd of the row differs from the
            fp64 one by more than a quarter of a slab's bar, that slab's bar is four times that fp32 error (printed).

What the rows would catch (one-line mistakes in the code they reach; the first was run on a scratch build, the rest are argued):

  views on H != W planes, both orders               H for W in a row stride of store_view* / load_view* (2 * H for 2 * W in load_view4's
                                                    mode 1 fails every mode-1 backward row of the 16-byte kernels)
  cpg 12, 20 on the two-pass backward               the `cl < cpg` guard of a ragged GCH block dropped: the next slab's dy and part[]
                                                    written with this slab's statistics (NaN-free but wrong), the last slab out of bounds
  <F, UPW> and P rows                               a unit -> (channel, part) map that assumes P == 1 or UPW == 1, uab / usd indexed by wave
  N * groups = 1, 3, 5, 7, 9, 17                    a gx_xcd_tile that is no bijection when the grid is no multiple of 8: a slab nobody
                                                    wrote stays NaN
  small kernel with idle threads, m = 4096          `act` missing on a load or a store, the per-channel LDS sums walking the idle tail
  stage kernel at F = 8, stage = 128 KB             KEEP = false re-reading y with the other offset, the dynamic LDS attribute below the stage
  chunked path, cpg 3, Cout 5, two chunks           the chunk record's 8-wide rows indexed by cpg or Cout, `chunks` taken as 4
  deferred reduce                                   a clash round that drops or repeats a record (three different calls share a destination), an
                                                    immediate reduce that overwrites (two of them come after the queue is full)
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F64 = torch.float64
EPS = 1e-5
NAN = float('nan')
MARGIN, NUDGE, MAX_PASSES, MAX_MOVED = 1e-4, 0.01, 3, 1e-3
FIELDS = ('kernel', 'vec', 'F', 'UPW', 'P', 'threads', 'grid', 'lds', 'CT', 'KEEP', 'WP', 'chunks', 'nsplit0', 'nsplit1', 'nsplit_in')


# ===================================================================================================== the case tables
def plan(kernel, **fields):
    """A whole gx_gn_last_plan record: the fields named, every other one 0."""
    assert set(fields) <= set(FIELDS), fields
    return dict(dict.fromkeys(FIELDS, 0), kernel=kernel, **fields)


def REG(F_, UPW, P, threads):
    return dict(family='reg', vec=1, F=F_, UPW=UPW, P=P, fthreads=threads, bthreads=threads)


def SMALL(threads):
    return dict(family='small', vec=1, F=0, UPW=0, P=0, fthreads=threads, bthreads=threads)


def TWOPASS(vec, fthreads, bthreads):
    return dict(family='twopass', vec=vec, F=0, UPW=0, P=0, fthreads=fthreads, bthreads=bthreads)


def R(rid, cpg, H, W, N, groups, cls, tails=()):
    return dict(id=rid, cpg=cpg, H=H, W=W, N=N, groups=groups, cls=cls, tails=frozenset(tails))


def fwd_plan(r, nsplit_in=1):
    c = r['cls']
    return plan('fwd_' + c['family'], vec=c['vec'], F=c['F'], UPW=c['UPW'], P=c['P'], threads=c['fthreads'],
                grid=r['N'] * r['groups'], nsplit_in=nsplit_in)


def bwd_plan(r, nsplit0=1, nsplit1=0):
    c = r['cls']
    return plan('bwd_' + c['family'], vec=c['vec'], F=c['F'], UPW=c['UPW'], P=c['P'], threads=c['bthreads'],
                grid=r['N'] * r['groups'], nsplit0=nsplit0, nsplit1=nsplit1)


# ---- gx_gn_relu_fwd and gx_gn_relu_bwd (one plain gradient source): the same rows serve both.  N * groups (the grid of the
# backward register kernels, whose gx_xcd_tile remaps blockIdx.x) takes 1, 3, 5, 7, 9 and 17 as well as multiples of 8; the prime
# counts need N or groups beyond 3.  The largest operand is 1 MB.
ROWS = [
    R('reg-f1u1-cpg2-8x32-grid17', 2, 8, 32, 17, 1, REG(1, 1, 1, 128)),
    R('reg-f1u2-cpg32-16x16-grid9', 32, 16, 16, 3, 3, REG(1, 2, 1, 1024)),
    R('reg-f2u1-cpg4-32x16-grid5', 4, 32, 16, 1, 5, REG(2, 1, 1, 256)),
    R('reg-f2u2-cpg32-16x32-grid7', 32, 16, 32, 7, 1, REG(2, 2, 1, 1024)),
    R('reg-f4u1-cpg16-32x32-grid3', 16, 32, 32, 1, 3, REG(4, 1, 1, 1024)),
    R('reg-f4u2-cpg32-64x16-grid1', 32, 64, 16, 1, 1, REG(4, 2, 1, 1024)),
    R('reg-f8p1-cpg16-32x64-grid8', 16, 32, 64, 4, 2, REG(8, 1, 1, 1024)),
    R('reg-f8p2-cpg4-128x32-grid6', 4, 128, 32, 2, 3, REG(8, 1, 2, 512)),
    R('reg-f8p4-cpg4-64x128-grid2', 4, 64, 128, 1, 2, REG(8, 1, 4, 1024)),
    R('reg-f8p8-cpg2-128x128-grid3', 2, 128, 128, 3, 1, REG(8, 1, 8, 1024)),
    R('reg-f8p16-cpg1-128x256-grid5', 1, 128, 256, 5, 1, REG(8, 1, 16, 1024)),
    R('small-cpg3-4x4-12-of-64-threads', 3, 4, 4, 2, 3, SMALL(64), {'idle_threads'}),
    R('small-cpg5-4x8', 5, 4, 8, 3, 2, SMALL(64), {'idle_threads'}),
    R('small-cpg8-8x16-256-threads', 8, 8, 16, 1, 3, SMALL(256)),
    R('small-cpg64-8x8-1024-threads-m4096', 64, 8, 8, 2, 1, SMALL(1024)),
    R('small-cpg4-4x4-n130-param-reduce-256', 4, 4, 4, 130, 1, SMALL(64), {'reduce_256'}),
    R('twopass-cpg3-16x16-f256-b64', 3, 16, 16, 2, 2, TWOPASS(1, 256, 64)),
    R('twopass-cpg3-32x32-f512-b256', 3, 32, 32, 1, 3, TWOPASS(1, 512, 256)),
    R('twopass-cpg12-64x64-f1024-b1024-ragged-second-block', 12, 64, 64, 2, 2, TWOPASS(1, 1024, 1024), {'gch_ragged'}),
    R('twopass-cpg20-16x16-three-blocks', 20, 16, 16, 3, 1, TWOPASS(1, 512, 64), {'gch_ragged', 'gch_three'}),
    R('twopass-cpg64-16x16-pow2-refused-by-plan-reg', 64, 16, 16, 1, 2, TWOPASS(1, 1024, 64), {'reg_refused'}),
    R('twopass-cpg128-4x4-not-small', 128, 4, 4, 2, 1, TWOPASS(1, 512, 64), {'small_refused'}),
    R('twopass-scalar-cpg2-2x2', 2, 2, 2, 3, 3, TWOPASS(0, 256, 64)),
    R('twopass-scalar-cpg3-8x2', 3, 8, 2, 2, 2, TWOPASS(0, 256, 64)),
    R('twopass-scalar-cpg8-1024x2-f1024', 8, 1024, 2, 1, 2, TWOPASS(0, 1024, 256)),
]
ROW = {r['id']: r for r in ROWS}

# ---- statistics under cancellation: y = 1000 + 0.5 rnd, statistics-only launches (the rstd bound is what is being checked)
OFFSET_ROWS = [
    R('offset-reg-f4u1-cpg16-32x32', 16, 32, 32, 1, 3, REG(4, 1, 1, 1024)),
    R('offset-twopass-cpg12-64x64', 12, 64, 64, 2, 2, TWOPASS(1, 1024, 1024)),
]

# ---- destination / source views on rectangular planes, both orders where the family allows it (the scalar kernels need W = 2)
VIEW_ROWS = [
    R('view-reg-cpg4-32x16', 4, 32, 16, 1, 5, REG(2, 1, 1, 256)),
    R('view-reg-cpg4-16x32', 4, 16, 32, 3, 1, REG(2, 1, 1, 256)),
    R('view-small-cpg5-4x8', 5, 4, 8, 3, 2, SMALL(64)),
    R('view-small-cpg5-8x4', 5, 8, 4, 2, 3, SMALL(64)),
    R('view-twopass-cpg3-16x32', 3, 16, 32, 2, 2, TWOPASS(1, 256, 64)),
    R('view-twopass-cpg3-32x16', 3, 32, 16, 1, 3, TWOPASS(1, 256, 64)),
    R('view-scalar-cpg3-8x2', 3, 8, 2, 2, 2, TWOPASS(0, 256, 64)),
]
VIEW_CASES = [(r, mode) for r in VIEW_ROWS for mode in (1, 2)]

# ---- partial slabs: one row of each family
PART_ROWS = [ROW['reg-f2u1-cpg4-32x16-grid5'], ROW['small-cpg5-4x8'], ROW['twopass-cpg3-16x16-f256-b64'],
             ROW['twopass-scalar-cpg3-8x2']]
PART_FWD_CASES = [(r, ns, b) for r in PART_ROWS for ns in (1, 2, 3) for b in (False, True)]
PART_BWD_CASES = [(r, ns, mode) for r in PART_ROWS for ns in (2, 3) for mode in (0, 1, 2)]


# ---- gx_gn_relu_bwd_proj
def PR(rid, cpg, H, W, N, groups, Cout, kernel, wps, gate=False, **fields):
    """kernel / fields: the declared record (grid, vec and WP are filled in per case); wps: the wpart / bpart settings to run."""
    return dict(id=rid, cpg=cpg, H=H, W=W, N=N, groups=groups, Cout=Cout, kernel=kernel, wps=tuple(wps), gate=gate, fields=fields)


def STAGE(F_, P, Cout, HW):
    return dict(F=F_, UPW=1, P=P, threads=1024, lds=Cout * HW * 4, CT=4, KEEP=int(F_ < 8))


PROJ_ROWS = [
    # gn_relu_bwd_stage_kernel<F, 4, WP, KEEP>: one unit per wave, 1024 threads, Cout == 4
    PR('stage-f1-cpg16-16x16-grid9', 16, 16, 16, 3, 3, 4, 'bwd_stage', (0, 1), **STAGE(1, 1, 4, 256)),
    PR('stage-f2-cpg16-16x32-grid7-gate', 16, 16, 32, 1, 7, 4, 'bwd_stage', (0, 1), gate=True, **STAGE(2, 1, 4, 512)),
    PR('stage-f4-cpg16-32x32-grid5', 16, 32, 32, 5, 1, 4, 'bwd_stage', (0, 1), **STAGE(4, 1, 4, 1024)),
    PR('stage-f8-cpg16-32x64-grid3', 16, 32, 64, 1, 3, 4, 'bwd_stage', (0, 1), **STAGE(8, 1, 4, 2048)),
    PR('stage-f8-cpg4-64x128-grid8-128k-boundary-gate', 4, 64, 128, 2, 4, 4, 'bwd_stage', (0, 1), gate=True, **STAGE(8, 4, 4, 8192)),
    # gn_relu_bwd_reg_kernel<F, UPW, true>: UPW = 2, fewer than 1024 threads, Cout != 4
    PR('staged-upw2-cpg32-16x16-cout4', 32, 16, 16, 1, 3, 4, 'bwd_reg_staged', (1,), F=1, UPW=2, P=1, threads=1024, lds=4 * 256 * 4),
    PR('staged-256-threads-cpg4-32x32-cout3', 4, 32, 32, 3, 3, 3, 'bwd_reg_staged', (0,), F=4, UPW=1, P=1, threads=256,
       lds=3 * 1024 * 4),
    PR('staged-cout8-cpg16-32x32', 16, 32, 32, 1, 5, 8, 'bwd_reg_staged', (1,), F=4, UPW=1, P=1, threads=1024, lds=8 * 1024 * 4),
    # gn_relu_bwd_reg_kernel<F, UPW, false> with a mode-3 source: 8 x 8192 x 4 = 256 KB does not stage
    PR('reg-mode3-cpg4-64x128-cout8-unstaged', 4, 64, 128, 1, 2, 8, 'bwd_reg', (0,), F=8, UPW=1, P=4, threads=1024),
    PR('small-mode3-cpg8-8x8-cout3', 8, 8, 8, 2, 3, 3, 'bwd_small', (0,), threads=128),
    PR('twopass-mode3-cpg3-16x16-cout2', 3, 16, 16, 2, 2, 2, 'bwd_twopass', (0,), threads=64),
    # gn_bwd_proj_split_*: 4096-pixel chunks
    PR('split-two-chunks-cpg8-64x128-cout4', 8, 64, 128, 1, 2, 4, 'bwd_split', (0, 1), threads=256, CT=4, chunks=2),
    PR('split-cpg3-64x128-cout5-ct8-gate', 3, 64, 128, 1, 3, 5, 'bwd_split', (1,), gate=True, threads=256, CT=8, chunks=2),
    PR('split-four-chunks-cpg4-128x128-cout1', 4, 128, 128, 2, 1, 1, 'bwd_split', (0, 1), threads=256, CT=4, chunks=4),
]
PROJ_CASES = [(r, wp) for r in PROJ_ROWS for wp in r['wps']]


def proj_plan(r, wp):
    chunks = r['fields'].get('chunks', 0)
    return plan(r['kernel'], vec=1, grid=r['N'] * r['groups'] * max(chunks, 1), WP=wp, **r['fields'])


TABLES = {'rows': ROWS, 'offset': OFFSET_ROWS, 'views': VIEW_ROWS, 'parts': PART_ROWS, 'proj': PROJ_ROWS}
INPUT_ROWS = ROWS + VIEW_ROWS + PROJ_ROWS          # every shape build_inputs serves (the offset rows check statistics only)

# ---- deferred parameter reduce: (C, groups) of the queued calls, N = 2, 4 x 4 planes; SHARED calls write one set of buffers
DEFER_SHAPES = [(8, 2), (16, 2), (24, 2)]
DEFER_ROUNDS = {'two-tables-and-clash-rounds': (50, (3, 20, 49)), 'queue-overflow': (131, (5, 128, 129))}

# ---- refusals the host decides before it touches the device: (entry point, what is wrong, message)
REFUSALS = [
    ('gx_gn_relu_bwd_proj', 'wpart on a small-kernel shape', 'fused 1x1 weight gradient unsupported'),
    ('gx_gn_relu_bwd_proj', 'wpart on an unstaged register shape', 'fused 1x1 weight gradient unsupported'),
    ('gx_gn_relu_bwd_proj', 'wpart on a chunked shape with the plain workspace', 'fused 1x1 weight gradient unsupported'),
    ('gx_gn_relu_bwd_proj', 'workspace below the query', 'workspace too small'),
    ('gx_gn_relu_fwd_parts', 'nsplit = 0', 'nsplit must be >= 1'),
    ('gx_gn_relu_fwd_parts', 'bias without y_sum', 'y_sum is required'),
    ('gx_gn_relu_bwd_parts', 'nsplit = 0', 'nsplit >= 1'),
]
# gx_gn_relu_bwd_proj_fuses_wgrad(C, H, W, groups, Cout) == 0 / != 0
NOT_FUSED = [(8, 64, 128, 2, 8), (24, 8, 8, 3, 3), (6, 16, 16, 2, 2), (8, 6, 8, 2, 4)]
FUSED = [(16, 64, 128, 4, 4), (16, 64, 128, 2, 4), (9, 64, 128, 3, 5), (48, 16, 16, 3, 4)]


def check_refusal(name, what):
    """One REFUSALS entry.  The host refuses before it touches any pointer: without a GPU every pointer is a non-null dummy; with
    one, every pointer is the same 4 MB device buffer (larger than any operand here), so that a refusal that stopped refusing
    fails this test and not the device."""
    import re
    from genesis_amd import _lib
    if torch.cuda.is_available():
        arena = torch.full((1 << 20,), NAN, dtype=torch.float32, device=DEV)
        d = ctypes.c_void_p(arena.data_ptr())
    else:
        d = ctypes.c_void_p(16)
    message = [m for n, w, m in REFUSALS if (n, w) == (name, what)][0]
    with pytest.raises(_lib.GenesisHipError, match=re.escape(message)):
        if name == 'gx_gn_relu_bwd_proj':
            N, C, H, W, groups, Cout = {'wpart on a small-kernel shape': (2, 24, 8, 8, 3, 3),
                                        'wpart on an unstaged register shape': (1, 8, 64, 128, 2, 8),
                                        'wpart on a chunked shape with the plain workspace': (1, 16, 64, 128, 2, 4),
                                        'workspace below the query': (1, 16, 64, 128, 2, 4)}[what]
            nb = _lib.query('gx_gn_relu_bwd_proj_ws_bytes', N, C, H, W, groups, Cout)
            wp = None
            if what.startswith('wpart'):
                wp = d
                if 'plain workspace' in what:
                    assert nb > _lib.query('gx_gn_relu_bwd_ws_bytes', N, C)
                    nb = _lib.query('gx_gn_relu_bwd_ws_bytes', N, C)
            else:
                nb = _lib.query('gx_gn_relu_bwd_ws_bytes', N, C) - 4
            _lib.call(name, d, d, d, d, d, N, C, H, W, groups, d, Cout, d, None, d, d, d, d, wp, wp, d, nb, None)
        elif name == 'gx_gn_relu_fwd_parts':
            ns, bias, ysum = (0, None, d) if what == 'nsplit = 0' else (1, d, None)
            _lib.call(name, d, ns, 0, bias, ysum, d, d, 1, 8, 8, 8, 2, EPS, d, 8, 0, 0, None, 0, 0, 0, d, d, None)
        else:
            _lib.call(name, d, d, d, d, d, 1, 8, 8, 8, 2, d, 8, 0, 0, 0, 0, None, 0, 0, 0, 1, 0, d, d, d, d, d, 1 << 20, None)


# ===================================================================================================== inputs and references (CPU)
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def pre_activation(y, gamma, beta, groups):
    """xhat * gamma + beta in float64."""
    return F.group_norm(y.double(), groups, gamma.double(), beta.double(), EPS)


@functools.lru_cache(maxsize=None)
def build_inputs(cpg, H, W, N, groups):
    """y, gamma, beta (fp32, CPU) with no fp64 pre-activation within MARGIN of zero, and what the nudging did."""
    C = cpg * groups
    y = rnd(N, C, H, W, seed=8, scale=2.0) + 0.3
    gamma, beta = 1 + 0.3 * rnd(C, seed=9), 0.2 * rnd(C, seed=10)
    moved = torch.zeros_like(y, dtype=torch.bool)
    passes = 0
    while True:
        pre = pre_activation(y, gamma, beta, groups)
        near = pre.abs() < MARGIN
        if not bool(near.any()) or passes == MAX_PASSES:
            break
        # d pre / d y has the sign of gamma: move y so that pre moves away from zero
        direction = torch.where(pre >= 0, 1.0, -1.0) * torch.sign(gamma.double()).view(1, C, 1, 1)
        y = torch.where(near, y + NUDGE * direction.float(), y)
        moved |= near
        passes += 1
    return dict(y=y, gamma=gamma, beta=beta, passes=passes, near=int(near.sum()), moved=float(moved.float().mean()))


def inputs_of(r):
    inp = build_inputs(r['cpg'], r['H'], r['W'], r['N'], r['groups'])
    assert inp['near'] == 0 and inp['passes'] <= MAX_PASSES and inp['moved'] <= MAX_MOVED, (r['id'], inp['passes'], inp['near'], inp['moved'])
    return inp


def stats64(y, groups):
    N = y.shape[0]
    v = y.double().reshape(N * groups, -1)
    mean, var = v.mean(1), v.var(1, unbiased=False)
    return mean, 1.0 / torch.sqrt(var + EPS), var, (v * v).mean(1), v.shape[1]


def resample(a, mode):
    """What a mode-`mode` view holds of a: a itself, its nearest-neighbour 2x enlargement, or a[..., ::2, ::2]."""
    return a if mode == 0 else F.interpolate(a, scale_factor=2.0 if mode == 1 else 0.5, mode='nearest')


def view_shape(N, ctot, H, W, mode):
    return (N, ctot, H, W) if mode == 0 else ((N, ctot, 2 * H, 2 * W) if mode == 1 else (N, ctot, H // 2, W // 2))


def reference(inp, groups, dtype, sources=(), proj=None):
    """relu(gn(y)) and, for gradient sources [(G [N,ctot,Hd,Wd], c0, mode)] or a following 1x1 conv proj = (g_out, w, gate), the
    gradients by autograd; everything in `dtype`."""
    y, gm, bt = (inp[k].detach().clone().to(dtype).requires_grad_(True) for k in ('y', 'gamma', 'beta'))
    C = y.shape[1]
    a = F.relu(F.group_norm(y, groups, gm, bt, EPS))
    out = dict(a=a.detach())
    loss = None
    for G, c0, mode in sources:
        t = (resample(a, mode) * G[:, c0:c0 + C].to(dtype)).sum()
        loss = t if loss is None else loss + t
    if proj is not None:
        g_out, w, gate = proj
        o = F.conv2d(a, w.to(dtype)[:, :, None, None])
        loss = ((o if gate is None else o * gate.to(dtype)) * g_out.to(dtype)).sum()
        out['wpart'] = torch.einsum('nqp,ncp->nqc', g_out.to(dtype).flatten(2), a.detach().flatten(2))
        out['bpart'] = g_out.to(dtype).flatten(2).sum(2)
    if loss is not None:
        dy, dg, db = torch.autograd.grad(loss, (y, gm, bt))
        out.update(dy=dy, dgamma=dg, dbeta=db, dbias=dy.sum((0, 2, 3)))
    return out


def slab_close(got, ref, ref32, blocks, rtol, atol, what):
    """|got - ref| <= atol + rtol max|ref| within each of `blocks` equal leading blocks; NaN in got fails.  ref32 (the same
    quantity by torch in fp32 on the CPU): a block whose fp32 error exceeds a quarter of its bar gets four times that error."""
    g = got.detach().cpu().double().reshape(blocks, -1)
    r = ref.detach().double().reshape(blocks, -1)
    bar = atol + rtol * r.abs().amax(1)
    if ref32 is not None:
        e32 = (ref32.detach().double().reshape(blocks, -1) - r).abs().amax(1)
        wide = e32 > bar / 4
        if bool(wide.any()):
            print('%s: fp32 CPU torch errs by up to %.3e against a bar of %.3e in %d of %d blocks: their bar is 4x that error'
                  % (what, float(e32[wide].max()), float(bar[wide].min()), int(wide.sum()), blocks))
            bar = torch.where(wide, 4 * e32, bar)
    err = (g - r).abs().amax(1)
    ok = err <= bar
    print('%s: worst block err / bar = %.3f' % (what, float((err / bar).nan_to_num(nan=float('inf')).max())))
    assert bool(ok.all()), '%s: %d of %d blocks off; first block %d: err %.3e, bar %.3e' % (
        what, int((~ok).sum()), blocks, int((~ok).nonzero()[0]), float(err[~ok][0]), float(bar[~ok][0]))


def check_stats(mean, rstd, y, groups, what):
    mref, rref, var, ey2, m = stats64(y, groups)
    merr = (mean.cpu().double() - mref).abs()
    mbar = 2.0 ** -23 * mref.abs() + 1e-9 * float(y.abs().max())
    rerr = (rstd.cpu().double() - rref).abs() / rref
    rbar = 2.0 ** -23 + m * 2.0 ** -52 * ey2 / var
    print('%s: mean err / bar %.3f, rstd err / bar %.3f' % (what, float((merr / mbar).nan_to_num(nan=float('inf')).max()),
                                                          float((rerr / rbar).nan_to_num(nan=float('inf')).max())))
    assert bool((merr <= mbar).all()), '%s: mean off by %.3e (bar %.3e)' % (what, float(merr.max()), float(mbar.min()))
    assert bool((rerr <= rbar).all()), '%s: rstd off by %.3e relative (bar %.3e)' % (what, float(rerr.max()), float(rbar.min()))


# ===================================================================================================== device plumbing
def dnan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def dev(t):
    return t.to(device=DEV, dtype=torch.float32).contiguous()


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    from genesis_amd import hip_ops
    return hip_ops._stream()


def last_plan(query, *args, **kw):
    """The record of the launch just made, which must be what the plan query (hip_ops.gn_fwd_plan / gn_bwd_plan) answers for the
    arguments of that launch."""
    from genesis_amd import hip_ops
    got, would = hip_ops.gn_last_plan(), getattr(hip_ops, query)(*args, **kw)
    assert got == would, (query, args, kw, got, would)
    return got


def dview(v):
    """(buffer [N, ctot, Hd, Wd], c0, mode) or None -> the four C arguments of a destination / source view."""
    return [None, 0, 0, 0] if v is None else [ptr(v[0]), int(v[0].shape[1]), int(v[1]), int(v[2])]


def run_fwd(r, y, gamma, beta, d0, d1, parts=None):
    """-> mean, rstd, the launch's record.  parts = (slabs, nsplit, stride, bias, y_sum): gx_gn_relu_fwd_parts."""
    from genesis_amd import _lib
    N, C, H, W, groups = r['N'], r['cpg'] * r['groups'], r['H'], r['W'], r['groups']
    mean, rstd = dnan(N * groups), dnan(N * groups)
    tail = [ptr(gamma), ptr(beta), N, C, H, W, groups, EPS] + dview(d0) + dview(d1) + [ptr(mean), ptr(rstd), _stream()]
    if parts is None:
        _lib.call('gx_gn_relu_fwd', ptr(y), *tail)
    else:
        slabs, nsplit, stride, bias, ysum = parts
        _lib.call('gx_gn_relu_fwd_parts', ptr(slabs), nsplit, stride, ptr(bias), ptr(ysum), *tail)
    return mean, rstd, last_plan('gn_fwd_plan', N, C, H, W, groups, 1 if parts is None else parts[1])


def nan_workspace(nbytes):
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device=DEV)        # (read as floats: NaN)


def run_bwd(r, y, gamma, beta, mean, rstd, s0, s1=None):
    """s = (buffer, c0, mode, nsplit, stride[, ctot]) -> dy, dgamma, dbeta, dbias, the launch's record (gx_gn_relu_bwd_parts; nsplit 1:
    what gx_gn_relu_bwd passes)."""
    from genesis_amd import _lib
    N, C, H, W, groups = r['N'], r['cpg'] * r['groups'], r['H'], r['W'], r['groups']
    dy, dg, db, dbias = dnan(N, C, H, W), dnan(C), dnan(C), dnan(C)
    nb = _lib.query('gx_gn_relu_bwd_ws_bytes', N, C)
    ws = nan_workspace(nb)

    def src(s):
        if s is None:
            return [None, 0, 0, 0, 1, 0]
        ctot = s[5] if len(s) > 5 else s[0].shape[1]          # (a buffer of slabs is flat: its channel count comes along)
        return [ptr(s[0]), int(ctot), int(s[1]), int(s[2]), int(s[3]), int(s[4])]
    _lib.call('gx_gn_relu_bwd_parts', ptr(y), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd), N, C, H, W, groups, *src(s0), *src(s1),
              ptr(dy), ptr(dg), ptr(db), ptr(dbias), ptr(ws), nb, _stream())
    return dy, dg, db, dbias, last_plan('gn_bwd_plan', N, C, H, W, groups, g0_mode=s0[2], g0_ctot=src(s0)[1], g0_nsplit=s0[3],
                                        g1_nsplit=s1[3] if s1 else 0, ws_bytes=nb)


def check_grads(r, got, ref, ref32, what, dy_rtol=1e-4, dy_atol=1e-5):
    N, groups = r['N'], r['groups']
    dy, dg, db, dbias = got
    slab_close(dy, ref['dy'], ref32['dy'], N * groups, dy_rtol, dy_atol, what + ' dy')
    for name, t in (('dgamma', dg), ('dbeta', db), ('dbias', dbias)):
        slab_close(t, ref[name], ref32[name], groups, 1e-4, 1e-4, '%s %s' % (what, name))


def wide_view(N, C, H, W, mode, lo, hi):
    """A NaN destination / source buffer of lo + C + hi channels for a mode-`mode` view of an [N, C, H, W] tensor."""
    return dnan(*view_shape(N, lo + C + hi, H, W, mode))


def check_dest(buf, c0, C, ref, ref32, blocks, what):
    """The view's channels against ref, every other channel of the buffer still NaN."""
    assert bool(torch.isnan(buf[:, :c0]).all()) and bool(torch.isnan(buf[:, c0 + C:]).all()), what + ': a channel outside the view was written'
    slab_close(buf[:, c0:c0 + C].contiguous(), ref, ref32, blocks, 1e-5, 1e-5, what)


# ===================================================================================================== forward and plain backward
@functools.lru_cache(maxsize=None)
def _plain_reference(rid):
    r = ROW[rid]
    inp = inputs_of(r)
    N, C, H, W = inp['y'].shape
    G = rnd(N, C, H, W, seed=11)
    return inp, G, reference(inp, r['groups'], F64, [(G.double(), 0, 0)]), reference(inp, r['groups'], torch.float32, [(G, 0, 0)])


@pytest.mark.parametrize('r', ROWS, ids=[r['id'] for r in ROWS])
def test_forward_row(r):
    """gx_gn_relu_fwd into a channel slice of a wider NaN buffer, then the statistics-only launch (dst0 = NULL): the same record,
    the same mean / rstd bits."""
    inp, _, ref, ref32 = _plain_reference(r['id'])
    N, C, H, W, groups = r['N'], r['cpg'] * r['groups'], r['H'], r['W'], r['groups']
    y, gamma, beta = dev(inp['y']), dev(inp['gamma']), dev(inp['beta'])
    d0 = wide_view(N, C, H, W, 0, 2, 1)
    mean, rstd, got = run_fwd(r, y, gamma, beta, (d0, 2, 0), None)
    assert got == fwd_plan(r), (got, fwd_plan(r))
    check_stats(mean, rstd, inp['y'], groups, r['id'])
    check_dest(d0, 2, C, ref['a'], ref32['a'], N * groups, r['id'] + ' out')
    mean2, rstd2, got2 = run_fwd(r, y, gamma, beta, None, None)
    assert got2 == fwd_plan(r), (got2, fwd_plan(r))
    assert torch.equal(mean2, mean) and torch.equal(rstd2, rstd)


@pytest.mark.parametrize('r', OFFSET_ROWS, ids=[r['id'] for r in OFFSET_ROWS])
def test_statistics_of_a_large_offset(r):
    """y = 1000 + 0.5 rnd: E[y^2] / var ~ 1e7, the one-pass fp64 variance's share of the rstd bound."""
    N, C, H, W, groups = r['N'], r['cpg'] * r['groups'], r['H'], r['W'], r['groups']
    y = 1000 + 0.5 * rnd(N, C, H, W, seed=8)
    mean, rstd, got = run_fwd(r, dev(y), dev(1 + 0.3 * rnd(C, seed=9)), dev(0.2 * rnd(C, seed=10)), None, None)
    assert got == fwd_plan(r), (got, fwd_plan(r))
    check_stats(mean, rstd, y, groups, r['id'])


@pytest.mark.parametrize('r', ROWS, ids=[r['id'] for r in ROWS])
def test_backward_row(r):
    """gx_gn_relu_bwd with one plain gradient source; mean / rstd are the float64 reference's, rounded once."""
    inp, G, ref, ref32 = _plain_reference(r['id'])
    mref, rref = stats64(inp['y'], r['groups'])[:2]
    got = run_bwd(r, dev(inp['y']), dev(inp['gamma']), dev(inp['beta']), dev(mref), dev(rref), (dev(G), 0, 0, 1, 0))
    assert got[4] == bwd_plan(r), (got[4], bwd_plan(r))
    check_grads(r, got[:4], ref, ref32, r['id'])


# ===================================================================================================== views
def _view_setup(r, mode1):
    """Destination / source 0: channels [3, 3 + C) of a same-size concat buffer; 1: channels [1, 1 + C) of a mode-`mode1` buffer."""
    inp = inputs_of(r)
    N, C, H, W = inp['y'].shape
    return inp, N, C, H, W, (3, 2), (1, 2)


@pytest.mark.parametrize('r,mode1', VIEW_CASES, ids=['%s-mode%d' % (r['id'], m) for r, m in VIEW_CASES])
def test_forward_views(r, mode1):
    inp, N, C, H, W, (lo0, hi0), (lo1, hi1) = _view_setup(r, mode1)
    groups = r['groups']
    ref, ref32 = reference(inp, groups, F64), reference(inp, groups, torch.float32)
    d0, d1 = wide_view(N, C, H, W, 0, lo0, hi0), wide_view(N, C, H, W, mode1, lo1, hi1)
    mean, rstd, got = run_fwd(r, dev(inp['y']), dev(inp['gamma']), dev(inp['beta']), (d0, lo0, 0), (d1, lo1, mode1))
    assert got == fwd_plan(r), (got, fwd_plan(r))
    check_stats(mean, rstd, inp['y'], groups, r['id'])
    pad = lambda n, t: torch.full((N, n) + tuple(t.shape[2:]), NAN, dtype=F64)      # noqa: E731
    for name, buf, lo, hi, mode in (('dst0', d0, lo0, hi0, 0), ('dst1', d1, lo1, hi1, mode1)):
        want, want32 = resample(ref['a'], mode), resample(ref32['a'], mode)
        whole = torch.cat([pad(lo, want), want, pad(hi, want)], 1)                  # the concat buffer the view is a slice of
        assert tuple(buf.shape) == tuple(whole.shape)
        assert torch.equal(torch.isnan(buf).cpu(), torch.isnan(whole)), '%s %s: written outside the view, or not written inside' % (r['id'], name)
        check_dest(buf, lo, C, want, want32, N * groups, '%s %s (mode %d)' % (r['id'], name, mode))


@pytest.mark.parametrize('r,mode1', VIEW_CASES, ids=['%s-mode%d' % (r['id'], m) for r, m in VIEW_CASES])
def test_backward_views(r, mode1):
    inp, N, C, H, W, (lo0, hi0), (lo1, hi1) = _view_setup(r, mode1)
    groups = r['groups']
    G0 = rnd(*view_shape(N, lo0 + C + hi0, H, W, 0), seed=11)
    G1 = rnd(*view_shape(N, lo1 + C + hi1, H, W, mode1), seed=12)
    srcs = [(G0, lo0, 0), (G1, lo1, mode1)]
    ref = reference(inp, groups, F64, [(g.double(), c0, m) for g, c0, m in srcs])
    ref32 = reference(inp, groups, torch.float32, srcs)
    mref, rref = stats64(inp['y'], groups)[:2]
    got = run_bwd(r, dev(inp['y']), dev(inp['gamma']), dev(inp['beta']), dev(mref), dev(rref), (dev(G0), lo0, 0, 1, 0),
                  (dev(G1), lo1, mode1, 1, 0))
    assert got[4] == bwd_plan(r, 1, 1), (got[4], bwd_plan(r, 1, 1))
    check_grads(r, got[:4], ref, ref32, '%s mode %d' % (r['id'], mode1))


# ===================================================================================================== partial slabs
def _slabs(shape, nsplit, seed, pad=64):
    """nsplit slabs of `shape`, numel + pad floats apart (the padding is NaN) -> the device buffer, its stride, the slab views."""
    numel = 1
    for s in shape:
        numel *= s
    stride = numel + pad
    buf = dnan(nsplit * stride)
    views = []
    for z in range(nsplit):
        buf[z * stride:z * stride + numel] = dev(rnd(*shape, seed=seed + z)).reshape(-1)
        views.append(buf[z * stride:z * stride + numel].view(*shape))
    return buf, stride, views


def _slab_order_sum(views):
    s = views[0].clone()
    for v in views[1:]:
        s = s + v                     # fp32 on the device, in slab order
    return s


@pytest.mark.parametrize('r,nsplit,with_bias', PART_FWD_CASES, ids=['%s-nsplit%d-%s' % (r['id'], ns, 'bias' if b else 'nobias') for r, ns, b in PART_FWD_CASES])
def test_forward_partial_slabs(r, nsplit, with_bias):
    """gx_gn_relu_fwd_parts: y_sum = ((p0 + p1) + p2) + bias bit for bit; mean, rstd and both destinations bit for bit what
    gx_gn_relu_fwd makes of that y_sum."""
    N, C, H, W, groups = r['N'], r['cpg'] * r['groups'], r['H'], r['W'], r['groups']
    gamma, beta = dev(1 + 0.3 * rnd(C, seed=9)), dev(0.2 * rnd(C, seed=10))
    buf, stride, views = _slabs((N, C, H, W), nsplit, 20)
    bias = dev(rnd(C, seed=30)) if with_bias else None
    want_sum = _slab_order_sum(views)
    if with_bias:
        want_sum = want_sum + bias.view(1, C, 1, 1)
    ysum = dnan(N, C, H, W)
    d0, d1 = wide_view(N, C, H, W, 0, 1, 2), wide_view(N, C, H, W, 2, 2, 1)
    mean, rstd, got = run_fwd(r, None, gamma, beta, (d0, 1, 0), (d1, 2, 2), parts=(buf, nsplit, stride, bias, ysum))
    assert got == fwd_plan(r, nsplit), (got, fwd_plan(r, nsplit))
    assert torch.equal(ysum, want_sum)
    e0, e1 = wide_view(N, C, H, W, 0, 1, 2), wide_view(N, C, H, W, 2, 2, 1)
    emean, erstd, got = run_fwd(r, want_sum.contiguous(), gamma, beta, (e0, 1, 0), (e1, 2, 2))
    assert got == fwd_plan(r), (got, fwd_plan(r))
    assert torch.equal(mean, emean) and torch.equal(rstd, erstd)
    for a, b in ((d0, e0), (d1, e1)):
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))
    assert bool(torch.isfinite(d0[:, 1:1 + C]).all()) and bool(torch.isfinite(d1[:, 2:2 + C]).all())
    # statistics only on the slabs: the same statistics, y_sum written, nothing else
    ysum2 = dnan(N, C, H, W)
    mean2, rstd2, got = run_fwd(r, None, gamma, beta, None, None, parts=(buf, nsplit, stride, bias, ysum2))
    assert got == fwd_plan(r, nsplit), (got, fwd_plan(r, nsplit))
    assert torch.equal(mean2, mean) and torch.equal(rstd2, rstd) and torch.equal(ysum2, want_sum)


@pytest.mark.parametrize('r,nsplit,mode0', PART_BWD_CASES, ids=['%s-nsplit%d-mode%d' % (r['id'], ns, m) for r, ns, m in PART_BWD_CASES])
def test_backward_partial_slabs(r, nsplit, mode0):
    """gx_gn_relu_bwd_parts: source 0 is `nsplit` slabs in mode `mode0`, source 1 the other slab count in the next mode; bit for
    bit the same call on the slab-order fp32 sums, and the float64 reference of those sums."""
    inp = inputs_of(r)
    N, C, H, W = inp['y'].shape
    groups = r['groups']
    mode1, nsplit1 = (mode0 + 1) % 3, 5 - nsplit
    b0, st0, v0 = _slabs(view_shape(N, C + 3, H, W, mode0), nsplit, 40)
    b1, st1, v1 = _slabs(view_shape(N, C + 2, H, W, mode1), nsplit1, 50)
    s0, s1 = _slab_order_sum(v0), _slab_order_sum(v1)
    mref, rref = stats64(inp['y'], groups)[:2]
    ops = [dev(inp['y']), dev(inp['gamma']), dev(inp['beta']), dev(mref), dev(rref)]
    got = run_bwd(r, *ops, (b0, 2, mode0, nsplit, st0, C + 3), (b1, 1, mode1, nsplit1, st1, C + 2))
    assert got[4] == bwd_plan(r, nsplit, nsplit1), (got[4], bwd_plan(r, nsplit, nsplit1))
    summed = run_bwd(r, *ops, (s0.contiguous(), 2, mode0, 1, 0), (s1.contiguous(), 1, mode1, 1, 0))
    assert summed[4] == bwd_plan(r, 1, 1)
    for name, a, b in zip(('dy', 'dgamma', 'dbeta', 'dbias'), got[:4], summed[:4]):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), '%s differs from the call on the summed sources' % name
    srcs = [(s0.cpu(), 2, mode0), (s1.cpu(), 1, mode1)]
    ref = reference(inp, groups, F64, [(g.double(), c0, m) for g, c0, m in srcs])
    check_grads(r, got[:4], ref, reference(inp, groups, torch.float32, srcs), '%s nsplit %d mode %d' % (r['id'], nsplit, mode0))


# ===================================================================================================== projected backward
@functools.lru_cache(maxsize=None)
def _proj_reference(rid):
    r = [p for p in PROJ_ROWS if p['id'] == rid][0]
    inp = inputs_of(r)
    N, C, H, W = inp['y'].shape
    g_out, w = rnd(N, r['Cout'], H, W, seed=11), 0.5 * rnd(r['Cout'], C, seed=12)
    gate = torch.tensor(0.7) if r['gate'] else None
    return (inp, g_out, w, gate, reference(inp, r['groups'], F64, proj=(g_out, w, gate)),
            reference(inp, r['groups'], torch.float32, proj=(g_out, w, gate)))


@pytest.mark.parametrize('r,wp', PROJ_CASES, ids=['%s-wp%d' % (r['id'], wp) for r, wp in PROJ_CASES])
def test_projected_backward_row(r, wp):
    """gx_gn_relu_bwd_proj: the gradient is gate * w^T g_out, formed on load; wpart / bpart (ungated, per image) when asked for."""
    from genesis_amd import _lib
    inp, g_out, w, gate, ref, ref32 = _proj_reference(r['id'])
    N, C, H, W = inp['y'].shape
    groups, Cout = r['groups'], r['Cout']
    fuses = bool(_lib.query('gx_gn_relu_bwd_proj_fuses_wgrad', C, H, W, groups, Cout))
    assert fuses == (r['kernel'] in ('bwd_stage', 'bwd_reg_staged', 'bwd_split')) and (fuses or not wp)
    mref, rref = stats64(inp['y'], groups)[:2]
    dy, dg, db, dbias = dnan(N, C, H, W), dnan(C), dnan(C), dnan(C)
    wpart, bpart = (dnan(N, Cout, C), dnan(N, Cout)) if wp else (None, None)
    nb = _lib.query('gx_gn_relu_bwd_proj_ws_bytes', N, C, H, W, groups, Cout)
    ws = nan_workspace(nb)
    ops = [dev(inp['y']), dev(inp['gamma']), dev(inp['beta']), dev(mref), dev(rref), dev(g_out), dev(w), None if gate is None else dev(gate)]
    _lib.call('gx_gn_relu_bwd_proj', *[ptr(t) for t in ops[:5]], N, C, H, W, groups, ptr(ops[5]), Cout, ptr(ops[6]), ptr(ops[7]),
              ptr(dy), ptr(dg), ptr(db), ptr(dbias), ptr(wpart), ptr(bpart), ptr(ws), nb, _stream())
    got = last_plan('gn_bwd_plan', N, C, H, W, groups, g0_mode=3, g0_ctot=Cout, g0_nsplit=0, want_wpart=wp, ws_bytes=nb)
    assert got == proj_plan(r, wp), (got, proj_plan(r, wp))
    check_grads(r, (dy, dg, db, dbias), ref, ref32, r['id'])
    if wp:
        slab_close(wpart, ref['wpart'], ref32['wpart'], N, 1e-4, 1e-4, r['id'] + ' wpart')
        slab_close(bpart, ref['bpart'], ref32['bpart'], N, 1e-4, 1e-4, r['id'] + ' bpart')


# ===================================================================================================== deferred parameter reduce
@pytest.mark.parametrize('name', sorted(DEFER_ROUNDS))
def test_deferred_parameter_reduce(name):
    """gx_defer_flush_gn: rounds of 48 records, clash rounds for records that share a destination, and -- beyond the queue's 128
    -- the immediate, accumulating reduce.  Every destination = its zeroed start + the direct results of its calls: bit for bit
    with one record; for the three DIFFERENT calls that share one, within 1e-6 of the sum of the contributions' magnitudes
    against their float64 sum (two fp32 roundings: 1.2e-7).  In the overflow round two of the sharing calls come after the
    queue is full: the second of them reduces immediately onto what the first left there, so before the flush the destination
    must hold exactly their fp32 sum -- an immediate reduce that overwrote would leave the second alone."""
    from genesis_amd import hip_ops as hip
    count, shared = DEFER_ROUNDS[name]
    N, H, W = 2, 4, 4
    calls = []
    for i in range(count):
        C, groups = DEFER_SHAPES[(0 if i in shared else i) % len(DEFER_SHAPES)]
        y, g = dev(rnd(N, C, H, W, seed=100 + i, scale=2.0) + 0.3), dev(rnd(N, C, H, W, seed=400 + i))
        gamma, beta = dev(1 + 0.3 * rnd(C, seed=9)), dev(0.2 * rnd(C, seed=10))
        mref, rref = stats64(y.cpu(), groups)[:2]
        calls.append((y, gamma, beta, dev(mref), dev(rref), groups, g))
    direct = [hip.gn_relu_bwd(*c[:6], (c[6], 0, 0), want_dbias=True)[1:] for c in calls]
    torch.cuda.synchronize()
    shared_out = tuple(torch.zeros(DEFER_SHAPES[0][0], device=DEV) for _ in range(3))
    outs = [shared_out if i in shared else tuple(torch.zeros(c[0].shape[1], device=DEV) for _ in range(3)) for i, c in enumerate(calls)]
    late = [i for i in shared if i >= 128]
    st = hip.defer_state()
    st.on = True
    try:
        for c, o in zip(calls, outs):
            hip.gn_relu_bwd(*c[:6], (c[6], 0, 0), want_dbias=True, out=o)
        for i, o in enumerate(outs):
            if i < 128 and i not in shared:
                assert float(o[0].abs().max()) == 0.0, 'the queued reduce of call %d ran before the flush' % i
        for j, got in enumerate(shared_out):          # the immediate reduces so far, in call order, each onto the last
            want = torch.zeros_like(got)
            for i in late:
                want = want + direct[i][j]
            assert torch.equal(got, want), 'shared destination %d before the flush' % j
        hip.defer_flush()
        torch.cuda.synchronize()
    finally:
        st.on = False
        hip.defer_discard()
    for i, (o, d) in enumerate(zip(outs, direct)):
        if i not in shared:
            for got, one in zip(o, d):
                assert torch.equal(got, one), 'destination of call %d' % i
    for j, got in enumerate(shared_out):
        parts = [direct[i][j].double() for i in shared]
        want, mag = sum(parts), sum(p.abs() for p in parts)
        assert bool(((got.double() - want).abs() <= 1e-6 * mag).all()), 'shared destination %d' % j
        assert bool((mag > 0).all())


# ===================================================================================================== refusals and queries
@pytest.mark.parametrize('name,what', [(n, w) for n, w, _ in REFUSALS], ids=['%s-%s' % (n, w.replace(' ', '-')) for n, w, _ in REFUSALS])
def test_refusals(name, what):
    check_refusal(name, what)


def test_fuses_wgrad_query():
    from genesis_amd import _lib
    for args in NOT_FUSED:
        assert _lib.query('gx_gn_relu_bwd_proj_fuses_wgrad', *args) == 0, args
    for args in FUSED:
        assert _lib.query('gx_gn_relu_bwd_proj_fuses_wgrad', *args) != 0, args

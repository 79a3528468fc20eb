"""The dense layer, its one-launch backward pair, the [in,out]-layout matmul and the LSTM kernels of genesis_amd/csrc/gx_dense.hip at
every launch plan the host dispatch (gx_dense.hip, the extern "C" block) can pick: both workgroup sizes, every state of the
vectorisation flags and every condition that turns one off, the pair / dx-only / dw-only launches, the masks, the bias-gradient
copies, the accumulate bits, the dx chunk plans of the matmul and the sequence / step choice of the LSTM wrappers.

Dense and matmul rows run on EXACT operands: x, w, b, g and the accumulate bases are integers in [-3, 3], the mask source y holds
multiples of 1/8 in [-1, 2] (exact zeros, negatives, positives).  Every product and partial sum is then a multiple of 1/8 far
below 2^24 / 8 -- representable in fp32 in any summation order -- so the assertion is torch.equal against the fp64 CPU reference
cast to float32 (the cast is asserted lossless first).  The one exception is the forward ELU where the pre-activation is <= 0
(expm1f): those entries alone take test_linear's rtol 1e-5 / atol 1e-5 against fp64 F.elu.  A subset reruns on rnd() floats at the
bars tests/test_kernels_gpu.py applies to the same outputs (integers up to 3 would survive a 16-bit product).  Every operand and
destination is a view inside a larger allocation: 16 rows and 4 floats of margin on each side, NaN around the inputs (between the
rows too), a sentinel around the destinations that is checked bit for bit.  Which branch a row reaches is DECLARED in its table row
and derived again from the restated dispatch in tests/test_dense_plans_cpu.py.

What each class would catch (one-line mistakes in the branch it reaches; argued from the code, never run):

  1024 threads, ragged contraction (1028, 1030)     the k16 loop striding 4 waves (`+= 64`: twelve waves add every step four times),
                                                    `k16 <= Kc`, a float4 guard `kb + 3 < Kc` off by one, part[] summed over 4 of
                                                    the 16 waves, a scalar guard `kb < Kc` that reads K..K+3 (NaN padding, next row)
  contraction shorter than one step (1, 3, 5, 7)    a wave that skips the part[] store when its loop never ran (LDS garbage summed),
                                                    an epilogue that divides the work by nw
  vec_w = 1, vec_x = 0 (pointer / row stride)       a 16-byte load of x chosen on K % 4 alone, vec_x passed for vec_w (or the two
                                                    swapped at the launch), lda used for ldb
  vec_w = 0 with K % 4 == 0                         aligned16(w) dropped from the rule, vec_x not tied to vec_w
  vec on, contraction % 16 != 0 (20, 36)            `kb < Kc` replaced by `k16 + 16 <= Kc` (the last step dropped)
  ragged M / N (3, 5, 17, 33, 1)                    a_ok / b_ok or `ci < I && cj < J` dropped: the NaN rows around the operands enter
                                                    the sums, the sentinel around the destination is overwritten
  strided x / y / g / dx (ld = n + pad)             an index that multiplies by the width where the row stride belongs
  act x bias                                        bias added after the activation, bias[ci], ELU with `s >= 0`, act code 2
                                                    (accumulate) left on the forward's ELU
  pair launch                                       gy_dx from N, `blockIdx.y <= gy_dx`, the dw half indexed with blockIdx.y (not
                                                    - gy_dx), threads from M alone, the mask dropped from one half
  dx-only / dw-only                                 threads from the wrong extent, `dx_act & 7` lost (the dw bits reach the dx
                                                    epilogue), out_dw touched by a launch that does not produce it
  masks, y holding exact 0 / -1 / negatives         ReLU `m >= 0`, ELU derivative `m` or `m + 1` also where m > 0, the ELU bit
                                                    (act & 4) not passed to the dw half, the mask read with g's alignment only
  y unaligned, g aligned                            `aligned16(y)` dropped from `vec`: a 16-byte load of the mask off a 4-byte
                                                    boundary
  db / db2, more than one column tile               `bx == 0` dropped (every column tile writes db -- and ADDS it K/16 times when
                                                    accumulating), rs2 forgotten in one of the two arms, rsum summed over jj < 3
  accumulate bits                                   bit 1 / bit 2 swapped, dw += without db += (code 10 -> 2), dx += on the dw half
  matmul_nn plans (128,128,65), (128,192,86)        `nchunk` for `used` at the reduce (reads workspace nobody wrote: NaN-filled
                                                    here), cols not rounded to 64 (a chunk boundary inside a staged float4),
                                                    c_end unclamped at N (reads past the row), grid.x = nchunk
  matmul_nn 4-wide last chunk / N = 4 / 1028        `c0 + q < c_end` dropped, `n0 >= N` dropped in the forward's second column
                                                    block, the dw kernel's n_ok dropped
  matmul_nn two k / row tiles (33 x 70)             `k0 + r < K` dropped at the dw store, the clamp `K - 1` on the x read dropped
  LSTM H = 48, 80; B = 1, 16, 33                    `k16 += 64` with a wrong bound (waves 0..2 only / wave 0 twice), a_ok dropped
                                                    (rows past B read), `b < B` dropped at the epilogue (state of the next step
                                                    overwritten: value check of the next step)
  LSTM_SEQ wiring                                   the wrong buffer handed to lstm_seq_* (dc for dgates, c for h), `1 <= T`, a
                                                    capacity test on T alone, the fallback missing past 128 workgroups
  refusals                                          a GX_CHECK_ARG that stopped refusing (16-byte loads of w_hh / w / g, a grid
                                                    that cannot be resident at once)
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
NAN = float('nan')
SENT = 777.0                      # around every destination; checked bit for bit
MARGIN_ROWS, MARGIN_FLOATS = 16, 4
ACTS = (None, 'relu', 'elu')
ALL6 = tuple((a, b) for a in ACTS for b in (True, False))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def close(a, b, rtol=1e-4, atol=1e-4, msg=''):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert err <= atol + rtol * ref, '%s max err %.3e (ref max %.3e)' % (msg, err, ref)


def ints(*shape, seed=0):
    """Integers in [-3, 3] as float32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, shape, generator=g).float()


def eighths(*shape, seed=0):
    """Multiples of 1/8 in [-1, 2] as float32 with an exact 0, -1 (ELU derivative 0), a negative and a positive planted."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(-8, 17, shape, generator=g).float() / 8
    flat = y.view(-1)
    for i, v in enumerate((0.0, -1.0, -0.375, 1.25)[:flat.numel()]):
        flat[i * (flat.numel() // 4) if flat.numel() >= 8 else i] = v
    return y


# ------------------------------------------------------------------------------------------------------------ the case tables
# Forward rows of gx_linear_fwd_ld.  x_pad / y_pad: row stride minus width; x_off / w_off: elements past a 16-byte boundary.
# Declared: threads, (vec_w, vec_x), what turns each flag off, the axes that are no multiple of 16, tail (the contraction is no
# multiple of 16 x waves: some waves run one more step than others).
def _fwd(id_, M, N, K, threads, vec_w, vec_x, w_why=None, x_why=None, ragged='', tail=True, x_pad=0, x_off=0, w_off=0, y_pad=0,
         flt=False):
    return dict(id=id_, M=M, N=N, K=K, threads=threads, vec_w=vec_w, vec_x=vec_x, w_why=w_why, x_why=x_why, ragged=ragged,
                tail=tail, x_pad=x_pad, x_off=x_off, w_off=w_off, y_pad=y_pad, combos=ALL6, flt=flt)


FWD_ROWS = [
    _fwd('3x5x1028', 3, 5, 1028, 1024, 1, 1, ragged='MNK', flt=True),
    _fwd('3x5x1030', 3, 5, 1030, 1024, 0, 0, 'K%4', 'vec_w', ragged='MNK', flt=True),
    _fwd('17x33x20', 17, 33, 20, 256, 1, 1, ragged='MNK', x_pad=8, y_pad=7, flt=True),
    _fwd('7x5x3', 7, 5, 3, 256, 0, 0, 'K%4', 'vec_w', ragged='MNK'),
    _fwd('1x1x1', 1, 1, 1, 256, 0, 0, 'K%4', 'vec_w', ragged='MNK'),
    _fwd('16x16x16', 16, 16, 16, 256, 1, 1, ragged='', tail=True),
    _fwd('33x17x70', 33, 17, 70, 256, 0, 0, 'K%4', 'vec_w', ragged='MNK', x_pad=6, y_pad=5, flt=True),
    _fwd('17x5x20 x+1', 17, 5, 20, 256, 1, 0, None, 'x_ptr', ragged='MNK', x_off=1),
    _fwd('17x5x20 ldx=25', 17, 5, 20, 256, 1, 0, None, 'ldx%4', ragged='MNK', x_pad=5, flt=True),
    _fwd('9x18x24 w+1', 9, 18, 24, 256, 0, 0, 'w_ptr', 'vec_w', ragged='MNK', w_off=1, flt=True),
    _fwd('5x4x1280 ldx=1284', 5, 4, 1280, 1024, 1, 1, ragged='MN', tail=False, x_pad=4),
    _fwd('5x4x1040 x+1', 5, 4, 1040, 1024, 1, 0, None, 'x_ptr', ragged='MN', x_off=1),
]
FWD_CASES = [(r['id'], a, b) for r in FWD_ROWS for a, b in r['combos']]


# Backward rows of gx_linear_bwd_ex.  kind: pair (dx and dw in one launch), dx, dw.  mask: None / relu / elu (y is an INPUT).
# db: none / db / db2 (db and its second copy).  acc: the dx_accumulate bit mask (1: dx +=, 2: dw / db +=).  dx_pad: None (dx in
# a fresh tensor) or the padding of the row-strided destination (out_dx, or accumulate_dx's base when acc & 1).
def _bwd(id_, kind, M, N, K, threads, vec, why=None, mask=None, db='none', acc=0, ragged='MNK', x_pad=0, g_pad=0, g_off=0, y_off=0,
         dx_pad=None, flt=False):
    return dict(id=id_, kind=kind, M=M, N=N, K=K, threads=threads, vec=vec, why=why, mask=mask, db=db, acc=acc, ragged=ragged,
                x_pad=x_pad, g_pad=g_pad, g_off=g_off, y_off=y_off, dx_pad=dx_pad, flt=flt)


BWD_ROWS = [
    _bwd('pair 3x1028x5', 'pair', 3, 1028, 5, 1024, 1, mask='relu', db='db', flt=True),
    _bwd('pair 1030x5x3', 'pair', 1030, 5, 3, 1024, 0, 'N%4', mask='elu', db='db2', flt=True),
    _bwd('pair 17x36x20', 'pair', 17, 36, 20, 256, 1, g_pad=4, x_pad=4, flt=True),
    _bwd('pair 7x5x3', 'pair', 7, 5, 3, 256, 0, 'N%4', mask='relu', db='db'),
    _bwd('pair 1x1x1', 'pair', 1, 1, 1, 256, 0, 'N%4', db='db'),
    _bwd('pair 17x36x20 elu', 'pair', 17, 36, 20, 256, 1, mask='elu', db='db', g_pad=4),
    _bwd('pair 17x36x20 ldg=41', 'pair', 17, 36, 20, 256, 0, 'ldg%4', mask='elu', db='db2', g_pad=5, flt=True),
    _bwd('pair 17x36x20 g+1', 'pair', 17, 36, 20, 256, 0, 'g_ptr', db='db', g_off=1),
    _bwd('pair 17x36x20 y+1', 'pair', 17, 36, 20, 256, 0, 'y_ptr', mask='relu', g_pad=4, y_off=1),
    _bwd('pair 17x20x35 acc0', 'pair', 17, 20, 35, 256, 1, db='db'),
    _bwd('pair 17x20x35 acc1', 'pair', 17, 20, 35, 256, 1, mask='relu', db='db', acc=1, dx_pad=5, x_pad=5),
    _bwd('pair 17x20x35 acc2', 'pair', 17, 20, 35, 256, 1, mask='elu', db='db2', acc=2, flt=True),
    _bwd('pair 17x20x35 acc3', 'pair', 17, 20, 35, 256, 1, mask='elu', db='db2', acc=3, dx_pad=0),
    _bwd('pair 17x20x35 out_dx', 'pair', 17, 20, 35, 256, 1, mask='relu', dx_pad=9),
    _bwd('dx 5x1028x7', 'dx', 5, 1028, 7, 1024, 1, mask='relu', flt=True),
    _bwd('dx 17x20x33', 'dx', 17, 20, 33, 256, 1, flt=True),
    _bwd('dx 17x20x33 elu y+1', 'dx', 17, 20, 33, 256, 0, 'y_ptr', mask='elu', y_off=1),
    _bwd('dx 3x1030x5 elu', 'dx', 3, 1030, 5, 1024, 0, 'N%4', mask='elu'),
    _bwd('dx 17x20x35 acc1', 'dx', 17, 20, 35, 256, 1, mask='elu', acc=1, dx_pad=5),
    _bwd('dx 17x20x35 acc3', 'dx', 17, 20, 35, 256, 1, mask='relu', acc=3, dx_pad=0),
    _bwd('dx 7x5x35 out_dx', 'dx', 7, 5, 35, 256, 0, 'N%4', dx_pad=7, g_pad=6),
    _bwd('dx 17x20x35 out_dx relu', 'dx', 17, 20, 35, 256, 0, 'ldg%4', mask='relu', dx_pad=4, g_pad=1),
    _bwd('dw 1030x6x35', 'dw', 1030, 6, 35, 1024, 0, 'N%4', mask='relu', db='db', flt=True),
    _bwd('dw 7x5x35', 'dw', 7, 5, 35, 256, 0, 'N%4', db='db2', flt=True),
    _bwd('dw 17x20x35 elu acc2', 'dw', 17, 20, 35, 256, 1, mask='elu', db='db2', acc=2),
    _bwd('dw 33x17x3 elu', 'dw', 33, 17, 3, 256, 0, 'N%4', mask='elu'),
    _bwd('dw 17x20x35 acc2', 'dw', 17, 20, 35, 256, 1, db='db', acc=2, x_pad=5, g_pad=4),
    _bwd('dw 1028x4x35 relu acc2', 'dw', 1028, 4, 35, 1024, 1, mask='relu', db='db', acc=2),
]

# gx_matmul_nn_*: M x K x N.  plan = (nchunk, cols, used) of the dx launch; grids of the forward, dw and dx launches.
def _nn(M, K, N, plan, fwd_grid, dw_grid, dx_grid, x_off=0, need_dx=True, need_dw=True, out_dw=False):
    return dict(id='%dx%dx%d%s%s%s%s' % (M, K, N, ' x+1' if x_off else '', '' if need_dx else ' no dx', '' if need_dw else ' no dw',
                                         ' out_dw' if out_dw else ''),
                M=M, K=K, N=N, plan=plan, fwd_grid=fwd_grid, dw_grid=dw_grid, dx_grid=dx_grid, x_off=x_off, need_dx=need_dx,
                need_dw=need_dw, out_dw=out_dw)


NN_ROWS = [
    _nn(3, 5, 8196, (128, 128, 65), (1, 9), (1, 33), (65, 1, 1), out_dw=True),
    _nn(33, 70, 260, (5, 64, 5), (5, 1), (5, 2), (5, 2, 2), x_off=1),
    _nn(3, 8, 4, (1, 64, 1), (1, 1), (1, 1), (1, 1, 1)),
    _nn(9, 17, 1028, (17, 64, 17), (2, 2), (2, 5), (17, 1, 1), x_off=1, out_dw=True),
    _nn(2, 3, 16388, (128, 192, 86), (1, 17), (1, 65), (86, 1, 1)),
    _nn(5, 6, 144, (3, 64, 3), (1, 1), (1, 1), (3, 1, 1)),
    _nn(33, 70, 260, (5, 64, 5), (5, 1), (5, 2), (5, 2, 2), need_dx=False, out_dw=True),
    _nn(3, 5, 8196, (128, 128, 65), (1, 9), (1, 33), (65, 1, 1), x_off=1, need_dw=False),
]

# LSTMFn / ARPriorKLFn with hip.LSTM_SEQ on: (T, B, H) -> the launches taken and the grid (H / 16, ceil(B / 16))
SEQ_ROWS = [
    dict(T=3, B=33, H=48, path='seq', grid=(3, 3)),
    dict(T=16, B=2, H=16, path='seq', grid=(1, 1)),
    dict(T=1, B=3, H=16, path='step', grid=(1, 1)),          # T == 1: the per-step branch
    dict(T=17, B=2, H=16, path='step', grid=(1, 1)),         # over the 16 steps of one launch
    dict(T=2, B=129, H=256, path='step', grid=(16, 9)),      # 144 workgroups > 128
]
LSTM_SHAPES = [(3, 1, 5, 48), (2, 16, 8, 80), (3, 33, 7, 16), (1, 17, 4, 48), (17, 2, 3, 16)]        # (T, B, D, H)
CELL_SHAPES = [(5, 7, 48), (16, 20, 80), (33, 3, 16)]                                               # (B, Din, H)


def row_by_id(rows, id_):
    hits = [r for r in rows if r['id'] == id_]
    assert len(hits) == 1, id_
    return hits[0]


# ------------------------------------------------------------------------------------------------- operands and references (CPU)
def embed_start(ld, off):
    """Element offset of a view inside its allocation: 16 rows and 4 floats of margin, then `off` elements (16 ld + 4 is a
    multiple of 4, so the view starts `off` floats past a 16-byte boundary)."""
    return MARGIN_ROWS * ld + MARGIN_FLOATS + off


def fwd_operands(row, bias, exact=True):
    M, N, K = row['M'], row['N'], row['K']
    if exact:
        return dict(x=ints(M, K, seed=1), w=ints(N, K, seed=2), b=ints(N, seed=3) if bias else None)
    return dict(x=rnd(M, K, seed=1), w=rnd(N, K, seed=2, scale=1.0 / math.sqrt(K)), b=rnd(N, seed=3) if bias else None)


def fwd_reference(ops, act, dtype=F64):
    """-> (pre-activation, result) in `dtype`."""
    pre = ops['x'].to(dtype) @ ops['w'].to(dtype).t()
    if ops['b'] is not None:
        pre = pre + ops['b'].to(dtype)
    return pre, (F.relu(pre) if act == 'relu' else F.elu(pre) if act == 'elu' else pre)


def bwd_operands(row, exact=True):
    M, N, K = row['M'], row['N'], row['K']
    mk = ints if exact else rnd
    ops = dict(x=mk(M, K, seed=1), w=mk(N, K, seed=2) if exact else rnd(N, K, seed=2, scale=1.0 / math.sqrt(K)), g=mk(M, N, seed=4),
               y=None, base_dx=mk(M, K, seed=5), base_dw=mk(N, K, seed=6), base_db=mk(N, seed=7), base_db2=mk(N, seed=8))
    if row['mask']:
        ops['y'] = eighths(M, N, seed=9) if exact else rnd(M, N, seed=9)
    return ops


def bwd_reference(row, ops, dtype=F64):
    """-> dict(dx, dw, db, db2) in `dtype`, accumulate bases included where the row's bits say so."""
    g, x, w = ops['g'].to(dtype), ops['x'].to(dtype), ops['w'].to(dtype)
    if row['mask']:
        y = ops['y'].to(dtype)
        one, zero = torch.ones_like(y), torch.zeros_like(y)
        g = g * torch.where(y > 0, one, y + 1 if row['mask'] == 'elu' else zero)
    out = dict(dx=g @ w, dw=g.t() @ x, db=g.sum(0), db2=g.sum(0))
    if row['acc'] & 1:
        out['dx'] = out['dx'] + ops['base_dx'].to(dtype)
    if row['acc'] & 2:
        for k in ('dw', 'db', 'db2'):
            out[k] = out[k] + ops['base_' + k].to(dtype)
    return out


def nn_operands(row, exact=True):
    M, K, N = row['M'], row['K'], row['N']
    if exact:
        return dict(x=ints(M, K, seed=1), w=ints(K, N, seed=2), g=ints(M, N, seed=3))
    return dict(x=rnd(M, K, seed=1), w=rnd(K, N, seed=2, scale=1 / math.sqrt(K)), g=rnd(M, N, seed=3))


def nn_reference(ops, dtype=F64):
    x, w, g = (ops[k].to(dtype) for k in ('x', 'w', 'g'))
    return dict(y=x @ w, dx=g @ w.t(), dw=x.t() @ g)


def lossless(ref64):
    """The fp64 reference cast to float32, after asserting that the cast loses nothing."""
    r32 = ref64.float()
    assert torch.equal(r32.double(), ref64), 'the fp64 reference is not representable in fp32'
    return r32


# ------------------------------------------------------------------------------------------------------- views on the device
class View(object):
    """`t` ([M, n] or [n]) as a device view with row stride n + pad, `off` floats past a 16-byte boundary, inside an allocation
    filled with `fill`: 16 rows and 4 floats of margin before and after, `pad` floats between the rows."""

    def __init__(self, t, pad=0, off=0, fill=NAN, want_ptr=None):
        self.shape = tuple(t.shape) if t.dim() == 2 else (1, t.numel())
        M, n = self.shape
        self.ld = n + pad
        self.start = embed_start(self.ld, off)
        self.buf = torch.full((self.start + M * self.ld + MARGIN_ROWS * self.ld + MARGIN_FLOATS,), fill, device=DEV)
        self.fill = fill
        v = self.buf.as_strided((M, n), (self.ld, 1), self.start)
        v.copy_(t.view(M, n))
        self.v = v if t.dim() == 2 else v[0]
        assert self.buf.data_ptr() % 16 == 0
        assert self.v.data_ptr() % 16 == (4 * off if want_ptr is None else want_ptr), (self.v.data_ptr() % 16, off)

    def margins_intact(self):
        """Bit for bit: everything in the allocation outside the view still holds the fill."""
        b = self.buf.clone()
        b.as_strided(self.shape, (self.ld, 1), self.start).fill_(self.fill)
        return torch.equal(b.view(torch.int32), torch.full_like(b, self.fill).view(torch.int32))


def dest(shape, base=None, pad=0):
    """A destination: NaN (or the accumulate base) inside, the sentinel around."""
    return View(torch.full(shape, NAN) if base is None else base, pad=pad, fill=SENT)


def zeros_view(*shape, off=0):
    return View(torch.zeros(*shape), off=off, fill=0.0).v


# ------------------------------------------------------------------------------------------------------------ dense, forward
def run_fwd(row, act, bias, exact):
    M, N, K = row['M'], row['N'], row['K']
    ops = fwd_operands(row, bias, exact)
    x = View(ops['x'], pad=row['x_pad'], off=row['x_off'])
    w = View(ops['w'], off=row['w_off'])
    b = View(ops['b']) if bias else None
    y = dest((M, N), pad=row['y_pad'])
    assert x.v.stride(0) == K + row['x_pad'] and w.v.is_contiguous() and y.v.stride(0) == N + row['y_pad']
    out = hip.linear_fwd(x.v, w.v, b.v if bias else None, act, out=y.v)
    assert out.data_ptr() == y.v.data_ptr()
    torch.cuda.synchronize()
    assert y.margins_intact(), 'the forward wrote outside its destination'
    pre, ref = fwd_reference(ops, act)
    got = y.v.cpu()
    if not exact:
        close(got, ref, rtol=1e-5, atol=1e-5, msg='y')
        return
    if act == 'elu':
        ex = pre <= 0                                # expm1f: the only inexact values of these rows
        assert torch.equal(got[~ex], lossless(ref[~ex]))
        if bool(ex.any()):
            close(got[ex], ref[ex], rtol=1e-5, atol=1e-5, msg='ELU, pre-activation <= 0')
    else:
        assert torch.equal(got, lossless(ref)), float((got.double() - ref).abs().max())


@pytest.mark.parametrize('rid,act,bias', FWD_CASES)
def test_linear_fwd_exact(rid, act, bias):
    run_fwd(row_by_id(FWD_ROWS, rid), act, bias, True)


@pytest.mark.parametrize('rid,act,bias', [(r['id'], a, b) for r in FWD_ROWS if r['flt'] for a, b in (('elu', True), (None, False),
                                                                                                    ('relu', True))])
def test_linear_fwd_float(rid, act, bias):
    run_fwd(row_by_id(FWD_ROWS, rid), act, bias, False)


# ----------------------------------------------------------------------------------------------------------- dense, backward
def run_bwd(row, exact):
    M, N, K, kind, acc = row['M'], row['N'], row['K'], row['kind'], row['acc']
    ops = bwd_operands(row, exact)
    if row['mask'] and exact:
        y0 = ops['y']
        assert bool((y0 == 0).any()) and bool((y0 < 0).any()) and bool((y0 > 0).any()) and bool((y0 == -1).any())
    x = View(ops['x'], pad=row['x_pad'])
    w = View(ops['w'])
    g = View(ops['g'], pad=row['g_pad'], off=row['g_off'])
    y = View(ops['y'], pad=row['g_pad'], off=row['y_off']) if row['mask'] else None
    kw = dict(need_dx=kind != 'dw', need_dw=kind != 'dx', need_db=row['db'] != 'none')
    dx = dw = db = db2 = None
    if kind != 'dw' and row['dx_pad'] is not None:
        dx = dest((M, K), ops['base_dx'] if acc & 1 else None, pad=row['dx_pad'])
        kw['accumulate_dx' if acc & 1 else 'out_dx'] = dx.v
    else:
        assert not acc & 1
    if kind != 'dx' or acc & 2:                # (a dx-only launch with the dw bit set: its out_dw must stay as it is)
        dw = dest((N, K), ops['base_dw'] if acc & 2 else None)
        kw['out_dw'] = dw.v
        kw['accumulate_dw'] = bool(acc & 2)
    if kind != 'dx' and row['db'] != 'none':
        db = dest((N,), ops['base_db'] if acc & 2 else None)
        kw['out_db'] = db.v
        if row['db'] == 'db2':
            db2 = dest((N,), ops['base_db2'] if acc & 2 else None)
            kw['out_db2'] = db2.v
    kept = dw.buf.clone() if (dw is not None and kind == 'dx') else None
    rdx, rdw, rdb = hip.linear_bwd(x.v, w.v, y.v if y else None, g.v, row['mask'], **kw)
    torch.cuda.synchronize()
    for d, name in ((dx, 'dx'), (dw, 'dw'), (db, 'db'), (db2, 'db2')):
        assert d is None or d.margins_intact(), 'the backward wrote outside ' + name
    ref = bwd_reference(row, ops)
    got = {}
    if kind != 'dw':
        got['dx'] = rdx
        assert dx is None or rdx.data_ptr() == dx.v.data_ptr()
    else:
        assert rdx is None
    if kind != 'dx':
        got['dw'] = dw.v
        assert rdw.data_ptr() == dw.v.data_ptr()
        if db is not None:
            got['db'] = db.v
        else:
            assert rdb is None
        if db2 is not None:
            got['db2'] = db2.v
    else:
        assert rdw is None and rdb is None
        if kept is not None:
            assert torch.equal(dw.buf.view(torch.int32), kept.view(torch.int32)), 'a dx-only launch touched out_dw'
    for name, t in got.items():
        if exact:
            assert torch.equal(t.cpu(), lossless(ref[name])), (name, float((t.cpu().double() - ref[name]).abs().max()))
        else:
            close(t, ref[name], rtol=1e-4, atol=1e-5, msg=name)


@pytest.mark.parametrize('rid', [r['id'] for r in BWD_ROWS])
def test_linear_bwd_exact(rid):
    run_bwd(row_by_id(BWD_ROWS, rid), True)


@pytest.mark.parametrize('rid', [r['id'] for r in BWD_ROWS if r['flt']])
def test_linear_bwd_float(rid):
    run_bwd(row_by_id(BWD_ROWS, rid), False)


# ------------------------------------------------------------------------------------------------------------------ matmul_nn
def _nan_ws(monkeypatch):
    """The dx workspace starts as NaN: a reduce over chunks nobody wrote shows."""
    monkeypatch.setattr(hip, '_ws', lambda nb, dev: torch.full((max(int(nb), 16),), 0xFF, dtype=torch.uint8, device=dev))


def run_nn(row, exact, monkeypatch):
    M, K, N = row['M'], row['K'], row['N']
    _nan_ws(monkeypatch)
    ops = nn_operands(row, exact)
    ref = nn_reference(ops)
    x = View(ops['x'], off=row['x_off'])
    w, g = View(ops['w']), View(ops['g'])
    assert x.v.is_contiguous() and w.v.is_contiguous() and g.v.is_contiguous()
    y = hip.matmul_nn_fwd(x.v, w.v)
    dw = dest((K, N)) if row['out_dw'] else None
    dx, rdw = hip.matmul_nn_bwd(x.v, w.v, g.v, need_dx=row['need_dx'], need_dw=row['need_dw'], out_dw=dw.v if dw else None)
    torch.cuda.synchronize()
    assert (dx is None) == (not row['need_dx']) and (rdw is None) == (not row['need_dw'])
    got = dict(y=y)
    if row['need_dx']:
        got['dx'] = dx
    if row['need_dw']:
        got['dw'] = rdw
        if dw is not None:
            assert rdw.data_ptr() == dw.v.data_ptr() and dw.margins_intact(), 'dw written outside its destination'
    elif dw is not None:
        assert dw.margins_intact() and bool(torch.isnan(dw.v).all())
    for name, t in got.items():
        assert tuple(t.shape) == tuple(ref[name].shape)
        if exact:
            assert torch.equal(t.cpu(), lossless(ref[name])), (name, float((t.cpu().double() - ref[name]).abs().max()))
        else:
            tol = 2e-6 if name == 'y' else 5e-6
            close(t, ref[name], tol, tol, name)


@pytest.mark.parametrize('rid', [r['id'] for r in NN_ROWS])
def test_matmul_nn_exact(rid, monkeypatch):
    run_nn(row_by_id(NN_ROWS, rid), True, monkeypatch)


@pytest.mark.parametrize('rid', [r['id'] for r in NN_ROWS])
def test_matmul_nn_float(rid, monkeypatch):
    run_nn(row_by_id(NN_ROWS, rid), False, monkeypatch)


@pytest.mark.parametrize('M,K,N', [(r['M'], r['K'], r['N']) for r in NN_ROWS if 4 * math.isqrt(r['N'] // 4) ** 2 == r['N']
                                   and r['need_dx'] and r['need_dw'] and not r['out_dw']])
@pytest.mark.parametrize('frozen', [None, 'x', 'w'])
def test_matmul_nn_through_autograd_with_a_4d_weight(M, K, N, frozen, monkeypatch):
    from genesis_amd import functions as fn
    _nan_ws(monkeypatch)
    k = math.isqrt(N // 4)
    ops = nn_operands(dict(M=M, K=K, N=N))
    ref = nn_reference(ops)
    xd = ops['x'].to(DEV).requires_grad_(frozen != 'x')
    wd = ops['w'].to(DEV).view(K, 4, k, k).clone().requires_grad_(frozen != 'w')
    out = fn.MatmulNNFn.apply(xd, wd)
    out.backward(ops['g'].to(DEV))
    assert torch.equal(out.detach().cpu(), lossless(ref['y']))
    assert xd.grad is None if frozen == 'x' else torch.equal(xd.grad.cpu(), lossless(ref['dx']))
    assert wd.grad is None if frozen == 'w' else (wd.grad.shape == wd.shape and torch.equal(wd.grad.view(K, N).cpu(), lossless(ref['dw'])))


# ------------------------------------------------------------------------------------------------------------------- refusals
def _lstm_seq_fwd(T, B, H, w_off=0):
    return lambda: hip.lstm_seq_fwd(zeros_view(T * B, 4 * H).view(T, B, 4 * H), zeros_view(4 * H, H, off=w_off), zeros_view(4 * H),
                                    zeros_view(T * B, 4 * H).view(T, B, 4 * H), zeros_view(T * B, H).view(T, B, H),
                                    zeros_view(T * B, H).view(T, B, H))


def _lstm_seq_bwd(T, B, H):
    return lambda: hip.lstm_seq_bwd(zeros_view(T * B, H).view(T, B, H), zeros_view(4 * H, H), zeros_view(T * B, 4 * H).view(T, B, 4 * H),
                                    zeros_view(T * B, H).view(T, B, H), zeros_view(T * B, 4 * H).view(T, B, 4 * H),
                                    zeros_view(2 * B, H).view(2, B, H))


def _lstm_step_fwd(B, H, h_prev=False, c_prev=False, w_off=0):
    return lambda: hip.lstm_step_fwd(zeros_view(B, 4 * H), zeros_view(B, H) if h_prev else None, zeros_view(B, H) if c_prev else None,
                                     zeros_view(4 * H, H, off=w_off), zeros_view(4 * H), zeros_view(B, 4 * H), zeros_view(B, H),
                                     zeros_view(B, H))


REFUSALS = {      # id -> (call, the C entry point its message must name)
    'matmul_nn_fwd w+1': (lambda: hip.matmul_nn_fwd(zeros_view(2, 4), zeros_view(4, 8, off=1)), 'gx_matmul_nn_fwd'),
    'matmul_nn_fwd N=6': (lambda: hip.matmul_nn_fwd(zeros_view(2, 4), zeros_view(4, 6)), 'gx_matmul_nn_fwd'),
    'matmul_nn_bwd w+1': (lambda: hip.matmul_nn_bwd(zeros_view(2, 4), zeros_view(4, 8, off=1), zeros_view(2, 8)), 'gx_matmul_nn_bwd'),
    'matmul_nn_bwd g+1': (lambda: hip.matmul_nn_bwd(zeros_view(2, 4), zeros_view(4, 8), zeros_view(2, 8, off=1)), 'gx_matmul_nn_bwd'),
    'matmul_nn_bwd dw+1': (lambda: hip.matmul_nn_bwd(zeros_view(2, 4), zeros_view(4, 8), zeros_view(2, 8),
                                                     out_dw=zeros_view(4, 8, off=1)), 'gx_matmul_nn_bwd'),
    'matmul_nn_bwd N=6': (lambda: hip.matmul_nn_bwd(zeros_view(2, 4), zeros_view(4, 6), zeros_view(2, 6)), 'gx_matmul_nn_bwd'),
    'lstm_seq_fwd T=17': (_lstm_seq_fwd(17, 2, 16), 'gx_lstm_seq_fwd'),
    'lstm_seq_bwd T=17': (_lstm_seq_bwd(17, 2, 16), 'gx_lstm_seq_bwd'),
    'lstm_seq_fwd B=129 H=256': (_lstm_seq_fwd(2, 129, 256), 'gx_lstm_seq_fwd'),
    'lstm_seq_bwd B=129 H=256': (_lstm_seq_bwd(2, 129, 256), 'gx_lstm_seq_bwd'),
    'lstm_seq_fwd w_hh+1': (_lstm_seq_fwd(2, 2, 16, w_off=1), 'gx_lstm_seq_fwd'),
    'lstm_step_fwd w_hh+1': (_lstm_step_fwd(2, 16, True, True, w_off=1), 'gx_lstm_step_fwd'),
    'lstm_step_fwd h_prev without c_prev': (_lstm_step_fwd(2, 16, True, False), 'gx_lstm_step_fwd'),
    'lstm_step_bwd no incoming gradient': (lambda: hip.lstm_step_bwd(None, None, zeros_view(64, 16), zeros_view(2, 64), zeros_view(2, 16),
                                                                     None, None, zeros_view(2, 64), zeros_view(2, 16)),
                                           'gx_lstm_step_bwd'),
}


@pytest.mark.parametrize('case', sorted(REFUSALS))
def test_refused_shapes(case):
    """Refused by a GX_CHECK_ARG ahead of every launch: GX_EINVAL (-1) with a message that names the entry point.  The operands are
    zeros of the refused shape inside their allocations: had a refusal gone, nothing would be out of range, only wrong."""
    call, entry = REFUSALS[case]
    with pytest.raises(GenesisHipError) as e:
        call()
    msg = str(e.value)
    assert 'failed (-1)' in msg and (entry + ':') in msg.split('failed (-1)', 1)[1], msg


# ----------------------------------------------------------------------------------------------------------------------- LSTM
PNAMES = ('w_ih', 'w_hh', 'b_ih', 'b_hh')


def _lstm_params(D, H, seed=5):
    g0 = torch.Generator().manual_seed(seed)
    return [(torch.rand(s, generator=g0) * 2 - 1) * 0.3 for s in ((4 * H, D), (4 * H, H), (4 * H,), (4 * H,))]


def _lstm_ref(T, B, D, H):
    """fp64 nn.LSTM and its autograd -> (x, g, params, out, dx, parameter gradients)."""
    ref = torch.nn.LSTM(D, H).double()
    params = _lstm_params(D, H)
    rp = (ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0)
    for p, v in zip(rp, params):
        p.data.copy_(v)
    x, g = rnd(T, B, D, seed=1), rnd(T, B, H, seed=2)
    xr = x.double().requires_grad_()
    out, _ = ref(xr)
    (out * g.double()).sum().backward()
    return x, g, params, out.detach(), xr.grad, [p.grad for p in rp]


def _lstm_run(x, g, params):
    from genesis_amd import functions as fn
    ps = [p.to(DEV).requires_grad_() for p in params]
    xg = x.to(DEV).requires_grad_()
    out = fn.LSTMFn.apply(xg, *ps)
    (out * g.to(DEV)).sum().backward()
    return [out.detach(), xg.grad] + [p.grad for p in ps]


def _lstm_check(got, ref):
    _, _, _, out_ref, dx_ref, pg_ref = ref
    close(got[0], out_ref, rtol=1e-5, atol=1e-5, msg='h')
    close(got[1], dx_ref, rtol=1e-4, atol=1e-5, msg='dx')
    for t, r, name in zip(got[2:], pg_ref, PNAMES):
        close(t, r, rtol=1e-4, atol=1e-5, msg='d' + name)


@pytest.mark.parametrize('T,B,D,H', LSTM_SHAPES)
def test_lstm_fn_against_fp64(T, B, D, H):
    """H = 48, 80: the forward's four waves do unequal work; B = 1, 16, 33: one ragged, one exact, three row tiles."""
    ref = _lstm_ref(T, B, D, H)
    _lstm_check(_lstm_run(*ref[:3]), ref)


@pytest.mark.parametrize('used', ['h+c', 'h', 'c'])
@pytest.mark.parametrize('state', [True, False])
@pytest.mark.parametrize('B,Din,H', CELL_SHAPES)
def test_lstm_cell_fn_against_fp64(B, Din, H, state, used):
    from genesis_amd import functions as fn
    ref = torch.nn.LSTMCell(Din, H).double()
    params = _lstm_params(Din, H, seed=6)
    rp = (ref.weight_ih, ref.weight_hh, ref.bias_ih, ref.bias_hh)
    for p, v in zip(rp, params):
        p.data.copy_(v)
    inp, gh, gc = rnd(B, Din, seed=1), rnd(B, H, seed=2), rnd(B, H, seed=3)
    hp, cp = (rnd(B, H, seed=4, scale=0.8), rnd(B, H, seed=5, scale=1.5)) if state else (None, None)

    def loss(h, c, dev):
        parts = ([(h * gh.to(dev).to(h.dtype)).sum()] if 'h' in used else []) + ([(c * gc.to(dev).to(c.dtype)).sum()] if 'c' in used else [])
        return sum(parts)
    leaves_r = [t.double().requires_grad_() if t is not None else None for t in (inp, hp, cp)]
    h_r, c_r = ref(leaves_r[0], (leaves_r[1], leaves_r[2]) if state else None)
    loss(h_r, c_r, 'cpu').backward()
    leaves = [t.to(DEV).requires_grad_() if t is not None else None for t in (inp, hp, cp)]
    ps = [p.to(DEV).requires_grad_() for p in params]
    h, c = fn.LSTMCellFn.apply(leaves[0], leaves[1], leaves[2], *ps)
    close(h, h_r, rtol=1e-5, atol=1e-5, msg='h')
    close(c, c_r, rtol=1e-5, atol=1e-5, msg='c')
    loss(h, c, DEV).backward()
    for t, r, name in zip(leaves, leaves_r, ('dinp', 'dh_prev', 'dc_prev')):
        if t is not None:
            close(t.grad, r.grad, rtol=1e-4, atol=1e-5, msg=name)
    for t, r, name in zip(ps, rp, PNAMES):
        close(t.grad, r.grad, rtol=1e-4, atol=1e-5, msg='d' + name)


def _spy(monkeypatch):
    calls = {}
    for name in ('lstm_seq_fwd', 'lstm_seq_bwd', 'lstm_step_fwd', 'lstm_step_bwd'):
        def wrap(*a, _real=getattr(hip, name), _n=name):
            calls[_n] = calls.get(_n, 0) + 1
            return _real(*a)
        monkeypatch.setattr(hip, name, wrap)
    return calls


def _expect_calls(calls, row, on):
    T = row['T']
    if on and row['path'] == 'seq':
        assert calls == dict(lstm_seq_fwd=1, lstm_seq_bwd=1), calls
    else:
        assert calls == dict(lstm_step_fwd=T, lstm_step_bwd=T), calls
    calls.clear()


@pytest.mark.parametrize('row', SEQ_ROWS, ids=lambda r: '%(T)dx%(B)dx%(H)d' % r)
def test_lstm_fn_with_the_whole_sequence_switch(row, monkeypatch):
    """LSTMFn with hip.LSTM_SEQ on against the same call with it off: outputs and every gradient bit for bit, and the launches the
    row declares (counted at the wrappers); the switched-off run against fp64 nn.LSTM."""
    T, B, H, D = row['T'], row['B'], row['H'], 5
    assert hip.lstm_seq_capacity(B, H) == (16 if row['grid'][0] * row['grid'][1] <= 128 else 0)
    ref = _lstm_ref(T, B, D, H)
    calls = _spy(monkeypatch)
    monkeypatch.setattr(hip, 'LSTM_SEQ', False)
    off = _lstm_run(*ref[:3])
    _expect_calls(calls, row, False)
    _lstm_check(off, ref)
    monkeypatch.setattr(hip, 'LSTM_SEQ', True)
    on = _lstm_run(*ref[:3])
    _expect_calls(calls, row, True)
    for name, a, b in zip(('h', 'dx') + PNAMES, on, off):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))


@pytest.mark.parametrize('row', SEQ_ROWS, ids=lambda r: '%(T)dx%(B)dx%(H)d' % r)
def test_ar_prior_kl_fn_with_the_whole_sequence_switch(row, monkeypatch):
    from genesis_amd import functions as fn
    T, B, H, D = row['T'], row['B'], row['H'], 8
    K = T + 1
    g0 = torch.Generator().manual_seed(3)
    mk = lambda *s: ((torch.rand(*s, generator=g0) * 2 - 1) * 0.3).to(DEV)  # noqa: E731
    params = [mk(4 * H, D), mk(4 * H, H), mk(4 * H), mk(4 * H), mk(2 * D, H), mk(2 * D)]
    z, log_q, gk = rnd(K, B, D, seed=1).to(DEV), rnd(K, B, seed=2).to(DEV), rnd(K, B, seed=3).to(DEV)

    def run():
        ps = [p.clone().requires_grad_() for p in params]
        zz, lq = z.clone().requires_grad_(), log_q.clone().requires_grad_()
        kl = fn.ARPriorKLFn.apply(zz, lq, *ps)
        (kl * gk).sum().backward()
        return [kl.detach(), zz.grad, lq.grad] + [p.grad for p in ps]
    calls = _spy(monkeypatch)
    monkeypatch.setattr(hip, 'LSTM_SEQ', False)
    off = run()
    _expect_calls(calls, row, False)
    monkeypatch.setattr(hip, 'LSTM_SEQ', True)
    on = run()
    _expect_calls(calls, row, True)
    assert all(bool(torch.isfinite(t).all()) for t in off)
    for i, (a, b) in enumerate(zip(on, off)):
        assert torch.equal(a, b), (i, float((a - b).abs().max()))


# --------------------------------------------------------------------------------------------- the autograd wrappers around them
@pytest.mark.parametrize('act', [None, 'relu'])
@pytest.mark.parametrize('bias,frozen', [(False, None), (True, None), (True, 'x'), (True, 'w'), (True, 'b'), (False, 'x'), (False, 'w')])
def test_linear_fn_3d_input_1x1_weight_and_frozen_operands(bias, frozen, act):
    """fn.linear with x [2,5,20] and a conv-shaped weight [7,20,1,1]; x, w and b take turns at not requiring a gradient (the
    need_dx / need_dw / need_db combinations of LinearFn.backward); exact operands, every gradient that is asked for present."""
    from genesis_amd import functions as fn
    x, w, b, g = ints(2, 5, 20, seed=1), ints(7, 20, 1, 1, seed=2), ints(7, seed=3) if bias else None, ints(2, 5, 7, seed=4)
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    br = b.double().requires_grad_() if bias else None
    yr = F.linear(xr, wr.view(7, 20), br)
    yr = F.relu(yr) if act else yr
    (yr * g.double()).sum().backward()
    xd, wd = x.to(DEV).requires_grad_(frozen != 'x'), w.to(DEV).requires_grad_(frozen != 'w')
    bd = b.to(DEV).requires_grad_(frozen != 'b') if bias else None
    y = fn.linear(xd, wd, bd, act)
    assert y.shape == (2, 5, 7) and torch.equal(y.detach().cpu(), lossless(yr.detach()))
    (y * g.to(DEV)).sum().backward()
    for name, t, r in (('x', xd, xr), ('w', wd, wr), ('b', bd, br)):
        if t is None:
            continue
        if frozen == name:
            assert t.grad is None, name
        else:
            assert t.grad is not None, 'the gradient of %s was dropped' % name
            assert t.grad.shape == t.shape and torch.equal(t.grad.cpu(), lossless(r.grad)), name


@pytest.mark.parametrize('exact', [True, False])
def test_two_head_linear_fn_with_scalar_heads_at_an_odd_column(exact):
    """TwoHeadLinearFn at (M, K, n1, n2) = (9, 20, 5, 7): both backward launches scalar (N % 4 != 0), the second head's columns
    start at column 5 of a 12-wide buffer (unaligned, ldg % 4 == 0) and its dh is added to the first's."""
    from genesis_amd import functions as fn
    mk = ints if exact else rnd
    h, w1, b1, w2, b2, g = mk(9, 20, seed=1), mk(5, 20, seed=2), mk(5, seed=3), mk(7, 20, seed=4), mk(7, seed=5), mk(9, 12, seed=6)
    ps = [t.double().requires_grad_() for t in (h, w1, b1, w2, b2)]
    ref = torch.cat((F.linear(ps[0], ps[1], ps[2]), F.linear(ps[0], ps[3], ps[4])), 1)
    ref.backward(g.double())
    pd = [t.to(DEV).requires_grad_() for t in (h, w1, b1, w2, b2)]
    out = fn.TwoHeadLinearFn.apply(*pd)
    out.backward(g.to(DEV))
    if exact:
        assert torch.equal(out.detach().cpu(), lossless(ref.detach()))
    else:
        close(out, ref, 2e-6, 2e-6, 'fwd')
    for a, b_, n in zip(pd, ps, ('dh', 'dw1', 'db1', 'dw2', 'db2')):
        if exact:
            assert torch.equal(a.grad.cpu(), lossless(b_.grad)), n
        else:
            close(a.grad, b_.grad, 5e-6, 5e-6, n)

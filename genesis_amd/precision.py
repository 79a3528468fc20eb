"""Matmul precision of the conv layers that multiply on the 16-bit matrix pipe, in torch's vocabulary
(torch.set_float32_matmul_precision).  One switch over the three kernel families of gx_matmul_precision
(include/genesis_hip.h):

  'highest'  every product of those layers on the fp32 matrix pipe;
  'high'     the default: fp32-equivalent products from three fp16 / six bf16 piece products;
  'medium'   every operand of those layers rounded once to bf16 (round to nearest even), one bf16 product per fp32 product,
             fp32 accumulation and fp32 tensors -- about 2^-8 relative error per product, fp32's exponent range.

torch's own global setting is NOT read: its default, 'highest', would change this project's default.  The environment variable
GENESIS_MATMUL_PRECISION=highest|high|medium sets the default of a fresh process (the one switch for an unchanged train.py).
Change the level between iterations: packed weights and captured graphs of the step machinery follow it on their next use
(trainer.TrainStep re-records its weight cache and re-captures its graphs at the next step(); the unchanged loop's captured
graphs are keyed by the level), and a backward pass whose forward ran at another level raises.  Several ranks: every rank must
set the same level (not checked).

A second switch, set_tapconv_precision('default' | 'medium'), does the same for the layers this one leaves on the fp32 pipe: the
small-level tap convs (gx_conv.hip's tap-conv kernels) and the strip weight gradient of the 72 x 72 canvas (gx_wstrip.hip) --
gx_tapconv_precision.  'medium' rounds their operands once to bf16 as above; 'default' is today's arithmetic.  The environment
variable GENESIS_TAPCONV_PRECISION=default|medium sets its default.  The two switches are independent; the step machinery keys
its packed state by both (key()), so a change of either between iterations re-records and re-captures, and a change between a
forward and its backward raises."""

LEVELS = ('highest', 'high', 'medium')
TAPCONV_MODES = {'default': 0, 'medium': 3}


def _lib():
    from . import _lib as L
    return L


def set_matmul_precision(precision):
    """'highest' | 'high' | 'medium' for the 16-bit-pipe conv families (gx_matmul_precision).  Returns None, like torch's."""
    if precision not in LEVELS:
        raise ValueError("matmul precision must be one of %s, got %r" % (', '.join(repr(v) for v in LEVELS), precision))
    L = _lib()
    rc = int(L.load().gx_matmul_precision(LEVELS.index(precision)))
    if rc < 0:
        raise L.GenesisHipError('gx_matmul_precision failed (%d): %s' % (rc, L.last_error()))


def get_matmul_precision():
    """The level in force: 'highest' | 'high' | 'medium', or None when the three families' modes were set one by one
    (gx_kq_precision / gx_wgq_precision / gx_wino_precision, or their environment variables) to no common level."""
    lv = level()
    return LEVELS[lv] if 0 <= lv < len(LEVELS) else None


def level():
    """The level as gx_matmul_precision_get returns it (0, 1, 2; GX_MATMUL_MIXED = 3): what the step machinery keys its packed
    state by, and what an autograd node records at its forward."""
    return int(_lib().load().gx_matmul_precision_get())


def check_backward(fwd_level):
    """Raises if the level changed since the forward whose backward is about to run (functions.ctx_bound)."""
    now = level()
    if now != fwd_level:
        names = LEVELS + ('mixed',)
        raise _lib().GenesisHipError(
            'matmul precision changed between a forward (%s) and its backward (%s): packed operands are laid out per level -- '
            'change it between iterations' % (names[fwd_level], names[now]))


def set_tapconv_precision(precision):
    """'default' | 'medium' for the tap-conv kernels and the strip weight gradient (gx_tapconv_precision).  Returns None."""
    if precision not in TAPCONV_MODES:
        raise ValueError("tap-conv precision must be one of %s, got %r" % (', '.join(repr(v) for v in TAPCONV_MODES), precision))
    L = _lib()
    rc = int(L.load().gx_tapconv_precision(TAPCONV_MODES[precision]))
    if rc < 0:
        raise L.GenesisHipError('gx_tapconv_precision failed (%d): %s' % (rc, L.last_error()))


def get_tapconv_precision():
    """The tap-conv mode in force: 'default' | 'medium'."""
    m = tap_mode()
    return next(k for k, v in TAPCONV_MODES.items() if v == m)


def tap_mode():
    """The tap-conv mode as gx_tapconv_precision_get returns it (0 or 3)."""
    return int(_lib().load().gx_tapconv_precision_get())


def key():
    """(matmul level, tap-conv mode): what the step machinery keys its packed state and captured graphs by, and what an autograd
    node records at its forward (check_backward_key)."""
    return (level(), tap_mode())


def check_backward_key(fwd_key):
    """Raises if either switch changed since the forward whose backward is about to run (functions.ctx_bound)."""
    now = key()
    if now[0] != fwd_key[0]:
        check_backward(fwd_key[0])
    if now[1] != fwd_key[1]:
        names = {v: k for k, v in TAPCONV_MODES.items()}
        raise _lib().GenesisHipError(
            'tap-conv precision changed between a forward (%s) and its backward (%s): packed operands are laid out per mode -- '
            'change it between iterations' % (names.get(fwd_key[1], fwd_key[1]), names.get(now[1], now[1])))

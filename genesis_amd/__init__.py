from .precision import get_matmul_precision, set_matmul_precision  # noqa: F401
from .precision import get_tapconv_precision, set_tapconv_precision  # noqa: F401


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """Import replacement for torch.nn.utils.clip_grad_norm_ on the HIP device: one reduction over all gradients, one in-place scale,
    no host read (genesis_amd.grad_guard.clip_grad_norm_, loaded on first use)."""
    from .grad_guard import clip_grad_norm_ as impl
    return impl(parameters, max_norm, norm_type, error_if_nonfinite, foreach)


def ModelEMA(model, decay, warmup=False):
    """Averaged weights for an unchanged loop: one launch per update, `with ema.applied():` to evaluate on them
    (genesis_amd.ema.ModelEMA, loaded on first use)."""
    from .ema import ModelEMA as impl
    return impl(model, decay, warmup)

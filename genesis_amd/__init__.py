from .precision import get_matmul_precision, set_matmul_precision  # noqa: F401
from .precision import get_tapconv_precision, set_tapconv_precision  # noqa: F401

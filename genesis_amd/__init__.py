from .precision import get_matmul_precision, set_matmul_precision  # noqa: F401

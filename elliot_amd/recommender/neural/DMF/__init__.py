from .deep_matrix_factorization import DMF  # noqa: F401

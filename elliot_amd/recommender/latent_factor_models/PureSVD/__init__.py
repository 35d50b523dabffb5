from .pure_svd import PureSVD  # noqa: F401

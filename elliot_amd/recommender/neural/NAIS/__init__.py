from .nais import NAIS  # noqa: F401

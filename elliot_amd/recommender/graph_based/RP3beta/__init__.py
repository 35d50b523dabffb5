from .rp3beta import RP3beta  # noqa: F401

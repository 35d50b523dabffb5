from .bprslim import BPRSlim  # noqa: F401

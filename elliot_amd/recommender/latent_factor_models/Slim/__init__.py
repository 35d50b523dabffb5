from .slim import Slim  # noqa: F401

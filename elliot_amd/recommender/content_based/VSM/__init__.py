from .vector_space_model import VSM  # noqa: F401

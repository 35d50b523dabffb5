from .userautorec import UserAutoRec  # noqa: F401

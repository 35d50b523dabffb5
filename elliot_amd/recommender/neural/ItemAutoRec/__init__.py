from .itemautorec import ItemAutoRec  # noqa: F401

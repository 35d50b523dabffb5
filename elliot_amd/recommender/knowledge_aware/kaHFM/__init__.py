from .kahfm import KaHFM

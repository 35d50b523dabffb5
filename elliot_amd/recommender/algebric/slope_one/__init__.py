from .slope_one import SlopeOne

from .delay import DelayFilter, DelayFilterBase  # noqa: F401
from .sensitivity import ComputeSystemSensitivity  # noqa: F401

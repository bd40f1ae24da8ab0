from .delay import DelayFilter, DelayFilterBase  # noqa: F401
from .sensitivity import ComputeSystemSensitivity  # noqa: F401
from .flagging import RFIMaskChisqHighDelay, RFITransientVisMask, RFIVisMask  # noqa: F401
from .transform import ReduceBase, ReduceChisq, ReduceVar  # noqa: F401

from .sensitivity import ComputeSystemSensitivity  # noqa: F401

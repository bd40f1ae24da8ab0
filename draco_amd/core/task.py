"""Tiny stand-in for caput's ``ContainerTask`` + ``config.Property`` [3P].

Config attributes are plain class attributes with the reference's names and defaults;
they can be overridden per instance by keyword (``DirtyMapMaker(nside=64)``) or from a
YAML-style dict (``task.read_config({"nside": 64})``), which is all the pipeline runner
does with them.  ``setup`` / ``process`` keep the reference signatures.
"""

from __future__ import annotations

import logging


class PipelineStopIteration(Exception):
    """Raised by a task's ``process`` when it has nothing more to produce (caput's ``PipelineStopIteration`` [3P])."""


class CaputConfigError(Exception):
    """A task's configuration does not fit what it was given (caput's ``config.CaputConfigError`` [3P])."""


class ContainerTask:
    _config_names: tuple = ()

    def __init__(self, **params):
        self.log = logging.getLogger(f"draco_amd.{type(self).__name__}")
        self.read_config(params)

    def read_config(self, params):
        for k, v in dict(params).items():
            if k not in self._all_config():
                raise AttributeError(f"{type(self).__name__} has no config property {k!r}")
            default = getattr(type(self), k)
            if default is not None and not isinstance(default, bool) and isinstance(default, (int, float)):
                v = type(default)(v)
            elif isinstance(default, bool):
                v = bool(v)
            setattr(self, k, v)

    @classmethod
    def _all_config(cls):
        names = ()
        for c in cls.__mro__:
            names += tuple(getattr(c, "_config_names", ()))
        return names

    def setup(self, *args):
        pass

    def process(self, *args):
        raise NotImplementedError

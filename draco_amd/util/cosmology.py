"""A small LambdaCDM background cosmology: what ``draco_amd.analysis.powerspec`` needs of ``cora.util.cosmology.Cosmology``
[3P] and nothing more -- ``comoving_distance(z)``, ``H(z)`` and ``_unit_distance``.

Distances are in h^-1 Mpc (cora's default ``unit="cosmo"`` as ``powerspec.py:1326-1369`` reads it): with ``H0 = 100 h
km/s/Mpc``

    comoving_distance(z) = (c / 100 km/s/Mpc) int_0^z dz' / E(z'),   E(z)^2 = Om (1 + z)^3 + Ok (1 + z)^2 + OL,

the line-of-sight comoving distance; radiation is left out.  ``H(z) = H0 E(z)`` is in s^-1, and ``_unit_distance`` is
one h^-1 Mpc in metres, so ``H(z) * _unit_distance / 1000`` is in km h / (Mpc s).

The defaults are a flat Planck-2018-like set (``H0 = 67.66``, ``omega_b = 0.04897``, ``omega_c = 0.26067``, ``omega_l =
0.69036``).  NOT CHECKED AGAINST CORA: neither cora's default parameters nor its units could be compared with these.
"""

from __future__ import annotations

import numpy as np

C_LIGHT = 299792458.0  # m / s
MEGA_PARSEC = 3.0856775814913673e22  # m (IAU 2015: 648000 / pi au, au = 149597870700 m)
_GL_ORDER = 64


class Cosmology:
    """LambdaCDM with ``H0`` in km/s/Mpc and the density parameters of baryons, cold dark matter and the cosmological
    constant today; ``omega_k = 1 - omega_b - omega_c - omega_l`` (taken as 0 below 1e-12)."""

    def __init__(self, H0=67.66, omega_b=0.04897, omega_c=0.26067, omega_l=0.69036):
        self.H0 = float(H0)
        self.omega_b = float(omega_b)
        self.omega_c = float(omega_c)
        self.omega_l = float(omega_l)
        self.omega_m = self.omega_b + self.omega_c
        k = 1.0 - (self.omega_m + self.omega_l)
        self.omega_k = 0.0 if abs(k) < 1e-12 else k
        self._unit_distance = MEGA_PARSEC / (self.H0 / 100.0)
        self._nodes, self._weights = np.polynomial.legendre.leggauss(_GL_ORDER)

    def _params(self):
        return (self.H0, self.omega_b, self.omega_c, self.omega_l)

    def __eq__(self, other):
        return isinstance(other, Cosmology) and self._params() == other._params()

    def __hash__(self):
        return hash(self._params())

    def __repr__(self):
        return f"Cosmology(H0={self.H0}, omega_b={self.omega_b}, omega_c={self.omega_c}, omega_l={self.omega_l})"

    def E(self, z):
        """``H(z) / H0``."""
        a = 1.0 + np.asarray(z, dtype=np.float64)
        return np.sqrt(self.omega_m * a**3 + self.omega_k * a**2 + self.omega_l)

    def H(self, z):
        """The Hubble rate in s^-1."""
        return self.H0 * 1.0e3 / MEGA_PARSEC * self.E(z)

    def comoving_distance(self, z):
        """The line-of-sight comoving distance to redshift ``z`` (scalar or array) in h^-1 Mpc: Gauss-Legendre of
        order 64 on ``[0, z]`` in float64 (the integrand is smooth: exact to rounding for any redshift of the 21 cm
        line)."""
        z = np.asarray(z, dtype=np.float64)
        zz = 0.5 * z[..., np.newaxis] * (self._nodes + 1.0)
        integral = 0.5 * z * np.sum(self._weights / self.E(zz), axis=-1)
        d = C_LIGHT / 1.0e5 * integral
        return float(d) if d.ndim == 0 else d

"""
Friction factors of spheroids (swarmrl/utils/utils.py:380-457), restated from
the formulas the reference cites: Perrin's translational factors
(https://link.springer.com/article/10.1007/BF02838005) and rotational factors
(https://en.wikipedia.org/wiki/Perrin_friction_factors).

Both take the semi-axis along the symmetry axis, the equatorial semi-axis and
the dynamic viscosity (plain numbers or pint quantities) and return the pair
(about / along the symmetry axis, about / along an equatorial axis).
"""

import numpy as np


def calc_ellipsoid_friction_factors_translation(
    axial_semiaxis, equatorial_semiaxis, dynamic_viscosity
):
    """
    Translational friction of a spheroid dragged along its symmetry axis
    (gamma_ax) and along an equatorial axis (gamma_eq).  With the eccentricity
    e = sqrt(1 - (short / long)^2) and the long semi-axis a:

    prolate, L = ln((1 + e) / (1 - e)):
        gamma_ax = 16 pi eta a e^3 / ((1 + e^2) L - 2 e)
        gamma_eq = 32 pi eta a e^3 / (2 e + (3 e^2 - 1) L)
    oblate (and the sphere's limit):
        gamma_ax = 8 pi eta a e^3 / (e sqrt(1 - e^2) - (1 - 2 e^2) asin e)
        gamma_eq = 16 pi eta a e^3 / (-e sqrt(1 - e^2) + (1 + 2 e^2) asin e)
    """
    prolate = axial_semiaxis > equatorial_semiaxis
    long_, short = (
        (axial_semiaxis, equatorial_semiaxis) if prolate else (equatorial_semiaxis, axial_semiaxis)
    )
    # (the ratio as a plain number: quantities need not support numpy's functions)
    ecc = np.sqrt(1 - float(short**2 / long_**2))
    scale = np.pi * dynamic_viscosity * long_ * ecc**3
    if prolate:
        log_term = np.log((1 + ecc) / (1 - ecc))
        gamma_ax = 16 * scale / ((1 + ecc**2) * log_term - 2 * ecc)
        gamma_eq = 32 * scale / (2 * ecc + (3 * ecc**2 - 1) * log_term)
    else:
        root = ecc * np.sqrt(1 - ecc**2)
        asin = np.arcsin(ecc)
        gamma_ax = 8 * scale / (root - (1 - 2 * ecc**2) * asin)
        gamma_eq = 16 * scale / (-root + (1 + 2 * ecc**2) * asin)
    return gamma_ax, gamma_eq


def calc_ellipsoid_friction_factors_rotation(
    axial_semiaxis, equatorial_semiaxis, dynamic_viscosity
):
    """
    Rotational friction of a spheroid about its symmetry axis (gamma_ax) and
    about an equatorial axis (gamma_eq): Perrin's factors times the friction
    8 pi eta a b^2 of the sphere of equal volume.  With p = axial / equatorial
    and xi = sqrt(|p^2 - 1|) / p:

        S    = 2 atanh(xi) / xi (prolate),  2 atan(xi) / xi (oblate)
        f_ax = (4 / 3) (p^2 - 1) / (2 p^2 - S)
        f_eq = (4 / 3) (p^-2 - p^2) / (2 - S (2 - p^-2))
    """
    p = float(axial_semiaxis / equatorial_semiaxis)
    xi = np.sqrt(np.abs(p**2 - 1)) / p
    s_factor = 2 * (np.arctanh(xi) if p > 1 else np.arctan(xi)) / xi
    f_ax = 4.0 / 3.0 * (p**2 - 1) / (2 * p**2 - s_factor)
    f_eq = 4.0 / 3.0 * (p**-2 - p**2) / (2 - s_factor * (2 - p**-2))
    sphere = 8 * np.pi * dynamic_viscosity * axial_semiaxis * equatorial_semiaxis**2
    return sphere * f_ax, sphere * f_eq

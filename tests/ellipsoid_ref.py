"""
The Gay-Berne pair of the ellipsoid path in numpy fp64, TEST INFRASTRUCTURE
ONLY: ESPResSo's documented potential with k2 = 1, nu = 1, mu = 2 (so chi' = 0
and the well depth depends on u_i . u_j alone), shifted at the cutoff.

    r = x_j - x_i,  rh = r / |r|,  a = rh . u_i,  b = rh . u_j,  c = u_i . u_j
    chi   = (k^2 - 1) / (k^2 + 1)
    g     = 1 - (chi / 2) [(a + b)^2 / (1 + chi c) + (a - b)^2 / (1 - chi c)]
    sigma = sigma0 / sqrt(g),   eps = eps0 / sqrt(1 - chi^2 c^2)
    X     = sigma0 / (|r| - sigma + sigma0),  Xc the same at r_cut
    U     = 4 eps [X^12 - X^6 - Xc^12 + Xc^6]     (|r| < r_cut)

Every function broadcasts over leading axes; vectors have a last axis of 2.
"""

import numpy as np


def chi_of(kappa):
    return (kappa**2 - 1.0) / (kappa**2 + 1.0)


def _parts(r, ui, uj, kappa, sigma0):
    r, ui, uj = (np.asarray(v, np.float64) for v in (r, ui, uj))
    chi = chi_of(kappa)
    dist = np.sqrt((r * r).sum(-1))
    rh = r / dist[..., None]
    a, b, c = (rh * ui).sum(-1), (rh * uj).sum(-1), (ui * uj).sum(-1)
    g = 1.0 - 0.5 * chi * ((a + b) ** 2 / (1.0 + chi * c) + (a - b) ** 2 / (1.0 - chi * c))
    sigma = sigma0 / np.sqrt(g)
    return chi, dist, rh, a, b, c, g, sigma


def overlap_x(r, ui, uj, kappa, sigma0):
    """X = sigma0 / (|r| - sigma + sigma0) (inf or negative: |r| - sigma + sigma0 <= 0)."""
    _, dist, _, _, _, _, _, sigma = _parts(r, ui, uj, kappa, sigma0)
    with np.errstate(divide="ignore"):
        return sigma0 / (dist - sigma + sigma0)


def energy(r, ui, uj, kappa, sigma0, eps0, r_cut):
    chi, dist, _, _, _, c, _, sigma = _parts(r, ui, uj, kappa, sigma0)
    eps = eps0 / np.sqrt(1.0 - chi**2 * c**2)
    x = sigma0 / (dist - sigma + sigma0)
    xc = sigma0 / (r_cut - sigma + sigma0)
    u = 4.0 * eps * (x**12 - x**6 - xc**12 + xc**6)
    return np.where(dist < r_cut, u, 0.0)


def force_torque(r, ui, uj, kappa, sigma0, eps0, r_cut):
    """Analytic force on i (+dU/dr, r = x_j - x_i) and z-torque on i
    (-(u_i x dU/du_i)_z) by the chain rule through (|r|, a, b, c); zero
    outside the cutoff."""
    chi, dist, rh, a, b, c, g, sigma = _parts(r, ui, uj, kappa, sigma0)
    ui, uj = np.asarray(ui, np.float64), np.asarray(uj, np.float64)
    one_m = 1.0 - chi**2 * c**2
    eps = eps0 / np.sqrt(one_m)
    x = sigma0 / (dist - sigma + sigma0)
    xc = sigma0 / (r_cut - sigma + sigma0)
    u = 4.0 * eps * (x**12 - x**6 - xc**12 + xc**6)
    # dU/dX X^2 / sigma0 at X and at Xc
    w = 4.0 * eps * (12.0 * x**13 - 6.0 * x**7) / sigma0
    wc = 4.0 * eps * (12.0 * xc**13 - 6.0 * xc**7) / sigma0
    du_dr = -w                       # at fixed sigma
    du_dsigma = w - wc
    du_dg = du_dsigma * (-0.5 * sigma / g)
    p, m = (a + b) / (1.0 + chi * c), (a - b) / (1.0 - chi * c)
    dg_da, dg_db = -chi * (p + m), -chi * (p - m)
    dg_dc = 0.5 * chi**2 * (p**2 - m**2)
    du_da, du_db = du_dg * dg_da, du_dg * dg_db
    du_dc = du_dg * dg_dc + u * chi**2 * c / one_m
    # d a / d r = (u_i - a rh) / |r|, likewise b
    grad = (du_dr[..., None] * rh
            + du_da[..., None] * (ui - a[..., None] * rh) / dist[..., None]
            + du_db[..., None] * (uj - b[..., None] * rh) / dist[..., None])
    dudu = du_da[..., None] * rh + du_dc[..., None] * uj
    torque = -(ui[..., 0] * dudu[..., 1] - ui[..., 1] * dudu[..., 0])
    inside = dist < r_cut
    return np.where(inside[..., None], grad, 0.0), np.where(inside, torque, 0.0)

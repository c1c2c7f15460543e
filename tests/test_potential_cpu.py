"""
The gridded external potential without a GPU: the numpy restatement of the
device's fixed fp32 sequence (tests/potential_ref.py) against an fp64
restatement of the reference's construction (espresso.py:1026-1036:
np.pad(mode="wrap"), element (0, 0, 0) at -h / 2, trilinear gradient), an
exactness property of the sequence, and SwarmEngine.add_external_potential's
host validation (with the add_flowfield / add_lattice_boltzmann refusals).
"""

import numpy as np
import pytest

import potential_ref as pr
from oracle import oracle

BOX = [35.0, 20.0, 28.0]  # three different edge lengths


def _max_step(phi):
    """max |phi[cell] - phi[neighbour cell]| over the periodic grid."""
    return max(float(np.max(np.abs(np.roll(phi, -1, axis=a) - phi))) for a in range(3))


def _positions(rng, shape, n_random):
    """Random positions plus, per axis, two inside the first and two inside
    the last half cell."""
    h = np.asarray(BOX) / np.asarray(shape)
    pos = rng.random((n_random, 3)) * BOX
    edge = []
    for a in range(3):
        for frac in (0.1, 0.45):
            lo = rng.random(3) * BOX
            lo[a] = frac * 0.5 * h[a]
            hi = rng.random(3) * BOX
            hi[a] = BOX[a] - frac * 0.5 * h[a]
            edge += [lo, hi]
    return np.concatenate([pos, np.asarray(edge)]), h


@pytest.mark.parametrize("dims,shape", [(2, (7, 5, 1)), (3, (5, 3, 4))])
def test_restatement_matches_the_reference_construction(dims, shape):
    """Bound (derived, not fitted): 16 * 2^-24 * max|dphi| / min h -- six fp32
    roundings of magnitudes up to 2 max|dphi| and the 2^-24 truncation of the
    weight t, each divided by the spacing."""
    rng = np.random.default_rng(11)
    pos, h = _positions(rng, shape, 300)
    if dims == 2:
        pos[:, 2] = 0.0
    i, j, k = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    phi = (3.0 * np.sin(2 * np.pi * i / shape[0]) * np.cos(2 * np.pi * j / shape[1])
           + np.cos(2 * np.pi * k / shape[2]) + rng.normal(size=shape)).astype(np.float32)
    q = np.stack([oracle.to_fixed(pos[:, a], BOX[a])[0] for a in range(3)])
    for a in range(dims):  # both half cells at the periodic seam occur on every axis
        P = q[a].astype(np.uint64) * np.uint64(shape[a])
        assert np.any(P < (1 << 31)) and np.any(P >= shape[a] * (1 << 32) - (1 << 31)), a
    F = pr.potential_force(phi, q, pr.inv_spacing(h), dims)
    folded = (q.astype(np.float64) / 2.0 ** 32 * np.asarray(BOX)[:, None]).T
    ref = pr.reference_force(phi.astype(np.float64), folded, h)
    hs = h[:dims]
    bound = 16 * 2.0 ** -24 * _max_step(phi) / hs.min()
    err = np.max(np.abs(F.astype(np.float64) - ref))
    print("potential restatement dims", dims, "max error", err, "bound", bound)
    assert np.max(np.abs(ref[:dims])) > 0.1  # a field worth comparing
    assert err <= bound
    if dims == 2:
        assert np.all(F[2] == 0.0) and np.all(ref[2] == 0.0)


def test_linear_potential_gives_the_exact_constant_force():
    """phi linear in the cell index along x: away from the seam both
    x-differences are the same fp32 number, so Fx = -(dphi inv_hx) exactly
    whatever the weights, and Fy = 0."""
    rng = np.random.default_rng(12)
    shape = (7, 5, 1)
    h = np.asarray(BOX) / np.asarray(shape)
    step = np.float32(0.375)
    phi = (step * np.arange(7, dtype=np.float32))[:, None, None] * np.ones(shape, np.float32)
    pos = rng.random((400, 3)) * BOX
    q = np.stack([oracle.to_fixed(pos[:, a], BOX[a])[0] for a in range(3)])
    inv_h = pr.inv_spacing(h)
    F = pr.potential_force(phi, q, inv_h, 2)
    i0, i1, _ = pr.grid_coords(q[0], 7)
    inside = i1 == i0 + 1  # not across the seam (cells 6 -> 0)
    assert np.count_nonzero(inside) > 200 and np.count_nonzero(~inside) > 10
    assert np.all(F[0][inside] == -(step * inv_h[0]))
    assert np.all(F[1] == 0.0)
    # across the seam the ramp falls back by six steps
    assert np.all(F[0][~inside] == -((np.float32(0.0) - np.float32(6) * step) * inv_h[0]))


def test_grid_coords_are_exact_at_cell_centres_and_faces():
    n = 5
    q = np.array([0, (1 << 32) // 10, (1 << 32) // 10 - 1, (1 << 31), (1 << 32) - 1], np.uint32)
    i0, i1, t = pr.grid_coords(q, n)
    # q = 0: the box face, half-way between the last and the first cell centre
    assert (i0[0], i1[0], t[0]) == (4, 0, np.float32(0.5))
    # q n just at / below 2^31 (q = 2^32 / 10 rounded down): the first centre
    assert i0[1] == 4 and i1[1] == 0 and t[1] > np.float32(0.999)
    assert i0[3] == 2 and i1[3] == 3 and t[3] == 0.0  # q = 1/2: the centre of cell 2 (2.5 / 5)
    assert i0[4] == 4 and i1[4] == 0 and t[4] < np.float32(0.5)


# ------------------------------------------------- host validation (no GPU)
def _runner(tmp_path, n_dims=2, n_colloids=20):
    from test_rod_cpu import _runner as rod_runner

    return rod_runner(tmp_path, n_dims=n_dims, n_colloids=n_colloids)


def _pot(ureg, shape=(10, 5, 1), value=1.0):
    return ureg.Quantity(np.full(shape, value), "sim_energy")


def _h(ureg, h=(5.0, 10.0, 50.0)):
    return ureg.Quantity(np.asarray(h, float), "micrometer")


def test_add_external_potential_keeps_the_field_and_sums_equal_grids(tmp_path):
    ureg, runner = _runner(tmp_path)
    runner.add_external_potential(_pot(ureg), _h(ureg))
    assert runner._potential["phi"].shape == (10, 5, 1)
    assert runner._potential["phi"].dtype == np.float64
    assert np.array_equal(runner._potential["h"], [5.0, 10.0, 50.0])
    assert len(runner.system.constraints) == 1
    runner.add_external_potential(_pot(ureg, value=0.25), _h(ureg))  # ESPResSo sums constraints
    assert np.all(runner._potential["phi"] == 1.25)
    assert len(runner.system.constraints) == 1
    with pytest.raises(NotImplementedError, match="different grids"):
        runner.add_external_potential(_pot(ureg, (5, 5, 1)), _h(ureg, (10.0, 10.0, 50.0)))
    assert np.all(runner._potential["phi"] == 1.25)
    # the unit conversion: joule -> sim_energy
    ureg2, runner2 = _runner(tmp_path / "b")
    e = ureg2.Quantity(np.full((10, 5, 1), 1.0), "sim_energy").m_as("joule")
    runner2.add_external_potential(ureg2.Quantity(2.0 * e, "joule"), _h(ureg2))
    np.testing.assert_allclose(runner2._potential["phi"], 2.0, rtol=1e-12)


def test_add_external_potential_refusals(tmp_path):
    ureg, runner = _runner(tmp_path)
    with pytest.raises(ValueError,
                       match=r"potential must have shape \(n_cells_x, n_cells_y, n_cells_z\)"):
        runner.add_external_potential(ureg.Quantity(np.ones((10, 5)), "sim_energy"), _h(ureg))
    with pytest.raises(ValueError, match="Grid spacings must have length of 3"):
        runner.add_external_potential(_pot(ureg), _h(ureg, (5.0, 10.0)))
    with pytest.raises(ValueError, match="tile the box"):
        runner.add_external_potential(_pot(ureg), _h(ureg, (5.0, 9.0, 50.0)))
    with pytest.raises(ValueError, match="one cell in z"):
        runner.add_external_potential(_pot(ureg, (10, 5, 2)), _h(ureg, (5.0, 10.0, 25.0)))
    bad = np.ones((10, 5, 1))
    bad[3, 2, 0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        runner.add_external_potential(ureg.Quantity(bad, "sim_energy"), _h(ureg))
    assert runner._potential is None and runner.system.constraints == []
    # a 3-D engine takes nz > 1
    ureg3, runner3 = _runner(tmp_path / "c", n_dims=3)
    runner3.add_external_potential(_pot(ureg3, (10, 5, 2)), _h(ureg3, (5.0, 10.0, 25.0)))
    assert runner3._potential["phi"].shape == (10, 5, 2)
    # not after the first integrate
    runner.integration_initialised = True
    with pytest.raises(RuntimeError, match="after the first call to integrate"):
        runner.add_external_potential(_pot(ureg), _h(ureg))


def test_external_potential_and_rod_refuse_each_other(tmp_path):
    from test_rod_cpu import _rod_args

    ureg, runner = _runner(tmp_path / "a")
    runner.add_external_potential(_pot(ureg), _h(ureg))
    with pytest.raises(NotImplementedError, match="external potential"):
        runner.add_rod(**_rod_args(ureg))
    assert runner._rod is None and len(runner.colloids) == 20
    ureg, runner = _runner(tmp_path / "b")
    runner.add_rod(**_rod_args(ureg))
    with pytest.raises(NotImplementedError, match="external potential"):
        runner.add_external_potential(_pot(ureg), _h(ureg))
    assert runner._potential is None and runner.system.constraints == []


def test_flowfield_and_lattice_boltzmann_refuse_the_brownian_thermostat(tmp_path):
    """The reference's messages (espresso.py:887-891, 967-971)."""
    ureg, runner = _runner(tmp_path)
    assert runner.params.thermostat_type == "brownian"
    with pytest.raises(RuntimeError) as exc:
        runner.add_flowfield(ureg.Quantity(np.zeros((2, 2, 1, 3)), "sim_velocity"),
                             ureg.Quantity(1.0, "sim_mass/sim_time"), _h(ureg))
    assert str(exc.value) == ("Coupling to a flowfield does not work with a Brownian thermostat."
                              " Use 'langevin'.")
    with pytest.raises(RuntimeError) as exc:
        runner.add_lattice_boltzmann(agrid=ureg.Quantity(1.0, "micrometer"))
    assert str(exc.value) == ("Coupling to lattice boltzmann does not work with a Brownian"
                              " thermostat. Use 'langevin'.")

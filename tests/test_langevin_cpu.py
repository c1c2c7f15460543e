"""
The Langevin thermostat and the flow field without a GPU: the CPU restatement
of the kernel's fixed fp32 sequence (tests/csrc/langevin_oracle.c) against the
fp64 statement of the scheme (tests/langevin_ref.py) -- flow sampling, the
deterministic drift, the stationary variances of the discrete scheme, the
carry of the velocities from run to run -- and SwarmEngine's host logic under
thermostat_type="langevin" (add_flowfield, the out-of-scope combinations).
"""

import numpy as np
import pytest

import langevin_oracle as lo
import langevin_ref as lr
from oracle import oracle

TWO32 = 2.0 ** 32


def _params(box, dt, kT, species, seed=5):
    return oracle.make_params(box, dt, kT, 1.0, seed, species)


# ------------------------------------------------------------ flow sampling
def test_flow_sample_matches_the_reference_construction():
    """An 8 x 4 grid (not square: a transposed index shows).  Tolerance
    4 * 2^-24 * max|u| per component: three rounded operations per
    interpolation stage."""
    rng = np.random.default_rng(21)
    box = np.array([16.0, 12.0, 12.0])
    shape = (8, 4, 1)
    h = box / np.asarray(shape)
    u = rng.uniform(-1.0, 1.0, size=shape + (3,)).astype(np.float32)
    centres = np.array([[(i + 0.5) * h[0], (j + 0.5) * h[1], 0.0]
                        for i in range(8) for j in range(4)])
    faces = np.array([[i * h[0], (j + 0.25) * h[1], 0.0] for i in range(8) for j in range(4)]
                     + [[(i + 0.75) * h[0], j * h[1], 0.0] for i in range(8) for j in range(4)])
    edges = []
    for a in range(2):  # the half cells at both box edges, where the field wraps
        for frac in (0.1, 0.45, 0.9):
            lo_, hi_ = rng.random(3) * box, rng.random(3) * box
            lo_[a], hi_[a] = frac * 0.5 * h[a], box[a] - frac * 0.5 * h[a]
            edges += [lo_, hi_]
    pos = np.concatenate([centres, faces, np.asarray(edges), rng.random((200, 3)) * box])
    pos[:, 2] = 0.0
    q = np.stack([oracle.to_fixed(pos[:, a], box[a])[0] for a in range(3)])
    for a in range(2):  # both half cells at the periodic seam occur on each axis
        P = q[a].astype(np.uint64) * np.uint64(shape[a])
        assert np.any(P < (1 << 31)) and np.any(P >= shape[a] * (1 << 32) - (1 << 31)), a
    got = lo.flow_sample(u, q)
    folded = (q.astype(np.float64) / TWO32 * box[:, None]).T
    ref = lr.flow_sample(u, folded, h)
    umax = float(np.max(np.abs(u[..., :2])))
    bound = 4 * 2.0 ** -24 * umax
    err = np.max(np.abs(got.T.astype(np.float64) - ref[:, :2]))
    print("flow sampling: max error", err, "bound", bound)
    assert np.max(np.abs(ref[:, :2])) > 0.5  # a field worth comparing
    assert err <= bound
    # at a cell centre the value is the cell's own
    got_c = got[:, :32].T.reshape(8, 4, 2)
    assert np.max(np.abs(got_c - u[:, :, 0, :2])) <= bound


# -------------------------------------------------------- deterministic drift
def test_deterministic_drift_follows_the_fp64_recurrence():
    """kT = 0, one particle, a uniform flow and a constant force, 100
    sub-steps.  Displacement within 1e-4 relative plus 100 L 2^-32 (about
    3 * 2^-24 relative per step sums to below 2e-5; one fixed-point rounding
    per step)."""
    L = 40.0
    box = [L, L, L]
    dt, m, gt, gflow = 0.01, 2.0, 3.0, 5.0  # dt (gt + gflow) / m = 0.04
    p = _params(box, dt, 0.0, [(1.0, gt, 7.0, m, 3.0)])
    uflow = np.zeros((4, 4, 1, 3), np.float32)
    uflow[..., 0], uflow[..., 1] = 1.5, -0.75
    f = np.array([0.8, 0.3])
    st = oracle.state_from_positions(np.array([[11.0, 23.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]),
                                     box)
    x0 = oracle.unwrapped(st, box)[0, :2]
    f_ext = np.array([[f[0]], [f[1]], [0.0]], np.float32)
    out, v, w, info = lo.lv_run(p, st, np.zeros((3, 1)), np.zeros(1), np.zeros(1, np.uint8),
                                np.zeros(1, np.float32), np.zeros(1, np.float32), 100,
                                f_ext=f_ext, flow=(uflow, gflow))
    x_ref, v_ref = lr.recurrence(x0, [0.0, 0.0], 100, dt, m, gt, f_ext[:2, 0].astype(np.float64),
                                 gamma_flow=gflow, flow=lambda x: uflow[0, 0, 0, :2])
    disp = oracle.unwrapped(out, box)[0, :2] - x0
    disp_ref = x_ref - x0
    tol = 1e-4 * np.abs(disp_ref) + 100 * L * 2.0 ** -32
    print("drift", disp, "fp64", disp_ref, "tolerance", tol)
    assert np.all(np.abs(disp_ref) > 0.3)  # the particle went somewhere
    assert np.all(np.abs(disp - disp_ref) <= tol)
    assert np.all(np.abs(v[:2, 0] - v_ref) <= 1e-4 * np.abs(v_ref))
    assert w[0] == 0.0 and out["ang"][0] == st["ang"][0]


# -------------------------------------------------------- stationary variances
def test_stationary_variances_of_the_discrete_scheme():
    """4 x 2048 free particles, area fraction below 1e-4, a = dt gamma / m =
    0.2, sampled after 200 sub-steps.  <v^2> per axis is (kT / m) / (1 - a/2)
    within 7 % (at least 4.4 sigma at 8192 samples; the seed is fixed), and so
    is <omega^2> with a_r; the naive kT / m lies outside."""
    n, envs, steps = 2048, 4, 200
    L = 9200.0
    box = [L, L, L]
    kT, dt, m, gt, inertia, gr = 1.3, 0.01, 1.0, 20.0, 2.0, 30.0
    a_t, a_r = dt * gt / m, dt * gr / inertia
    assert a_t == pytest.approx(0.2) and n * np.pi / L ** 2 <= 1e-4
    p = _params(box, dt, kT, [(1.0, gt, gr, m, inertia)], seed=77)
    side = 46  # a jittered lattice: nobody within reach of a neighbour
    rng = np.random.default_rng(3)
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)
    vs, ws, pairs = [], [], 0
    for e in range(envs):
        pos = np.zeros((n, 3))
        pos[:, :2] = (ij[:n] + 0.5 + rng.uniform(-0.2, 0.2, (n, 2))) * (L / side)
        st = oracle.state_from_positions(pos, np.tile([1.0, 0.0, 0.0], (n, 1)), box)
        _, v, w, info = lo.lv_run(p, st, np.zeros((3, n)), np.zeros(n), np.zeros(n, np.uint8),
                                  np.zeros(n, np.float32), np.zeros(n, np.float32), steps, env=e)
        vs.append(v)
        ws.append(w)
        pairs += info["pairs"]
    assert pairs == 0  # no pair ever formed
    v = np.concatenate(vs, axis=1).astype(np.float64)
    w = np.concatenate(ws).astype(np.float64)
    want_v, want_w = lr.stationary_variance(kT, m, a_t), lr.stationary_variance(kT, inertia, a_r)
    got = [np.mean(v[0] ** 2), np.mean(v[1] ** 2), np.mean(w ** 2)]
    print("variances", got, "expected", want_v, want_v, want_w)
    assert abs(got[0] / want_v - 1.0) <= 0.07
    assert abs(got[1] / want_v - 1.0) <= 0.07
    assert abs(got[2] / want_w - 1.0) <= 0.07
    assert abs((kT / m) / want_v - 1.0) > 0.07  # the discrete factor is told apart
    assert np.all(v[2] == 0.0)
    assert abs(np.mean(v[0])) < 5 * np.sqrt(want_v / v.shape[1])  # no drift


# ------------------------------------------------------------------ carry-over
def _dense_case(n=60, seed=9):
    rng = np.random.default_rng(seed)
    box = [24.0, 18.0, 24.0]
    species = [(1.0, 2.0, 3.0, 0.5, 0.8), (0.7, 1.5, 2.0, 0.3, 0.4)]
    p = _params(box, 0.005, 0.4, species, seed=123)
    side = int(np.ceil(np.sqrt(n)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)
    pos = np.zeros((n, 3))
    pos[:, :2] = (ij[:n] + 0.5 + rng.uniform(-0.3, 0.3, (n, 2))) * [box[0] / side, box[1] / side]
    ang = rng.uniform(0, 2 * np.pi, n)
    st = oracle.state_from_positions(pos, np.stack([np.cos(ang), np.sin(ang), 0 * ang], 1), box)
    sp = (np.arange(n) % 2).astype(np.uint8)
    fs = rng.uniform(1.0, 3.0, n).astype(np.float32)
    tz = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    return p, st, sp, fs, tz


def test_velocities_carry_from_run_to_run():
    """run(10) then run(10) equals run(20) bit for bit (reuse_forces = 0)."""
    p, st, sp, fs, tz = _dense_case()
    n = len(sp)
    z3, z1 = np.zeros((3, n), np.float32), np.zeros(n, np.float32)
    a, va, wa, ia = lo.lv_run(p, st, z3, z1, sp, fs, tz, 20)
    b, vb, wb, ib = lo.lv_run(p, st, z3, z1, sp, fs, tz, 10)
    assert np.any(vb != 0.0) and np.any(wb != 0.0)
    b, vb, wb, ib2 = lo.lv_run(p, b, vb, wb, sp, fs, tz, 10, step0=10)
    assert ia["pairs"] > 0 and ia["pairs"] == ib["pairs"] + ib2["pairs"]
    for k in ("q", "img", "ang"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(va, vb) and np.array_equal(wa, wb)
    # and the velocities matter: a second run from rest differs
    c, vc, wc, _ = lo.lv_run(p, b, z3, z1, sp, fs, tz, 1, step0=20)
    d, vd, wd, _ = lo.lv_run(p, b, vb, wb, sp, fs, tz, 1, step0=20)
    assert not np.array_equal(c["q"], d["q"])


# ------------------------------------------------- host logic (no GPU)
def _runner(tmp_path, n_dims=2, n_colloids=5, thermostat="langevin", periodic=True, **colloid_kw):
    from swarmrl_amd.engine import MDParams, SwarmEngine
    from swarmrl_amd.units import UnitRegistry

    ureg = UnitRegistry()
    params = MDParams(
        ureg=ureg,
        fluid_dyn_viscosity=ureg.Quantity(8.9e-4, "pascal * second"),
        WCA_epsilon=0.1 * ureg.Quantity(300, "kelvin") * ureg.boltzmann_constant,
        temperature=ureg.Quantity(300, "kelvin"),
        box_length=ureg.Quantity(3 * [50], "micrometer"),
        time_step=ureg.Quantity(0.0001, "second"),
        time_slice=ureg.Quantity(0.1, "second"),
        write_interval=ureg.Quantity(0.1, "second"),
        thermostat_type=thermostat,
        periodic=periodic,
    )
    runner = SwarmEngine(params, n_dims=n_dims, out_folder=tmp_path, write_chunk_size=1)
    if n_colloids:
        kw = dict(mass=ureg.Quantity(1.0, "sim_mass"),
                  rinertia=ureg.Quantity(3 * [1.0], "sim_rinertia"))
        kw.update(colloid_kw)
        runner.add_colloids(n_colloids, ureg.Quantity(1.0, "micrometer"),
                            ureg.Quantity(np.array([25, 25, 0]), "micrometer"),
                            ureg.Quantity(20, "micrometer"), type_colloid=0, **kw)
    return ureg, runner


def _flow(ureg, shape=(10, 5, 1, 3), value=1.0):
    return ureg.Quantity(np.full(shape, value), "sim_velocity")


def _gamma(ureg, g=2.0):
    return ureg.Quantity(g, "sim_mass/sim_time")


def _h(ureg, h=(5.0, 10.0, 50.0)):
    return ureg.Quantity(np.asarray(h, float), "micrometer")


def test_add_flowfield_keeps_the_field_and_sums_equal_grids(tmp_path):
    ureg, runner = _runner(tmp_path)
    runner.add_flowfield(_flow(ureg), _gamma(ureg), _h(ureg))
    assert runner._flow["u"].shape == (10, 5, 1, 3) and runner._flow["gamma"] == 2.0
    assert np.array_equal(runner._flow["h"], [5.0, 10.0, 50.0])
    assert len(runner.system.constraints) == 1
    runner.add_flowfield(_flow(ureg, value=0.25), _gamma(ureg), _h(ureg))
    assert np.all(runner._flow["u"] == 1.25) and len(runner.system.constraints) == 1
    with pytest.raises(NotImplementedError, match="different grids or with different friction"):
        runner.add_flowfield(_flow(ureg), _gamma(ureg, 3.0), _h(ureg))
    with pytest.raises(NotImplementedError, match="different grids or with different friction"):
        runner.add_flowfield(_flow(ureg, (5, 5, 1, 3)), _gamma(ureg), _h(ureg, (10.0, 10.0, 50.0)))
    assert np.all(runner._flow["u"] == 1.25)
    # the unit conversion: micrometer / second is the simulation's velocity unit
    ureg2, runner2 = _runner(tmp_path / "b")
    runner2.add_flowfield(ureg2.Quantity(np.full((10, 5, 1, 3), 3e-6), "meter/second"),
                          ureg2.Quantity(1.0, "sim_mass/sim_time"), _h(ureg2))
    np.testing.assert_allclose(runner2._flow["u"], 3.0, rtol=1e-12)


def test_add_flowfield_refusals(tmp_path):
    ureg, runner = _runner(tmp_path)
    with pytest.raises(ValueError) as exc:
        runner.add_flowfield(ureg.Quantity(np.ones((10, 5, 3)), "sim_velocity"), _gamma(ureg),
                             _h(ureg))
    assert str(exc.value) == "flowfield must have shape (n_cells_x, n_cells_y, n_cells_z, 3)"
    with pytest.raises(ValueError) as exc:
        runner.add_flowfield(_flow(ureg), _gamma(ureg), _h(ureg, (5.0, 10.0)))
    assert str(exc.value) == "Grid spacings must have length of 3"
    with pytest.raises(ValueError, match="tile the box"):
        runner.add_flowfield(_flow(ureg), _gamma(ureg), _h(ureg, (5.0, 9.0, 50.0)))
    with pytest.raises(ValueError, match="one cell in z"):
        runner.add_flowfield(_flow(ureg, (10, 5, 2, 3)), _gamma(ureg), _h(ureg, (5.0, 10.0, 25.0)))
    with pytest.raises(ValueError, match="one non-negative scalar"):
        runner.add_flowfield(_flow(ureg), ureg.Quantity([1.0, 2.0], "sim_mass/sim_time"), _h(ureg))
    bad = np.ones((10, 5, 1, 3))
    bad[3, 2, 0, 1] = np.inf
    with pytest.raises(ValueError, match="finite"):
        runner.add_flowfield(ureg.Quantity(bad, "sim_velocity"), _gamma(ureg), _h(ureg))
    assert runner._flow is None and runner.system.constraints == []
    runner.integration_initialised = True
    with pytest.raises(RuntimeError, match="after the first call to integrate"):
        runner.add_flowfield(_flow(ureg), _gamma(ureg), _h(ureg))
    # the Brownian refusal is the reference's, unchanged
    ureg_b, brownian = _runner(tmp_path / "b", thermostat="brownian")
    with pytest.raises(RuntimeError) as exc:
        brownian.add_flowfield(_flow(ureg_b), _gamma(ureg_b), _h(ureg_b))
    assert str(exc.value) == ("Coupling to a flowfield does not work with a Brownian thermostat."
                              " Use 'langevin'.")


def test_langevin_needs_mass_and_rinertia(tmp_path):
    ureg, runner = _runner(tmp_path, n_colloids=0)
    with pytest.raises(ValueError, match="you must set a particle mass"):
        runner.add_colloids(2, ureg.Quantity(1.0, "micrometer"),
                            ureg.Quantity(np.array([25, 25, 0]), "micrometer"),
                            ureg.Quantity(20, "micrometer"))


def test_out_of_scope_combinations_are_refused_before_the_engine_exists(tmp_path):
    """Decided on the host: the first integrate raises before any device is
    asked for."""
    from test_rod_cpu import _rod_args

    ureg, runner = _runner(tmp_path / "a", n_dims=3)
    with pytest.raises(NotImplementedError, match="2d engines only"):
        runner.integrate(1)
    ureg, runner = _runner(tmp_path / "b", periodic=False)
    with pytest.raises(NotImplementedError, match="non-periodic"):
        runner.integrate(1)
    ureg, runner = _runner(tmp_path / "c")
    with pytest.raises(NotImplementedError, match="a rod under the Langevin thermostat"):
        runner.add_rod(**_rod_args(ureg))
    assert runner._rod is None and len(runner.colloids) == 5
    ureg, runner = _runner(tmp_path / "d", n_colloids=0)
    with pytest.raises(NotImplementedError, match="brownian thermostat only"):
        runner.add_colloids(2, ureg.Quantity(1.0, "micrometer"),
                            ureg.Quantity(np.array([25, 25, 0]), "micrometer"),
                            ureg.Quantity(20, "micrometer"), aspect_ratio=2.0,
                            mass=ureg.Quantity(1.0, "sim_mass"),
                            rinertia=ureg.Quantity(3 * [1.0], "sim_rinertia"))
    with pytest.raises(NotImplementedError, match="brownian thermostat only"):
        runner.add_colloids(2, ureg.Quantity(1.0, "micrometer"),
                            ureg.Quantity(np.array([25, 25, 0]), "micrometer"),
                            ureg.Quantity(20, "micrometer"),
                            gamma_translation=ureg.Quantity([1.0, 2.0, 3.0],
                                                            "sim_force/sim_velocity"),
                            mass=ureg.Quantity(1.0, "sim_mass"),
                            rinertia=ureg.Quantity(3 * [1.0], "sim_rinertia"))
    ureg, runner = _runner(tmp_path / "e")
    with pytest.raises(NotImplementedError, match="lattice Boltzmann"):
        runner.add_lattice_boltzmann(agrid=ureg.Quantity(1.0, "micrometer"))


def test_reference_flow_case_on_the_restatement(tmp_path):
    """CI/espresso_tests/unit_tests/test_flow.py's inputs and SwarmEngine's
    default seed on the CPU restatement, 1000 slices: its two assertions (mean
    x > L / 2, all x < L) hold after every slice, from the first one on (the
    overlap removal, in which the flow acts too, has already carried the
    swimmers downstream), and the swimmers stay inside the arena."""
    import langevin_flow_case as fc

    ureg, runner, force_fn, box_l, case = fc.build(tmp_path)
    assert np.stack(runner._pos[0])[:, 0].mean() < box_l[0] / 2.0  # not so at the start
    failed = []

    def check(s, pos):
        if not (np.mean(pos[:, 0]) > box_l[0] / 2.0 and np.all(pos[:, 0] < box_l[0])):
            failed.append(s)

    st, vel, om = fc.restate(runner, case, 1000, check)
    assert failed == []
    pos = oracle.unwrapped(st, box_l)
    r = np.hypot(pos[:, 0] - box_l[0] / 2.0, pos[:, 1] - box_l[1] / 2.0)
    assert np.all(r < box_l[0] / 2.0)
    assert np.all(np.isfinite(vel)) and np.any(vel[:2] != 0.0) and np.any(om != 0.0)

"""
The reference's test_flow_and_potential (CI/espresso_tests/unit_tests/
test_flow.py) set up through SwarmEngine (a helper, not a test): swimmers
advected by a flow inside a circular arena drawn by a gridded potential, a
heavy-particle Langevin thermostat and ConstForceAndTorque.  build() needs no
GPU (the engine is created at the first integrate); restate() runs the same
case on the CPU restatement from the engine's own host-side numbers.
"""

import numpy as np

import langevin_oracle as lo
from oracle import oracle


def build(out_folder):
    """Returns (ureg, engine, force_fn, box_l, case) with case the numbers
    restate() needs."""
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.engine import MDParams, SwarmEngine
    from swarmrl_amd.force_functions import ForceFunction
    from swarmrl_amd.units import UnitRegistry, ensure_quantity_array

    ureg = UnitRegistry()
    langevin_friction_scale = 1e-6  # to avoid double friction (see the reference's test)
    params = MDParams(
        ureg=ureg,
        fluid_dyn_viscosity=ureg.Quantity(8.9e-3, "pascal * second"),
        WCA_epsilon=ureg.Quantity(300, "kelvin") * ureg.boltzmann_constant,
        temperature=ureg.Quantity(300, "kelvin") / langevin_friction_scale,
        box_length=ureg.Quantity(3 * [100], "micrometer"),
        time_step=ureg.Quantity(0.1, "second") / 100,
        time_slice=ureg.Quantity(0.01, "second"),
        write_interval=ureg.Quantity(5, "second"),
        thermostat_type="langevin",
    )
    runner = SwarmEngine(params, out_folder=out_folder, write_chunk_size=1, n_dims=2)
    n_cells = 100
    box_l = params.box_length.m_as("sim_length")
    agrid_SI = params.box_length[0] / n_cells
    agrid = box_l[0] / n_cells
    xs = np.linspace(0.5 * agrid, box_l[0] - 0.5 * agrid, num=n_cells, endpoint=True)
    ys = xs
    xv, yv = np.meshgrid(xs, ys)
    flow = 3 * np.stack([np.ones_like(xv), 0.1 * np.cos(yv) * np.sin(xv), np.zeros_like(xv)],
                        axis=2)
    flow = ureg.Quantity(flow, "micrometer/second")
    rs = np.sqrt((xv - box_l[0] / 2.0) ** 2 + (yv - box_l[0] / 2.0) ** 2)
    boundary_mask = rs > box_l[0] / 2.0 - agrid
    coll_radius = ureg.Quantity(1, "micrometer")
    gamma = 6 * np.pi * params.fluid_dyn_viscosity * coll_radius
    spacings = ensure_quantity_array([agrid_SI, agrid_SI, params.box_length[2]], ureg)
    runner.add_flowfield(flow[:, :, np.newaxis, :], gamma, spacings)
    swim_vel = ureg.Quantity(5, "micrometer/second")
    swim_force = gamma * swim_vel
    potential = 2 * (swim_force + np.max(flow) * gamma) * agrid_SI * boundary_mask
    runner.add_external_potential(potential[:, :, np.newaxis], spacings)
    gamma_trans_reduced = gamma * langevin_friction_scale
    gamma_rot_increased = (8 * np.pi * params.fluid_dyn_viscosity * coll_radius ** 3
                           / langevin_friction_scale)
    active_ang_vel = ureg.Quantity(4 * np.pi / 180, "1/second")
    relaxation = ureg.Quantity(0.01, "second")
    partcl_mass = gamma * relaxation
    partcl_rinertia = gamma_rot_increased * relaxation
    runner.add_colloids(
        10, coll_radius, ureg.Quantity([50, 50, 0], "micrometer"),
        ureg.Quantity(30, "micrometer"),
        gamma_translation=gamma_trans_reduced, gamma_rotation=gamma_rot_increased,
        mass=partcl_mass, rinertia=ensure_quantity_array(3 * [partcl_rinertia], ureg),
    )
    active_force = swim_force.m_as("sim_force")
    active_torque = (active_ang_vel * gamma_rot_increased).m_as("sim_torque")
    model = dummy_models.ConstForceAndTorque(active_force, [0, 0, active_torque])
    case = {"force": float(active_force), "torque": float(active_torque),
            "eps": float(params.WCA_epsilon.m_as("sim_energy"))}
    return ureg, runner, ForceFunction({"0": model}), np.asarray(box_l, float), case


def restate(runner, case, n_slices, check=None):
    """The engine's integrate(n_slices) on the CPU restatement: the overlap
    removal of 1000 steps, then slices of steps_per_slice sub-steps with
    reuse_forces.  check(slice, unwrapped positions): called after every
    slice.  Returns (state, vel, omega)."""
    n = runner.n_particles
    box = runner._box
    p = oracle.make_params(box, runner._time_step, runner._kT(), case["eps"], runner.seed,
                           [tuple(runner._species_keys[0])])
    potential = (runner._potential["phi"], runner._potential["h"])
    flow = (runner._flow["u"], runner._flow["gamma"])
    sp = np.zeros(n, np.uint8)
    st = oracle.state_from_positions(np.stack(runner._pos[0]), np.stack(runner._dir[0]), box)
    st, _ = lo.sd_run(p, st, sp, 1000, potential=potential, flow=flow)
    reuse = lo.ReuseForces(st)
    vel, om = np.zeros((3, n), np.float32), np.zeros(n, np.float32)
    fs = np.full(n, case["force"], np.float32)
    tz = np.full(n, case["torque"], np.float32)
    k = runner.params.steps_per_slice
    for s in range(n_slices):
        st, vel, om, _ = reuse.run(p, st, vel, om, sp, fs, tz, k, step0=s * k,
                                   potential=potential, flow=flow)
        if check is not None:
            check(s + 1, oracle.unwrapped(st, box))
    return st, vel, om

/*
 * swarmrl_amd.h -- C ABI of the MI355X active-Brownian swarm engine.
 *
 * This is the drop-in boundary that replaces the ESPResSo calls made by
 * SwarmRL's engine adapter (reference: swarmrl/engine/espresso.py).  Every
 * entry point below names the reference call site it stands in for.  The
 * ABI uses only plain C types and pointers: no torch, no HIP types (a HIP
 * stream is passed as `void*`).  All functions return SWARM_OK (0) or an
 * error code; the message of the last error on the calling thread is
 * returned by swarm_last_error().  No C++ exception crosses this boundary.
 *
 * Error codes map onto the Python exceptions the reference raises:
 *   SWARM_EINVAL    -> ValueError   (bad configuration, espresso.py:180-182, 252-288)
 *   SWARM_ESTATE    -> RuntimeError (mutation after first integrate, espresso.py:300-305)
 *   SWARM_EDEVICE   -> RuntimeError (HIP runtime failure)
 *   SWARM_ECAPACITY -> ValueError   (size beyond what this build supports)
 *
 * Units: simulation units of the reference (espresso.py:211-234):
 * length 1 um, time 1 s, energy 293 K * k_B.
 *
 * State representation (identical in the CPU oracle and on the GPU):
 *   position  : per axis a uint32 fraction of the box (q * L / 2^32) plus an
 *               int32 image counter; unwrapped x = (img + q / 2^32) * L.
 *   orientation (2-D): uint32 angle, theta = a * 2 pi / 2^32.
 *   orientation (3-D): fp32 unit director [3], rotated each sub-step by
 *               the rotation vector (Rodrigues) and renormalised.
 * Index g = env * n_particles + i.  Device arrays are axis-major [3][E*N].
 */
#ifndef SWARMRL_AMD_H
#define SWARMRL_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWARM_MAX_SPECIES 16
#define SWARM_MAX_CONES 16
#define SWARM_MAX_DETECTED_TYPES 8

#define SWARM_OK 0
#define SWARM_EINVAL 1
#define SWARM_ESTATE 2
#define SWARM_EDEVICE 3
#define SWARM_ECAPACITY 4

/* Physical parameters of one engine (all envs share them).
 * Mirrors MDParams (espresso.py:30-88) after unit conversion, plus the
 * per-particle friction/mass registered by add_colloid_on_point
 * (espresso.py:376-413).  A "species" is one distinct
 * (radius, gamma_t, gamma_r, mass, rinertia) combination. */
typedef struct swarm_params {
  int32_t n_dims;   /* 2 or 3 (espresso.py:143-152, n_dims) */
  int32_t periodic; /* MDParams.periodic (espresso.py:270) */
  double box[3];    /* box_l (espresso.py:267) */
  double time_step; /* system.time_step (espresso.py:268) */
  double kT;        /* Brownian thermostat kT (espresso.py:1171, 1179-1184) */
  double wca_epsilon; /* WCA epsilon (espresso.py:814-819) */
  uint64_t seed;    /* thermostat seed (espresso.py:1183) */
  int32_t n_species;
  /* ESPResSo's integrator.run(k, reuse_forces=True) (espresso.py:1304-1306):
   * the Brownian propagator takes each step's forces from the force
   * calculation that ended the previous step, and a run with reuse_forces
   * does not recompute them first -- so sub-step 0 of every run uses the
   * swim force, torque and director of the previous run's last force
   * calculation (the actions set since then act from sub-step 1).
   * 1: that semantics (SwarmEngine's default, as the reference);
   * 0: every sub-step uses the current actions. */
  int32_t reuse_forces;
  double radius[SWARM_MAX_SPECIES];
  double gamma_t[SWARM_MAX_SPECIES];  /* 6 pi eta r  (espresso.py:108-113) */
  double gamma_r[SWARM_MAX_SPECIES];  /* 8 pi eta r^3 */
  double mass[SWARM_MAX_SPECIES];     /* used for the BD thermal velocity */
  double rinertia[SWARM_MAX_SPECIES]; /* used for the BD thermal omega */
} swarm_params_t;

/* Raw device pointers of the SoA state, for zero-copy consumers. */
typedef struct swarm_device_views {
  uint32_t *q;        /* [3][E*N] */
  int32_t *img;       /* [3][E*N] */
  uint32_t *ang;      /* [E*N]    */
  float *f_swim;      /* [E*N]    */
  float *torque_z;    /* [E*N]    */
  float *f_ext;       /* [3][E*N] */
  float *vel;         /* [3][E*N] (written by the last sub-step of a run) */
  float *omega_z;     /* [E*N]    */
  uint8_t *species;   /* [N]      */
  int32_t n_envs;
  int32_t n_particles;
  int32_t n_dims;
  int32_t reserved0;
  float *dir3;        /* [3][E*N] 3-D directors */
  float *torque_xy;   /* [2][E*N] 3-D torque x, y */
  float *omega_xy;    /* [2][E*N] 3-D angular velocity x, y */
} swarm_device_views_t;

/* A confining or user wall (espresso.py:667-800): a WCA constraint with
 * sigma = r_particle * 2^(-1/6), cutoff = r_particle (the wall type has
 * radius 0) and the engine's epsilon, acting on every particle.
 *   kind 0 = espressomd.shapes.Wall: dist = n . x_folded - offset
 *            (add_confining_walls, espresso.py:683-697);
 *   kind 1 = the vertical Rhomboid of add_walls (espresso.py:765-784):
 *            corner + s a + t b (s, t in [0, 1]), a and b in the xy plane,
 *            spanning the whole box in z; distance in the xy plane.
 * A particle on or inside a wall (dist <= 0) is a constraint violation:
 * it is counted (swarm_engine_wall_violations) and gets no wall force. */
typedef struct swarm_wall {
  int32_t kind;
  int32_t reserved;
  double normal[3]; /* kind 0 */
  double offset;    /* kind 0 */
  double corner[3]; /* kind 1 */
  double a[3];      /* kind 1 */
  double b[3];      /* kind 1 */
} swarm_wall_t;

#define SWARM_MAX_WALLS 16

/* Vision-cone parameters (SubdividedVisionCones,
 * swarmrl/observables/subdivided_vision_cones.py:25-60). */
typedef struct swarm_vision_params {
  float vision_range;
  float vision_half_angle;
  int32_t n_cones;
  int32_t n_types;                       /* len(detected_types) */
  int32_t detected_types[SWARM_MAX_DETECTED_TYPES];
  float rims[SWARM_MAX_CONES + 1];       /* -a + k*2a/n, computed in fp32 */
} swarm_vision_params_t;

typedef struct swarm_engine swarm_engine_t;

/* Thread-local message of the last failing call. */
const char *swarm_last_error(void);

/* Build provenance (no reference counterpart): the 12-hex-digit hash of the
 * HIP sources and this header the library was compiled from
 * (__graft_entry__.build, swarmrl_amd._capi.source_hash); swarmrl_amd._capi
 * warns when it differs from the checkout it runs in. */
const char *swarm_build_id(void);

/* Engine construction: replaces espressomd.System(...) + _init_system +
 * part.add for all particles (espresso.py:192-196, 236-288, 415-441).
 * `species` is [n_particles]: index into the per-species arrays of params. */
int swarm_engine_create(const swarm_params_t *params, int32_t n_envs,
                        int32_t n_particles, const int32_t *species,
                        swarm_engine_t **out);
void swarm_engine_destroy(swarm_engine_t *e);

/* Bind all later launches to a HIP stream (hipStream_t as void*). */
int swarm_engine_set_stream(swarm_engine_t *e, void *hip_stream);

/* Initial state from host fp64 arrays pos[E][N][3] (unwrapped) and
 * dir[E][N][3]; replaces part.add(pos=...) + _rotate_colloid_to_2d
 * (espresso.py:428-449). */
int swarm_engine_upload_state(swarm_engine_t *e, const double *pos,
                              const double *director);

/* Exact state transfer in the engine's own number format (host arrays):
 * q/img [3][E*N], ang [E*N].  Used for checkpoints and bit-exact parity. */
int swarm_engine_upload_raw(swarm_engine_t *e, const uint32_t *q,
                            const int32_t *img, const uint32_t *ang);
int swarm_engine_download_raw(swarm_engine_t *e, uint32_t *q, int32_t *img,
                              uint32_t *ang);

/* Synchronous copy of the state to host fp64 arrays [E][N][3]; replaces
 * the particle property getters used by get_particle_data and the Colloid
 * snapshot (espresso.py:1216-1225, 1320-1336).  Any pointer may be NULL. */
int swarm_engine_download_state(swarm_engine_t *e, double *pos_unwrapped,
                                double *director, double *velocity);

/* Per-particle swim force and z-torque [E*N]; replaces
 * coll.swimming = {"f_swim": ...} and coll.ext_torque = ...
 * (espresso.py:1228-1235).  on_device = 0: host arrays (copied);
 * 1: device arrays copied on the engine stream; 2: device arrays BOUND
 * (zero copy): later launches read them directly, so the caller keeps them
 * alive and unchanged until the next set_actions call. */
int swarm_engine_set_actions(swarm_engine_t *e, const float *f_swim,
                             const float *torque_z, int32_t on_device);

/* Per-particle external force [E*N][3] (host); replaces p.ext_force. */
int swarm_engine_set_external_force(swarm_engine_t *e, const double *f_ext);

/* new_direction handling of manage_forces (espresso.py:1236-1249): in 2-D
 * rotate about +-z so the director equals dir; in 3-D set the director to
 * dir (normalised).  dir [E*N][3], mask [E*N]. */
int swarm_engine_set_directors(swarm_engine_t *e, const double *dir,
                               const uint8_t *mask);

/* 3-D only: the x and y components of the lab-frame torque [2][E*N]
 * (the z component is set_actions' torque_z); replaces coll.ext_torque =
 * action.torque (espresso.py:1230-1235).  on_device as in set_actions
 * (0 host, 1 device copy; binding is not offered). */
int swarm_engine_set_torque_xy(swarm_engine_t *e, const float *torque_xy,
                               int32_t on_device);

/* 3-D directors in the engine's own format (host fp32 [3][E*N]), for
 * checkpoints and bit-exact parity. */
int swarm_engine_upload_directors(swarm_engine_t *e, const float *dir3);
int swarm_engine_download_directors(swarm_engine_t *e, float *dir3);

/* Walls (see swarm_wall_t); replaces add_confining_walls / add_walls
 * (espresso.py:667-800).  Replaces any previous set; n_walls <= 16. */
int swarm_engine_set_walls(swarm_engine_t *e, const swarm_wall_t *walls,
                           int32_t n_walls);

/* Gridded external potential; replaces add_external_potential
 * (espresso.py:995-1036: np.pad(mode="wrap") + constraints.PotentialField).
 * phi is host fp32 [nx][ny][nz] in simulation energy units (copied), value
 * [i][j][k] at the cell centre ((i + .5) hx, (j + .5) hy, (k + .5) hz);
 * spacing = {hx, hy, hz}.  The field is periodic and interpolated
 * (tri)linearly; the force, minus the interpolant's gradient at the
 * particle's folded position, is added to the external force of every
 * particle in every BD sub-step and overlap-removal step (fixed fp32
 * sequence: swarm_potential.cuh).  Replaces a previous field; phi = NULL
 * removes it (the other arguments are then ignored).  SWARM_EINVAL for a
 * count < 1, a non-finite value or spacing, nz != 1 on a 2-D engine,
 * n_a h_a differing from the box length by more than 1e-9 relative, more
 * than 2^31 - 1 stored values (a 2-D engine stores four per cell), or an
 * engine with a rod.  Moves no particle: a
 * pending build stays valid. */
int swarm_engine_set_potential_field(swarm_engine_t *e, const float *phi,
                                     int32_t nx, int32_t ny, int32_t nz,
                                     const double *spacing);

/* Number of (particle, sub-step) wall contacts with dist <= 0 since the
 * engine was created (ESPResSo raises for those; synchronous). */
int swarm_engine_wall_violations(swarm_engine_t *e, uint64_t *count);

/* A rigid rod (EspressoMD.add_rod, espresso.py:546-665: a centre particle
 * and n - 1 VIRTUAL_SITES_RELATIVE beads): particles [first, first + n) of
 * every env, the centre first, bead k (k = 0 .. n - 2) in signed slot
 * m_k = (-1)^k (k / 2 + 1) at centre + m_k delta u (u the centre's
 * director, delta = (length - thickness) / (n - 1)).  The rod's species
 * carries its radius (thickness / 2) and its frictions (gamma_t =
 * friction_trans, gamma_r = friction_rot, mass = rinertia = 0).  fixed: the
 * centre does not translate (fix = [fixed, fixed, True], espresso.py:631); it
 * still rotates. */
typedef struct swarm_rod {
  int32_t first;
  int32_t n;
  double delta;
  int32_t fixed;
  int32_t reserved;
} swarm_rod_t;

/* Replaces the part.add / vs_auto_relate_to calls of add_rod
 * (espresso.py:626-660); call once, before the first run, like
 * swarm_engine_set_walls.  The beads are placed onto the centre's line.
 * From then on every sub-step (and the overlap removal, in which the rod
 * does not move) runs in one workgroup per env that sums the rod's contact
 * forces and torque, steps the centre and re-places the beads; the engine
 * runs no cluster windows and declines swarm_engine_prebuild,
 * swarm_engine_defer_build, swarm_engine_prebuild_noise and
 * swarm_engine_hint_defer_check.  2-D periodic boxes without walls; n odd,
 * n <= 255; at most 4096 particles per env; one rod per engine; not under
 * the Langevin thermostat. */
int swarm_engine_set_rod(swarm_engine_t *e, const swarm_rod_t *rod);

/* Ellipsoidal colloids (espresso.py:802-832 and 420-436): the aspect ratio
 * every particle shares (axial over equatorial semi-axis; the species'
 * radius is the equatorial one) and per species the translational friction
 * along the director (gamma_par = gamma_translation[2] of the 2-D body
 * frame, espresso.py:427-449) and across it in the plane (gamma_perp =
 * gamma_translation[1]).  The rotational friction about lab z stays
 * swarm_params_t::gamma_r. */
typedef struct swarm_ellipsoids {
  double aspect_ratio;
  double gamma_par[SWARM_MAX_SPECIES];
  double gamma_perp[SWARM_MAX_SPECIES];
} swarm_ellipsoids_t;

/* Replaces the gay_berne.set_params calls of _setup_interactions
 * (espresso.py:802-832: k2 = 1, nu = 1, mu = 2, sig = (r_i + r_j) 2^(-1/6),
 * eps = wca_epsilon) and the per-axis gamma of part.add (espresso.py:420-436);
 * call once, before the first swarm_engine_integrate or
 * swarm_engine_remove_overlap (SWARM_ESTATE afterwards).  With aspect_ratio
 * != 1 every pair interacts by Gay-Berne, shifted at the cutoff
 * 2 (r_i + r_j) max(k, 1 / k) (espresso.py:830 for equal radii), and the
 * per-env cell grid is re-derived for the widest of them; with aspect_ratio
 * = 1 the pairs stay WCA and only the friction is per axis.  A pair that
 * penetrates to X = sigma0 / (|r| - sigma + sigma0) >= 1.25 (or
 * |r| - sigma + sigma0 <= 0) contributes the force and torque at X = 1.25
 * and is counted, per visit and sub-step, in swarm_engine_wall_violations.
 * From then on every sub-step and the overlap removal (in which the
 * Gay-Berne force and torque act too) run in one workgroup per env; the
 * engine runs no cluster windows and declines swarm_engine_prebuild,
 * swarm_engine_defer_build, swarm_engine_prebuild_noise and
 * swarm_engine_hint_defer_check.  SWARM_EINVAL for a rod, walls, a
 * potential, the Langevin thermostat, a non-periodic box, n_dims = 3,
 * aspect_ratio <= 0, a non-positive friction or a cutoff of half the box or
 * more;
 * SWARM_ECAPACITY when the env's state does not fit the 160 KB of LDS of one
 * workgroup (the message states the particle limit). */
int swarm_engine_set_ellipsoids(swarm_engine_t *e, const swarm_ellipsoids_t *ell);

/* The Langevin thermostat; replaces integrator.set_vv() +
 * thermostat.set_langevin of MDParams(thermostat_type="langevin")
 * (espresso.py:1171-1190).  A setter and not a field of swarm_params_t, whose
 * layout is fixed.  Call once, before the first swarm_engine_integrate or
 * swarm_engine_remove_overlap (SWARM_ESTATE afterwards).  From then on every
 * sub-step is inertial, with swarm_params_t::mass and ::rinertia per species
 * and the velocities (swarm_device_views_t::vel, ::omega_z; zero at the call)
 * as integrator state that carries from run to run: per sub-step, with one
 * force evaluation F (pairs, walls, potential, external and swim force),
 *   v     += (dt / m) (F + gamma_flow u(x) - (gamma_t + gamma_flow) v
 *                        + sqrt(24 kT gamma_t / dt) (U - 1/2))     per axis
 *   omega += (dt / I) (t_z - gamma_r omega + sqrt(24 kT gamma_r / dt) (U - 1/2))
 *   x += dt v,  theta += dt omega
 * (velocity Verlet in leapfrog form with the friction at the half-step
 * velocity; U uniform in [0, 1): the noise has the Gaussian's first two
 * moments.  Fixed fp32 sequence: swarm_langevin.cuh).  The overlap removal
 * stays steepest descent and leaves the velocities alone.  Every sub-step
 * and the overlap removal run in one workgroup per env; the engine runs no
 * cluster windows and declines swarm_engine_prebuild,
 * swarm_engine_defer_build, swarm_engine_prebuild_noise and
 * swarm_engine_hint_defer_check.  Walls, a gridded potential and external
 * forces act as under the Brownian thermostat.  SWARM_EINVAL for n_dims = 3,
 * a non-periodic box, a rod, ellipsoids, a mass or rinertia that is not
 * positive, or a step the explicit friction cannot integrate
 * (dt gamma_t / m >= 2 or dt gamma_r / I >= 2; the message names the ratio);
 * SWARM_ECAPACITY when the env's state does not fit the 160 KB of LDS of one
 * workgroup (the message states the particle limit). */
int swarm_engine_set_langevin(swarm_engine_t *e);

/* Coupling to a gridded flow field; replaces add_flowfield's
 * constraints.FlowField (espresso.py:940-993): the drag gamma (u(x) - v) on
 * every particle, u host fp32 [nx][ny][nz][3] in simulation velocity units
 * (copied), value [i][j][k] at the cell centre as for
 * swarm_engine_set_potential_field, periodic and interpolated linearly at
 * the particle's folded position (2-D: nz = 1, the z component is unused).
 * In the overlap removal the flow acts with v = 0.  Replaces a previous
 * field; u = NULL removes it.  The grid rules and their SWARM_EINVAL are
 * those of swarm_engine_set_potential_field (a 2-D engine stores eight
 * values per cell); SWARM_EINVAL also on an engine without
 * swarm_engine_set_langevin, for a negative or non-finite gamma, and when
 * dt (gamma_t + gamma) / m >= 2.  Moves no particle. */
int swarm_engine_set_flow_field(swarm_engine_t *e, const float *u, int32_t nx,
                                int32_t ny, int32_t nz, const double *spacing,
                                double gamma);

/* The velocities in the engine's own format (host fp32: vel [3][E*N], omega
 * [E*N]): under the Langevin thermostat they are state, to be restored with
 * the raw positions.  Download: either pointer may be NULL. */
int swarm_engine_upload_velocities(swarm_engine_t *e, const float *vel,
                                   const float *omega);
int swarm_engine_download_velocities(swarm_engine_t *e, float *vel, float *omega);

/* RotateRod's reward on the device (rod_rotation.py:87-219 with
 * compute_torque_partition_on_rod, colloid_utils.py:29-117), all in fp64:
 *   step = wrapped (centre angle - hist_ang[e]) in degrees, pushed into the
 *          env's ring [history]; mean over its filled entries (the
 *          reference's nanmean over a NaN-initialised roll);
 *   w_i  = |u x sum_b grad(1 / |r_b - r_i|^12)| + 1e-8 over the rod's
 *          particles b (xy of the unwrapped positions, no minimum image, u
 *          the rod's director), normalised over the n_agents colloids;
 *   out[e][a] = scale * mean * w_a / sum w   (partition = 0: scale * mean /
 *          n_agents).
 * agent_idx [n_agents] device int32; hist_ang [E] uint32, ring [E][history]
 * fp64 and count [E] int32 are the task's device state (hist_ang: the
 * centre's angle at initialisation, count zeroed), updated by the call; out
 * device fp32 [E][n_agents].  Asynchronous on the engine stream. */
int swarm_rod_reward(swarm_engine_t *e, const int32_t *agent_idx, int32_t n_agents,
                     uint32_t *hist_ang, double *ring, int32_t *count, int32_t history,
                     double scale, int32_t partition, float *out);

/* Steepest-descent overlap removal (espresso.py:1161-1168): n_steps of
 * dp = clamp(gamma * F, -max_disp, max_disp) per free coordinate. */
int swarm_engine_remove_overlap(swarm_engine_t *e, int32_t n_steps,
                                double gamma, double max_displacement);

/* Both reuse_forces slots as the engine holds them (host; any pointer may be
 * NULL): f_prev, tz_prev fp32 [2][E*N], ang_prev uint32 [2][E*N], and on a
 * 3-D engine dir3_prev fp32 [2][3][E*N] and txy_prev fp32 [2][2][E*N] (left
 * alone in 2-D).  Slot p is read by the windows whose device window counter
 * has parity p.  For tests and diagnostics; synchronous. */
int swarm_engine_download_reuse_slots(swarm_engine_t *e, float *f_prev,
                                      float *tz_prev, uint32_t *ang_prev,
                                      float *dir3_prev, float *txy_prev);

/* A placement group of the reset plan: particles [first, first + count) of
 * every env are drawn uniformly in the disc (2-D) or ball (3-D) of this
 * radius round this centre (add_colloids, espresso.py:459-544), each with a
 * uniform director. */
typedef struct swarm_reset_group {
  int32_t first;
  int32_t count;
  double centre[3];
  double radius;
} swarm_reset_group_t;

/* What swarm_engine_reset_envs puts a listed env back to.  pos and director:
 * host fp64 [E][N][3] with the meaning they have for
 * swarm_engine_upload_state (copied, converted by its rules and kept on the
 * device): the home state, which every particle outside the groups and every
 * particle of a group of radius 0 returns to.  groups: n_groups disjoint
 * particle ranges (NULL with n_groups = 0: every particle goes home).
 * Replaces a previous plan.  Moves no particle.  SWARM_EINVAL for
 * overlapping or out-of-range groups, a negative or non-finite radius or
 * centre, and a radius above half the shortest box edge. */
int swarm_engine_set_reset_plan(swarm_engine_t *e, const double *pos,
                                const double *director,
                                const swarm_reset_group_t *groups,
                                int32_t n_groups);

/* Episodic reset in place: the envs with env_mask[env] != 0 (host uint8 [E];
 * NULL: every env) are put back to a fresh random start on the device; the
 * engine, its buffers and captured graphs stay.  Per listed env:
 *   - grouped particles are drawn anew (Philox key (seed lo, seed hi ^ env),
 *     counter (particle, reset ordinal lo, hi, 0x30 + block); the ordinal
 *     counts this engine's non-empty reset calls from 0; DESIGN.md section 3
 *     states the fp32 sequence), the others return to their home state;
 *   - velocities, angular velocities, the actions (f_swim, torque_z,
 *     torque_xy; written through a binding of swarm_engine_set_actions with
 *     on_device = 2 as well) are zeroed and both reuse_forces slots are as on
 *     a fresh engine after its overlap removal;
 *   - sd_steps steps of the overlap removal run on the listed envs alone
 *     (sd_steps = 0: placement only).
 * An env that is not listed is not touched by a single store.  The device
 * step counter, the window counter and the wall-violation count go on: the
 * noise of the next run continues the engine's stream.  Flushes a pending
 * check and discards a pending build like swarm_engine_remove_overlap.
 * Asynchronous on the engine stream apart from the copy of the env list; not
 * to be captured into a graph.  An empty mask is a no-op.  SWARM_ESTATE
 * without a reset plan; SWARM_EINVAL on an engine with a rod, ellipsoids or
 * the Langevin thermostat, and for sd_steps < 0. */
int swarm_engine_reset_envs(swarm_engine_t *e, const uint8_t *env_mask,
                            int32_t sd_steps, double gamma,
                            double max_displacement);

/* swarm_engine_reset_envs for the envs a device mask marks (d_mask: device
 * uint8 [E], non-zero: reset), without a host copy and without a
 * synchronisation: every launch has a grid that does not depend on the mask's
 * contents, so the call can be captured into a graph and replayed with other
 * mask contents.  A marked env gets exactly what a listed env of
 * swarm_engine_reset_envs gets (placement, zeroed velocities and actions,
 * both reuse_forces slots, its candidate lists dropped, sd_steps of the
 * overlap removal); only the draw counter differs: the ordinal is
 * 2^63 | c_env, c_env the device-mask resets this env has had so far (a
 * per-env device counter, bumped for marked envs only), so the k-th reset of
 * an env is the same whatever the other envs do and the ordinals 0, 1, ... of
 * swarm_engine_reset_envs are not disturbed.  An unmarked env is not touched
 * by a single store; an all-zero mask changes nothing.  The host cannot know
 * whether an env was marked: a pending check is flushed and a pending build
 * discarded whatever the mask holds.  SWARM_ESTATE without a reset plan;
 * SWARM_EINVAL on an engine with a rod, ellipsoids or the Langevin
 * thermostat, for sd_steps < 0 and for a null mask. */
int swarm_engine_reset_marked(swarm_engine_t *e, const uint8_t *d_mask,
                              int32_t sd_steps, double gamma,
                              double max_displacement);

/* counts (host uint32 [E]): per env, the resets swarm_engine_reset_marked has
 * given it (0 before a reset plan is set).  Synchronous. */
int swarm_engine_reset_counts(swarm_engine_t *e, uint32_t *counts);

/* n_steps Brownian-dynamics sub-steps with WCA pair forces; replaces
 * system.integrator.run(k, reuse_forces=True, recalc_forces=False)
 * (espresso.py:1304-1306).  Asynchronous on the engine stream. */
int swarm_engine_integrate(swarm_engine_t *e, int32_t n_steps);

/* Launch the next integration window's position-only preparation (cluster
 * decomposition) on `stream` (a hipStream_t; NULL = engine stream), so it
 * can overlap the observable and policy work that produces the slice's
 * actions (espresso.py:1253-1306: manage_forces precedes integrator.run and
 * cannot change positions).  The caller orders `stream` after the last
 * position change and the engine stream after `stream` (events); the next
 * swarm_engine_integrate consumes the preparation.  Any position change in
 * between (upload, remove_overlap) discards it.  No-op for engines on the
 * global path.  n_steps_hint is unused (kept for the noise variant below). */
int swarm_engine_prebuild(swarm_engine_t *e, void *stream, int32_t n_steps_hint);

/* Defer the next window's cluster decomposition instead (latency-bound 2-D
 * engines with the three-launch build): its three stages -- counting sort,
 * pair search, cluster build -- then ride along as extra workgroups in the
 * slice's next engine-bound launches, swarm_vision_cone (stages 1 and 2)
 * and swarm_engine_policy_mlp_sample (stage 3), on the engine stream with
 * no second stream, fork or join (espresso.py:1253-1306: the positions do
 * not change between manage_forces and integrator.run).  Stages no launch
 * carried run at the next swarm_engine_integrate.  *deferred = 0 when the
 * engine cannot defer (use swarm_engine_prebuild). */
int swarm_engine_defer_build(swarm_engine_t *e, int32_t *deferred);

/* Same contract for the noise table of latency-bound engines: the normals
 * of the next min(n_steps_hint, 128) sub-steps, computed on `stream` (it
 * depends on the step counter only, so it may run beside the build).  No-op
 * for engines without a noise table. */
int swarm_engine_prebuild_noise(swarm_engine_t *e, void *stream, int32_t n_steps_hint);

/* Counters of the cluster windows since the engine was created (or the
 * last reset), summed over the envs: out4[0] windows whose pair search
 * filtered the candidate lists prepared during the previous run, out4[1]
 * windows whose pair search waited for the fresh build sort instead (the
 * lists could not be used), out4[2] windows re-run exactly on the global
 * path, out4[3] windows checked.  Measurement only (bench.py); reset != 0
 * zeroes them after reading. */
int swarm_engine_build_stats(swarm_engine_t *e, uint64_t *out4, int32_t reset);

/* A window's check in the reward launch.  Latency-bound periodic 2-D engines
 * whose pair search filters candidate lists (unless SWARMRL_AMD_DEFER_CHECK = 0
 * at creation; other engines ignore the hint) can run the exact check of an
 * integration window as extra workgroups of the reward launch that follows
 * it (swarm_field_distance / swarm_field_transform after
 * swarm_engine_defer_build) instead of a launch of its own.
 *
 * swarm_engine_hint_defer_check announces, for the next
 * swarm_engine_integrate call only, that such a reward launch follows: the
 * call then leaves the check of its last window pending.  A pending check is
 * host-side state; it is enqueued as a launch of its own by
 * swarm_engine_flush_check and at the head of every other entry that takes
 * the engine, except swarm_engine_defer_build, swarm_engine_device_views and
 * a swarm_engine_set_stream that keeps the stream (they touch no device
 * state).  A caller that captures the stream into a graph must call
 * swarm_engine_flush_check before the capture ends: a graph captured with the
 * check pending would replay without it.
 *
 * swarm_engine_check_stats: windows whose check rode in a reward launch since
 * creation (or the last reset), summed over the envs, by outcome: out4[0] the
 * other workgroups, which always run ahead of the verdict, kept their
 * results; they did their work again because out4[1] the env had big clusters
 * (the check workgroup integrates them), out4[2] the candidate lists turned
 * out unusable, out4[3] the window was re-run exactly. */
int swarm_engine_hint_defer_check(swarm_engine_t *e);
int swarm_engine_flush_check(swarm_engine_t *e);
int swarm_engine_check_stats(swarm_engine_t *e, uint64_t *out4, int32_t reset);

/* Diagnostics of the last integration window, per env (host arrays [E],
 * either may be NULL): fallback 0 = cluster path, 1 = flagged by the build
 * (cluster > 64 lanes or neighbour overflow), 2 = re-run on the global path;
 * waves = 64-lane waves the env's clusters were packed into. */
int swarm_engine_window_stats(swarm_engine_t *e, int32_t *fallback,
                              int32_t *waves);

/* Kernel timing for measurement (bench.py roofline): returns the summed
 * duration (ms) and count of the eager k_cluster_run launches recorded since
 * the previous call (HIP events on the engine stream; waits for them), then
 * enables (1) or disables (0) recording.  While recording, a window captured
 * into a HIP graph gets event-record nodes (hipEventRecordExternal) around
 * its run-kernel node instead: see swarm_engine_profile_graph. */
int swarm_engine_profile(swarm_engine_t *e, int32_t enable, double *run_ms,
                         int32_t *launches);

/* Run-kernel durations inside captured graphs (bench.py roofline: the kernel
 * timed as it runs in the replayed episode): after a replay of a
 * graph captured with recording enabled has been launched, waits for the
 * device and writes the time (ms) between the event nodes around every
 * captured run node, in capture order, to ms_out[0..cap), and (cal_out, may
 * be NULL) the time between the two event nodes of an empty pair recorded
 * right after each run node -- what a pair of event nodes adds by itself --
 * and their count to *launches (each value is the latest replay's).
 * release = 1 then destroys the events (only once no graph holding them
 * replays again). */
int swarm_engine_profile_graph(swarm_engine_t *e, int32_t release, float *ms_out,
                               float *cal_out, int32_t cap, int32_t *launches);

/* The same captured run nodes timed by the kernel itself: each records the
 * earliest start of its blocks and the latest end of its waves on the
 * device's constant-rate wall clock.  reset = 1: clears the stamps on
 * `stream` (before a replay); reset = 0: waits for the device and writes the
 * durations (ms, end - start) of the captured run nodes, in capture order,
 * to ms_out[0..cap) (each the latest replay's).  *launches = the number of
 * stamped nodes (at most 512; swarm_engine_profile_graph's release resets
 * the count). */
int swarm_engine_profile_stamps(swarm_engine_t *e, int32_t reset, void *stream, float *ms_out,
                                int32_t cap, int32_t *launches);

/* The workgroup roles of the launches between the captured run nodes,
 * stamped the same way while profiling (stamp slot k: the k_check after the
 * k-th run node and the next window's build / observable / policy launches
 * up to the next run).  Writes, for slot k and role q (k_check, build sort,
 * vision grid, field, pair search, vision cone, cluster build, policy MLP,
 * then three progress marks: pair filter lists tested, pair filter output
 * reserved, vision-cone bins summed; *n_roles = 11, swarm::kRoles),
 * us_out[2 (k n_roles + q) + 0 / 1] = the role's earliest
 * start / latest end in microseconds after the k-th run node's end (NaN
 * where the role did not run), for entries below cap.  Waits for the
 * device; reset with swarm_engine_profile_stamps. */
int swarm_engine_profile_roles(swarm_engine_t *e, double *us_out, int32_t cap, int32_t *n_roles);

/* Kernel timing for measurement (bench.py roofline): builds the next 2-D
 * cluster window from the current positions, then launches its run kernel
 * `reps` times back to back between two HIP events on the engine stream and
 * returns the mean duration (ms) per launch; the exact check follows
 * (untimed).  The repeats integrate the same window again and again on one
 * decomposition, so the state afterwards is for measurement only (re-upload
 * it to continue a simulation).  SWARM_ESTATE unless the engine runs 2-D
 * cluster windows. */
int swarm_engine_time_run(swarm_engine_t *e, int32_t n_steps, int32_t reps,
                          double *run_ms);

/* Diagnostics: 32 shader-clock stamps of the last cluster build's phases
 * (env 0), filled only by builds compiled with -DSWARM_PHASE_TIMING. */
int swarm_engine_debug_phases(swarm_engine_t *e, uint64_t *out32);
/* Diagnostics (SWARM_PHASE_TIMING builds fill it; zeros otherwise): per run
 * wave w of the last cluster window, out[4w..4w+3] = realtime stamps (100 MHz)
 * at the wave's entry and end, its pair passes and pair count. */
int swarm_engine_debug_wave_stamps(swarm_engine_t *e, uint64_t *out, int32_t n_words);

/* Trajectory recording (espresso.py:1110-1159: _update_traj_holder at every
 * write interval, chunks written to HDF5) without a host synchronisation, so
 * it can sit inside a captured HIP graph.  swarm_engine_traj_ring allocates
 * a ring of `capacity` entries for env `env` in host-pinned, device-mapped,
 * coherent memory and returns its host address: bytes [0, 8) hold the count
 * of entries recorded so far (uint64), entry k % capacity starts at byte
 * 64 + (k % capacity) * entry_bytes.  swarm_engine_traj_record launches, on
 * the engine stream, the copy of the env's state into the next slot (the
 * slot index is a device counter, so graph replays fill successive slots)
 * and then publishes the new count.  The caller drains entries
 * [drained, count) with swarm_traj_entry_to_host, and must do so before
 * `capacity` newer ones overwrite them.  Entry layout: uint64 step counter,
 * uint32 q[D][N], int32 img[D][N], then uint32 ang[N] (2-D) or float
 * dir[3][N] (3-D), then float vel[D][N]. */
int swarm_engine_traj_ring(swarm_engine_t *e, int32_t capacity, int32_t env,
                           void **host_ring, int64_t *entry_bytes);
int swarm_engine_traj_record(swarm_engine_t *e);
/* One ring entry -> fp64 [N][3] arrays exactly as swarm_engine_download_state
 * converts the live state (unwrapped positions, directors, velocities) and
 * its step counter; any output may be NULL.  Host only (no device access). */
int swarm_traj_entry_to_host(const swarm_engine_t *e, const void *entry, double *pos,
                             double *director, double *velocity, uint64_t *step);

/* Total number of BD sub-steps integrated so far (the noise counter). */
int64_t swarm_engine_step_count(const swarm_engine_t *e);

int swarm_engine_device_views(swarm_engine_t *e, swarm_device_views_t *v);

/* Vision cones for n_agents agents (distinct indices into [0,N), device int32),
 * radii[N] device fp32 (radius of the SEEN colloid by list position,
 * subdivided_vision_cones.py:199-203); out device fp32
 * [E][n_agents][n_cones][n_types].  Replaces
 * SubdividedVisionCones.compute_observable (subdivided_vision_cones.py:241-258).
 * types[N] device int32: particle type of every colloid. */
int swarm_vision_cone(swarm_engine_t *e, const swarm_vision_params_t *vp,
                      const int32_t *agent_idx, int32_t n_agents,
                      const float *radii, const int32_t *types, float *out);

/* swarm_vision_cone with the caller's promise that agent_idx, radii and
 * types stay allocated and unchanged while the engine lives (the
 * SubdividedVisionCones observable keeps them).  The engine remembers the
 * arguments: when the next build is deferred (swarm_engine_defer_build),
 * the slice's reward launch (swarm_field_transform / swarm_field_distance)
 * also builds the vision grid of the positions it sees, and the next call
 * with the same arguments -- the next slice's observable, nothing having
 * moved the colloids in between -- runs the cone without a grid launch. */
int swarm_vision_cone_persistent(swarm_engine_t *e, const swarm_vision_params_t *vp,
                                 const int32_t *agent_idx, int32_t n_agents,
                                 const float *radii, const int32_t *types, float *out);

/* The observable and the rollout policy of an actor-critic agent in one
 * launch: swarm_vision_cone_persistent's cones into `features` ([E][n_agents]
 * [n_cones][n_types], n_cones * n_types <= 4) and, from them, the actor MLP +
 * Gumbel sampling of swarm_policy_mlp_sample (features as its observation,
 * d_in = n_cones * n_types, k <= 4 actions, hidden <= 256; weights read in
 * place) into out_idx / out_logp / out_f / out_t[E * n_agents] (agent
 * e * n_agents + a, the flattened observable's order; out_logits optional).
 * Replaces SubdividedVisionCones.compute_observable + FlaxModel.compute_action
 * + the sampling and action-table lookup of ActorCriticAgent.calc_action
 * (subdivided_vision_cones.py:241-258, actor_critic.py:159-184,
 * flax_network.py:153-195, gumbel_distribution.py:37-40).  agent_state:
 * device call counters, one per agent (n_state >= E * n_agents; each call
 * draws agent a's uniforms with counter agent_state[a] and advances it).
 * Runs on the engine's stream; a deferred build rides along as in the two
 * calls it replaces.  Sampling parity is statistical, as for
 * swarm_policy_mlp_sample; the logits may differ from that kernel's in the
 * last bits (the hidden units are summed in another split). */
int swarm_engine_vision_policy(swarm_engine_t *e, const swarm_vision_params_t *vp,
                               const int32_t *agent_idx, int32_t n_agents, const float *radii,
                               const int32_t *types, float *features, const float *w1,
                               const float *b1, int32_t hidden, const float *w2, const float *b2,
                               int32_t k, uint64_t seed, uint64_t *agent_state, int32_t n_state,
                               float explore_p, const float *f_table, const float *t_table,
                               int64_t *out_idx, float *out_logp, float *out_f, float *out_t,
                               float *out_logits);

/* Distances to a source for the concentration-field observable and the
 * gradient-sensing task (concentration_field.py:84-108,
 * gradient_sensing.py:92-126): for agent a of env e,
 *   p      = unwrapped_pos / box_scale (fp64),
 *   d_cur  = || fp32(source/box_scale - p) ||,
 *   d_prev = same for the history position,
 * then (if update_history) history <- current.  History is kept as raw
 * engine coordinates hist_q/hist_img [3][E*n_agents] (device).
 * init_only != 0: only copy the current positions into the history. */
int swarm_field_distance(swarm_engine_t *e, const int32_t *agent_idx,
                         int32_t n_agents, const double source[3],
                         const double box_scale[3], uint32_t *hist_q,
                         int32_t *hist_img, float *d_cur, float *d_prev,
                         int32_t update_history, int32_t init_only);

/* Fused field observable / reward for an affine decay f(d) = a + b d:
 * out[e][a] = scale * (f(d_cur) - f(d_prev)) (concentration_field.py:
 * 102-104), clipped at 0 when clip_at_zero (gradient_sensing.py:117-118);
 * the history is updated.  Distances as in swarm_field_distance. */
int swarm_field_transform(swarm_engine_t *e, const int32_t *agent_idx,
                          int32_t n_agents, const double source[3],
                          const double box_scale[3], uint32_t *hist_q,
                          int32_t *hist_img, float decay_a, float decay_b,
                          float scale, int32_t clip_at_zero, float *out);

/* The history of swarm_field_distance / swarm_field_transform after a
 * swarm_engine_reset_marked: for every agent of an env with d_mask[env] != 0
 * (device uint8 [E]) history <- current position, what init_only does for
 * every env; the history of an unmarked env is not stored to.  No host copy,
 * no synchronisation, a grid that does not depend on the mask: capturable. */
int swarm_field_history_marked(swarm_engine_t *e, const uint8_t *d_mask,
                               const int32_t *agent_idx, int32_t n_agents,
                               uint32_t *hist_q, int32_t *hist_img);

/* Parity helper: all pairs (i<j) of env `env` closer than `cutoff`
 * (minimum image if periodic) as int32 [max_pairs][2] (host), count in
 * *n_pairs; returns SWARM_ECAPACITY if more than max_pairs. */
int swarm_engine_neighbor_pairs(swarm_engine_t *e, int32_t env, double cutoff,
                                int32_t *pairs, int32_t max_pairs,
                                int32_t *n_pairs);

/* Pairwise scaled distances for ParticleSensing / SpeciesSearch
 * (particle_sensing.py:95-121, species_search.py:97-130): for every env e,
 * agent a < n_agents and sensed column m in [m0, m0 + mc),
 *   out[e][m - m0][a] = || (fp32(x_sensed[m]) - fp32(x_agent[a])) / box_scale ||
 * with unwrapped positions (no minimum image, as the reference).  Indices
 * are device int32 into [0, N); out is device fp32 [E][mc][n_agents]. */
int swarm_pair_distances(swarm_engine_t *e, const int32_t *agent_idx, int32_t n_agents,
                         const int32_t *sensed_idx, int32_t m0, int32_t mc,
                         const double box_scale[3], float *out);

/* Fused action sampling for the device rollout path (all pointers device):
 * per agent a < n, over logits [n][k] fp32 (k <= 64):
 *   idx  = argmax_j(logits_j - log(-log u_j))     gumbel_distribution.py:37-40
 *   idx  = RandomExploration(idx) when explore_p > 0 (random_exploration.py:54-71)
 *   logp = log(softmax(logits)_idx + 1e-8)         flax_network.py:185-192
 *   out_f = f_table[idx], out_t = t_table[idx]     actor_critic.py:159-184
 * u from Philox4x32-10 keyed by seed; state = n_state >= ceil(n / 64) uint64
 * call counters of device memory (one per group of 64 agents; zero-initialise
 * once), advanced on every call so graph replays draw fresh numbers.
 * Asynchronous on `stream` (hipStream_t, NULL = default stream).
 * Replaces the jnp sampling chain of FlaxModel.compute_action. */
int swarm_sample_actions(const float *logits, int32_t n, int32_t k, uint64_t seed,
                         uint64_t *state, int32_t n_state, float explore_p,
                         const float *f_table, const float *t_table, int64_t *out_idx,
                         float *out_logp, float *out_f, float *out_t, void *stream);

/* The whole rollout policy of FlaxModel.compute_action
 * (networks/flax_network.py:153-195) for the reference's actor-critic MLP
 * (Dense(hidden) -> ReLU -> Dense(k), CI/espresso_tests/integration_tests/
 * test_rl_trainers.py:17-26) in one launch:
 *   logits = W2 relu(W1 obs_a + b1) + b2        (fp32; torch Linear layouts
 *            W1 [hidden][d_in], W2 [k][hidden], read in place)
 * followed by exactly the sampling of swarm_sample_actions (same counters,
 * same bits for the same logits).  obs [n][d_in]; d_in <= 16, hidden <= 256,
 * k <= 16.  out_logits [n][k] is optional (NULL: not written).  The critic
 * head is not evaluated (the rollout does not read it). */
int swarm_policy_mlp_sample(const float *obs, int32_t n, int32_t d_in, const float *w1,
                            const float *b1, int32_t hidden, const float *w2, const float *b2,
                            int32_t k, uint64_t seed, uint64_t *state, int32_t n_state,
                            float explore_p, const float *f_table, const float *t_table,
                            int64_t *out_idx, float *out_logp, float *out_f, float *out_t,
                            float *out_logits, void *stream);

/* swarm_policy_mlp_sample, also carrying the last stage of engine e's
 * deferred build (swarm_engine_defer_build) as extra workgroups of the same
 * launch when it is pending; same arguments and results otherwise. */
int swarm_engine_policy_mlp_sample(swarm_engine_t *e, const float *obs, int32_t n,
                                   int32_t d_in, const float *w1, const float *b1,
                                   int32_t hidden, const float *w2, const float *b2,
                                   int32_t k, uint64_t seed, uint64_t *state,
                                   int32_t n_state, float explore_p, const float *f_table,
                                   const float *t_table, int64_t *out_idx, float *out_logp,
                                   float *out_f, float *out_t, float *out_logits,
                                   void *stream);

/* The whole rollout policy of FlaxModel.compute_action
 * (networks/flax_network.py:153-195) for a deep actor-critic MLP with
 * n_hidden = 2 or 3 hidden ReLU layers (the three-layer network of
 * CI/unit_tests/force_function/test_force_fn.py:38-45) in one launch:
 *   h_1 = relu(W_1 obs_a + b_1),  h_l = relu(W_l h_{l-1} + b_l),
 *   logits = Wa h_L + ba                         (fp32, f32 matrix instructions)
 * followed by exactly the sampling of swarm_sample_actions (same counters,
 * same bits for the same logits).  obs [n][d_in].  widths, w and b are HOST
 * arrays of n_hidden entries, read at call time (the launch is capturable):
 * widths[l] the units of hidden layer l, w[l] / b[l] the device pointers of
 * its torch Linear weight [widths[l]][widths[l - 1]] (w[0]: [widths[0]][d_in])
 * and bias, read in place; wa [k][widths[n_hidden - 1]], ba [k].
 * 2 <= n_hidden <= 3, every width <= 128, d_in <= 32, k <= 16; outside these
 * limits the call returns an error and launches nothing.  out_logits [n][k]
 * is optional (NULL: not written).  The critic head is not evaluated.  An
 * engine's deferred build does not ride along in this launch: the stages no
 * launch carried run at the next swarm_engine_integrate. */
int swarm_policy_deep_sample(const float *obs, int32_t n, int32_t d_in, int32_t n_hidden,
                             const int32_t *widths, const float *const *w,
                             const float *const *b, const float *wa, const float *ba,
                             int32_t k, uint64_t seed, uint64_t *state, int32_t n_state,
                             float explore_p, const float *f_table, const float *t_table,
                             int64_t *out_idx, float *out_logp, float *out_f, float *out_t,
                             float *out_logits, void *stream);

/* Kernel timing for measurement (bench.py's roofline of the PPO update):
 * the summed duration (ms) and count of the k_ppo_grads launches this
 * thread made through swarm_ppo_epoch_grad since the previous call (HIP
 * events on the caller's stream around each epoch's launches; waits for
 * them), then enables recording with `enable` back-to-back launches of the
 * (deterministic) gradient kernel per epoch, or disables it (0).  Not for
 * use under graph capture. */
int swarm_ppo_profile(int32_t enable, double *grads_ms, int32_t *launches);

/* The gradient of one PPO epoch -- ProximalPolicyLoss._calculate_loss
 * differentiated by jax.value_and_grad (swarmrl/losses/
 * proximal_policy_loss.py:62-138, :160-168) with its GAE value function
 * (value_functions/generalized_advantage_estimate.py:42-72) -- for the
 * actor-critic MLP Dense(hidden) -> ReLU -> {Dense(k) logits, Dense(1)
 * value}.  Samples are T time slices x S agent columns, sample t * S + col:
 * x [T*S][d_in], actions [T*S] (int64), old_logp [T*S], rewards [T][S].
 * Parameters in torch Linear layouts: w1 [hidden][d_in], b1 [hidden],
 * wa [k][hidden], ba [k], wc [1][hidden], bc [1].  Writes grad =
 * d loss / d params, concatenated as w1 | b1 | wa | ba | wc | bc
 * (hidden*d_in + hidden + k*hidden + k + hidden + 1 floats).  The loss:
 *   sum -min(r A, clip(r, 1 - clip_eps, 1 + clip_eps) A)
 *   - entropy_coef * sum -(p + 1e-8) log(p + 1e-8)
 *   + 0.5 * sum huber(V, R)
 * with r = exp(log(p_a + 1e-8) - old_logp), A the GAE advantages
 * normalised by mean and population std (+ fp32 eps) and held constant,
 * R = A_raw + V differentiated through V as in the reference.
 * d_in <= 32, hidden <= 256, k <= 16, T*S < 2^31.  workspace: device
 * memory of at least swarm_ppo_workspace_bytes(T, S, d_in, hidden, k)
 * bytes.  Deterministic (fixed reduction order).  Asynchronous on
 * `stream`. */
int64_t swarm_ppo_workspace_bytes(int32_t T, int32_t S, int32_t d_in, int32_t hidden,
                                  int32_t k);
int swarm_ppo_epoch_grad(const float *x, int32_t T, int32_t S, int32_t d_in,
                         const int64_t *actions, const float *old_logp, const float *rewards,
                         const float *w1, const float *b1, int32_t hidden, const float *wa,
                         const float *ba, int32_t k, const float *wc, const float *bc,
                         float gamma, float lambda, float clip_eps, float entropy_coef,
                         void *workspace, int64_t workspace_bytes, float *grad, void *stream);

/* swarm_ppo_epoch_grad for the deep actor-critic MLP of
 * swarm_policy_deep_sample: n_hidden = 2 or 3 hidden ReLU layers, then
 * {Dense(k) logits, Dense(1) value}.  The same loss, GAE and reference
 * semantics (proximal_policy_loss.py:62-138, :160-168;
 * generalized_advantage_estimate.py:42-72): R = A_raw + V differentiated
 * through V, only the normalised advantages constant, entropy eps 1e-8.
 * widths, w and b are HOST arrays of n_hidden entries read at call time (the
 * launches are capturable), w / b holding device pointers of the torch
 * Linear weights [widths[l]][widths[l - 1]] (w[0]: [widths[0]][d_in]) and
 * biases; wa [k][widths[n_hidden - 1]], ba [k], wc [1][widths[n_hidden - 1]],
 * bc [1].  Writes grad = d loss / d params concatenated as
 * w1 | b1 | ... | wL | bL | wa | ba | wc | bc.  2 <= n_hidden <= 3, every
 * width <= 128, d_in <= 32, k <= 16, T*S < 2^31: outside these limits the
 * calls return an error (workspace_bytes: -1) and launch nothing.
 * workspace: device memory of at least swarm_ppo_deep_workspace_bytes(...)
 * bytes.  The products run on the f32 matrix instructions; block partials
 * are summed in fp64 in a fixed order (deterministic, no floating-point
 * atomics).  The optimizer step stays the caller's.  Asynchronous on
 * `stream`. */
int64_t swarm_ppo_deep_workspace_bytes(int32_t T, int32_t S, int32_t d_in, int32_t n_hidden,
                                       const int32_t *widths, int32_t k);
int swarm_ppo_deep_epoch_grad(const float *x, int32_t T, int32_t S, int32_t d_in,
                              const int64_t *actions, const float *old_logp,
                              const float *rewards, int32_t n_hidden, const int32_t *widths,
                              const float *const *w, const float *const *b, const float *wa,
                              const float *ba, int32_t k, const float *wc, const float *bc,
                              float gamma, float lambda, float clip_eps, float entropy_coef,
                              void *workspace, int64_t workspace_bytes, float *grad,
                              void *stream);

/* The optimizer of the PPO update (torch.optim.Adam as TorchModel builds it
 * for the optax optimizer of swarmrl/networks/flax_network.py:42-79): the six tensors
 * w1 | b1 | wa | ba | wc | bc of swarm_ppo_epoch_grad, updated in place with
 * their first / second moments and per-tensor step counts (device fp32, as
 * torch's capturable Adam keeps them).  weight_decay 0, no amsgrad. */
typedef struct {
  float lr, beta1, beta2, eps;
  float *param[6];
  float *exp_avg[6];
  float *exp_avg_sq[6];
  float *step[6];
} swarm_adam_t;

/* One PPO epoch with the optimizer step fused into its last launch: the
 * gradient of swarm_ppo_epoch_grad (written to grad, the parameters read
 * from adam->param) followed by the Adam step of torch's fused Adam
 * (step += 1; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2;
 * p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps), fp32).
 * Replaces swarm_ppo_epoch_grad + optimizer.step() (three launches fewer per
 * epoch).  The workspace must be zero-filled before its first use (the
 * kernel leaves its ticket at zero after each call). */
int swarm_ppo_epoch_step(const float *x, int32_t T, int32_t S, int32_t d_in,
                         const int64_t *actions, const float *old_logp, const float *rewards,
                         int32_t hidden, int32_t k, float gamma, float lambda, float clip_eps,
                         float entropy_coef, const swarm_adam_t *adam, void *workspace,
                         int64_t workspace_bytes, float *grad, void *stream);

/* swarm_ppo_epoch_grad, swarm_ppo_epoch_step and swarm_ppo_deep_epoch_grad
 * for a trajectory in which envs ended episodes on their own
 * (swarm_engine_reset_marked): the same calls plus dones (device uint8
 * [T][S / per_env], non-zero: the env was reset after step t) and per_env,
 * column col of the T x S grid belonging to env col / per_env.  Where
 * dones[t][env] is set the advantage estimate treats step t as the last step
 * is treated -- delta_t = r_t - V_t, nothing carried in from t + 1 -- and in
 * the backward pass later values do not reach earlier returns.  The
 * normalisation of the advantages runs over all T x S samples.  With all-zero
 * dones the gradient is bit-identical to the call without.  SWARM_EINVAL for
 * null dones and for a per_env below 1 or not dividing S; otherwise the
 * limits, workspaces and determinism of the calls they extend. */
int swarm_ppo_epoch_grad_ep(const float *x, int32_t T, int32_t S, int32_t d_in,
                            const int64_t *actions, const float *old_logp, const float *rewards,
                            const float *w1, const float *b1, int32_t hidden, const float *wa,
                            const float *ba, int32_t k, const float *wc, const float *bc,
                            float gamma, float lambda, float clip_eps, float entropy_coef,
                            void *workspace, int64_t workspace_bytes, float *grad, void *stream,
                            const uint8_t *dones, int32_t per_env);
int swarm_ppo_epoch_step_ep(const float *x, int32_t T, int32_t S, int32_t d_in,
                            const int64_t *actions, const float *old_logp, const float *rewards,
                            int32_t hidden, int32_t k, float gamma, float lambda, float clip_eps,
                            float entropy_coef, const swarm_adam_t *adam, void *workspace,
                            int64_t workspace_bytes, float *grad, void *stream,
                            const uint8_t *dones, int32_t per_env);
int swarm_ppo_deep_epoch_grad_ep(const float *x, int32_t T, int32_t S, int32_t d_in,
                                 const int64_t *actions, const float *old_logp,
                                 const float *rewards, int32_t n_hidden, const int32_t *widths,
                                 const float *const *w, const float *const *b, const float *wa,
                                 const float *ba, int32_t k, const float *wc, const float *bc,
                                 float gamma, float lambda, float clip_eps, float entropy_coef,
                                 void *workspace, int64_t workspace_bytes, float *grad,
                                 void *stream, const uint8_t *dones, int32_t per_env);

/* The rollout policy of an ensemble of n_members independent actor-critic
 * MLPs in one launch.  Replaces the per-member policy calls of the
 * reference's EnsembleTraining, which trains every member in a process and
 * an engine of its own (training_routines/ensemble_submit.py:93-138).
 * Member m owns agents [m * n_per, (m + 1) * n_per) of the flat batch:
 * obs [n_members][n_per][d_in]; parameters stacked in torch Linear layouts,
 * w1 [n_members][hidden][d_in], b1 [n_members][hidden],
 * w2 [n_members][k][hidden], b2 [n_members][k]; seeds: n_members uint64 of
 * DEVICE memory (member m's Philox key); state [n_members][n_state_per]
 * uint64 call counters, n_state_per >= ceil(n_per / 64) (zero-initialise
 * once).  Outputs [n_members * n_per]; out_logits [n_members * n_per][k] is
 * optional (NULL: not written).  A workgroup serves one member; the agent
 * index that keys Philox and the counter groups of 64 agents are local to
 * the member, and the lanes per agent follow from n_per.
 * Contract: member m's out_idx, out_logp, out_f, out_t, out_logits and
 * advanced counters are bit-identical to swarm_policy_mlp_sample called on
 * member m's slices alone with seeds[m] and state[m], whoever shares the
 * launch.  d_in <= 16, hidden <= 256, k <= 16, 1 <= n_members <= 1024;
 * outside these limits the call returns an error and launches nothing.
 * Asynchronous on `stream`, capturable. */
int swarm_policy_ensemble_sample(const float *obs, int32_t n_members, int32_t n_per,
                                 int32_t d_in, const float *w1, const float *b1, int32_t hidden,
                                 const float *w2, const float *b2, int32_t k,
                                 const uint64_t *seeds, uint64_t *state, int32_t n_state_per,
                                 float explore_p, const float *f_table, const float *t_table,
                                 int64_t *out_idx, float *out_logp, float *out_f, float *out_t,
                                 float *out_logits, void *stream);

/* The gradient of one PPO epoch (swarm_ppo_epoch_grad) for each of
 * n_members independent actor-critic MLPs, in the same four launches with
 * the member as the outer grid dimension.  Replaces the per-member updates
 * of the reference's EnsembleTraining
 * (training_routines/ensemble_submit.py:93-138).  Data is member-major:
 * x [n_members][T*S][d_in], actions / old_logp [n_members][T*S],
 * rewards [n_members][T][S]; S = agent columns per member, sample t * S + col
 * inside a member.  Parameters stacked: w1 [n_members][hidden][d_in],
 * b1 [n_members][hidden], wa [n_members][k][hidden], ba [n_members][k],
 * wc [n_members][1][hidden], bc [n_members][1].  grad is laid out for the
 * stacked tensors,
 *   w1 [M][hidden*d_in] | b1 [M][hidden] | wa [M][k*hidden] | ba [M][k] |
 *   wc [M][hidden] | bc [M]                        (M = n_members)
 * so consecutive views of it match the stacked parameters.  Every member
 * has its own advantage normalisation and workspace slices, and every
 * decision (kernel variants, number of gradient blocks) is taken from the
 * member's own T*S; block partials are sized by the blocks a member
 * launches.
 * Contract: member m's segments of grad are bit-identical to
 * swarm_ppo_epoch_grad on member m's data and parameters alone.
 * Deterministic.  The limits of swarm_ppo_epoch_grad, and
 * 1 <= n_members <= 1024; outside them the calls return an error
 * (workspace_bytes: -1) and launch nothing.  workspace: device memory of at
 * least swarm_ppo_ensemble_workspace_bytes(...) bytes.  The optimizer step
 * stays the caller's (one elementwise Adam over the stacked tensors is
 * n_members independent Adams).  Asynchronous on `stream`, capturable. */
int64_t swarm_ppo_ensemble_workspace_bytes(int32_t n_members, int32_t T, int32_t S,
                                           int32_t d_in, int32_t hidden, int32_t k);
int swarm_ppo_ensemble_epoch_grad(const float *x, int32_t n_members, int32_t T, int32_t S,
                                  int32_t d_in, const int64_t *actions, const float *old_logp,
                                  const float *rewards, const float *w1, const float *b1,
                                  int32_t hidden, const float *wa, const float *ba, int32_t k,
                                  const float *wc, const float *bc, float gamma, float lambda,
                                  float clip_eps, float entropy_coef, void *workspace,
                                  int64_t workspace_bytes, float *grad, void *stream);

/* The rollout policy of an ensemble of n_members independent deep
 * actor-critic MLPs (swarm_policy_deep_sample's network: n_hidden = 2 or 3
 * hidden ReLU layers) in one launch.  Replaces the per-member policy calls
 * of the reference's EnsembleTraining, one process and engine per member
 * (training_routines/ensemble_submit.py:93-138).  Member m owns agents
 * [m * n_per, (m + 1) * n_per): obs [n_members][n_per][d_in].  widths, w and
 * b are HOST arrays of n_hidden entries read at call time; w[l] is the
 * device pointer of the stacked [n_members][widths[l]][widths[l-1]]
 * (widths[-1] = d_in), b[l] of [n_members][widths[l]];
 * wa [n_members][k][widths[n_hidden-1]], ba [n_members][k].  seeds:
 * n_members uint64 of DEVICE memory; state [n_members][n_state_per] uint64
 * call counters, n_state_per >= ceil(n_per / 64) (zero-initialise once).
 * Outputs [n_members * n_per]; out_logits [n_members * n_per][k] is optional
 * (NULL: not written).  A workgroup is one counter group of 64 agents of
 * one member; agent and group indices are local to the member.
 * Contract: member m's out_idx, out_logp, out_f, out_t, out_logits and
 * advanced counters are bit-identical to swarm_policy_deep_sample called on
 * member m's slices alone with seeds[m] and state[m], whoever shares the
 * launch.  The limits of swarm_policy_deep_sample (2 <= n_hidden <= 3,
 * widths <= 128, d_in <= 32, k <= 16) and 1 <= n_members <= 1024; outside
 * them the call returns an error and launches nothing.  Asynchronous on
 * `stream`, capturable. */
int swarm_policy_deep_ensemble_sample(const float *obs, int32_t n_members, int32_t n_per,
                                      int32_t d_in, int32_t n_hidden, const int32_t *widths,
                                      const float *const *w, const float *const *b,
                                      const float *wa, const float *ba, int32_t k,
                                      const uint64_t *seeds, uint64_t *state,
                                      int32_t n_state_per, float explore_p, const float *f_table,
                                      const float *t_table, int64_t *out_idx, float *out_logp,
                                      float *out_f, float *out_t, float *out_logits,
                                      void *stream);

/* The gradient of one PPO epoch (swarm_ppo_deep_epoch_grad) for each of
 * n_members independent deep actor-critic MLPs, in the same four launches
 * with the member as the outer grid dimension.  Replaces the per-member
 * updates of the reference's EnsembleTraining
 * (training_routines/ensemble_submit.py:93-138).  Data is member-major as
 * in swarm_ppo_ensemble_epoch_grad: x [n_members][T*S][d_in], actions /
 * old_logp [n_members][T*S], rewards [n_members][T][S].  widths, w and b are
 * HOST arrays read at call time, w[l] / b[l] the device pointers of the
 * stacked [n_members][widths[l]][widths[l-1]] / [n_members][widths[l]];
 * wa [n_members][k][H], ba [n_members][k], wc [n_members][1][H],
 * bc [n_members][1] (H = widths[n_hidden-1]).  grad is laid out for the
 * stacked tensors,
 *   w1 [M][..] | b1 [M][..] | ... | wL | bL | wa [M][k*H] | ba [M][k] |
 *   wc [M][H] | bc [M]                             (M = n_members)
 * each segment member-major, so consecutive views of it match the stacked
 * parameters.  Every member has its own values, advantages, GAE partials
 * and block partials, and every decision (GAE variant, number of gradient
 * blocks min(ceil(T*S / 64), 256)) is taken from the member's own T*S;
 * block partials are sized by the blocks a member launches.
 * Contract: member m's segments of grad are bit-identical to
 * swarm_ppo_deep_epoch_grad on member m's data and parameters alone,
 * whoever shares the launch.  Deterministic, no floating-point atomics.
 * The limits of swarm_ppo_deep_epoch_grad (2 <= n_hidden <= 3, widths <=
 * 128, d_in <= 32, k <= 16, T*S < 2^31) and 1 <= n_members <= 1024; outside
 * them the calls return an error (workspace_bytes: -1) and launch nothing.
 * workspace: device memory of at least
 * swarm_ppo_deep_ensemble_workspace_bytes(...) bytes; a smaller one is
 * SWARM_EINVAL and nothing is launched.  The first call of a network shape
 * on a device must not be under stream capture (it raises the kernel's
 * dynamic LDS limit).  The optimizer step stays the caller's.  Asynchronous
 * on `stream`, capturable. */
int64_t swarm_ppo_deep_ensemble_workspace_bytes(int32_t n_members, int32_t T, int32_t S,
                                                int32_t d_in, int32_t n_hidden,
                                                const int32_t *widths, int32_t k);
int swarm_ppo_deep_ensemble_epoch_grad(const float *x, int32_t n_members, int32_t T, int32_t S,
                                       int32_t d_in, const int64_t *actions,
                                       const float *old_logp, const float *rewards,
                                       int32_t n_hidden, const int32_t *widths,
                                       const float *const *w, const float *const *b,
                                       const float *wa, const float *ba, int32_t k,
                                       const float *wc, const float *bc, float gamma,
                                       float lambda, float clip_eps, float entropy_coef,
                                       void *workspace, int64_t workspace_bytes, float *grad,
                                       void *stream);

/* Random Network Distillation distance (the intrinsic reward of
 * swarmrl/intrinsic_reward/random_network_distillation.py:126-143 with the
 * networks of rnd_configs.py:17-38): for every observation a < n of x
 * [n][d_in] (device fp32), target and predictor networks Dense(width) ->
 * ReLU -> Dense(width) -> ReLU -> Dense(width), and
 *   out[a] = (sum_k |t_k - p_k|^order)^(1/order)      (ZnNL OrderNDifference).
 * target / predictor: host arrays of the six device parameter pointers
 * w1 [width][d_in], b1, w2 [width][width], b2, w3 [width][width], b3 (torch
 * Linear layouts, read in place).  width = 32, d_in <= 16.  Asynchronous on
 * `stream`. */
int swarm_rnd_distance(const float *x, int32_t n, int32_t d_in, int32_t width,
                       const float *const *target, const float *const *predictor,
                       int32_t order, float *out, void *stream);

/* The per-env RND intrinsic reward added to the task reward (the device
 * path of random_network_distillation.py:126-143 followed by the
 * `task + intrinsic` of actor_critic.py calc_reward): x [n_envs * per_env]
 * [d_in] observations (env-major), the metric of every observation into
 * metric[n_envs * per_env] (as swarm_rnd_distance), r_e = mean of env e's
 * metrics (fp64 sum in a fixed order), clipped to [clip_lo, clip_hi] when
 * clip != 0, into env_reward[n_envs], and
 *   rewards[e][a] = base[e][a] + r_e   (base NULL: r_e).
 * workspace: device memory of swarm_rnd_env_workspace_bytes(n_envs, per_env)
 * bytes, zeroed before its first use (the call leaves it ready for the
 * next one; one workspace per concurrent caller).  One launch, asynchronous
 * on `stream`; no host synchronisation. */
int swarm_rnd_env_reward(const float *x, int32_t n_envs, int32_t per_env, int32_t d_in,
                         int32_t width, const float *const *target,
                         const float *const *predictor, int32_t order, int32_t clip,
                         float clip_lo, float clip_hi, const float *base, float *metric,
                         float *env_reward, float *rewards, void *workspace,
                         int64_t workspace_bytes, void *stream);
int64_t swarm_rnd_env_workspace_bytes(int32_t n_envs, int32_t per_env);

/* Training the RND predictor (RNDReward.update of
 * swarmrl/intrinsic_reward/random_network_distillation.py:102-123: ZnNL
 * SimpleTraining.train_model with MeanPowerLoss(order) and optax.adam).
 *
 * swarm_rnd_targets: y[a][width] = target(x[a]) for every observation a < n
 * of x [n][d_in] (device fp32), each output summed in the order of
 * swarm_rnd_distance's forward.  target: host array of the six device
 * parameter pointers, as swarm_rnd_distance.
 *
 * swarm_rnd_train_epoch: the ceil(n / batch_size) minibatch steps of one
 * epoch, in order, in one workgroup that keeps the predictor and its Adam
 * moments on chip.  Step s takes the rows perm[s B .. s B + B) of x and y
 * (perm [n] int64, a permutation of 0 .. n - 1 as torch.randperm returns it;
 * the last batch may be short, its mean is over its own size): predictor
 * forward, loss mean(|pred - y|^loss_order), backward, and the Adam step of
 * swarm_ppo_epoch_step on adam's six tensors w1 | b1 | w2 | b2 | w3 | b3
 * (torch Linear layouts), their moments and step counts, all updated in
 * place.  Every sum runs in a fixed order and there are no floating-point
 * atomics: the same bits on every run.  loss_out: device [ceil(n / B)],
 * receives each step's loss; NULL to skip.  Limits: width = 32, 1 <= d_in <=
 * 16, 1 <= batch_size <= 64, 0 <= n < 2^31, loss_order >= 1 (order 1: the
 * gradient is sign(d), 0 at d = 0); outside them the call returns an error
 * and launches nothing.  One launch per 32768 steps of the epoch (a bound on
 * the run time of a launch: below 0.4 s).  Both calls are asynchronous on `stream`. */
int swarm_rnd_targets(const float *x, int32_t n, int32_t d_in, int32_t width,
                      const float *const *target, float *y, void *stream);
int swarm_rnd_train_epoch(const float *x, const float *y, const int64_t *perm, int32_t n,
                          int32_t d_in, int32_t width, int32_t batch_size, int32_t loss_order,
                          const swarm_adam_t *adam, float *loss_out, void *stream);

/* Neighbour reductions for the classical agents (all pointers device):
 * get_colloids_in_vision of bechinger_models.py:156-171 (range + cone) and
 * lymburn_model.py:113-125 (range only, half_angle < 0), fused with the
 * sums those agents take over the neighbours it returns.  pos, dir and vel
 * [E][N][3] fp64 (pos unwrapped; vel may be NULL), types [N];
 * candidates: j != agent with bit types[j] set in cand_type_mask.  Per env
 * e and agent a, out[e][a][12] (fp64) = {count, sum 1/(2 pi |d|), sum d (3),
 * sum |d|^2, sum dir_j (3), sum v_j (3)} with d = x_j - x_agent.
 * Asynchronous on `stream`. */
int swarm_neighbor_reduce(const double *pos, const double *dir, const double *vel,
                          const int32_t *types, int32_t n_envs, int32_t n,
                          const int32_t *agent_idx, int32_t n_agents,
                          uint32_t cand_type_mask, double vision_range,
                          double half_angle, double *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SWARMRL_AMD_H */

/* include/sph_hip.h -- C ABI of libsph_hip.so, the MI355X (gfx950) SPH step library.
 *
 * This is the drop-in boundary for the hot path of oadrian/GPUFluidSimulator: it
 * replaces the extern "C" seam between the host class and the CUDA kernels,
 * /root/reference/SPH/particleSystem.cuh:3-30 (definitions particleSystem.cu:422-535).
 * The reference seam passes an 88-byte AoS `Particle*` and a device-resident
 * `SimParams*` to every call; here the device state (sorted SoA arrays, cell table,
 * sort scratch) lives in an opaque context and parameters travel by value.  A
 * binary-compatible rendition of the reference's own 19 symbols is declared in
 * include/sph_compat_seam.h on top of these entry points.
 *
 * Conventions
 *   - plain C types only; every pointer is a HOST pointer unless the name ends in
 *     `_dev` (then it is a device pointer on the context's GPU);
 *   - every function returns 0 on success or a negative SPH_E* code; the message is
 *     available from sph_last_error() (thread-local).  The reference's convention is
 *     abort-on-error (checkCudaErrors -> exit, common/inc/helper_cuda.h:566-579); the
 *     host class in include/particleSystem.h restores that behaviour on top;
 *   - all work is enqueued on the context's stream (sph_set_stream; default: the NULL
 *     stream like the reference) and is asynchronous unless the function returns data
 *     to the host; one context must not be used from two host threads at once;
 *   - there is NO CPU fallback: without a gfx950 device sph_create fails.
 *
 * What is ABI and what is not (every entry point belongs to exactly one class; the class is repeated as a tag in front of the
 * declarations that are NOT stable ABI):
 *   STABLE ABI     what a host class, a driver or a launcher binds; kept across versions (SPH_ABI_VERSION changes otherwise):
 *                  sph_abi_version sph_last_error sph_device_count sph_select_device sph_selected_device sph_default_params
 *                  sph_grid_dim_for_edge | sph_create sph_create_slab sph_create_slab_layers sph_destroy sph_set_stream
 *                  sph_set_params sph_get_params sph_sync sph_num_particles sph_capacity sph_ghost_layers sph_set_precision
 *                  sph_get_precision | sph_upload sph_set_by_index sph_reset_lattice sph_download sph_download_owned
 *                  sph_positions_dev sph_download_positions4 sph_snapshot_save sph_snapshot_load sph_snapshot_info |
 *                  sph_set_colliders sph_get_colliders sph_set_collider_bodies sph_get_collider_impulses | sph_emit sph_remove sph_count_in_regions |
 *                  sph_obstacle_lattice sph_obstacle_build sph_obstacle_set_grid sph_obstacle_clear sph_obstacle_set_motion
 *                  sph_obstacle_get sph_obstacle_read sph_obstacle_sample sph_obstacle_build_mesh sph_obstacle_build_mesh_dev
 *                  sph_obstacle_build_obj sph_obstacle_set_pose sph_obstacle_get_pose sph_obstacle_set_sensor sph_obstacle_get_load
 *                  sph_obstacle_select sph_obstacle_selected sph_obstacle_installed sph_obstacle_clear_all
 *                  sph_obstacle_set_body sph_obstacle_get_body |
 *                  sph_camera_look_at sph_render sph_render_read sph_render_image_dev sph_surface_defaults sph_render_surface
 *                  sph_render_surface_read sph_solid_defaults sph_render_set_solids sph_render_get_solids | sph_mesh_defaults sph_mesh_lattice sph_mesh_extract sph_mesh_read sph_mesh_dev
 *                  sph_mesh_save_obj |
 *                  sph_hash sph_sort sph_build_cells sph_density sph_force sph_collide sph_integrate sph_step sph_step_phased
 *                  sph_force_collide_integrate | sph_timing_enable sph_timing_get sph_timing_reset | the z-slab phase calls
 *                  (sph_migrants_* sph_slab_counts sph_halo_* sph_layer_histogram) | sph_rccl_unique_id
 *                  sph_rccl_transport_create/_destroy sph_local_hub_* sph_local_transport_* | sph_slab_create sph_slab_destroy
 *                  sph_slab_step sph_slab_sync sph_slab_set_wait_timeout sph_slab_set_protocol sph_slab_recut sph_slab_ping
 *                  sph_slab_failed sph_slab_timing_enable/_reset/_get
 *   [introspect]   read-only views for parity tests, profiles and bench lines; may grow or change with the implementation:
 *                  sph_get_keys sph_get_order sph_get_cell_range sph_get_cells sph_cell_key sph_download_forces sph_sort_stats
 *                  sph_mesh_field_dims sph_mesh_field_read sph_obstacle_mesh_stats sph_sort_forms sph_last_sort_skipped sph_slab_stats sph_slab_counters sph_slab_in_place_merges
 *                  sph_slab_exchanges sph_slab_one_clamped sph_slab_recut_stats sph_slab_early_force_stats sph_slab_protocol sph_rccl_transport_info
 *   [tuning]       switches whose defaults are the product's settings; in fp32 results do not depend on them (A/B runs):
 *                  sph_set_sort_mode sph_set_direct_hull sph_set_pair_small_launch sph_set_block_order sph_slab_set_early_force
 *   [test hook]    exist for tests and measurement harnesses only: sph_test_trust_mover_hint sph_slab_test_raise_flag
 *                  sph_slab_test_set_hop_seq sph_slab_test_hop_state
 *                  sph_rccl_transport_selftest sph_loop_transport_create/_destroy sph_memory_stats sph_test_fail_alloc
 *                  sph_test_scan sph_test_lower_bounds sph_test_guard sph_test_guard_check
 */
#ifndef SPH_HIP_H
#define SPH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPH_ABI_VERSION 2

enum {
    SPH_OK = 0,
    SPH_E_INVALID = -1,   /* bad argument */
    SPH_E_DEVICE = -2,    /* HIP runtime error, no device, wrong architecture */
    SPH_E_NOMEM = -3,     /* device or host allocation failed */
    SPH_E_CAPACITY = -4,  /* more particles / ghosts than the context was created for */
    SPH_E_STATE = -5,     /* phase called out of order */
    SPH_E_PEER = -6       /* slab step: a neighbouring rank reported a failure and stopped (its own error says why) */
};

typedef struct sph_ctx sph_ctx;

/* Replaces `struct SimParams` (SPH/particles_kernel.cuh:36-50) plus the physics macros of
 * particles_kernel.cuh:20-33, which the reference bakes in at compile time.  The reference
 * never reads SimParams.gravity / colliderPos / colliderRadius in any kernel (setGravity is a
 * physics no-op), so they are not part of the device parameters; the collider
 * sphere has an API of its own here, which makes it push the fluid (sph_set_colliders).
 * Legal values (sph_create / sph_set_params refuse a bad grid, box, h, mass or radius):
 *   box_max > box_min on every axis, anywhere; grid 1..4096 per axis; h > 0, mass > 0, particle_radius > 0;
 *   rest_density, gravity_y: any finite value;  gas_constant >= 0 (0: p = 0 everywhere);
 *   viscosity >= 0 (0: no viscous force and the pressure force unchanged, as the reference's formulas give);
 *   wall_eps >= 0, below half the box edge;  wall_damping: any finite factor (0 stops, -1 reflects);
 *   restitution >= 0;  collision_param >= 0.
 * The neighbour search is the reference's 27-cell stencil: with a cell edge below h, neighbours beyond it are missed, as
 * in the reference.  The mixed-precision density pass (sph_set_precision) assumes cells at most 12 h wide: up to that edge
 * it keeps its tolerance (measured per cell width in DESIGN.md section 4; tests/test_gpu_mixed_walks.py runs 1.25, 4 and 12 h).
 * tests/test_gpu_physics_params.py holds the step to a float64 model of these formulas across these ranges. */
typedef struct sph_params {
    float box_min[3];        /* SimParams.boxMin                                   */
    float box_max[3];        /* SimParams.boxMax                                   */
    uint32_t grid[3];        /* cells per axis; the reference uses gridDim for all three */
    float h;                 /* m_H            0.1                                  */
    float mass;              /* MASS           65                                   */
    float rest_density;      /* REST_DENS      1000                                 */
    float gas_constant;      /* GAS_CONSTANT   2000                                 */
    float viscosity;         /* VISC           250                                  */
    float gravity_y;         /* GRAVITY * G_MODIFIER = -9.81f * 11000               */
    float wall_eps;          /* EPS_F          1e-5                                 */
    float wall_damping;      /* DAMPING_FACTOR -0.75 (particleSystem.cu:376)        */
    float restitution;       /* RESTITUTION    0                                    */
    float collision_param;   /* COLLISION_PARAM 1.0                                 */
    float particle_radius;   /* SimParams.particleRadius 1/64 (particleSystem.cpp:51) */
} sph_params;

/* Phases of one step, in the order of ParticleSystem::update's CUDA branch
 * (SPH/particleSystem.cpp:773-795); names follow dumpBenchmark (:697-716). */
enum {
    SPH_PH_ZINDEX = 0,   /* cudaMapZIndex            -> sph_hash            */
    SPH_PH_SORT,         /* cudaSortParticles        -> sph_sort (radix sort + reorder) */
    SPH_PH_BGRID,        /* cudaConstructBGrid + cudaConstructGridArray -> sph_build_cells */
    SPH_PH_DENS,         /* cudaComputeDensities     -> sph_density         */
    SPH_PH_FORCE,        /* cudaComputeForces        -> sph_force           */
    SPH_PH_COLLISION,    /* cudaParticleCollisions   -> sph_collide         */
    SPH_PH_INTEGRATE,    /* cudaIntegrate            -> sph_integrate       */
    SPH_PH_COUNT
};

/* ---- library ------------------------------------------------------------------------- */
int sph_abi_version(void);
const char* sph_last_error(void);
/* number of visible HIP devices, or a negative code; *is_gfx950 (optional) tells whether
 * device 0 is a gfx950.  Replaces cudaInit/findCudaDevice (particleSystem.cu:427-436). */
int sph_device_count(int* is_gfx950);

/* Choose the HIP device that contexts created with device = -1 use (default 0): the cudaSetDevice of
 * findCudaDevice behind the reference's `-device=N` flag (common/inc/helper_cuda.h:845,
 * particleSystem.cu:427-436, particles.cpp:676-706).  Fails if the device is not a gfx950. */
int sph_select_device(int device);
int sph_selected_device(void);

/* Fill *p with the reference's constants for a box of dimensions box_dims centred on the
 * origin (particleSystem.cpp:50-62) and the given grid. */
void sph_default_params(sph_params* p, const float box_dims[3], const uint32_t grid[3]);
/* nextPow2((uint)(edge / (0.66666f * h))): the reference's grid formula, particleSystem.cpp:46 */
uint32_t sph_grid_dim_for_edge(float edge, float h);

/* ---- context ------------------------------------------------------------------------- */
/* Whole-domain context for up to `capacity` particles on HIP device `device` (-1: the device chosen
 * with sph_select_device).
 * Replaces the allocateArray calls of _initialize (particleSystem.cpp:121-124). */
int sph_create(sph_ctx** out, int device, uint32_t capacity, const sph_params* p);
/* z-slab context (multi-GPU): owns the cell layers [z_lo, z_hi) of the global grid and keeps
 * one ghost layer on either side (up to ghost_capacity particles each). */
int sph_create_slab(sph_ctx** out, int device, uint32_t capacity, const sph_params* p,
                    uint32_t z_lo, uint32_t z_hi, uint32_t ghost_capacity);
/* The same with `ghost_layers` = 1 or 2 ghost cell layers per side (sph_create_slab: 1).  Two are what the ONE-MESSAGE slab
 * step needs (sph_slab_set_protocol): a rank then holds two layers of each neighbour's particles and recomputes the densities
 * of the inner one itself, instead of receiving them in a message of their own.  ghost_capacity then bounds the particles
 * of BOTH layers of a side. */
int sph_create_slab_layers(sph_ctx** out, int device, uint32_t capacity, const sph_params* p,
                           uint32_t z_lo, uint32_t z_hi, uint32_t ghost_capacity, uint32_t ghost_layers);
uint32_t sph_ghost_layers(const sph_ctx* c);        /* 0 for a whole-domain context */
void sph_destroy(sph_ctx* c);                       /* freeArray x4, particleSystem.cpp:180-183 */
int sph_set_stream(sph_ctx* c, void* hip_stream);   /* hipStream_t; NULL = default stream */
/* The per-update SimParams upload, :723.  Legal at any stage; the grid cannot change.  A caller between two phases goes on where
 * it was: the stage and the results of the phases that have run stay, and every later phase uses the new values.  Where the BOX
 * moved between two phases, the cell keys and the cell table in use are still those of the old box until the next sph_hash: the
 * neighbour stencil of that step is that of the cells the keys in use were computed with (the old box), its walls are the new
 * box's, and the integrate's keys for the next step are the new box's.  The next sort is the full one
 * (tests/test_gpu_context_walk.py holds such a step to the float64 model with exactly this stencil). */
int sph_set_params(sph_ctx* c, const sph_params* p);
int sph_get_params(const sph_ctx* c, sph_params* p);
int sph_sync(sph_ctx* c);                           /* threadSync, particleSystem.cu:467 */
uint32_t sph_num_particles(const sph_ctx* c);       /* owned particles */
uint32_t sph_capacity(const sph_ctx* c);

/* Arithmetic of the neighbour passes.  SPH_PRECISION_F32 (default): everything in fp32, the reference's
 * precision.  SPH_PRECISION_MIXED_F16 (BASELINE config 5): positions, velocities, densities and forces are
 * stored and integrated in fp32; inside the DENSITY traversal the per-pair arithmetic and the per-row
 * accumulators are packed fp16 (two candidates per lane-instruction) on coordinates relative to a reference point
 * of the wave in units of h (x as a coarse + a fine half, one reference per group of lanes that lie within 6 h in
 * y and z and 1000 h in x: right at any extent of the wave while a cell is at most 12 h wide), with NORMALISED kernel sums (the reference's densities ~2e6 do not
 * fit fp16); row sums are added up in fp32 and scaled once.  The force and collision passes stay fp32 (decided on
 * a device measurement).  Looser tolerance: DESIGN.md section 4.
 * A mixed density depends on which 64 slots share a wave (the reference point is the wave's).  A slab context's waves are
 * not the whole-domain context's, so in mixed precision an N-slab run (sph_slab_step) equals the one-context run to the mixed
 * tolerance, NOT bit for bit, under either message protocol (sph_slab_set_protocol); where the packed fp16 arithmetic is exact
 * the two agree to fp32 rounding (tests/test_gpu_slabs_mixed.py holds both). */
enum { SPH_PRECISION_F32 = 0, SPH_PRECISION_MIXED_F16 = 1 };
int sph_set_precision(sph_ctx* c, int precision);
int sph_get_precision(const sph_ctx* c);

/* ---- state transfer ------------------------------------------------------------------- */
/* Replace the particle set: n particles, xyz triples; index[i] is the immutable creation
 * index (Particle::index), NULL = 0..n-1.  Replaces copyArrayToDevice of the AoS array
 * (particleSystem.cpp:920,960).  Density/pressure/forces are reset to 0. */
int sph_upload(sph_ctx* c, uint32_t n, const float* pos_xyz, const float* vel_xyz, const uint32_t* index);
/* Overwrite position and/or velocity (xyz triples, either may be NULL) of the particles whose creation
 * index lies in [first_index, first_index + count), wherever they sit in the sorted arrays -- no
 * round trip of the whole state: replaces the host edit + copyArrayToDevice(start, count) of addSphere /
 * setArray (particleSystem.cpp:928-961).  Densities and forces of the current step become stale: the
 * next step starts with sph_hash as after sph_upload (the sort still only moves the particles whose
 * cell changed).  A slab context changes the particles it owns and ignores the others. */
int sph_set_by_index(sph_ctx* c, uint32_t first_index, uint32_t count, const float* pos_xyz, const float* vel_xyz);
/* Generate the dam-break lattice ON THE DEVICE (no host arrays, no PCIe): particles with creation index
 * index_start .. index_start+count of an (nx, ny, nz) lattice in the min corner of the box, spacing 2R,
 * zero velocity, counter-based jitter (amplitude from jitter_dims, NULL = the box; jitter = 0 switches it
 * off).  Bit-identical to sph_ic_dam_break / gpufluidsimulator_amd.ic.dam_break_lattice.  Like sph_upload it replaces the set:
 * the by-index position buffer of a whole-domain context reads (0, 0, 0, 0) for every index outside the range.  Replaces
 * initGrid + the AoS upload of reset(CONFIG_GRID) (SPH/particleSystem.cpp:839-874, 909-920). */
int sph_reset_lattice(sph_ctx* c, const uint32_t lattice[3], int jitter, const float jitter_dims[3],
                      uint64_t index_start, uint32_t count);
/* Gather the state BY CREATION INDEX relative to index_base: out[(index-index_base)*3+k].  The output
 * arrays hold index_count entries (x3 for the vectors); particles whose creation index lies outside
 * [index_base, index_base + index_count) are skipped, nothing beyond the arrays is written.
 * Any pointer may be NULL.  (The reference never copies particles back in CUDA mode; this is
 * the additive getArray of the north star.) */
int sph_download(sph_ctx* c, uint32_t index_base, uint32_t index_count, float* pos_xyz, float* vel_xyz, float* density,
                 float* pressure);
/* The owned particles compactly, in slot order: n x xyz, n x xyz, n creation indices (any may be NULL).
 * What a slab driver needs to move whole particles between ranks (re-balancing). */
int sph_download_owned(sph_ctx* c, float* pos_xyz, float* vel_xyz, uint32_t* index);
/* [introspect] */ int sph_download_forces(sph_ctx* c, uint32_t index_base, uint32_t index_count, float* fpress_xyz, float* fvisc_xyz,
                        float* dv_xyz, int32_t* collision_count);
/* The `gl_pos` analogue of cudaIntegrate (particleSystem.cu:416-419): float4 (x,y,z,1) per
 * creation index, written by sph_integrate / sph_step.  Device pointer, n*16 bytes. */
int sph_positions_dev(sph_ctx* c, void** out_dev);
int sph_download_positions4(sph_ctx* c, float* pos_xyzw);

/* ---- sphere colliders (the reference's SimParams.colliderPos / colliderRadius, which no kernel of the reference reads) ----
 * A context holds 0 (the default) to SPH_MAX_COLLIDERS solid spheres, each with a centre c, a radius R > 0 and a velocity u,
 * all in box coordinates.  The velocity is kinematic: the fluid never pushes a sphere (unless the sphere has a body with a mass:
 * sph_set_collider_bodies below).  On EVERY integrate the context
 * performs (sph_step, sph_step_phased / sph_integrate, sph_force_collide_integrate, sph_slab_step), after the integration and
 * the wall rule, each particle with position x and velocity v goes through the spheres in order j = 0..n-1:
 *
 *     d = x - c_j ; r2 = d.d ; Rp = R_j + wall_eps
 *     if r2 < Rp*Rp:
 *         nrm = r2 > 0 ? d / sqrt(r2) : (0, 1, 0)
 *         x   = c_j + Rp * nrm
 *         wn  = (v - u_j) . nrm
 *         if wn < 0:  v += (wall_damping - 1) * wn * nrm
 *
 * (fp32, each operation rounded, sums left to right: the normal part of the velocity relative to the sphere is scaled by
 * wall_damping, as the walls do).  A particle that any sphere moved goes through the wall rule once more, so it stays in the
 * box; the next step's cell key is that of the final position.  Where spheres overlap, their ORDER decides the result: a
 * later sphere may push a particle back into an earlier one.  After each step the centres advance on the host,
 * c_j = c_j + dt * u_j in fp32 -- once per step, however many launches the step's force pass takes (a slab step: up to three).
 * A sphere placed over fluid moves particles by up to R in one step; in a slab run such a particle must still land where the
 * slab step accepts arrivals (sph_slab_step, sph_slab_set_protocol: within the neighbour's slab), so place spheres over fluid
 * with R below a cell edge or move them in from outside the fluid.  In a slab run every rank holds the same spheres (positions
 * are global) and applies all of them to the particles it owns; ghosts arrive already pushed.
 * Snapshots do not carry colliders: sph_snapshot_load leaves the set as it is.  The reference seam (sph_compat_seam.h) has
 * none.  With no collider set, the step launches exactly the kernels it launches without this feature. */
#define SPH_MAX_COLLIDERS 8
typedef struct sph_collider {
    float center[3];
    float radius;
    float velocity[3];
    float pad;          /* ignored */
} sph_collider;
/* Replace the set by n spheres (n = 0 clears it).  n > SPH_MAX_COLLIDERS, a radius that is not finite or not positive, or a
 * centre or velocity that is not finite: SPH_E_INVALID, and the set is left unchanged. */
int sph_set_colliders(sph_ctx* c, uint32_t n, const sph_collider* colliders);
/* The current set with the ADVANCED centres: *n spheres into out (room for SPH_MAX_COLLIDERS; may be NULL if only *n is wanted).
 * On a tracked context (below) the centres and velocities live on the device: the call then synchronises the context's stream. */
int sph_get_colliders(const sph_ctx* c, uint32_t* n, sph_collider* out);

/* ---- spheres the fluid pushes back: the impulse sensor and free bodies ---------------------------------------------------------
 * A context with colliders may hold one BODY per sphere.  While bodies are set the context is TRACKED:
 *
 * Tracking.  In every integrate, where sphere j's branch `if wn < 0` above adds k * nrm (k = (wall_damping - 1) * wn) to a
 * particle's velocity, the same particle also forms  t = -(mass * (k * nrm))  -- fp32 products, each rounded (k itself, k * nrm
 * as the velocity takes it, and the one by mass), no multiply-add fusion; mass is sph_params.mass.  J_j is the sum of these terms over all owned particles of that step,
 * accumulated in float64: the momentum sphere j took from the fluid in the step.  Nothing else contributes -- not the position
 * projection, not the wall pass that follows it -- and the particle rule itself does not change by one bit.  The order of the
 * sum is fixed (lanes of a 64-slot wave in ascending order, then waves in ascending order within 256 equal runs of waves, then
 * the runs in ascending order): two runs of the same calls give the same bits in J, in the centres and in every particle.  No
 * floating-point atomic is involved.  A run is K = ceil(waves / 256) rounded up to a multiple of 4 waves long, waves =
 * ceil(owned particles / 64): run t is the waves [t K, min((t + 1) K, waves)), so the last run that holds a wave may be short
 * and the runs behind it are empty.  Every partial sum starts at 0.0 -- a wave's sum for sphere j (only a wave in which j kicked
 * a lane has one), a run's sum of its waves' sums, and J_j over the runs that hold any wave's sum for any sphere.
 *
 * Sensor.  sph_get_collider_impulses synchronises the context's stream and returns J of the LAST integrate (3 doubles per
 * sphere) and the number of integrates since tracking began; J / dt is the force on an obstacle.  It works for kinematic spheres
 * (mass 0) too.  On a context that is not tracked it returns *n = 0 and *steps = 0 (and SPH_OK).
 *
 * Free bodies.  After the step's force launch, once per step and on the device (the host never waits), sphere j with mass > 0
 * is updated in this order, per component a:
 *     u[a] = (float)(((double)u[a] + J_j[a] / (double)mass_j) + (double)dt * (double)accel_j[a])     float64, one rounding to fp32
 *     wall rule of the particles on (c[a], u[a]) with eps = R_j and the context's wall_damping:
 *         if c - R < box_min: c = box_min + R, u *= wall_damping ;  if c + R > box_max: c = box_max - R, u *= wall_damping
 *     c[a] = c[a] + dt * u[a]                                                                        fp32, as for a kinematic sphere
 * so the wall rule puts the centre into [box_min + R, box_max - R] and the advance that follows moves it by one step's
 * dt * u from there: a centre that has left that range by this much is put back by the next update.  A sphere with mass 0 keeps
 * the caller's velocity and only advances, by the same fp32 expression as on an untracked context.  Spheres do NOT collide with
 * each other, and a free body's push on the fluid is the kinematic rule above with its current velocity.
 *
 * sph_set_collider_bodies(n == number of colliders) starts tracking (or, on a tracked context, replaces the bodies and keeps the
 * centres, the velocities, J and the step count); n == 0 stops it and leaves the spheres kinematic where they are.  It writes none of the
 * context's step flags.  sph_set_colliders drops the bodies: the new set is kinematic and untracked, and a caller who never calls
 * sph_set_collider_bodies keeps the behaviour described above call for call, kernel for kernel.  sph_set_params on a tracked
 * context refreshes R + wall_eps on the device.  Device buffers (24 bytes per sphere and 64 particles of CAPACITY, plus one word
 * per 64 particles) are allocated when tracking is first switched on.
 *   SPH_E_STATE    a slab context: a rank's partial sums would need an all-reduce per step, and the N-slab = one-context bit
 *                  identity would not hold.  Out of scope.
 *   SPH_E_INVALID  n neither 0 nor the collider count; a mass that is negative or not finite; an accel that is not finite.
 * In every refused case nothing has changed.  Snapshots do not carry bodies, as they do not carry colliders. */
typedef struct sph_collider_body {
    float mass;       /* 0: kinematic (its velocity is the caller's; the default) ; > 0 and finite: a free body */
    float accel[3];   /* constant acceleration of a free body, e.g. (0, gravity_y, 0); ignored for mass 0 */
} sph_collider_body;
int sph_set_collider_bodies(sph_ctx* c, uint32_t n, const sph_collider_body* bodies);
/* *n spheres; J: 3 doubles per sphere (room for SPH_MAX_COLLIDERS; may be NULL); steps may be NULL.  Synchronises. */
int sph_get_collider_impulses(sph_ctx* c, uint32_t* n, double* J, uint64_t* steps);

/* ---- solid obstacles of any shape: a signed-distance grid the fluid collides with (no counterpart in the reference) --------------
 * A whole-domain context holds SPH_MAX_OBSTACLES obstacle slots (SEVERAL OBSTACLES below; a caller who never selects a slot
 * works with slot 0 alone, and everything up to that section describes one slot).  An OBSTACLE is a regular grid of signed distances phi (phi < 0 inside the solid), sampled
 * trilinearly, built on the device from analytic shapes (sph_obstacle_build) or uploaded by the caller (sph_obstacle_set_grid:
 * the door for voxelised meshes).  It is static, translates uniformly, or turns about a pivot (THE POSE below).  After EVERY integrate -- the fused one of sph_step and
 * sph_force_collide_integrate, and sph_integrate -- a pass of its own pushes the owned particles out of the solid; a context
 * without an obstacle launches and allocates exactly what a library without this section does.
 *
 * THE RULE (fp32, every operation rounded, no multiply-add fusion, sums left to right, IEEE division and square root;
 * tests/obstacle_model.py is the same arithmetic in numpy and gives every particle bit for bit: the pass reads the integrate's
 * STORED output, so there is neither a tolerance nor a tie).
 * GRID.  dims = (n_x, n_y, n_z), each 2..SPH_OBSTACLE_MAX_DIM, n_x*n_y*n_z <= SPH_OBSTACLE_MAX_NODES; origin finite; spacing
 * s > 0 and finite.  One float per node, x fastest: node (i, j, k) is phi[(k*n_y + j)*n_x + i] and sits at
 * origin + ((float)i*s, (float)j*s, (float)k*s).  On installation every phi is clamped to [-D, D], D = s * (float)(n_x + n_y +
 * n_z): no distance over the lattice exceeds D, and the clamp bounds the rounding error of the interpolation.  A phi that is
 * not finite is refused.
 * MOTION.  The grid has an offset `off` and a velocity `u`, both (0, 0, 0) by default: the field a particle at x sees is the
 * grid's at x - off.  After each step, once per step and on the host, off[k] = off[k] + dt * u[k] in fp32 -- where the spheres'
 * centres advance; a step without particles still moves it.  The motion belongs to the context: installing another grid keeps
 * it, sph_obstacle_clear resets it, and the offset only advances while a grid is installed.  The grid moves WITH the solid, and
 * a particle outside the grid is never in contact: build a moving obstacle with bounds that cover the box along its whole path.
 * SAMPLE at x.  Per axis k:  q = x[k] - off[k] ;  g = (q - origin[k]) / s.  If !(g >= 0) || !(g < (float)(n_k - 1)) on any axis
 * the point is OUTSIDE the grid: no contact (NaN and +-inf land here).  Else i_k = (int)g, f_k = g - (float)i_k, the eight nodes
 * are P_abc = phi at (i_x + a, i_y + b, i_z + c), and with lerp(p, q, t) = p + t * (q - p):
 *     phi = lerp( lerp( lerp(P000, P100, fx), lerp(P010, P110, fx), fy ),
 *                 lerp( lerp(P001, P101, fx), lerp(P011, P111, fx), fy ), fz )
 *     gx  = lerp( lerp(P100 - P000, P110 - P010, fy), lerp(P101 - P001, P111 - P011, fy), fz )
 *     gy  = lerp( lerp(P010 - P000, P110 - P100, fx), lerp(P011 - P001, P111 - P101, fx), fz )
 *     gz  = lerp( lerp(P001 - P000, P101 - P100, fx), lerp(P011 - P010, P111 - P110, fx), fy )
 * (the gradient in node units: no division by s)
 *     len2 = (gx*gx + gy*gy) + gz*gz ;  n = (gx, gy, gz) / sqrtf(len2) per component, or (0, 1, 0) unless len2 is finite and > 0
 * PUSH.  After the integration, the wall rule and the spheres (with their wall pass), for every owned particle (x, v), with
 * eps = wall_eps:
 *     hit = false
 *     repeat up to SPH_OBSTACLE_PUSH_ITERATIONS times:
 *         sample phi, n at x ;  if outside or !(phi < eps): stop
 *         wn = ((v.x - u.x)*n.x + (v.y - u.y)*n.y) + (v.z - u.z)*n.z
 *         if wn < 0:  k = (wall_damping - 1) * wn ;  v = v + k * n   (per component)
 *         t = eps - phi ;  x = x + t * n                              (per component) ;  hit = true
 *     if hit: the wall rule on x, y, z once more, as after the spheres
 * One iteration lands on phi = eps where phi is a true distance (|grad phi| = 1).  The interpolated field of a box has
 * |grad phi| between about 0.15 and 1.4 within half a spacing of its surface, near edges and corners (a float64 measurement):
 * hence four iterations.  GEOMETRY IS RESOLVED TO THE SPACING: the zero level of the interpolated field cuts a box's corners by
 * up to about 0.4 s, and an obstacle thinner than a particle's path in one step can be tunnelled through.
 * A particle with `hit` gets its new position and velocity, its row (x, y, z, 1) of the by-index position buffer and, in the
 * fused step, the next step's cell key and mover mark; a particle without is not written at all.  No floating-point atomic is
 * involved, and the pass touches none of the context's step flags.
 * SHAPES (sph_obstacle_build): the union of 1..SPH_MAX_SHAPES shapes, one node per thread, p the node's position:
 *     SPH_SHAPE_SPHERE     centre a, radius r > 0:   d = p - a ;  phi = sqrtf((d.x*d.x + d.y*d.y) + d.z*d.z) - r
 *     SPH_SHAPE_BOX        centre a, half extents b > 0, rounding r >= 0 (axis-aligned):
 *                          q[k] = fabsf(p[k] - a[k]) - b[k] ;  o[k] = fmaxf(q[k], 0)
 *                          phi = (sqrtf((o.x*o.x + o.y*o.y) + o.z*o.z) + fminf(fmaxf(q.x, fmaxf(q.y, q.z)), 0)) - r
 *     SPH_SHAPE_CAPSULE    ends a != b, radius r > 0:   pa = p - a ;  ba = b - a
 *                          t = ((pa.x*ba.x + pa.y*ba.y) + pa.z*ba.z) / ((ba.x*ba.x + ba.y*ba.y) + ba.z*ba.z)
 *                          t = fminf(fmaxf(t, 0), 1) ;  d = pa - t*ba ;  phi = sqrtf((d.x*d.x + d.y*d.y) + d.z*d.z) - r
 *                          (ends so close that ba.ba is not a positive finite fp32 count as equal)
 *     SPH_SHAPE_HALFSPACE  point a, normal b: finite and non-zero, normalised on the host in double, each component rounded once
 *                          phi = ((p.x-a.x)*b.x + (p.y-a.y)*b.y) + (p.z-a.z)*b.z
 *                          (solid on the side the normal points AWAY from, as SPH_REGION_HALFSPACE)
 * invert != 0 negates the shape's phi (fluid inside a bowl is an inverted sphere); the union is fminf over the shapes in order;
 * then the clamp to [-D, D].
 * THE LATTICE OF A BUILD (sph_obstacle_lattice; in double on the host, each result rounded once): s = spacing, 0 meaning
 * 2 * particle_radius; bounds [lo, hi] the caller's, or the box where the pointer is NULL:
 *     n_k = ceil((hi_k - lo_k) / s) + 3 ;  origin_k = lo_k - s  (fp32)
 * Beyond the limits: SPH_E_CAPACITY.  The bounds let a fine grid sit around a pillar in a large box (the standard box of edge
 * 32 at s = 1/16 would exceed SPH_OBSTACLE_MAX_NODES).  Particles outside the grid are never in contact.
 *
 * All calls are legal at any stage of a step, like sph_set_colliders, and every later integrate uses the new state.
 *   SPH_E_STATE     a slab context (every call that would install a grid or a motion): the slab step makes up to three force
 *                   launches with holes and ghosts that arrive integrated.  Out of scope, as for render, mesh, emitters, bodies.
 *                   Also sph_obstacle_read / _sample without an obstacle.
 *   SPH_E_INVALID   what THE RULE excludes: dims, origin, spacing, a phi that is not finite, a shape count outside
 *                   1..SPH_MAX_SHAPES, an unknown kind, a field its kind uses that is not finite or out of range, bounds with
 *                   hi < lo or not finite, a motion that is not finite;
 *   SPH_E_CAPACITY  a lattice beyond SPH_OBSTACLE_MAX_DIM / SPH_OBSTACLE_MAX_NODES.
 * In every refused case nothing has changed and nothing was allocated.  SPH_E_NOMEM releases everything the call allocated and
 * leaves the context with NO obstacle.  Device buffers: 4 bytes per node and 4 per brick of 4 x 4 x 4 cells, freed by
 * sph_obstacle_clear and sph_destroy.  Installing over an obstacle waits for the context's stream first.  sph_set_params needs
 * no refresh (eps is read at every launch).  Snapshots do not carry obstacles, as they do not carry colliders. */
#define SPH_OBSTACLE_MAX_DIM 2048
#define SPH_OBSTACLE_MAX_NODES (1u << 27)
#define SPH_OBSTACLE_PUSH_ITERATIONS 4
#define SPH_MAX_SHAPES 16
enum { SPH_SHAPE_SPHERE = 0, SPH_SHAPE_BOX = 1, SPH_SHAPE_CAPSULE = 2, SPH_SHAPE_HALFSPACE = 3 };
typedef struct sph_shape { int32_t kind; int32_t invert; float a[3]; float b[3]; float r; } sph_shape;   /* 36 bytes */
typedef struct sph_obstacle_grid { uint32_t dims[3]; float origin[3]; float spacing; } sph_obstacle_grid;
/* Host helper: the lattice sph_obstacle_build would use (lo, hi: both NULL = the context's box).  *out untouched on error. */
int sph_obstacle_lattice(const sph_ctx* c, float spacing, const float lo[3], const float hi[3], sph_obstacle_grid* out);
/* Rasterise the union of n shapes on that lattice and install it: kernels on the context's stream, no host wait (unless it
 * replaces an obstacle). */
int sph_obstacle_build(sph_ctx* c, float spacing, const float lo[3], const float hi[3], uint32_t n, const sph_shape* shapes);
/* Install the caller's field (a host array of dims[0]*dims[1]*dims[2] floats, left untouched).  Copies: synchronises. */
int sph_obstacle_set_grid(sph_ctx* c, const sph_obstacle_grid* grid, const float* phi);
/* Remove the obstacle, free its buffers, motion back to 0 (waits for the stream if there was one).  Without one: SPH_OK. */
int sph_obstacle_clear(sph_ctx* c);
/* Offset and velocity of the grid; either may be NULL = keep. */
int sph_obstacle_set_motion(sph_ctx* c, const float offset[3], const float velocity[3]);
/* The installed grid (dims 0, 0, 0 = none) and the ADVANCED offset; any pointer may be NULL. */
int sph_obstacle_get(const sph_ctx* c, sph_obstacle_grid* grid, float offset[3], float velocity[3]);
/* The installed (clamped) field to the host.  Synchronises. */
int sph_obstacle_read(sph_ctx* c, float* phi);
/* SAMPLE on the device for n caller points (xyz triples) with the current offset: "how far is this point from the solid".
 * Outside the grid: phi = +inf, normal (0, 0, 0), inside_grid 0.  Any output may be NULL.  Synchronises. */
int sph_obstacle_sample(sph_ctx* c, uint32_t n, const float* pos_xyz, float* phi, float* normal_xyz, uint8_t* inside_grid);

/* ---- obstacles that turn, and the load the fluid puts on them ---------------------------------------------------------------------
 * THE POSE (sph_obstacle_set_pose; NULL = no pose: translation only, the rule above bit for bit).  The grid's own coordinates
 * are the BODY frame.  pivot is a point of the body frame, quat = (w, x, y, z) rotates body to world about it, omega is the
 * angular velocity in world axes, radians per unit of time.  off and u of sph_obstacle_set_motion keep their meaning, and the
 * pivot's place in the world is P[k] = pivot[k] + off[k], fp32, computed once per launch on the host.  The pose belongs to the
 * context like the motion: installing another grid keeps it, sph_obstacle_clear resets it to no pose, and it advances only while
 * a grid is installed.
 * Host state, float64, no contraction, only + - * / sqrt (tests/obstacle_pose_model.py repeats it exactly; no sin or cos):
 *     on set:          q = (double)quat / sqrt(((w*w + x*x) + y*y) + z*z)
 *     after each step, where the offset advances, with a[k] = (0.5 * (double)dt) * (double)omega[k]:
 *         w' = ((w - a0*x) - a1*y) - a2*z      x' = ((x + a0*w) + a1*z) - a2*y
 *         y' = ((y + a1*w) + a2*x) - a0*z      z' = ((z + a2*w) + a0*y) - a1*x
 *         q  = q' / sqrt(((w'*w' + x'*x') + y'*y') + z'*z')
 * This is the Cayley step: the angle per step is 2 atan(|omega| dt / 2), not |omega| dt -- at omega dt = 2e-3 it falls short by
 * a relative 3.3e-7.  A caller who wants an exact angle sets the pose itself every step.
 *     rot (row-major, body -> world; each entry computed in float64 as written, then rounded once to fp32):
 *         R00 = 1 - 2*(y*y + z*z)    R01 = 2*(x*y - w*z)        R02 = 2*(x*z + w*y)
 *         R10 = 2*(x*y + w*z)        R11 = 1 - 2*(x*x + z*z)    R12 = 2*(y*z - w*x)
 *         R20 = 2*(x*z - w*y)        R21 = 2*(y*z + w*x)        R22 = 1 - 2*(x*x + y*y)
 * Device rule of a posed context (fp32, each operation rounded, no fusion, sums left to right, as THE RULE).  SAMPLE at x:
 *     d[k] = x[k] - P[k]
 *     q[k] = ((R[0][k]*d[0] + R[1][k]*d[1]) + R[2][k]*d[2]) + pivot[k]
 *     g[k] = (q[k] - origin[k]) / s
 * then the inside test, the gather, phi and the normal nb of SAMPLE above (the body normal); the world normal, NOT renormalised:
 *     n[k] = (R[k][0]*nb[0] + R[k][1]*nb[1]) + R[k][2]*nb[2]
 * PUSH: the solid's velocity at the particle is us = u + omega x d,
 *     us[0] = u[0] + (omega[1]*d[2] - omega[2]*d[1])   us[1] = u[1] + (omega[2]*d[0] - omega[0]*d[2])
 *     us[2] = u[2] + (omega[0]*d[1] - omega[1]*d[0])
 *     wn = ((v.x - us[0])*n.x + (v.y - us[1])*n.y) + (v.z - us[2])*n.z
 * and everything after that is PUSH above: the kick, t = eps - phi, x = x + t*n, up to SPH_OBSTACLE_PUSH_ITERATIONS times (d is
 * recomputed from the moved x in every iteration), the wall rule.  sph_obstacle_sample on a posed context samples at world points
 * and returns the world normal by the same arithmetic.  A posed context with the identity quaternion uses the posed arithmetic;
 * its bits need not equal an unposed context's.
 *
 * THE LOAD (sph_obstacle_set_sensor, sph_obstacle_get_load).  While the sensor is on, in every obstacle push a particle whose
 * iteration takes the branch `wn < 0` adds k*n to its velocity as before -- no particle bit changes -- and also forms
 *     t[a] = -(mass * (k * n[a]))                                   fp32 products, each rounded, as the spheres' term
 *     tau[0] = (double)d[1]*(double)t[2] - (double)d[2]*(double)t[1]   and cyclic (exact products, one rounding)
 * with the fp32 d of that iteration; on an unposed context pivot = (0, 0, 0), so d = x - off and P = off.  J is the sum of t and
 * L the sum of tau over the owned particles, float64 from 0.0 in a fixed order: a lane adds its iterations in order; a wave adds
 * its kicked lanes in ascending order; the waves are added as the tracked spheres' are (256 runs of K = ceil(waves / 256) rounded
 * up to a multiple of 4 waves, ascending within a run, then the runs that hold a row in ascending order).  No floating-point
 * atomic is involved.  J is the momentum and L the angular momentum about `about` (the P of that push) the solid took in the
 * LAST integrate: J / dt is the force, L / dt the torque.  The position projection and the wall pass are not part of it.  `steps`
 * counts the integrates with a grid installed while the sensor was on; a step without particles counts and reads zeros.
 * A caller who reads the load and sets the pose each step drives a wheel by the fluid.
 * The sensor without an obstacle is legal and reads zeros; sph_obstacle_clear keeps the switch and zeroes the load and `steps`.
 * While the switch is off nothing is summed: J, L, `about` and `steps` stay what the last sensing integrate left, and switching
 * the sensor on again or installing another grid over the installed one keeps them too (`steps` goes on counting from there).
 * Device buffers (48 + 4 bytes per 64 particles of CAPACITY, and 72 bytes) are allocated when the sensor is first switched on
 * and freed by sph_destroy.  A context that calls none of the four launches and allocates exactly what it did before.
 *   SPH_E_STATE    a slab context (all four but sph_obstacle_get_pose).
 *   SPH_E_INVALID  a pivot, quaternion or omega that is not finite; a quaternion whose squared norm in double is 0 or not finite.
 * In every refused case nothing has changed and nothing was allocated.  The calls are legal at any stage and write none of the
 * context's step flags.  Out of scope: slab contexts, snapshots carrying the pose (free rigid bodies: THE BODY below). */
typedef struct sph_obstacle_pose { float pivot[3]; float quat[4]; float omega[3]; } sph_obstacle_pose;
int sph_obstacle_set_pose(sph_ctx* c, const sph_obstacle_pose* pose);
/* The ADVANCED pose: *posed 0 = none (then pivot, omega 0 and the identity); rot as the next launch takes it.  Any pointer may be NULL.
 * get -> set is NOT the identity: quat is the float64 state, sph_obstacle_pose.quat is float32 and sph_obstacle_set_pose normalises
 * again, so an advanced pose cannot be handed to another context bit for bit (a pose that was set and has not advanced can: by
 * the arguments of its set). */
int sph_obstacle_get_pose(const sph_ctx* c, int* posed, float pivot[3], double quat[4], float omega[3], float rot[9]);
int sph_obstacle_set_sensor(sph_ctx* c, int on);
/* J, L, about and steps of the last integrate; any pointer may be NULL.  Synchronises. */
int sph_obstacle_get_load(sph_ctx* c, double J[3], double L[3], float about[3], uint64_t* steps);

/* ---- free obstacle bodies: the fluid drives a slot's motion, on the device -----------------------------------------------------------
 * THE BODY (sph_obstacle_set_body; NULL = no body).  A slot with a body has a mass, moments of inertia and a choice `dof` of the
 * motions the fluid drives: its offset along the FREE axes, its spin about the pivot (SPIN: a free top; HINGE: about one fixed
 * world axis through the pivot).  While the body is set the slot's state -- off, u, pivot, omega (fp32), quat (float64) and the
 * derived rot[9] and P[3] of THE POSE -- lives in a block on the device.  The push, sph_obstacle_sample and the solids' march of
 * sph_render / sph_render_surface read off, u, rot, P, pivot and omega from it at kernel entry and are otherwise the posed,
 * sensing arithmetic above, operation for operation; the load's `about` is the block's P.  So a water wheel, a valve flap, a
 * float or a paddle on a rail runs inside sph_step(dt, n) and in the pictures with no host wait.
 * THE BODY STEP runs once per integrate of an installed body slot, behind that slot's load sum (also without particles: the load
 * is then zero).  Float64, no contraction, only + - * / sqrt, every product and sum rounded, sums left to right
 * (tests/obstacle_body_model.py repeats it exactly).  Its inputs are J and L as just summed, and dt:
 *     per axis a = 0, 1, 2:
 *         if FREE_a:  u[a] = (float)(((double)u[a] + J[a] / (double)mass) + (double)dt * (double)accel[a])
 *                     the wall rule of the particles on (off[a], u[a]) with lo[a], hi[a], eps = 0 and wall_damping      (fp32)
 *         off[a] = off[a] + dt * u[a]                                                   (fp32, as a kinematic slot)
 *     T[k] = L[k] + (double)dt * (double)torque[k]
 *     HINGE (e = axis / |axis| in double, w = (double)omega):
 *         s = ((w0*e0 + w1*e1) + w2*e2) + ((T0*e0 + T1*e1) + T2*e2) / (double)inertia[0]
 *         omega[k] = (float)(s * e[k])
 *     SPIN (Rd = the nine float64 expressions of rot BEFORE their rounding, from the current quat; I = (double)inertia):
 *         wb[k] = (Rd[0][k]*w0 + Rd[1][k]*w1) + Rd[2][k]*w2              Tb likewise from T
 *         h[k] = I[k] * wb[k]
 *         g = wb x h,  g[0] = wb1*h2 - wb2*h1 and cyclic
 *         wb'[k] = wb[k] + (Tb[k] - (double)dt * g[k]) / I[k]
 *         omega[k] = (float)((Rd[k][0]*wb'0 + Rd[k][1]*wb'1) + Rd[k][2]*wb'2)
 *     the Cayley step of THE POSE with the new fp32 omega; rot, each entry rounded once; P = pivot + off.
 * With dof = 0 this is the kinematic slot's advance moved to the device: particles, load and pose equal a kinematic, posed,
 * sensing slot bit for bit.  L is taken about the P of that push, so THE CALLER places the pivot at the centre of mass (SPIN)
 * or on the axis (HINGE); gravity (accel) exerts no torque.  lo and hi bound the slot's OFFSET, not its shape.
 * A body needs a pose (the identity quaternion will do) and switches the slot's sensor on, allocating its buffers as
 * sph_obstacle_set_sensor does, and -- at the slot's first body -- the block (128 bytes); sph_destroy frees both.  While a body
 * is set the host's copies are stale: sph_obstacle_get, _get_pose and _sample on that slot synchronise and read the block;
 * sph_obstacle_set_motion and _set_pose write it with a one-wave kernel whose values travel by value (no host wait), and take
 * effect at the next integrate.  sph_obstacle_set_body on a slot that has a body replaces the parameters and keeps the state.
 * sph_obstacle_set_body(NULL) synchronises, and the slot goes on kinematic from where it is (posed, sensing).
 * sph_obstacle_clear drops the body as it resets the pose; installing another grid keeps it; it advances only while a grid is
 * installed; snapshots do not carry it.  Both calls address the selected slot, are legal at any stage and write no step flag.
 *   SPH_E_STATE    a slab context; sph_obstacle_set_body on a slot without a pose; sph_obstacle_set_sensor(0) or
 *                  sph_obstacle_set_pose(NULL) on a slot that has a body.
 *   SPH_E_INVALID  a dof with unknown bits or with SPIN and HINGE; a mass that is not finite and > 0 with a FREE bit; a moment
 *                  (SPIN: all three, HINGE: inertia[0]) that is not finite and > 0; a HINGE axis that is not finite or is zero;
 *                  accel or torque not finite; lo or hi of a FREE axis not finite, or lo > hi.
 * In every refused case nothing has changed and nothing was allocated.  Out of scope: bodies colliding with each other or with
 * the box by their shape, gravity torque, slab contexts, snapshots. */
enum { SPH_BODY_FREE_X = 1, SPH_BODY_FREE_Y = 2, SPH_BODY_FREE_Z = 4, SPH_BODY_SPIN = 8, SPH_BODY_HINGE = 16 };
typedef struct sph_obstacle_body {
    uint32_t dof;       /* which motions the fluid drives; SPIN and HINGE exclude each other; 0 is legal (kinematic, on the device) */
    float mass;         /* > 0, finite, if any FREE bit */
    float inertia[3];   /* SPIN: principal moments about the pivot along the BODY axes, each > 0; HINGE: inertia[0] about the axis */
    float axis[3];      /* HINGE: a fixed world axis through the pivot, finite and non-zero; normalised on the host in double */
    float accel[3];     /* world; acts on the FREE axes (gravity) */
    float torque[3];    /* world; a constant external torque (a brake, a motor); HINGE uses its component along the axis */
    float lo[3], hi[3]; /* bounds of the slot's OFFSET on the FREE axes, lo <= hi: the wall rule with eps = 0 */
} sph_obstacle_body;
int sph_obstacle_set_body(sph_ctx* c, const sph_obstacle_body* body);
/* *has_body 0 = none (then *out is zeros); the parameters as they were set.  Either pointer may be NULL. */
int sph_obstacle_get_body(const sph_ctx* c, int* has_body, sph_obstacle_body* out);

/* ---- several obstacles per context: a vessel and a wheel, one push pass ------------------------------------------------------------
 * A whole-domain context holds SPH_MAX_OBSTACLES obstacle SLOTS.  Each slot is what "the obstacle" is in the sections around
 * this one: its grid and brick minima, offset and velocity, pose, sensor switch, sensor buffers and load, and the scratch and
 * stats of a mesh build.  sph_obstacle_select chooses the slot that EVERY sph_obstacle_* call addresses from then on (build,
 * set_grid, the three mesh builds, clear, set_motion, get, read, sample, set_pose, get_pose, set_sensor, get_load, mesh_stats,
 * lattice); the default is slot 0, so a caller who never selects sees a library of one obstacle call for call.
 * THE RULE.  After every integrate the INSTALLED slots act on each owned particle in ASCENDING SLOT ORDER: slot j applies PUSH --
 * posed or not, as that slot is -- to what slot j - 1 left, with its own off, u, P, rot, omega, its own guard eps + 0.25 s_j and
 * its own "wall rule once more if hit".  Each rule is unchanged to the bit: the pass equals tests/obstacle_model.py /
 * tests/obstacle_pose_model.py applied one after the other (tests/obstacle_set_model.py).  A particle no slot hit is not written;
 * one that some slot hit gets its final position and velocity, its by-index row and, in the fused step, the next key and mover
 * mark, all from the final position.  Where solids overlap the order decides, as for the spheres.  THE LOAD is per slot: the
 * terms of that slot's iterations with that slot's d, summed in the order given above; `about` and `steps` are per slot too.
 * Offsets and poses advance per slot where one slot's advance today, and only while that slot holds a grid.
 * ONE PASS.  While slot 0 is the only installed slot the library launches the kernels of one obstacle with their arguments.
 * Every other set is one launch that reads each position once and walks the installed slots in order (sph_obstacle.hip:
 * k_obstacle_push_set), followed by one load sum per sensing slot.
 * Installing into or clearing a slot waits for the stream only if THAT slot holds a grid, and leaves the other slots alone.  A
 * slot's sensor buffers are allocated when that slot's sensor is first switched on; sph_destroy frees them.  None of the four
 * calls below writes a step flag: they are legal at any stage of a step.
 *   SPH_E_INVALID  sph_obstacle_select with slot >= SPH_MAX_OBSTACLES;   SPH_E_STATE  a slab context (select, clear_all).
 * In both cases nothing has changed and nothing was allocated. */
#define SPH_MAX_OBSTACLES 4
int sph_obstacle_select(sph_ctx* c, uint32_t slot);
/* The selected slot (0 for a NULL or a slab context). */
uint32_t sph_obstacle_selected(const sph_ctx* c);
/* The number of slots that hold a grid; *mask (may be NULL): bit k = slot k. */
uint32_t sph_obstacle_installed(const sph_ctx* c, uint32_t* mask);
/* sph_obstacle_clear on every slot, and the selection back to 0. */
int sph_obstacle_clear_all(sph_ctx* c);

/* ---- obstacles from a triangle mesh: the mesh voxelised on the device into the grid above ----------------------------------------
 * sph_obstacle_build_mesh turns a closed triangle mesh -- host arrays, device arrays (sph_mesh_dev's pointers feed it with no host
 * trip) or a Wavefront OBJ file -- into a TRUNCATED signed distance on the lattice of sph_obstacle_build and installs it like any
 * other grid: the push, the motion, _get, _read, _sample and _clear do not know the difference.  A context that never calls these
 * allocates and launches what it did before.
 *
 * THE RULE (the conventions of THE RULE above: fp32, every operation rounded, no multiply-add fusion, sums left to right, IEEE
 * division and square root; tests/mesh_obstacle_model.py is the same arithmetic in numpy and gives every node bit for bit).
 * The lattice is that of sph_obstacle_build for the same spacing, lo, hi: node i of axis k sits at X = origin_k + (float)i * s.
 * Input: n_vertices xyz triples, n_triangles uint32 triples; band in nodes, 1..SPH_OBSTACLE_MESH_MAX_BAND, 0 meaning
 * SPH_OBSTACLE_MESH_DEFAULT_BAND; invert.  W = (float)band * s.  The result is phi = +-min(sqrtf(d2), W), negative inside;
 * invert != 0 then negates it; last the clamp to [-D, D] of every installation.
 * UNSIGNED PART.  A triangle (A, B, C) with the per-axis minimum lo_k and maximum hi_k of its vertices offers a candidate to
 * every node of the index box
 *     i_k in [ max(0, floorf(((lo_k - W) - origin_k) / s)),  min(n_k - 1, ceilf(((hi_k + W) - origin_k) / s)) ]
 * (the float is clamped to [0, n_k - 1] before it becomes an integer; the box is part of the rule).  The candidate at node P is
 * the minimum (fminf) of seg(A, B), seg(B, C), seg(C, A) and, where it applies, the plane term:
 *     seg(a, b):  pa = P - a ;  ba = b - a ;  t = ((pa.x*ba.x + pa.y*ba.y) + pa.z*ba.z) / ((ba.x*ba.x + ba.y*ba.y) + ba.z*ba.z)
 *                 t = fminf(fmaxf(t, 0), 1), or 0 unless ba.ba is a positive finite number
 *                 d = pa - t*ba ;  seg = (d.x*d.x + d.y*d.y) + d.z*d.z                  (the capsule's arithmetic without r)
 *     plane:      n = cross(B - A, C - A), cross(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x)
 *                 nn = (n.x*n.x + n.y*n.y) + n.z*n.z must be finite and > 0, and for (a, b) = (A, B), (B, C), (C, A):
 *                 c = cross(b - a, n) ;  (((P-a).x*c.x + (P-a).y*c.y) + (P-a).z*c.z) <= 0       (the projection is inside)
 *                 h = ((P-A).x*n.x + (P-A).y*n.y) + (P-A).z*n.z ;  the term is (h*h) / nn
 * d2 of a node is the minimum over all triangles that offer to it, +inf without any: one unsigned 32-bit atomic min on the bits
 * of a non-negative float, which does not depend on the order of arrival.
 * SIGN.  The parity of the mesh crossings on the ray from the node towards -x.  A triangle tests the columns (j, k) of the index
 * box of its y and z extents (the formula above without W, axes 1 and 2).  With q = (Y_j, Z_k), each of its three edges counts
 * once if, (lo, hi) being its two ends in canonical order (smaller z first, on equal z smaller y first: independent of the
 * winding),
 *     lo.z <= q.z && !(hi.z <= q.z)   and   (hi.y - lo.y)*(q.z - lo.z) - (hi.z - lo.z)*(q.y - lo.y) > 0
 * An odd count means the column crosses the triangle, at
 *     xc = A.x + ((n.y*(A.y - q.y)) + n.z*(A.z - q.z)) / n.x ;  g = (xc - origin_x) / s
 * A crossing whose g is not finite is LOST: it marks nothing and is counted.  Otherwise the triangle flips the parity bit of
 * mark i0 = g <= 0 ? 0 : (g > (float)(n_x - 1) ? n_x : (uint)ceilf(g)) of the column; a column has n_x + 1 marks, the last one
 * for crossings beyond the lattice.  Node i is inside iff the XOR of the marks 0..i of its column is 1; a column is ODD if the
 * XOR of all its marks is 1.  Both triangles that share an edge compute the edge's test from the same bits, so every column of a
 * closed mesh has an even total, whatever the rounding and the winding: odd columns mean an open mesh or lost crossings, and
 * they are counted, not guessed at.  One integer atomic XOR per mark: two builds of one mesh give the same bits, and so do two
 * builds with the triangles in another order.  No floating-point atomic.
 * A triangle with an index >= n_vertices or a vertex that is not finite is SKIPPED on the device and counted (the host form has
 * refused such input before; the device form cannot look).
 * LIMITS.  Deeper than W inside the solid the field is flat at -W, where the push's normal falls back to (0, 1, 0): band >= 2 is
 * needed for a correct trilinear gradient next to the surface.  That the mesh is closed is the CALLER's duty, and
 * sph_obstacle_mesh_stats is the sensor.  Geometry is resolved to the spacing, as for the analytic shapes.
 *
 * Errors as in the section above: SPH_E_STATE on a slab context; SPH_E_INVALID for a band beyond the maximum, a null argument,
 * no vertex or no triangle, bad bounds or spacing, and (host and OBJ forms) a vertex that is not finite, an index >= n_vertices,
 * a file that cannot be read or holds no face; SPH_E_CAPACITY from the lattice limits or more than
 * SPH_OBSTACLE_MESH_MAX_TRIANGLES triangles: all of them with nothing changed and nothing allocated.  SPH_E_NOMEM leaves the
 * context with NO obstacle and every byte released.  Scratch of a build, kept until the next installation, sph_obstacle_clear
 * or sph_destroy: 4 bytes per triangle plus 16 per 256 triangles, and one bit per node and column end (n_x + 1 bits per column,
 * rounded up to words).  The calls touch none of the context's step flags. */
#define SPH_OBSTACLE_MESH_MAX_BAND 16
#define SPH_OBSTACLE_MESH_DEFAULT_BAND 3
#define SPH_OBSTACLE_MESH_MAX_TRIANGLES (1u << 28)
typedef struct sph_obstacle_mesh_params { float spacing; uint32_t band; int32_t invert; } sph_obstacle_mesh_params;   /* all 0 = defaults */
/* Host arrays (left untouched): validates, copies to temporaries, voxelises and synchronises.  params NULL = defaults. */
int sph_obstacle_build_mesh(sph_ctx* c, const sph_obstacle_mesh_params* params, const float lo[3], const float hi[3],
                            uint32_t n_vertices, const float* pos_xyz, uint32_t n_triangles, const uint32_t* tri);
/* Device arrays on the context's GPU, read on the context's stream (sph_mesh_dev's pointers are valid arguments): kernels on that
 * stream, no host wait (unless it replaces an obstacle).  The arrays must stay valid until the stream has run the build. */
int sph_obstacle_build_mesh_dev(sph_ctx* c, const sph_obstacle_mesh_params* params, const float lo[3], const float hi[3],
                                uint32_t n_vertices, const void* pos_dev, uint32_t n_triangles, const void* tri_dev);
/* A Wavefront OBJ file: `v x y z` and `f` lines (entries a, a/b, a//c or a/b/c; negative indices are relative; polygons are
 * fanned from their first vertex), everything else ignored.  sph_mesh_save_obj writes %.9g: a saved mesh comes back bit for bit. */
int sph_obstacle_build_obj(sph_ctx* c, const sph_obstacle_mesh_params* params, const float lo[3], const float hi[3], const char* path);
/* [introspect] of the mesh-built obstacle: triangles used, triangles skipped, lost crossings, odd columns.  SPH_E_STATE unless the
 * installed obstacle came from a mesh.  Synchronises. */
int sph_obstacle_mesh_stats(sph_ctx* c, uint64_t out[4]);

/* ---- emitters and drains: particles enter and leave a running simulation (no counterpart in the reference, whose particle
 *      set is fixed at construction; sph_set_by_index, its addSphere, only rewrites particles that exist) -----------------------
 * Whole-domain contexts only: on a slab context all three calls return SPH_E_STATE (the slab step sizes its messages from the
 * previous step's counts, and the ranks would have to agree on who owns a new particle); the reference seam has none.
 *
 * A REGION selects particles by position x (fp32, every operation rounded, no multiply-add fusion, sums left to right:
 * tests/region_model.py is the same arithmetic in numpy and decides every particle identically):
 *   SPH_REGION_SPHERE     centre a, radius r:      d = x - a;  d.x*d.x + d.y*d.y + d.z*d.z < r*r                 (strict)
 *   SPH_REGION_BOX        corners a, b:            a[k] <= x[k] && x[k] < b[k] on all three axes  (half open: boxes that share
 *                                                  a face partition space)
 *   SPH_REGION_HALFSPACE  point a, normal b:       (x[0]-a[0])*b[0] + (x[1]-a[1])*b[1] + (x[2]-a[2])*b[2] < 0     (strict: the
 *                                                  side the normal points AWAY from)
 * A call takes 1..SPH_MAX_REGIONS regions and selects a particle that lies in ANY of them.  A kind outside the enum, or a
 * field its kind uses (sphere: a, r; box and half-space: a, b) that is not finite: SPH_E_INVALID. */
#define SPH_MAX_REGIONS 8
enum { SPH_REGION_SPHERE = 0, SPH_REGION_BOX = 1, SPH_REGION_HALFSPACE = 2 };
typedef struct sph_region {
    int32_t kind;
    float a[3];
    float b[3];
    float r;
} sph_region;   /* 32 bytes */
/* Append n particles (xyz triples; vel_xyz NULL = at rest) behind the owned ones.  index[i] is the creation index of particle
 * i; that no two live particles share an index is the CALLER's duty, as in sph_upload.  index = NULL hands out consecutive
 * indices from the context's next unused one -- one past the highest index uploaded, generated (sph_reset_lattice), loaded
 * (sph_snapshot_load) or emitted so far; sph_upload and sph_reset_lattice start it again from the set they install.  The first
 * index goes to *first_index_out (may be NULL).  The by-index position buffer (sph_positions_dev) shows (x, y, z, 1) at once.
 *   SPH_E_CAPACITY  n + sph_num_particles > capacity, or (index = NULL) an index would reach the capacity, which is the size
 *                   of the by-index buffers: a long faucet-plus-drain run passes the indices sph_remove returned;
 *   SPH_E_INVALID   a position that is not finite or outside [box_min, box_max], a velocity that is not finite, an explicit
 *                   index >= capacity.
 * On any error nothing has changed.  The new particles sit behind the sorted range, so the NEXT sort is the full stable sort
 * (not the merge): within a cell the residents come first, the emitted particles behind them in call order -- the order an
 * sph_upload of the same particles in the same sequence gives, bit for bit.  Copies from host memory: synchronises. */
int sph_emit(sph_ctx* c, uint32_t n, const float* pos_xyz, const float* vel_xyz, const uint32_t* index,
             uint32_t* first_index_out);
/* Delete the owned particles the regions select.  The survivors keep their relative slot order (a stable compaction on the
 * device), so the range stays in the order of the last sort and the next sort may take the merge path.  *n_removed (may be
 * NULL) is the number deleted; removed_index (may be NULL) receives the creation indices of the first min(n_removed, max_out)
 * of them in slot order; the row of each removed particle in the by-index position buffer becomes (0, 0, 0, 0), what
 * sph_upload writes for an index without a particle.  Densities and forces of the current step are dropped: until the next
 * step sph_download gives density and pressure 0 for every survivor (as for an emitted particle), and that step starts with
 * sph_hash, as after sph_set_by_index.  With nothing selected the context is left exactly as it was -- the next
 * step does what it would have done without the call.  Returns data to the host: synchronises. */
int sph_remove(sph_ctx* c, uint32_t n_regions, const sph_region* regions, uint32_t* n_removed, uint32_t* removed_index,
               uint32_t max_out);
/* The same selection without the removal -- a sensor: a fill level, "is the nozzle clear".  Changes nothing; synchronises. */
int sph_count_in_regions(sph_ctx* c, uint32_t n_regions, const sph_region* regions, uint32_t* count);

/* ---- pictures: the fluid rendered on the device as depth-tested sphere sprites ----------------------------------------------------
 * The reference hands its positions to an OpenGL point-sprite renderer (SPH/render_particles.cpp, SPH/shaders.cpp).  Here the
 * same look -- point sprites shaded as spheres, the rainbow ramp -- is a software pass on the device over the sorted positions:
 * no GL context, no copy of the state to the host.  Whole-domain contexts only.  A caller who never renders gets the launches
 * and the allocations of a library without this section.
 *
 * THE RULE (fp32, every operation rounded, no multiply-add fusion, sums left to right, IEEE division and square root;
 * tests/render_model.py is the same arithmetic in numpy and gives the same id and depth images bit for bit).
 * Eye space has +x right, +y up and +z FORWARD.  For a particle at (x, y, z), k = 0, 1, 2:
 *     pe[k] = ((rot[3k]*x + rot[3k+1]*y) + rot[3k+2]*z) + trans[k] ;  d = pe[2]
 * A particle with d < near_z or d > far_z draws nothing.  Its sprite, with R the style's radius:
 *     rp = (R * focal_px) / d ;  rp = min(rp, SPH_RENDER_MAX_RADIUS_PX) ;  rp = max(rp, 0.75f)
 *     cx = 0.5f*width + (focal_px*pe[0]) / d ;  cy = 0.5f*height - (focal_px*pe[1]) / d
 * (the floor of 0.75 px makes every visible particle cover at least one pixel centre).  Pixel (i, j), column i, row j, row 0
 * on top:
 *     u = ((i + 0.5f) - cx) / rp ;  v = ((j + 0.5f) - cy) / rp ;  mag = u*u + v*v ;  covered iff mag <= 1
 * (the reference's `if (mag > 1.0) discard`).  The fragment's depth is d, flat per sprite, as a point sprite's is.  Per pixel
 * the winner is the smallest d, among equal d the lowest SLOT (the particle's place in the owned range: the order of
 * sph_download_owned and sph_get_order).  Shading of the winner:
 *     nx = u ; ny = -v ; nz = sqrtf(1 - mag) ;  diffuse = max(0, (0.577f*nx + 0.577f*ny) + 0.577f*nz)
 *     channel8 = (uint8)(min(c*diffuse, 1.0f)*255.0f + 0.5f) ;  alpha = 255
 * with the colour c from the seven-colour ramp red, orange (1, 0.5, 0), yellow, green, cyan, blue, magenta:
 *     t clamped to [0, 1] ;  s = t*6 ;  i = min((int)s, 5) ;  f = s - (float)i ;  c = a + f*(b - a) per channel (a, b: colours i, i+1)
 *     SPH_COLOR_INDEX    t = (float)index / (float)index_count               (the reference's colouring)
 *     SPH_COLOR_SPEED    t = (|v| - lo) / (hi - lo),  |v| = sqrtf((vx*vx + vy*vy) + vz*vz)
 *     SPH_COLOR_DENSITY  t = (rho - lo) / (hi - lo),  rho of the last density pass: what sph_download reports (0 after an
 *                        upload, an emission or a removal)
 * A background pixel holds the style's background colour, id 0xFFFFFFFF and depth +inf.
 * How: every pixel has a 64-bit key (bits of d) << 32 | slot; d is a positive fp32, so its bits order as the float does, and one
 * 64-bit unsigned atomic min per fragment decides the pixel -- min does not depend on arrival order, so two renders of one
 * state give the same bits, and no floating-point atomic is involved. */
#define SPH_RENDER_MAX_RADIUS_PX 64
#define SPH_RENDER_MAX_SIZE 4096
typedef struct sph_camera {
    uint32_t width, height;        /* 1..SPH_RENDER_MAX_SIZE each */
    float rot[9];                  /* row-major world -> eye rotation */
    float trans[3];
    float focal_px;                /* > 0 */
    float near_z, far_z;           /* 0 < near_z < far_z */
} sph_camera;
enum { SPH_COLOR_INDEX = 0, SPH_COLOR_SPEED = 1, SPH_COLOR_DENSITY = 2 };
typedef struct sph_render_style {
    int32_t  color_mode;
    float    lo, hi;               /* SPH_COLOR_SPEED / SPH_COLOR_DENSITY */
    float    radius;               /* world units; 0 = params.particle_radius */
    uint32_t index_count;          /* SPH_COLOR_INDEX; 0 = sph_num_particles */
    uint8_t  background[4];        /* r, g, b, a */
} sph_render_style;
/* Host helper: the camera at `eye` looking at `target`, vertical field of view fovy_deg, focal_px = 0.5*height / tan(fovy/2).
 * The arithmetic is double and every field is rounded once to fp32; the kernels use only the struct's fields.  The upper
 * layers default to the reference's view: eye (0, 0, 3), target the origin, up +y, 60 degrees, 0.1 .. 100
 * (SPH/particles.cpp:64-65, 324) -- rot = diag(1, 1, -1), trans = (0, 0, 3).
 *   SPH_E_INVALID  eye == target, up parallel to the view direction, anything not finite, a size outside 1..4096, fovy outside
 *                  (0, 180), near_z <= 0 or far_z <= near_z.  *out is then untouched. */
int sph_camera_look_at(sph_camera* out, uint32_t width, uint32_t height, const float eye[3], const float target[3],
                       const float up[3], float fovy_deg, float near_z, float far_z);
/* Render the owned particles as they are now: three kernels queued on the context's stream, no host wait.  Legal at any
 * stage (also before the first step, between two phases, with no particle at all: all background); writes none of the context's
 * step flags and no particle array.  Device buffers (8 + 4 + 4 + 4 bytes per pixel) are allocated at the first call, again
 * when the image size changes (that call waits for the stream first), and freed by sph_destroy.
 *   SPH_E_INVALID  a size outside 1..4096, a camera field that is not finite, focal_px <= 0, near_z <= 0, far_z <= near_z, an
 *                  unknown colour mode, hi == lo (or either not finite) in a mode that uses them, a radius that is negative or
 *                  not finite: the previous image stays;
 *   SPH_E_STATE    a slab context: the ranks would have to composite their images.  Out of scope, as for emitters and bodies. */
int sph_render(sph_ctx* c, const sph_camera* camera, const sph_render_style* style);
/* The last image to the host: rgba width*height*4 bytes (r, g, b, a per pixel, rows top to bottom), id the winner's creation
 * index, depth its d.  Any pointer may be NULL.  Synchronises.  SPH_E_STATE if nothing was rendered yet. */
int sph_render_read(sph_ctx* c, uint8_t* rgba, uint32_t* id, float* depth);
/* The device pointer of the RGBA8 image of the last render, and its size, for a consumer on the same stream: what
 * sph_positions_dev is one stage earlier.  Valid until the next render of another size.  SPH_E_STATE if nothing was rendered. */
int sph_render_image_dev(sph_ctx* c, void** rgba_dev, uint32_t* width, uint32_t* height);

/* ---- pictures: the fluid as a SURFACE, in screen space -- sphere depth, thickness, smoothed depth, normals, a water-like shading ------
 * Same camera, same key image, same read-back as sph_render; the image-space half is new.  Nothing transcendental runs on the
 * device, no floating-point atomic, every sum in a fixed order.
 *
 * THE RULE (fp32, every operation rounded, no multiply-add fusion, sums left to right, IEEE division and square root;
 * tests/surface_model.py is the same arithmetic in numpy and gives every plane bit for bit).
 * FRAGMENTS.  pe, d, rp, cx, cy, u, v, mag and the coverage test mag <= 1 are sph_render's, above.  With R the style's radius
 * (0: params.particle_radius) a particle is drawn iff  d - R >= near_z && d <= far_z.  The fragment's depth is the sphere's:
 *     nz = sqrtf(1 - mag) ;  dz = d - R*nz            (so dz >= near_z > 0, and its bits order as the float does)
 * The key is (bits(dz) << 32) | slot: the smallest dz wins the pixel, among equal dz the lowest slot.  RAW DEPTH Z_0 is the
 * winner's dz, +inf on background.
 * THICKNESS (only if some absorb[k] > 0).  Every covered fragment, occluded or not, adds
 *     q = (uint32_t)(nz*16.0f + 0.5f)                 (0..16)
 * to the pixel's 32-bit word with an integer atomic add: the sum does not depend on the order of arrival.  At most 16 per
 * particle, hence sph_num_particles < 2^28.  World thickness  T = (float)count * (R*0.125f).
 * SMOOTHING.  r = smooth_radius_px, K = smooth_iterations, tau = depth_falloff (0: 4.0f*R).  Weights, computed on the host in
 * double and rounded once:  S[k] = (float)exp(-(k*k) / (2*sigma*sigma)), sigma = r/2, k = 0..r.  K == 0 or r == 0: Z_K = Z_0.
 * Else for it = 1..K, for every pixel (i, j): a background pixel stays +inf; otherwise zc = Z_{it-1}(i, j), num = den = 0, and
 * for dj = -r..r ascending, inside it di = -r..r ascending, where (i+di, j+dj) is inside the image and
 * zn = Z_{it-1}(i+di, j+dj) is finite:
 *     e = (zn - zc) / tau ;  q = 1.0f - e*e ;  if (q > 0) { w = (S[|di|]*S[|dj|]) * (q*q) ;  num = num + w*zn ;  den = den + w }
 * and Z_it(i, j) = num / den  (the centre tap gives den >= S[0]^2 = 1).  A neighbour further than tau in depth weighs exactly 0:
 * edges between sheets of fluid survive, the silhouette never grows.
 * NORMALS from Z = Z_K.  The eye-space point of a surface pixel, z = Z(i, j):
 *     P(i, j) = ( (((i + 0.5f) - 0.5f*width) * z) / focal_px ,  ((0.5f*height - (j + 0.5f)) * z) / focal_px ,  z )
 * ddx: fwd = P(i+1, j) - P(i, j), bwd = P(i, j) - P(i-1, j), each available only where that neighbour is inside the image and is
 * surface (finite Z).  Both: fwd if |fwd.z| <= |bwd.z|, else bwd.  One: that one.  None: (z/focal_px, 0, 0).
 * ddy: the same with fwd = P(i, j-1) - P(i, j) (row j-1 is +y), bwd = P(i, j) - P(i, j+1); none: (0, z/focal_px, 0).
 *     n = cross(ddy, ddx):  nx = ddy.y*ddx.z - ddy.z*ddx.y ;  ny = ddy.z*ddx.x - ddy.x*ddx.z ;  nz = ddy.x*ddx.y - ddy.y*ddx.x
 *     len2 = (nx*nx + ny*ny) + nz*nz ;  n = n / sqrtf(len2) per component ;  n = (0, 0, -1) unless len2 is finite and > 0
 * (a wall seen head-on has n = (0, 0, -1): it faces the eye).  Background: n = (0, 0, 0).
 * SHADING.  With P = P(i, j), L the style's light normalised on the host in double and rounded once:
 *     pl = sqrtf((P.x*P.x + P.y*P.y) + P.z*P.z) ;  V = (-P) / pl per component
 *     ndl = max(0, (n.x*L.x + n.y*L.y) + n.z*L.z)                               (every dot product in this order)
 *     H = L + V ;  hl = sqrtf((H.x*H.x + H.y*H.y) + H.z*H.z) ;  H = H / hl if hl > 0, else H = n
 *     spec = max(0, n.H), then five times spec = spec*spec                      (the 32nd power)
 *     ndv = min(max(n.V, 0), 1) ;  m = 1.0f - ndv ;  F = 0.02f + 0.98f * (((m*m)*(m*m))*m)
 *     base_k = flat_color ? tint_k : tint_k * c_k         (c: sph_render's ramp colour of the front particle, style.color_mode)
 *     tr_k = 1.0f / (1.0f + absorb_k*T) if the thickness pass ran, else 0       (a rational stand-in for Beer-Lambert: no exp)
 *     bg_k = (float)background[k] / 255.0f
 *     body_k = (base_k * (0.25f + 0.75f*ndl)) * (1.0f - tr_k) + bg_k*tr_k
 *     out_k = (body_k * (1.0f - F) + F) + specular*spec
 *     channel8 = (uint8)(min(max(out_k, 0), 1)*255.0f + 0.5f) ;  alpha = 255
 * id is the creation index of the front particle.  A background pixel holds the style's background colour, id 0xFFFFFFFF,
 * depth +inf, as after sph_render. */
#define SPH_SURFACE_MAX_RADIUS_PX 16
#define SPH_SURFACE_MAX_ITERATIONS 8
typedef struct sph_surface_style {
    uint32_t smooth_radius_px;   /* r: 0..SPH_SURFACE_MAX_RADIUS_PX; 0 = no smoothing */
    uint32_t smooth_iterations;  /* K: 0..SPH_SURFACE_MAX_ITERATIONS; 0 = no smoothing */
    float    depth_falloff;      /* tau, world units; 0 = 4 * the resolved sprite radius */
    int32_t  flat_color;         /* 1: base colour = tint; 0: tint * the ramp colour of the front particle (style.color_mode) */
    float    tint[3];
    float    absorb[3];          /* >= 0 per channel, per world unit of thickness; all 0 = no thickness pass at all */
    float    light[3];           /* eye space (+x right, +y up, +z forward); any non-zero finite vector */
    float    specular;           /* >= 0, strength of the highlight */
} sph_surface_style;
/* r 5, K 2, tau 0, flat 1, tint (0.25, 0.55, 0.95), absorb (6, 2, 0.5), light (1, 1, -1), specular 0.6 */
void sph_surface_defaults(sph_surface_style* s);
/* Render the owned particles as a surface.  Validates as sph_render does, is legal wherever sph_render is, writes none of the
 * step's flags and no particle array; its kernels are queued on the context's stream with no host wait (but for the call that
 * (re)allocates the image, as in sph_render).  The results land where sph_render's do: sph_render_read and
 * sph_render_image_dev give the RGBA8 image, id, and as depth the SMOOTHED depth Z_K.  The extra device buffers (4 + 4 + 4 + 12
 * bytes per pixel) are allocated at the first surface render only, and freed with the image.
 *   SPH_E_INVALID   what sph_render refuses; r or K out of range; depth_falloff negative or not finite; a tint, absorb or
 *                   specular that is negative or not finite; a light that is zero or not finite: the previous image stays;
 *   SPH_E_CAPACITY  sph_num_particles >= 2^28 (the thickness word);
 *   SPH_E_STATE     a slab context. */
int sph_render_surface(sph_ctx* c, const sph_camera* camera, const sph_render_style* style, const sph_surface_style* surface);
/* The extra planes of the last surface render to the host: raw_depth width*height floats (Z_0), thickness_q the counts (all 0
 * when the thickness pass was off), normal_xyz 3 floats per pixel.  Any pointer may be NULL.  Synchronises.  SPH_E_STATE unless
 * the last render was a surface render. */
int sph_render_surface_read(sph_ctx* c, float* raw_depth, uint32_t* thickness_q, float* normal_xyz);

/* ---- pictures: the SOLIDS -- the obstacle slots' distance grids ray-marched into both renderers -----------------------------------
 * Opt-in: while a solid style is set, sph_render and sph_render_surface also draw every obstacle slot that is installed and has
 * draw != 0, with the offset and pose the next push would see.  A context that never sets a style launches, allocates and
 * computes what it did without this section, obstacles installed or not.
 *
 * THE RULE (fp32, every operation rounded, no multiply-add fusion, sums left to right, IEEE division and square root; fminf and
 * fmaxf return the other operand when one is NaN; tests/solid_render_model.py is the same arithmetic in numpy and gives every
 * plane bit for bit).
 * RAY of pixel (i, j); half_w = 0.5f*width, half_h = 0.5f*height, focal = focal_px, rot and trans the camera's:
 *     ex = (((float)i + 0.5f) - half_w) / focal ;  ey = (half_h - ((float)j + 0.5f)) / focal ;  le = sqrtf((ex*ex + ey*ey) + 1.0f)
 *     O[k] = -((rot[k]*trans[0] + rot[3+k]*trans[1]) + rot[6+k]*trans[2])
 *     D[k] = (rot[k]*ex + rot[3+k]*ey) + rot[6+k]
 *     X(z)[k] = O[k] + z*D[k]                             (z is the eye-space depth: comparable with the fluid's d and Z_K)
 * CLIP, per slot, in its body frame.  Unposed: Ob = O - off, Db = D.  Posed (R = rot of sph_obstacle_set_pose, P = pivot + off),
 * with dO = O - P:
 *     Ob[k] = ((R[0][k]*dO[0] + R[1][k]*dO[1]) + R[2][k]*dO[2]) + pivot[k] ;  Db[k] = (R[0][k]*D[0] + R[1][k]*D[1]) + R[2][k]*D[2]
 * With lo_k = origin_k, hi_k = origin_k + (float)(n_k - 1)*s, for k = 0, 1, 2 in turn, from t0 = near_z, t1 = far_z:
 *     inv = 1.0f / Db[k] ;  ta = (lo_k - Ob[k])*inv ;  tb = (hi_k - Ob[k])*inv ;  t0 = fmaxf(t0, fminf(ta, tb)) ;  t1 = fminf(t1, fmaxf(ta, tb))
 * !(t0 <= t1) is a miss.  (A zero Db[k] gives infinities, or a NaN that the min and max drop.)
 * MARCH.  z = za = t0, open_run = (look.open != 0).  Up to SPH_SOLID_MAX_STEPS times:
 *     if !(z <= t1): miss.  Take the slot's SAMPLE at X(z) -- the rule of sph_obstacle_sample, posed or not.
 *     outside the grid:            a = 0.25f*s ;  za = z
 *     inside, phi < 0, open_run:   a = fmaxf(0.5f*(-phi), 0.25f*s) ;  za = z
 *     inside, phi < 0, otherwise:  zb = z, a crossing: the loop ends
 *     inside, !(phi < 0):          open_run = false ;  a = fmaxf(0.5f*phi, 0.25f*s) ;  za = z
 *     z = z + a / le
 * A ray that uses up the steps misses.  (0.5: an interpolated field's gradient reaches about 1.4, see the PUSH; the floor of a
 * quarter spacing: geometry is resolved to the spacing.  open: the stretch of solid in which the ray starts is invisible -- one
 * looks into an inverted sphere, a bowl, and sees its far inside wall.)
 * REFINE.  SPH_SOLID_BISECTIONS times:  zm = 0.5f*(za + zb) ;  sample at X(zm) ;  inside the grid and phi < 0: zb = zm, else za = zm.
 * The hit is z_s = zb; its world normal n is that of the sample that last set zb (a posed slot's: rot * body normal, not
 * renormalised, as in the push).
 * SHADE.  L the style's light, normalised on the host in double and rounded once (eye space, as the surface's):
 *     ne[k] = (rot[3k]*n[0] + rot[3k+1]*n[1]) + rot[3k+2]*n[2] ;  ndl = fmaxf(0, (ne[0]*L[0] + ne[1]*L[1]) + ne[2]*L[2])
 *     g = ambient + (1.0f - ambient)*ndl ;  c_k = fminf(fmaxf(color_k*g, 0), 1) ;  channel8 = (uint8)(c_k*255.0f + 0.5f) ;  alpha = 255
 * SEVERAL SLOTS.  The smallest z_s wins, among equal z_s the lowest slot.
 * sph_render.  A pixel goes to the solid iff it has a hit and either no sprite covers it or z_s < d of the winning sprite
 * (strict).  It then holds the solid's RGBA, id SPH_RENDER_ID_SOLID + slot and depth z_s; every other pixel is bit for bit what
 * it is with the style off.  (The march of a pixel stops at the first free sample at or behind the fluid's d: no later crossing
 * could win.)
 * sph_render_surface.  A pixel goes to the solid iff it has a hit and either it is background or z_s < Z_K.  It then holds RGBA,
 * id and depth as above, and its normal is ne.  Where the fluid wins and the ray has a hit behind it, the shading's bg_k is the
 * solid's c_k: water in a vessel lets the vessel show through by its thickness.  Z_0, the thickness and the smoothing are
 * untouched, and a fluid pixel's normal comes from Z_K as before.
 * How: one pixel per lane, a wave an 8 x 8 tile of pixels, behind the splat on the context's stream; the composition is a plain
 * store, no atomic, no host wait. */
#define SPH_RENDER_ID_SOLID  0xFFFFFFF0u   /* id plane: a pixel won by slot k reads SPH_RENDER_ID_SOLID + k */
#define SPH_SOLID_MAX_STEPS  512
#define SPH_SOLID_BISECTIONS 6
typedef struct sph_solid_look {
    int32_t draw;                  /* 0: the slot is not drawn */
    int32_t open;                  /* != 0: the stretch of solid in which a ray starts is invisible */
    float   color[3];              /* each in [0, 1] */
} sph_solid_look;
typedef struct sph_solid_style {
    sph_solid_look slot[SPH_MAX_OBSTACLES];
    float light[3];                /* eye space; any non-zero finite vector */
    float ambient;                 /* in [0, 1] */
} sph_solid_style;
/* draw 1, open 0, colour (0.72, 0.72, 0.75) for every slot, light (1, 1, -1), ambient 0.25 */
void sph_solid_defaults(sph_solid_style* s);
/* The style belongs to the context; NULL switches the solids off (the default).  Legal at any stage; writes no step flag,
 * launches nothing and allocates nothing.  The extra device planes (the solid's depth, slot and eye-space normal: 4 + 4 + 12 bytes
 * per pixel) are allocated at the first surface render with solids on and freed with the image; sph_render needs none.
 *   SPH_E_STATE     a slab context;
 *   SPH_E_INVALID   a colour, light or ambient that is not finite, a colour component or ambient outside [0, 1], a zero light;
 *   SPH_E_CAPACITY  sph_capacity >= SPH_RENDER_ID_SOLID (the id plane could not tell a solid from a particle).
 * In every refused case nothing has changed. */
int sph_render_set_solids(sph_ctx* c, const sph_solid_style* style);
/* *on = whether a style is set; *out = that style as it was given (untouched while off).  Either pointer may be NULL. */
int sph_render_get_solids(const sph_ctx* c, int* on, sph_solid_style* out);

/* ---- geometry: the fluid's surface as a triangle mesh, extracted on the device (no counterpart in the reference, which only draws
 *      into a GL window) ---------------------------------------------------------------------------------------------------------
 * A count field is splatted onto a regular lattice over the box, and the level set count >= iso_q is triangulated by cutting
 * every lattice cube into six tetrahedra.  Whole-domain contexts only.  Reads the sorted positions; writes none of the context's
 * step flags and no particle array.  A caller who never meshes gets the launches and the allocations of a library without this
 * section.
 *
 * THE RULE (fp32, every operation rounded, no multiply-add fusion, sums left to right, IEEE division and square root;
 * tests/mesh_model.py is the same arithmetic in numpy and gives counts, positions, normals and triangles bit for bit).
 * PARAMETERS.  s = spacing (0: params.particle_radius), r = radius (0: 3.0f * s), iso (0: 0.5f).  r / s <= SPH_MESH_MAX_REACH.
 * LATTICE (sph_mesh_lattice; in double on the host, each result rounded once):
 *     pad = ceil(r / s) + 1 ;  n_k = ceil((box_max_k - box_min_k) / s) + 1 + 2*pad ;  origin_k = box_min_k - (float)pad * s  (fp32)
 * Node i of axis k sits at X = origin_k + (float)i * s.  The pad leaves the outermost nodes at 0 for every particle inside the
 * box, so EVERY MESH IS CLOSED, also where fluid lies against a wall (particles outside the box can break that).  Limits: every
 * n_k <= SPH_MESH_MAX_DIM, n_x*n_y*n_z <= SPH_MESH_MAX_NODES (hence fewer than 2^32 vertices and triangles): else SPH_E_CAPACITY.
 * (The default r = 3.0f * s divided by s in double is 3 up to fp32 rounding: where the product rounded up, ceil gives a reach of
 * 4 and a pad of 5 -- s = 1/15 --, else 3 and 4 -- s = 1/64.  The default spacing, the particle radius 1/64, fits a box of edge up
 * to about 7.8: of the standard scenes only config 1's; configs 2 and 3 (edges 8 and 32) need a wider spacing and are refused
 * at the defaults.)
 * FIELD: one uint32 count per node.  For every owned particle p and every node of the lattice, r2 = r*r:
 *     dx = X - p.x (likewise dy, dz) ;  d2 = (dx*dx + dy*dy) + dz*dz ;  if d2 < r2:
 *         t = 1.0f - d2 / r2 ;  w = (t*t)*t ;  q = (uint32_t)(w*4096.0f + 0.5f) ;  count += q
 * with a 32-bit INTEGER atomic add: the sum does not depend on the order of arrival, and no floating-point atomic is involved.
 * (The kernel walks the nodes within ceil(r/s) + 1 of floor((p.x - origin_x) / s) per axis -- a superset of those that pass while
 * |X| / s stays below 2^20.)  A count overflows only with 2^20 particles within r of one node; that is not checked.
 *     v = iso*4096.0f + 0.5f ;  iso_q = max(1, v < 2^32 ? (uint32_t)v : 0xFFFFFFFF) ;  a node is INSIDE iff count >= iso_q  (integers)
 * CELLS.  The cube with base node (i, j, k), i < n_x - 1 and likewise j, k, has corners c = 0..7 with bit 0 = +x, bit 1 = +y,
 * bit 2 = +z, and is cut into the six Kuhn tetrahedra (0, e_a, e_a|e_b, 7) of the axis orders m = 0..5: xyz, xzy, yxz, yzx, zxy,
 * zyx.  Every edge of a tetrahedron joins corners cu, cv with cu a subset of cv: it is the LATTICE EDGE (node base + bits(cu),
 * direction d = cu ^ cv in 1..7), which neighbouring tetrahedra and neighbouring cubes share -- the triangulation is
 * face-compatible with nothing but 16 cases per tetrahedron.
 * VERTICES.  A lattice edge (node a, direction d) whose far node b = a + bits(d) is in the lattice and whose ends differ in
 * inside-ness owns one vertex.  With the counts Ca, Cb and the node positions Xa, Xb:
 *     t = ((float)iso_q - (float)Ca) / ((float)Cb - (float)Ca) ;  position = Xa + t*(Xb - Xa) per component
 *     G at a node = ((float)((int64)C(i+1,j,k) - (int64)C(i-1,j,k)), likewise y, z), neighbours outside the lattice counting 0
 *     g = Ga + t*(Gb - Ga) per component ;  len2 = (g.x*g.x + g.y*g.y) + g.z*g.z
 *     normal = (-g) / sqrtf(len2) per component, or (0, 0, 0) unless len2 is finite and > 0        (it points out of the fluid)
 * VERTEX ORDER: the node's linear index (k*n_y + j)*n_x + i ascending, then d ascending.  A node whose count equals iso_q gives
 * t = 0 on its edges: coincident vertices and triangles of zero area; the mesh stays closed combinatorially.
 * TRIANGLES are uint32 triples of vertex numbers.  Per tetrahedron with corners v0..v3 (XY: the vertex on the edge X-Y):
 *     one corner A unlike the other three B, C, D (in corner order):           (AB, AC, AD)
 *     two inside A, B and two outside C, D (each pair in corner order):        (AC, AD, BD) then (AC, BD, BC)
 * each wound so that (p1 - p0) x (p2 - p0) points from the inside corners to the outside ones.  That sign is a constant of
 * (m, case): it is evaluated with every vertex at its edge's midpoint against (centroid of the outside corners - centroid of the
 * inside corners), and where it is negative the last two vertices are swapped.
 * TRIANGLE ORDER: the cube's linear index (the same formula, on its base node) ascending, then m ascending, then as listed. */
#define SPH_MESH_MAX_REACH 8
#define SPH_MESH_MAX_DIM 2048
#define SPH_MESH_MAX_NODES (1u << 27)
typedef struct sph_mesh_params {
    float spacing;    /* s > 0; 0 = params.particle_radius */
    float radius;     /* r > 0; 0 = 3 * s */
    float iso;        /* > 0; 0 = 0.5 (a lone particle's count is 1 at its centre) */
} sph_mesh_params;
void sph_mesh_defaults(sph_mesh_params* p);      /* all three 0 */
/* Host helper: the lattice sph_mesh_extract would use for these parameters (NULL: the defaults) in this context's box.
 * SPH_E_INVALID / SPH_E_CAPACITY as sph_mesh_extract; dims and origin are then untouched. */
int sph_mesh_lattice(const sph_ctx* c, const sph_mesh_params* p, uint32_t dims[3], float origin[3]);
/* Extract the surface of the owned particles as they are now (p NULL: the defaults).  Queues the field and the counting kernels,
 * waits ONCE for the two totals (an export call, not part of a step), grows the vertex and triangle buffers if it must and queues
 * the kernels that fill them.  Legal at any stage, like sph_render: before the first step, between two phases, with no
 * particle (0 vertices, 0 triangles, SPH_OK).  Device buffers (8 bytes per lattice node and 2 words per 256 nodes; 24 bytes per
 * vertex, 12 per triangle) are allocated at the first extraction or when one must grow, and freed by sph_destroy.
 *   SPH_E_INVALID   a parameter that is negative or not finite; r / s > SPH_MESH_MAX_REACH;
 *   SPH_E_CAPACITY  the lattice limits above;
 *   SPH_E_STATE     a slab context: the ranks would have to share a lattice seam.  Out of scope, as for render, emitters and bodies.
 * In every refused case nothing has changed and nothing was allocated.  SPH_E_NOMEM: the mesh buffers are all released and there
 * is no mesh until the next extraction. */
int sph_mesh_extract(sph_ctx* c, const sph_mesh_params* p, uint32_t* n_vertices, uint32_t* n_triangles);
/* The last mesh to the host: 3 floats per vertex, 3 floats per vertex, 3 vertex numbers per triangle.  Any pointer may be NULL.
 * Synchronises.  SPH_E_STATE before any extraction (also for sph_mesh_dev, sph_mesh_save_obj, sph_mesh_field_dims / _read). */
int sph_mesh_read(sph_ctx* c, float* pos_xyz, float* normal_xyz, uint32_t* tri);
/* Device pointers of the last mesh for a consumer on the same stream (any may be NULL; the pointers are NULL while no extraction
 * has produced a vertex yet).  Valid until the next extraction. */
int sph_mesh_dev(sph_ctx* c, void** pos_dev, void** normal_dev, void** tri_dev, uint32_t* n_vertices, uint32_t* n_triangles);
/* Wavefront OBJ: "v x y z" and "vn x y z" per vertex with %.9g (an fp32 survives the round trip), "f a//a b//b c//c" per
 * triangle, 1-based.  Synchronises.  SPH_E_INVALID if the file cannot be written. */
int sph_mesh_save_obj(sph_ctx* c, const char* path);
/* The lattice of the last extraction: its dimensions (no synchronisation), and its counts, n_x*n_y*n_z words, x fastest
 * (synchronises). */
/* [introspect] */ int sph_mesh_field_dims(sph_ctx* c, uint32_t dims[3]);
/* [introspect] */ int sph_mesh_field_read(sph_ctx* c, uint32_t* counts);

/* State snapshot (checkpoint / resume; absent in the reference, whose device state is never
 * serialised -- SURVEY.md section 5).  The file holds the parameters and, IN SLOT ORDER, position,
 * velocity and creation index of every owned particle, so that a resumed run repeats the
 * original one bit for bit (the sort is stable), and behind them the next unused creation index (sph_emit; files without it
 * load as before).  Little-endian, see csrc/sph_capi.hip. */
int sph_snapshot_save(sph_ctx* c, const char* path);
/* Load into an existing context (same grid; capacity >= the stored particle count and > every stored creation index). */
int sph_snapshot_load(sph_ctx* c, const char* path);
/* Number of particles and the parameters stored in a snapshot (to size a context for it). */
int sph_snapshot_info(const char* path, uint32_t* n, sph_params* p);

/* introspection for per-phase parity tests (sorted order) */
/* [introspect] */ int sph_get_keys(sph_ctx* c, uint32_t* keys);          /* cell key per slot */
/* [introspect] */ int sph_get_order(sph_ctx* c, uint32_t* index);        /* creation index per slot */
/* [introspect] */ int sph_get_cell_range(sph_ctx* c, uint32_t cell, uint32_t* start, uint32_t* end);
/* occupied cells in ascending key order: {key, start, count}; returns the number written
 * (<= max_cells) or a negative code */
/* [introspect] */ int sph_get_cells(sph_ctx* c, uint32_t max_cells, uint32_t* key, uint32_t* start, uint32_t* count);
/* local cell key of global cell coordinates (x, y, z): (z_local*gy + y)*gx + x */
/* [introspect] */ uint32_t sph_cell_key(const sph_ctx* c, uint32_t x, uint32_t y, uint32_t z);

/* ---- phases (each replaces one seam call; see the SPH_PH_* table) ------------------------ */
int sph_hash(sph_ctx* c);
int sph_sort(sph_ctx* c);
int sph_build_cells(sph_ctx* c);
int sph_density(sph_ctx* c);
int sph_force(sph_ctx* c);
int sph_collide(sph_ctx* c);
int sph_integrate(sph_ctx* c, float dt);
/* n full time steps = n iterations of the loop body of ParticleSystem::update
 * (particleSystem.cpp:725-811), using the fused kernels (force+collision+integrate in one
 * neighbour traversal).  Results equal the phase-by-phase sequence to fp32 rounding. */
int sph_step(sph_ctx* c, float dt, uint32_t n_steps);
/* same, phase by phase (the exact call sequence of particleSystem.cpp:773-795) */
int sph_step_phased(sph_ctx* c, float dt, uint32_t n_steps);
/* the fused tail of sph_step on its own: force + collision + integrate in one neighbour traversal
 * (needs sph_density; slab drivers call it after the density halo exchange) */
int sph_force_collide_integrate(sph_ctx* c, float dt);

/* ---- device timing (replaces the host-side TIME_FUNCTION macros, particleSystem.h:20-24,
 *      which time launches, not kernels) ------------------------------------------------------ */
int sph_timing_enable(sph_ctx* c, int on);
/* sums of per-phase device milliseconds since the last reset, and the number of steps */
int sph_timing_get(sph_ctx* c, float ms[SPH_PH_COUNT], uint32_t* n_steps);
int sph_timing_reset(sph_ctx* c);
/* sort statistics: sorts run so far; how many of them took the merge path (only the particles whose
 * cell changed are sorted; same result as the full sort); how many of those found that no particle had
 * changed cell and did nothing at all (`skips`: the order, the keys and the cell table of the previous
 * step are still exact -- a fluid at rest; taken only when the device has already reported the count, the
 * host never waits for it); the mover count the device last reported; and the sum of the mover counts of
 * all sorts so far (movers_total: particles that changed cell, summed over steps).  Synchronises the stream.
 * Any pointer may be NULL. */
/* [introspect] */ int sph_sort_stats(sph_ctx* c, uint64_t* sorts, uint64_t* merges, uint64_t* skips, uint32_t* last_movers,
                   uint64_t* movers_total);
/* How the movers' sorts of the merge path were launched so far: out[0] both forms (the count lives on the device, each
 * kernel looks at it and leaves if it is not its turn), out[1] the one-block sort alone, out[2] the multi-block passes
 * alone -- the last two from the count the device last reported: the previous sort's in a host-paced (slab) context, at most
 * four sorts old in a whole-domain one (there with a margin: both forms while the count is within a quarter of the one-block
 * sort's capacity).  No synchronisation. */
/* [introspect] */ int sph_sort_forms(const sph_ctx* c, uint64_t out[3]);
/* merge = 1 (default): the sort takes the merge path while few particles change cell (up to 1/8 of them, by
 * the count the device last reported); 0: the full radix sort every step (what SPH_SORT_MERGE=0 in the
 * environment selects at sph_create time); 2: the merge path whenever the previous order is intact, whatever
 * the count (it is exact for any count; for tests).  Takes effect at the next sort. */
/* [tuning] */ int sph_set_sort_mode(sph_ctx* c, int merge);
/* The neighbour passes stage, per (dz, dy) row, the hull of a wave's candidate ranges through LDS.  A row whose hull
 * is longer than `slots` (default 512; usual hulls are ~80) is read straight from global memory by every lane instead
 * -- sparse particles next to a dense layer would otherwise stage thousands of slots for a handful of candidates each
 * and become the tail of the whole launch.  In SPH_PRECISION_F32 both ways give the same bits (same candidates, same order,
 * same arithmetic).  In SPH_PRECISION_MIXED_F16 they do NOT: the staged walk pairs fp16 candidates per 128-slot piece, the
 * direct walk per row, so the fp16 row sums differ within the mixed tolerance -- and since the way a wave goes depends on
 * its 63 wave-mates, mixed-mode results depend on this setting and on how a domain is cut into slabs.  The test in front
 * of the exact one is a heuristic (key span of the wave <= 64 cells: taken as "no hull beyond `slots`", which cells of
 * more than slots / 66 particles can break -- such a wave stages a long hull, slowly but correctly).
 * 0: every row direct; 0xFFFFFFFF: never (for tests and A/B runs).  Takes effect at the next launch. */
/* [tuning] */ int sph_set_direct_hull(sph_ctx* c, uint32_t slots);
/* A context that owns FEWER than `slots` particles launches the neighbour passes in workgroups of 128 threads instead of 256
 * (default 524288).  Waves do not depend on their block (wave-private LDS slices, no block barrier in the walk): same results
 * bit for bit; config 2's flowing dam steps 12 % faster this way, large launches lose ("small steps").
 * 0: never; 0xFFFFFFFF: always.  Takes effect at the next launch; SPH_PAIR_SMALL_SLOTS in the environment at create time does
 * the same for A/B runs. */
/* [tuning] */ int sph_set_pair_small_launch(sph_ctx* c, uint32_t slots);
/* The ORDER in which the neighbour passes' workgroups take the sorted slots (results do not depend on it).  xcd = 1
 * (default): each of the 8 XCDs walks one contiguous eighth of the slots; ztile = 1 (default): inside its eighth an XCD
 * walks strips of 2^strip_blocks_log2 workgroups (default 4: 16 workgroups = 4096 slots) through all cell layers of the
 * eighth before the next strip, so that the rows of neighbouring layers are re-used out of the XCD's L2: half the HBM-side
 * reads of the plain order.  0 / 0 restores the plain front-to-back order (A/B runs). */
/* [tuning] */ int sph_set_block_order(sph_ctx* c, int xcd, int ztile, uint32_t strip_blocks_log2);
/* 1 if the last sph_sort found that no particle had changed cell and left everything as it was (then
 * every count derived from the sorted order -- sph_slab_counts, sph_halo_count -- is that of the step
 * before), else 0.  No synchronisation. */
/* [introspect] */ int sph_last_sort_skipped(const sph_ctx* c);

/* ---- z-slab halo / migration (multi-GPU; no counterpart in the reference) ---------------- */
/* side: 0 = towards lower z (rank-1), 1 = towards higher z (rank+1).
 * Records are 8 floats: x, y, z, index bits, vx, vy, vz, 0. */
#define SPH_HALO_RECORD_FLOATS 8
/* after sph_hash + sph_sort: number of owned particles that left the slab through `side` */
int sph_migrants_count(sph_ctx* c, uint32_t count[2]);
/* everything a slab driver needs after the sort, in one device round trip:
 * {migrants down, owned in the lowest layer, owned in the highest layer, migrants up} */
int sph_slab_counts(sph_ctx* c, uint32_t count[4]);
/* pack them into buf_dev[side] (device, capacity records each) and drop them */
int sph_migrants_pack(sph_ctx* c, void* buf_dev[2], uint32_t capacity);
/* append n received particles (device records) to the owned set; call sph_hash+sph_sort again */
int sph_migrants_append(sph_ctx* c, const void* buf_dev, uint32_t n);
/* number of owned particles in the boundary layers (what the neighbours need as ghosts) */
int sph_halo_count(sph_ctx* c, uint32_t count[2]);
int sph_halo_pack(sph_ctx* c, void* buf_dev[2], uint32_t capacity);
/* same with the two counts supplied by the caller (a slab driver knows them from sph_slab_counts and
 * the migrant counts), which saves a device round trip; they are remembered for the density halo */
int sph_halo_pack_counts(sph_ctx* c, void* buf_dev[2], uint32_t capacity, const uint32_t count[2]);
/* install n_lo / n_hi ghost records received from the lower / upper neighbour */
int sph_halo_unpack(sph_ctx* c, const void* lo_dev, uint32_t n_lo, const void* hi_dev, uint32_t n_hi);
/* second exchange: (density, pressure) float2 of the same boundary particles, same order */
int sph_halo_pack_density(sph_ctx* c, void* buf_dev[2], uint32_t capacity);
int sph_halo_unpack_density(sph_ctx* c, const void* lo_dev, const void* hi_dev);
/* per z cell layer histogram of owned particles (global layer ids), for count-balanced cuts */
int sph_layer_histogram(sph_ctx* c, uint32_t* hist, uint32_t n_layers);

/* ---- the slab step under the C ABI: one call = one time step of this rank's slab, with its neighbours ------- */
/* How the messages of a step reach the two z-neighbours.  `exchange` moves four buffers at once: send_lo goes to
 * rank-1 (and arrives there in its recv_hi), send_hi to rank+1, recv_lo / recv_hi are filled by the neighbours;
 * a size of 0 means "nothing on that side" (domain ends, empty layers) -- both ends of a link compute the same sizes.
 *   host_buffers = 0 (product): the pointers are DEVICE pointers and the call enqueues the transfers on hip_stream
 *                    without blocking the host (RCCL: ncclSend/ncclRecv inside one group);
 *   host_buffers = 1 (tests): the pointers are pinned HOST buffers the library staged, the call blocks until its
 *                    receives are complete (several slabs of one GPU in one process; processes over gloo).
 * Return 0 or a negative SPH_E* code. */
enum { SPH_TAG_MIGRANTS = 1, SPH_TAG_HALO_A = 2, SPH_TAG_HALO_B = 3, SPH_TAG_MIGRANTS_REST = 4, SPH_TAG_PING = 5,
       SPH_TAG_RECUT_COUNTS = 6, SPH_TAG_RECUT = 7,
       SPH_TAG_ONE = 8,        /* the one-message step: header + leavers + two layers of residents, size fixed in advance */
       SPH_TAG_ONE_REST = 9 }; /* ... and what did not fit that size (exact; a burst) */
/* ZERO-INITIALISE the struct before filling it in (`sph_transport t = {0};`): sph_slab_create copies it by value, and
 * members added at its end (so far: `abort`, ABI v2 of round 4) must read as NULL in a caller built against an older
 * header -- there is no size field, a garbage `abort` pointer would be called on the first failure. */
typedef struct sph_transport {
    void* self;
    int (*exchange)(void* self, int tag, const void* send_lo, size_t send_lo_bytes, void* recv_lo, size_t recv_lo_bytes,
                    const void* send_hi, size_t send_hi_bytes, void* recv_hi, size_t recv_hi_bytes, void* hip_stream);
    int host_buffers;
    /* optional (may be NULL): take down everything the transport still has queued on a stream -- called when an exchange
     * failed or a neighbour stopped answering, so that no receive without a sender blocks a later synchronisation */
    void (*abort)(void* self);
} sph_transport;

/* RCCL transport over the direct xGMI links (librccl is loaded on first use): rank 0 makes the id, every rank gets
 * the same 128 bytes (the launcher broadcasts them) and joins the communicator with its rank. */
int sph_rccl_unique_id(uint8_t id[128]);
int sph_rccl_transport_create(sph_transport** out, const uint8_t id[128], int rank, int world, int device);
void sph_rccl_transport_destroy(sph_transport* t);
/* two messages of `bytes` and `bytes`/2 bytes from this rank to ITSELF through the transport's communicator (one
 * ncclGroup), compared on the host: checks the dlopen binding of librccl with real traffic on a one-GPU box */
/* [test hook] */ int sph_rccl_transport_selftest(sph_transport* t, size_t bytes);
/* What the communicator says about itself: {ncclCommCount, ncclCommUserRank, ncclCommCuDevice, ncclCommGetAsyncError}
 * (-1 where librccl lacks the call).  The multi-GPU bench prints them: a communicator of the wrong size, or one that sits on
 * another device than the slab's context, explains a hang or a slow run before any step is taken. */
/* [introspect] */ int sph_rccl_transport_info(const sph_transport* t, int out[4]);

/* Device-to-device transport between the slabs of ONE process that share a GPU (one thread per rank): the buffers are
 * device pointers, the copies are queued on the caller's comm stream behind the sender's event, nothing blocks on the
 * device -- the same stream/event edges as with RCCL, on a one-GPU box.  The host threads rendezvous with bounded
 * waits; message sizes and tags of both ends are compared (a disagreement is SPH_E_STATE, not a hang).  One hub per
 * group of ranks, one transport per rank; destroy the transports, then the hub. */
typedef struct sph_local_hub sph_local_hub;
int sph_local_hub_create(sph_local_hub** out, int world, int device);
void sph_local_hub_destroy(sph_local_hub* hub);
int sph_local_hub_set_timeout(sph_local_hub* hub, double seconds);
int sph_local_transport_create(sph_transport** out, sph_local_hub* hub, int rank);
void sph_local_transport_destroy(sph_transport* t);

/* Loop transport: ONE slab whose two neighbours are its own periodic images along z -- what it sends up arrives from below
 * with every position shifted down by `z_shift` (the height of the slab's owned layers), and the other way round.  The slab is
 * created as the middle rank of three (sph_slab_create(..., rank 1, world 3, ...)) on cell layers away from the box's z faces
 * and then does ALL the work of a rank between two neighbours -- migrants, both halo messages at their real sizes, ghost
 * unpack, boundary launches, the host wait -- on one device, with nothing else sharing it: the measured stand-in for a middle
 * rank of an N-GPU run that a one-GPU box allows (`bench.py --force-slab --periodic-z`).  Every message is held back by
 * latency_us + bytes / link_gbs (0 / 0: no delay) on the comm stream before it is delivered: the link is a parameter, not a
 * measurement.  sph_slab_ping does not apply (a slab cannot tell its images apart). */
/* [test hook] */ int sph_loop_transport_create(sph_transport** out, float z_shift, double link_gbs, double latency_us);
/* [test hook] */ void sph_loop_transport_destroy(sph_transport* t);

typedef struct sph_slab sph_slab;
/* Bind a slab context (sph_create_slab, particles uploaded) to its place in the chain of `world` slabs.  The halo
 * capacity is the context's ghost capacity; migrant_capacity (records per side and step, 0 = half the ghost capacity)
 * bounds the leavers / arrivals of one step and side (only 255 of them ride in the fixed-size message of every step).  The transport struct is copied.
 * A slab with a neighbour (world > 1) owns at least TWO cell layers, SPH_E_INVALID otherwise: its lowest and its highest layer are
 * two different boundary layers.  Two is enough -- such a slab has no interior -- for the three-group protocol; the one-message
 * step needs four (sph_slab_set_protocol, which refuses a thinner slab with SPH_E_STATE and leaves the slab as it was).
 * The step orders its streams by sequence numbers (hipStreamWriteValue32 / hipStreamWaitValue32 on a word of device memory) where the
 * device serves that pair -- tried once here, with both streams drained -- and by events otherwise; SPH_SLAB_HOPS=event in the
 * environment forces events (A/B runs, kernel traces: the runtime's wait is a spinning one-workgroup kernel).  The numbers are
 * 32 bits and the wait is "word >= number", so they must never wrap: a slab one of whose edges has reached 0x7FFFFFF0 -- half the
 * range, a week or more of stepping -- SWITCHES TO EVENTS for the rest of its life (it is not re-armed), on entry to its next
 * sph_slab_step, sph_slab_recut or sph_slab_ping; results do not depend on which of the two orders the streams. */
int sph_slab_create(sph_slab** out, sph_ctx* ctx, int rank, int world, const sph_transport* transport,
                    uint32_t migrant_capacity);
void sph_slab_destroy(sph_slab* s);
/* n time steps: sort, migrants, halo A, density, halo B, force + collision + integrate (csrc/sph_slab.hip), queued
 * on the context's stream and a second, high-priority stream; the host waits ONCE per step (for the layer counts),
 * behind the density pass of the slab's deep interior, and that wait is bounded (below).  A particle that crosses
 * more than one cell layer in a step ("far") is handled (one more wait on that step) as long as it lands in an
 * interior layer of the receiving slab; anything else is reported as SPH_E_STATE, never merged out of order. */
int sph_slab_step(sph_slab* s, float dt, uint32_t n_steps);
/* drains both streams; also reports what device-side checks of the last steps flagged */
int sph_slab_sync(sph_slab* s);
/* the step's wait gives up after `seconds` (default 120, or SPH_SLAB_TIMEOUT_S) with SPH_E_DEVICE: a neighbour that
 * stopped with an error never sends its messages */
int sph_slab_set_wait_timeout(sph_slab* s, double seconds);
/* {steps, particles sent away, steps with arrivals, ghosts received, host waits} */
/* [introspect] */ int sph_slab_stats(const sph_slab* s, uint64_t out[5]);
/* the same five + {in-place merges, steps with far arrivals, steps that needed a second migrant message} */
/* [introspect] */ int sph_slab_counters(const sph_slab* s, uint64_t out[8]);
/* of the steps with arrivals, those that merged them into the two boundary layers in place (the rest ran a pass over
 * all particles: more than 2048 arrivals on a side, or no valid cell table) */
/* [introspect] */ uint64_t sph_slab_in_place_merges(const sph_slab* s);
/* transport calls so far: 3 in a usual step (migrants, halo A, halo B), 4 when a side has more leavers than ride in the
 * fixed-size migrant message */
/* [introspect] */ uint64_t sph_slab_exchanges(const sph_slab* s);
/* one-message steps (sph_slab_set_protocol) whose size rule asked for more records than the message buffers hold on some link and
 * were sent at the buffers' size instead: a count beside the "second message" counts, 0 under the three-group protocol */
/* [introspect] */ uint64_t sph_slab_one_clamped(const sph_slab* s);
/* Re-cut (re-balancing): this slab takes over the cell layers [new_z_lo, new_z_hi) of the global grid.  Entirely on the
 * device, the context and the slab object are kept: the owned particles are split by their layer into "to rank - 1" |
 * "stay" | "to rank + 1" (stable), the leaving runs travel point to point through the slab's transport in chunks of the
 * halo buffers, arrivals from below are put in front of what stays and arrivals from above behind it -- the order of the
 * whole-domain sorted array, so an N-slab run keeps the bits of the one-context run across re-cuts -- and the next step
 * starts with a full stable sort, as after an upload.  COLLECTIVE: every rank of the chain calls it (a rank whose layers do
 * not change passes its old range), with cuts that agree across ranks; a particle moves at most ONE rank per call, i.e.
 * new cut r lies within [old cut r-1, old cut r+1] (gpufluidsimulator_amd/slab.py: single_hop_cuts steps a larger move).
 * SPH_E_CAPACITY if the new layers hold more particles than the context's capacity: that rank still takes part in every round of
 * the re-cut, so its neighbours' calls return SPH_OK, and it is failed the way a step fails -- the "abort" header goes out as the
 * first message of the step the neighbours take next, which returns SPH_E_PEER to them (and one step later to theirs); destroy
 * only.  Replaces nothing in the reference (single GPU); SURVEY.md section 8e "re-cut every K steps". */
int sph_slab_recut(sph_slab* s, uint32_t new_z_lo, uint32_t new_z_hi);
/* {re-cuts so far, particles that changed owner in them} */
/* [introspect] */ int sph_slab_recut_stats(const sph_slab* s, uint64_t out[2]);
/* Neighbour ping: `reps` timed rounds (+ one untimed round first) of ONE exchange-shaped group -- `bytes` to and from
 * rank - 1 and rank + 1, through this slab's transport, comm stream and halo buffers -- every word checked on arrival for
 * sender, direction and round.  out = {mean us per group, max us, wrong words}; event times on the comm stream, i.e. what a
 * step's group of that size costs the device (waiting for the neighbour included).  bytes: a multiple of 4, at most the halo
 * buffer ((ghost capacity + 1) * 32).  COLLECTIVE over the chain.  A neighbour that does not answer within the wait
 * time-out, an RCCL error or a wrong word is an error (the slab is failed); there is no fall-back to another transport. */
int sph_slab_ping(sph_slab* s, size_t bytes, uint32_t reps, double out[3]);
/* Where a step's time goes.  Host side, always measured: the step's one wait (WAIT), the host time in front of it (PRE:
 * hash, sort, bounds kernel and the migrant exchange being queued), behind it (POST: everything else being queued) and the
 * whole call (HOST), each {sum us, max us} over the steps since the last reset; WAITS_READY counts the waits that found the
 * header already there -- the host, not the device, paced those steps.  Device side, only between sph_slab_timing_enable(1)
 * and (0): an event pair around every transport call on the comm stream, per message group {calls, sum us, max us} -- the
 * time the group occupies the comm stream, the neighbour's lateness included.  (An event recorded on a stream costs the
 * device ~5 us at its next dispatch: switch it on for a probe pass, not for a timed one.)  _get drains the comm stream. */
enum {
    SPH_SLAB_T_STEPS = 0, SPH_SLAB_T_WAITS_READY = 1,
    SPH_SLAB_T_WAIT = 2,   /* [2] sum, [3] max */
    SPH_SLAB_T_PRE = 4, SPH_SLAB_T_POST = 6, SPH_SLAB_T_HOST = 8,
    SPH_SLAB_T_GROUPS = 10, /* + 3 * (tag - 1): {calls, sum us, max us} for SPH_TAG_MIGRANTS, _HALO_A, _HALO_B, _MIGRANTS_REST */
    SPH_SLAB_T_GROUPS_ONE = 22, /* {calls, sum us, max us} for SPH_TAG_ONE, then for SPH_TAG_ONE_REST (the one-message protocol) */
    SPH_SLAB_T_WORDS = 28
};
int sph_slab_timing_enable(sph_slab* s, int on);
int sph_slab_timing_reset(sph_slab* s);
int sph_slab_timing_get(sph_slab* s, double out[SPH_SLAB_T_WORDS]);
/* on = 1 (default): the fused force pass of the slab's innermost layers (at least six cell layers from either cut; slabs of
 * 11 owned layers and more) is queued IN FRONT of the step's host wait, behind the deep density, on a stream of its own: work
 * that needs nothing from a neighbour keeps the device busy while the migrant message and halo A are on their way, and its
 * tail runs beside the interior launch.  The step's time becomes nearly independent of the links' latency (DESIGN.md
 * section 6, measured on a slab between its periodic images: +3 us per step with fast links, -10 at 20 us per message
 * group, -30 at 40).  For ONE rank per device: ranks that share a GPU (rehearsals over the local / host transports) should
 * switch it off -- their big kernels then run beside each other all the time and evict each other's L2 working sets (two
 * 8.4 M-particle slabs on one GPU: 4.81 against 3.86 ms per step); the launchers do.  The launch covers at most 2^20 slots
 * of those layers (~150 us of k_force: what a link's latency needs; a longer one runs beside the interior launch for its whole
 * length and the two evict each other's L2 working sets -- a 16.7 M-particle slab: 3.90 against 3.69 ms); on > 1 sets that
 * number of slots (environment: SPH_SLAB_EARLY_SPAN).  A slab without neighbours (world 1) never launches it.  Same bits either way.
 * out = {steps that launched it, steps that used its result} (a step whose arrivals re-sort the slab discards it). */
/* [tuning] */ int sph_slab_set_early_force(sph_slab* s, int on);
/* The message protocol of a step.  3 (default): MIGRANTS (header + leavers) -> the host's wait -> HALO A (boundary layers) ->
 * HALO B (their densities), three dependent groups per step.  1: ONE group -- header, leavers and the RESIDENTS of the two
 * cell layers next to each cut in one message per neighbour ("a 2-layer halo, ghost densities recomputed
 * locally (one message)"): the receiver merges its own leavers into the copy (the order the neighbour will give them), computes
 * the densities of the inner ghost layer itself -- same candidates, same order, same bits in fp32 -- and the force pass needs no
 * message.  The message's size is fixed in advance by a rule on the counts both ends saw in the previous step's headers (margin
 * 1/16 + 1024 records, and never more than the message buffers hold: a size the rule puts beyond them is cut down to them,
 * sph_slab_one_clamped counts those steps); what does not fit follows in an exact second message (out[2] counts those); a step
 * whose counts themselves outgrow the buffers is SPH_E_CAPACITY on both ends of that link.  Both ends form the size from the same
 * counts AND their own buffers, so EVERY RANK OF A CHAIN MUST BE CREATED WITH THE SAME ghost capacity (sph_create_slab_layers) AND
 * migrant_capacity (sph_slab_create); the library does not exchange them, and ranks that differ disagree on a message size as
 * soon as a size is cut down (the local transport reports that, RCCL does not).  The first step after
 * sph_slab_create / sph_slab_recut / this call runs the three-group protocol to learn the counts.  Needs a context with two
 * ghost layers (sph_create_slab_layers) and slabs of >= 4 cell layers; a particle that crosses more than TWO layers in a step is
 * SPH_E_STATE under it.  COLLECTIVE in effect: every rank of the chain must run the same protocol.  Price: ~2x the halo bytes and
 * the density of one more layer per side; gain: two message latencies off the step's critical path.
 * Accepted on a SPH_PRECISION_MIXED_F16 context too.  There a ghost's recomputed density is computed in the RECEIVER's waves,
 * not the owner's: it is the owner's value wherever the packed fp16 arithmetic is exact and within the mixed tolerance of it
 * otherwise, so the two ends of a pair may use densities of one particle that differ by that much.  In
 * mixed precision an N-slab run equals the one-context run to the mixed tolerance, not bit for bit, under EITHER protocol
 * (sph_set_precision; tests/test_gpu_slabs_mixed.py).
 * sph_slab_protocol: out = {protocol, one-message steps so far, of which needed the second message}. */
int sph_slab_set_protocol(sph_slab* s, int groups);
/* [introspect] */ int sph_slab_protocol(const sph_slab* s, uint64_t out[3]);
/* [introspect] */ int sph_slab_early_force_stats(const sph_slab* s, uint64_t out[2]);
/* TEST HOOK: sph_upload / sph_set_by_index / sph_reset_lattice / sph_set_params make the next five movers' sorts of a
 * whole-domain context launch BOTH forms (the caller may have changed every particle: the count the device last reported says
 * nothing).  This takes that back, so that a test can put a changed state in front of a sort launched on the old count. */
/* [test hook] */ int sph_test_trust_mover_hint(sph_ctx* c);
/* TEST HOOK: raise sticky device-side error word `flag` (0: an arrival outside its boundary layer, 1: an arrival outside
 * the slab) as the insert / unpack kernels would; the next sph_slab_step then fails before it has sent anything. */
/* [test hook] */ int sph_slab_test_raise_flag(sph_slab* s, int flag);
/* TEST HOOKS: the sequence numbers of the write / wait-value edges (sph_slab_create).  _set_hop_seq drains every stream of the slab
 * (the comm stream under the wait time-out), then sets all five counters and all five words of device memory to `value`, so that
 * a test reaches the switch to events without a week of steps; SPH_E_STATE on a slab that orders its streams by events.  Call it
 * between steps, never from another thread while a call on this slab runs.  _hop_state: out = {1 while the slab orders by value,
 * 0 by events; the five counters}. */
/* [test hook] */ int sph_slab_test_set_hop_seq(sph_slab* s, uint32_t value);
/* [test hook] */ int sph_slab_test_hop_state(const sph_slab* s, uint32_t out[6]);
/* TEST HOOK: what this process's library holds right now: out = {live device bytes, live pinned bytes, live buffers}.  Counted
 * where the library allocates and frees (hipMemGetInfo on a shared card sees everybody's processes): an exact leak check. */
/* [test hook] */ void sph_memory_stats(uint64_t out[3]);
/* TEST HOOK: the k-th device or pinned allocation the library makes from now on returns the ordinary SPH_E_NOMEM -- a host-side
 * return, taken before any HIP call -- once; then the hook is disarmed.  k = 0 disarms it.  Process-wide. */
/* [test hook] */ void sph_test_fail_alloc(uint32_t k);
/* TEST HOOK: the library's one-block prefix sum (every count -> scan -> scatter pipeline uses it) on an array of the caller's:
 * out[i] = in[0] + ... + in[i - 1] and *total = the sum of all n, in unsigned arithmetic of `bits` (32 or 64) bits, wrap-around
 * included.  in, out (n values) and total (one) are host memory; n = 0 writes only *total = 0.  Waits for the result. */
/* [test hook] */ int sph_test_scan(sph_ctx* c, int bits, uint32_t n, const void* in, void* out, void* total);
/* TEST HOOK: the library's binary search (layer bounds, the merges of arrivals and ghosts, the sorts' ranks and the voxeliser's work
 * list all run it) through the lower-bounds kernel of the slab messages, on keys of the caller's: out[k] = the first i in [0, n]
 * with i == n or keys[i] >= targets[k], for k < m.  keys (n values in ascending order; equal keys allowed), targets and out
 * (m <= 32 values each) are host memory.  Waits for the result. */
/* [test hook] */ int sph_test_lower_bounds(sph_ctx* c, const uint32_t* keys, uint32_t n, const uint32_t* targets, uint32_t m, uint32_t* out);
/* TEST HOOK: guarded allocations.  While band_bytes (a multiple of 4096; any other value is refused and changes nothing) is not 0,
 * every device, pinned and mapped allocation the library makes has a band of that many bytes in front of the caller's range and
 * another behind it, filled with a pattern of 32-bit words: nonzero, below 512 (a subnormal as fp32) and varying with the position.
 * With fill_unzeroed the pattern also fills every range the library does not clear itself.  0 bytes: off for the allocations from
 * now on; a buffer keeps the bands it was given, and sph_memory_stats counts the caller's bytes in either mode.  Process-wide. */
/* [test hook] */ void sph_test_guard(uint32_t band_bytes, int fill_unzeroed);
/* TEST HOOK: waits for the device, compares both bands of every live guarded buffer of every owner, adds what the buffers freed
 * since the last check showed when they were freed, and writes the pattern back where it was damaged (the next check is clean).
 * out = {buffers checked, buffers damaged, the caller's bytes of the first damaged one, the byte offset of its first damaged word
 * as an int64: < 0 in front of the caller's range, >= 0 counted from its end}. */
/* [test hook] */ int sph_test_guard_check(uint64_t out[4]);
/* 0, or the first error of this slab: a slab that failed stays failed -- it has told its neighbours (they return
 * SPH_E_PEER at their next step), every later sph_slab_step returns the same error, and the state of its context is that
 * of a half-done step: download / destroy only */
int sph_slab_failed(const sph_slab* s);

#ifdef __cplusplus
}
#endif
#endif /* SPH_HIP_H */

// include/particleSystem.h -- host-side C++ class with the public interface of the reference's
// ParticleSystem (/root/reference/SPH/particleSystem.h:48-112), backed by libsph_hip.so.
//
// A program written against the reference header (its main loop, SPH/particles.cpp:176-192,
// 230-246, 306-318) compiles against this one unchanged: same class name, constructor, enums,
// methods and argument meaning.  Differences, all deliberate:
//   * headless: no OpenGL.  getCurrentReadBuffer()/getColorBuffer() return 0; positions are read
//     with getArray(POSITION) or through getPositionsDevice() (the `gl_pos` analogue).  The
//     reference constructor needs a GL context even in -benchmark mode.
//     Pictures come from the device renderer instead (setCamera / renderFrame / writeFrame, on top of
//     sph_render): the reference's sphere sprites and colour ramp, written as PPM files; or, with setRenderSurface, the
//     fluid as a smoothed surface (sph_render_surface).
//   * only the GPU mode exists: SEQUENTIAL / OMP_PARALLEL abort with a message (no CPU fallback).
//   * the grid follows the box: nextPow2((uint)(boxDims/(0.66666f*h))) per axis; the reference
//     always uses the BOX_SIZE macro, i.e. 32^3 whatever the box (particleSystem.cpp:46, A.2-3).
//   * reset(CONFIG_GRID) builds an exact lattice with a counter-based jitter (see
//     gpufluidsimulator_amd/ic.py); the reference's ceil(powf(N,1/3)) + rand() is not portable.
//   * additive API named by the north star: getArray / setArray / setSimParams, plus
//     getDensities(), getPositionsDevice(), phaseTimings(), saveState()/loadState().
//   * additive: particles enter and leave a running system (addParticles / emitSphere / removeParticles, on top of
//     sph_emit / sph_remove); the reference's particle set is fixed at construction.
//   * errors abort the process like checkCudaErrors (common/inc/helper_cuda.h:566-579).
#ifndef SPH_PARTICLESYSTEM_H
#define SPH_PARTICLESYSTEM_H

#include <cstdint>
#include <string>
#include <vector>

#include "sph_hip.h"

typedef unsigned int uint;

#if !defined(__HIPCC__) && !defined(HIP_INCLUDE_HIP_HIP_VECTOR_TYPES_H) && !defined(__VECTOR_TYPES_H__)
// the two CUDA vector types the reference interface uses (vector_types.h / vector_functions.h)
struct float3 { float x, y, z; };
struct uint3 { unsigned int x, y, z; };
static inline float3 make_float3(float x, float y, float z) { float3 v = {x, y, z}; return v; }
#endif

// SPH/particles_kernel.cuh:36-50, field for field, so that setSimParams() accepts the
// reference's struct.  gravity is carried but, as in the reference, no kernel reads it (SURVEY.md
// A.1); colliderPos / colliderRadius describe the collider sphere, which pushes the fluid while
// enableCollider(true) is set (off by default, as the reference's sphere is inert).
struct SimParams {
    float3 colliderPos;
    float colliderRadius;
    float3 gravity;
    float particleRadius;
    float3 boxMin;
    float3 boxMax;
    float3 boxDims;
    uint gridDim;
};

class ParticleSystem {
public:
    enum ParticleComputeMode {
        SEQUENTIAL,
        OMP_PARALLEL,
        CUDA_PARALLEL,
        HIP_PARALLEL = CUDA_PARALLEL   // what actually runs here
    };

    // Runs on the HIP device chosen with sph_select_device() (default 0), as the reference runs on
    // the device findCudaDevice() made current (`-device=N`).
    ParticleSystem(uint numParticles, float3 boxDims, ParticleComputeMode mode);
    // additive: an explicit grid instead of nextPow2(box / (0.66666 h)) per axis (a 0 keeps the formula)
    ParticleSystem(uint numParticles, float3 boxDims, ParticleComputeMode mode, uint3 gridDims);
    // additive: room for up to `capacity` particles (and creation indices below it), so that addParticles / emitSphere can
    // grow the system; anything below numParticles means numParticles, the fixed size of the other constructors
    ParticleSystem(uint numParticles, float3 boxDims, ParticleComputeMode mode, uint3 gridDims, uint capacity);
    ~ParticleSystem();

    enum ParticleConfig { CONFIG_RANDOM, CONFIG_GRID, _NUM_CONFIGS };
    enum ParticleArray { POSITION, VELOCITY };

    // n = m_solverIterations full time steps; fps is only logged (particleSystem.cpp:720,806)
    void update(float deltaTime, float fps);
    void reset(ParticleConfig config);                                // back to the constructed count, whatever was emitted or removed

    int getNumParticles() const { return (int)m_numParticles; }      // follows the context: addParticles / removeParticles change it
    int getCapacity() const { return (int)m_capacity; }
    unsigned int getCurrentReadBuffer() const { return 0; }   // no GL buffer in headless builds
    unsigned int getColorBuffer() const { return 0; }

    void dumpParticles(uint start, uint count);                       // rows by creation index, up to getCapacity()

    void setIterations(int i) { m_solverIterations = i; }
    void setGravity(float x) { m_params.gravity = make_float3(0.0f, x, 0.0f); }   // a physics no-op, as upstream
    // The collider sphere (sph_set_colliders): inert until enableCollider(true).  While it is enabled, update() hands
    // colliderPos / colliderRadius and the velocity to the context before its steps and reads the advanced centre back
    // into colliderPos after them.
    void setColliderPos(float3 x) { m_params.colliderPos = x; m_bodyLive = false; }
    float3 getColliderPos() { return m_params.colliderPos; }
    float getColliderRadius() { return m_params.colliderRadius; }
    float getParticleRadius() { return m_params.particleRadius; }
    float3 getBoxMin() { return m_params.boxMin; }
    float3 getBoxMax() { return m_params.boxMax; }

    void addSphere(int index, float* pos, float* vel, int r, float spacing);

    // ---- additive: emitters and drains (sph_emit / sph_remove / sph_count_in_regions of sph_hip.h) ---------------------------
    // Append n particles, 4 floats each like getArray (w ignored; vel may be null: at rest).  They take consecutive creation
    // indices from the system's next unused one; the first is returned.  Exceeding the capacity aborts like every error here.
    int addParticles(const float* pos, const float* vel, int n);
    // The lattice points of addSphere (same loops, same jitter stream) around pos[0..2], APPENDED instead of written over
    // existing particles, all with the velocity vel[0..2] (null: at rest).  Returns how many particles that were.
    int emitSphere(const float* pos, const float* vel, int r, float spacing);
    // Delete the particles inside any of the n regions (1..SPH_MAX_REGIONS); returns how many.  getArray() shows zeros in
    // the rows of creation indices that hold no particle.
    int removeParticles(const sph_region* regions, int n);
    int countParticles(const sph_region* regions, int n);      // the same selection, nothing removed

    // ---- additive: the collider sphere pushes the fluid (absent upstream, where it is drawn but inert) -----------------------
    void enableCollider(bool on);
    bool colliderEnabled() const { return m_colliderOn; }
    void setColliderRadius(float r) { m_params.colliderRadius = r; m_bodyLive = false; }
    void setColliderVelocity(float3 u) { m_colliderVel = u; m_bodyLive = false; }     // box units per unit time; kinematic unless the sphere has a mass
    float3 getColliderVelocity() const { return m_colliderVel; }
    // A mass > 0 makes the sphere a free body (sph_set_collider_bodies of sph_hip.h): the fluid pushes it, it falls under
    // `accel` (3 floats; null: none) and bounces off the walls; 0: back to kinematic.  While it is free the context moves it on
    // the device: update() hands the sphere over once -- and again after any of the set* calls above, which re-place it -- and
    // reads centre AND velocity back after its steps.  getColliderImpulse: the momentum the sphere took from the fluid in the
    // last step of the last update().  A KINEMATIC sphere is a sensor too once senseColliderImpulse(true) is set: update() then
    // gives it a body of mass 0 behind every sph_set_colliders (the sphere stays the caller's to move), which starts the tracking
    // anew each time: the context's count of integrates behind the impulse then runs per update(), not since the sensor was
    // switched on.  Zeros before the first update, and for a kinematic sphere without the sensor.
    void setColliderMass(float mass, const float* accel = nullptr);
    float getColliderMass() const { return m_colliderMass; }
    void senseColliderImpulse(bool on) { m_colliderSense = on; m_bodyLive = false; }
    void getColliderImpulse(double out[3]);

    // ---- additive: pictures without OpenGL (sph_render of sph_hip.h; the reference draws with render_particles.cpp) -----------
    // The view of the next renderFrame: an image of width x height, the camera at eye[0..2] looking at target[0..2], up +y.
    // Default: 640 x 480 and the reference's view -- eye (0, 0, 3), the origin, 60 degrees, 0.1 .. 100 (particles.cpp:64-65, 324).
    void setCamera(uint width, uint height, const float* eye, const float* target, float fovyDeg = 60.0f);
    // SPH_COLOR_INDEX (the reference's colouring; the default), or SPH_COLOR_SPEED / SPH_COLOR_DENSITY mapped from [lo, hi]
    void setRenderColor(int mode, float lo = 0.0f, float hi = 1.0f);
    // on: renderFrame draws the fluid as a surface (sph_render_surface: smoothed depth, normals, thickness, a water-like
    // shading) in the style *s (nullptr: sph_surface_defaults); off (the default): the sphere sprites of sph_render.
    void setRenderSurface(bool on, const sph_surface_style* s = nullptr);
    // on: renderFrame also draws the installed obstacle slots (sph_render_set_solids: their distance grids ray-marched into
    // either picture) in the style *s (nullptr: sph_solid_defaults); off (the default): the fluid alone.
    void setRenderSolids(bool on, const sph_solid_style* s = nullptr);
    // Queue one render of the particles as they are (asynchronous, no copy of the state); getFrameDevice: its RGBA8 image on
    // the device.  writeFrame: the last rendered image as a binary PPM (P6, RGB, no alpha), rows top to bottom.
    void renderFrame();
    void* getFrameDevice(uint* width, uint* height);
    void writeFrame(const char* path);

    // ---- additive: geometry (sph_mesh_extract of sph_hip.h; the reference has nothing here) ----------------------------------
    // The parameters of the next extractMesh / writeMeshOBJ (nullptr: sph_mesh_defaults -- spacing = the particle radius,
    // radius = three spacings, iso = 0.5).
    void setMeshParams(const sph_mesh_params* p = nullptr);
    // The surface of the particles as they are, extracted on the device: 3 floats per vertex, 3 per normal, 3 vertex numbers
    // per triangle, in the fixed order of the rule; returns the number of triangles.  Waits for the device.
    uint extractMesh(std::vector<float>& pos, std::vector<float>& nrm, std::vector<uint32_t>& tri);
    // Extract, and write a Wavefront OBJ (sph_mesh_save_obj).
    void writeMeshOBJ(const char* path);

    // ---- additive: solid obstacles of any shape (sph_obstacle_build of sph_hip.h; the reference has nothing here) -----------
    // The union of n analytic shapes, rasterised on the device over the whole box at `spacing` (0: the particle diameter; bounds
    // of nullptr: the box) and installed as the context's obstacle: every later update pushes the particles out of it.
    void setObstacles(const sph_shape* shapes, uint n, float spacing = 0.f, const float* lo = nullptr, const float* hi = nullptr);
    // The caller's own signed distances (a voxelised mesh): dims[0]*dims[1]*dims[2] floats, x fastest, negative inside.
    void setObstacleGrid(const sph_obstacle_grid& grid, const float* phi);
    // Offset and velocity of the grid (either may be nullptr = keep): the offset advances by dt * velocity once per step.
    void setObstacleMotion(const float* offset, const float* velocity);
    void clearObstacles();
    // A closed triangle mesh (nv xyz triples, nt index triples) voxelised on the device into a signed distance `band` nodes wide
    // (0: 3) and installed like the grid above (sph_obstacle_build_mesh); invert: the fluid is inside the mesh.
    void setObstacleMesh(const float* pos, uint nv, const uint* tri, uint nt, float spacing = 0.f, uint band = 0, bool invert = false,
                         const float* lo = nullptr, const float* hi = nullptr);
    // The same from a Wavefront OBJ file (sph_obstacle_build_obj).
    void setObstacleMeshOBJ(const char* path, float spacing = 0.f, uint band = 0, bool invert = false, const float* lo = nullptr,
                            const float* hi = nullptr);
    // used, skipped, lost crossings, odd columns of the mesh-built obstacle: a closed mesh gives out[2] = out[3] = 0
    void getObstacleMeshStats(uint64_t out[4]);
    // The obstacle as a rigid body that turns (sph_obstacle_set_pose): pivot a point of the grid's own frame, quat = (w, x, y, z)
    // body -> world about it, omega the angular velocity in world axes (nullptr: 0); the pose advances once per step.
    void setObstaclePose(const float pivot[3], const float quat[4], const float* omega = nullptr);
    void clearObstaclePose();
    // The load sensor (sph_obstacle_set_sensor / _get_load): J and L are the momentum and the angular momentum about the
    // pivot's place in the world that the obstacle took from the fluid in the last update; divide by the time step.
    void senseObstacleLoad(bool on);
    void getObstacleLoad(double J[3], double L[3]);
    // A free body (sph_obstacle_set_body): from then on the fluid drives the motions in body.dof on the device, inside update(),
    // with no host wait.  The selected obstacle needs a pose (setObstaclePose; the identity quaternion will do).
    // getObstacleState reads where a body (or a kinematic obstacle) is now; any pointer may be nullptr.  clearObstacleBody: the
    // obstacle goes on kinematic from where it is.
    void setObstacleBody(const sph_obstacle_body& body);
    void clearObstacleBody();
    void getObstacleState(float offset[3], float velocity[3], double quat[4], float omega[3]);
    // Several obstacles (sph_obstacle_select): the context holds SPH_MAX_OBSTACLES slots, and every obstacle member above
    // addresses the selected one (0 by default; clearObstacles() clears the selected slot).  They act in ascending slot order.
    void selectObstacle(uint slot);
    uint selectedObstacle();
    void clearAllObstacles();

    // ---- additive (absent upstream; named by BASELINE.json's north star) ------------------------
    // 4 floats per particle, by creation index (the original NVIDIA sample's layout), getCapacity() rows; the pointer
    // stays valid until the next getArray call.
    float* getArray(ParticleArray array);
    void setArray(ParticleArray array, const float* data, int start, int count);
    void setSimParams(const SimParams& p);
    const SimParams& getSimParams() const { return m_params; }
    const float* getDensities();                    // density per creation index
    void* getPositionsDevice();                     // device float4 (x,y,z,1) per creation index
    uint3 getGridSize() const { return m_grid; }
    sph_ctx* context() { return m_ctx; }
    // device-accurate per-phase times in ms since the last call (names as in dumpBenchmark)
    void enablePhaseTimings(bool on);
    bool phaseTimings(float ms[SPH_PH_COUNT], uint* steps);
    // checkpoint / resume (sph_snapshot_save / sph_snapshot_load); a resumed run is bit-identical
    void saveState(const std::string& path);
    void loadState(const std::string& path);
    // opt-in text log in the reference's dumpBenchmark format (particleSystem.cpp:697-716).  Two line styles, because the
    // reference has two: LOG_FRAMES is what its current source writes ("<int>sec ... frames:<n>frames"), LOG_OSCAR is the
    // form of its 18 committed logs (benchmarks/oscar/<N>/*.txt: "2.005sec ... FPS:189.322fps"), which is the only form its
    // benchmark.py:12 regex reads -- so a log written in that style can be summarised next to the published ones
    // (tools/bench_log_summary.py reads both).
    enum BenchmarkLogStyle { LOG_FRAMES = 0, LOG_OSCAR = 1 };
    void setBenchmarkLog(const std::string& path, double min_interval_ms = 2000.0 /* BENCHMARK_FREQ */,
                         BenchmarkLogStyle style = LOG_FRAMES);

protected:
    void _initialize(int numParticles);
    void _finalize();
    void uploadAll();
    void downloadAll();
    std::vector<float> spherePoints(const float* pos, int r, float spacing, uint limit);

    bool m_bInitialized;
    uint m_numParticles;
    uint m_numInitial;                               // what the constructor was given: reset() goes back to it
    uint m_capacity;                                 // rows of the by-index mirrors = capacity of the context
    std::vector<float> m_hPos, m_hVel, m_hDens;     // host mirrors: xyzw, xyzw, scalar
    std::vector<float> m_xyz, m_vxyz;                // packed xyz staging for the C ABI
    std::vector<uint32_t> m_live;                    // creation indices of the owned particles (downloadAll)
    SimParams m_params;
    float3 m_boxDims;
    uint3 m_grid;
    uint m_solverIterations;
    ParticleComputeMode m_compute_mode;
    sph_ctx* m_ctx;
    bool m_colliderOn;
    float3 m_colliderVel;
    float m_colliderMass;        // 0: kinematic
    float m_colliderAccel[3];
    bool m_colliderSense;        // a kinematic sphere gets a body of mass 0, for its impulse
    bool m_bodyLive;             // the context holds a body for the sphere (mass > 0: its centre and velocity are the device's)
    bool m_hostStale;
    sph_camera m_camera;
    sph_render_style m_renderStyle;
    bool m_surfaceOn;
    sph_surface_style m_surfaceStyle;
    std::vector<unsigned char> m_frame;              // RGBA staging of writeFrame
    sph_mesh_params m_meshParams;
    std::string m_logPath;
    void* m_log;
    double m_logLastMs, m_logGlobalMs, m_logFreqMs;
    int m_logStyle;
    unsigned long long m_logFrames;
};

extern "C" {
// Host-only twins of gpufluidsimulator_amd/ic.py (bit-identical output); no GPU needed.
void sph_ic_dam_break(const uint32_t lattice[3], const float box[3], int jitter, uint64_t start, uint64_t count,
                      float* pos_xyz, float* vel_xyz);
void sph_ic_random_box(uint64_t n, const float box[3], float speed, uint32_t seed, float fill, float* pos_xyz,
                       float* vel_xyz);
}

#endif  // SPH_PARTICLESYSTEM_H

// sph_obstacle.hip -- solid obstacles of any shape: grids of signed distances, one per obstacle slot of a whole-domain context,
// which the fluid collides with (sph_obstacle_lattice, _build, _set_grid, _clear, _set_motion, _get, _read, _sample, _select of
// include/sph_hip.h, which states the rule).  The reference has no counterpart.  A grid voxelised from a triangle mesh (sph_obstacle_mesh.hip) is installed
// through install_begin / install_finish below and is then this file's like any other.
//
//   k_obstacle_raster  one node per lane: the union of the analytic shapes, clamped                         (sph_obstacle_build)
//   k_obstacle_clamp   one node per lane: the clamp of an uploaded field                                    (sph_obstacle_set_grid)
//   k_obstacle_bricks  one brick of OBSTACLE_BRICK^3 cells per lane: the minimum over its (OBSTACLE_BRICK + 1)^3 nodes
//   k_obstacle_sample  one caller point per lane: the sample rule                                           (sph_obstacle_sample)
//   k_solid_march      one pixel per lane: the drawn slots ray-marched into a picture by that rule           (sph_render_set_solids)
//   k_obstacle_push    one owned slot per lane, behind every integrate of a context with an obstacle: the push; <POSED> for a
//                      solid that turns (sph_obstacle_set_pose), <SENSE> leaves the waves' sums of what the solid took
//   k_obstacle_push_set  the same for every installed set of slots but {slot 0}: the slots in ascending order, in one launch
//   k_obstacle_load    one block per sensing slot behind a sensing push: the waves' sums in a fixed order                    (sph_obstacle_get_load)
//   k_obstacle_body    one thread per BODY slot behind its load sum: J and L move the slot's device block on by dt           (sph_obstacle_set_body)
//   k_obstacle_body_put  one thread: what set_body, set_motion and set_pose write into that block, by value
// A BODY slot's push, sample and march are instantiations of the kernels above that read the block at entry (ob_overlay).
//
// The push is a pass of its own and not a fourth pack of k_force / k_integrate (sph_pairs.hip): the fused kernel sits at the edge
// of its occupancy, and an eight-node gather in its epilogue would cost it.  Reading the integrate's STORED output is also what
// makes the result equal tests/obstacle_model.py bit for bit.  Everything of the rule is fp32 with each operation rounded (fp
// contract off, IEEE division and square root).
#include "sph_device.hpp"

#include <cmath>
#include <cstring>
#include <type_traits>

namespace sph {

constexpr uint32_t OBSTACLE_THREADS = 256;
constexpr uint32_t OBSTACLE_BRICK_SH = 2;                         // a brick is 4 x 4 x 4 cells
constexpr uint32_t OBSTACLE_BRICK = 1u << OBSTACLE_BRICK_SH;
static_assert(OBSTACLE_THREADS % WAVE == 0, "a wave of the push is one 64-slot chunk of the movers' marks");

// the grid, its motion and its buffers as the kernels take them: by value
struct ObstacleArgs {
    const float* phi;
    const float* brick;
    float origin[3];
    float s;
    uint32_t n[3];
    float nm1[3];          // (float)(n - 1)
    uint32_t nb[3];        // bricks per axis: ceil((n - 1) / OBSTACLE_BRICK)
    float off[3], u[3];
};

// The rigid pose and the sensor's buffers as the push and the sample take them: by value, and as the LAST kernel argument rather
// than as fields of ObstacleArgs, so that the arguments of the plain instantiation keep their offsets and its code its text.
struct ObstaclePose {
    float rot[9];          // body -> world, row-major
    float pivot[3];        // a point of the body frame
    float P[3];            // the same point in the world: pivot + off (an unposed context: off)
    float omega[3];        // world axes
    double* rows;          // the sensor: six sums per wave
    uint32_t* mask;        // ... and whether the wave wrote them
};

// A BODY slot (sph_obstacle_set_body): the pose travels as for a posed slot, and the block's pointer behind it.  The BODY
// instantiations take this as their last argument; the others keep ObstaclePose, argument for argument.
struct ObstaclePoseBody {
    ObstaclePose X;
    const ObstacleBodyBlock* blk;
};
template <bool BODY> using PoseArg = std::conditional_t<BODY, ObstaclePoseBody, ObstaclePose>;
__device__ __forceinline__ ObstaclePose& pose_of(ObstaclePose& X) { return X; }
__device__ __forceinline__ ObstaclePose& pose_of(ObstaclePoseBody& X) { return X.X; }
__device__ __forceinline__ const ObstacleBodyBlock* block_of(const ObstaclePose&) { return nullptr; }
__device__ __forceinline__ const ObstacleBodyBlock* block_of(const ObstaclePoseBody& X) { return X.blk; }

// the shapes of one build: a kernel argument by value, like Spheres (the half-spaces' normals already normalised)
struct Shapes {
    sph_shape s[SPH_MAX_SHAPES];
    uint32_t n;
};

__device__ __forceinline__ float ob_lerp(float p, float q, float t) {
#pragma clang fp contract(off)
    return p + t * (q - p);
}

// The overlay of a BODY slot, at kernel entry: what the host holds of off, u, rot, P, pivot and omega is stale, the block has
// them.  The address is the same for every lane, so these are scalar loads; everything behind them is the posed arithmetic.
__device__ __forceinline__ void ob_overlay(ObstacleArgs& A, ObstaclePose& X, const ObstacleBodyBlock* __restrict__ b) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        A.off[k] = b->off[k]; A.u[k] = b->u[k];
        X.pivot[k] = b->pivot[k]; X.P[k] = b->P[k]; X.omega[k] = b->omega[k];
    }
#pragma unroll
    for (int k = 0; k < 9; k++) X.rot[k] = b->rot[k];
}

// the cell of x and the fractions inside it; false: outside the grid (NaN and +-inf too)
__device__ __forceinline__ bool ob_locate(const ObstacleArgs& A, float x, float y, float z, uint32_t i[3], float f[3]) {
#pragma clang fp contract(off)
    const float g0 = ((x - A.off[0]) - A.origin[0]) / A.s;
    const float g1 = ((y - A.off[1]) - A.origin[1]) / A.s;
    const float g2 = ((z - A.off[2]) - A.origin[2]) / A.s;
    if (!(g0 >= 0.f) || !(g0 < A.nm1[0]) || !(g1 >= 0.f) || !(g1 < A.nm1[1]) || !(g2 >= 0.f) || !(g2 < A.nm1[2])) return false;
    const int i0 = (int)g0, i1 = (int)g1, i2 = (int)g2;
    i[0] = (uint32_t)i0; i[1] = (uint32_t)i1; i[2] = (uint32_t)i2;
    f[0] = g0 - (float)i0; f[1] = g1 - (float)i1; f[2] = g2 - (float)i2;
    return true;
}

// the same on a posed context: d = x - P, the body-frame point R^T d + pivot, its cell.  d stays with the caller (omega x d,
// the torque's arm)
__device__ __forceinline__ bool ob_locate_posed(const ObstacleArgs& A, const ObstaclePose& X, float x, float y, float z, uint32_t i[3],
                                                float f[3], float d[3]) {
#pragma clang fp contract(off)
    const float d0 = x - X.P[0], d1 = y - X.P[1], d2 = z - X.P[2];
    d[0] = d0; d[1] = d1; d[2] = d2;
    const float q0 = ((X.rot[0] * d0 + X.rot[3] * d1) + X.rot[6] * d2) + X.pivot[0];
    const float q1 = ((X.rot[1] * d0 + X.rot[4] * d1) + X.rot[7] * d2) + X.pivot[1];
    const float q2 = ((X.rot[2] * d0 + X.rot[5] * d1) + X.rot[8] * d2) + X.pivot[2];
    const float g0 = (q0 - A.origin[0]) / A.s;
    const float g1 = (q1 - A.origin[1]) / A.s;
    const float g2 = (q2 - A.origin[2]) / A.s;
    if (!(g0 >= 0.f) || !(g0 < A.nm1[0]) || !(g1 >= 0.f) || !(g1 < A.nm1[1]) || !(g2 >= 0.f) || !(g2 < A.nm1[2])) return false;
    const int i0 = (int)g0, i1 = (int)g1, i2 = (int)g2;
    i[0] = (uint32_t)i0; i[1] = (uint32_t)i1; i[2] = (uint32_t)i2;
    f[0] = g0 - (float)i0; f[1] = g1 - (float)i1; f[2] = g2 - (float)i2;
    return true;
}

template <bool POSED>
__device__ __forceinline__ bool ob_locate_at(const ObstacleArgs& A, const ObstaclePose& X, float x, float y, float z, uint32_t i[3],
                                             float f[3], float d[3]) {
    if constexpr (POSED) return ob_locate_posed(A, X, x, y, z, i, f, d);
    else return ob_locate(A, x, y, z, i, f);
}

// the body normal of a posed context in world axes (not renormalised)
__device__ __forceinline__ void ob_world_normal(const ObstaclePose& X, float& nx, float& ny, float& nz) {
#pragma clang fp contract(off)
    const float b0 = nx, b1 = ny, b2 = nz;
    nx = (X.rot[0] * b0 + X.rot[1] * b1) + X.rot[2] * b2;
    ny = (X.rot[3] * b0 + X.rot[4] * b1) + X.rot[5] * b2;
    nz = (X.rot[6] * b0 + X.rot[7] * b1) + X.rot[8] * b2;
}

// lane l's value of a float64, as lane_value of sph_pairs.hip reads a float: two 32-bit readlanes
__device__ __forceinline__ double lane_value_f64(double v, uint32_t l) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), (int)l);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// phi and the unit normal in a cell: the eight-node gather (i[k] <= n[k] - 2, so every node is inside the array)
__device__ __forceinline__ void ob_sample_cell(const ObstacleArgs& A, const uint32_t i[3], const float f[3], float& phi, float& nx,
                                               float& ny, float& nz) {
#pragma clang fp contract(off)
    const uint32_t sy = A.n[0], sz = A.n[0] * A.n[1];
    const float* __restrict__ p = A.phi + ((size_t)i[2] * A.n[1] + i[1]) * A.n[0] + i[0];
    const float P000 = p[0], P100 = p[1], P010 = p[sy], P110 = p[sy + 1u];
    const float P001 = p[sz], P101 = p[sz + 1u], P011 = p[sz + sy], P111 = p[sz + sy + 1u];
    const float fx = f[0], fy = f[1], fz = f[2];
    phi = ob_lerp(ob_lerp(ob_lerp(P000, P100, fx), ob_lerp(P010, P110, fx), fy),
                  ob_lerp(ob_lerp(P001, P101, fx), ob_lerp(P011, P111, fx), fy), fz);
    const float gx = ob_lerp(ob_lerp(P100 - P000, P110 - P010, fy), ob_lerp(P101 - P001, P111 - P011, fy), fz);
    const float gy = ob_lerp(ob_lerp(P010 - P000, P110 - P100, fx), ob_lerp(P011 - P001, P111 - P101, fx), fz);
    const float gz = ob_lerp(ob_lerp(P001 - P000, P101 - P100, fx), ob_lerp(P011 - P010, P111 - P110, fx), fy);
    const float len2 = (gx * gx + gy * gy) + gz * gz;
    nx = 0.f; ny = 1.f; nz = 0.f;
    if (len2 > 0.f && len2 < INFINITY) {
        const float len = sqrtf(len2);
        nx = gx / len; ny = gy / len; nz = gz / len;
    }
}

// ---- the push ---------------------------------------------------------------------------------------------------------------
// One owned slot per lane, blocks of OBSTACLE_THREADS from the first owned slot: a wave is one 64-slot chunk of the marks.
// Nearly every wave is nowhere near a solid, so the kernel should cost what reading the positions costs: a lane reads its
// position (16 bytes), finds its cell and reads ONE word, the minimum of phi over the nodes of its brick.  WHY THAT IS ENOUGH:
// a lerp p + t * (q - p), 0 <= t < 1, lies between p and q but for its three roundings, each at most an ulp of 2 D (every phi is
// clamped to [-D, D], D <= 6144 s): about 7e-4 s apiece, under 0.01 s over the three levels.  So where the brick's minimum is
// at least eps + 0.25 s the interpolated phi is above eps, the rule's first iteration stops with `!(phi < eps)` and the particle
// is not touched -- whatever field the caller uploaded.  A wave in which no lane can be in contact (one ballot) leaves after 20
// bytes per lane.  The guard only ever SKIPS work whose outcome is known: the lanes it lets through run the rule as written,
// every later iteration with a full sample (the particle has moved).
// Fused (keys_out != null): a particle with `hit` also gets the next step's key, and, where the launch marked the movers, the
// wave's mask word is put right -- bit = (key != keyS[slot]) for the lanes that hit -- and the tile's count takes the difference
// of the popcounts with one integer atomic add (force_finish scans the counts afterwards).
// POSED (sph_obstacle_set_pose): the sample goes through the body frame and the solid's velocity at the particle is
// u + omega x d; the brick guard is applied to the body-frame cell and holds as it is.  SENSE (sph_obstacle_set_sensor): a lane
// that takes `wn < 0` also forms t = -(mass * (k * n)) and d x t and adds them, iteration by iteration, to six float64 sums of
// its own; the wave then adds its kicked lanes' sums in ascending lane order -- two scalar-indexed 32-bit reads per value, as
// push_out_of_spheres(..., SpheresTracked) reads its floats, no LDS, no atomics -- and lane 0 stores the row.  EVERY wave that
// owns a slot stores its mask word, 0 where it leaves at the guard's ballot, so k_obstacle_load never reads a row of an earlier
// launch.  <false, false> is the kernel without either, operation for operation.  BODY (sph_obstacle_set_body; only
// <true, true, true>): the overlay at entry, then <true, true> operation for operation.
template <bool POSED, bool SENSE, bool BODY = false>
__global__ __launch_bounds__(OBSTACLE_THREADS) void k_obstacle_push(float4* __restrict__ posi, float4* __restrict__ velr,
                                                                    float4* __restrict__ pos_by_index,
                                                                    uint32_t* __restrict__ keys_out,
                                                                    const uint32_t* __restrict__ keyS,
                                                                    uint64_t* __restrict__ mm_mask,
                                                                    uint32_t* __restrict__ mm_tile_cnt, uint32_t lo, uint32_t n,
                                                                    ObstacleArgs A, GridDesc g, Phys ph, PoseArg<BODY> Xa) {
#pragma clang fp contract(off)
    static_assert(!BODY || (POSED && SENSE), "a body slot is posed and sensing");
    ObstaclePose& X = pose_of(Xa);
    if constexpr (BODY) ob_overlay(A, X, block_of(Xa));
    const uint32_t rel = blockIdx.x * OBSTACLE_THREADS + threadIdx.x;
    const bool active = rel < n;
    const uint32_t slot = lo + (active ? rel : n - 1u);
    float4 pi = posi[slot];
    const float eps = ph.wall_eps;
    const float guard = eps + 0.25f * A.s;
    uint32_t ci[3];
    float cf[3], d[3];
    bool may = false;
    if (active && ob_locate_at<POSED>(A, X, pi.x, pi.y, pi.z, ci, cf, d)) {
        const uint32_t b = ((ci[2] >> OBSTACLE_BRICK_SH) * A.nb[1] + (ci[1] >> OBSTACLE_BRICK_SH)) * A.nb[0] + (ci[0] >> OBSTACLE_BRICK_SH);
        may = A.brick[b] < guard;
    }
    [[maybe_unused]] const bool row_owner = active && (threadIdx.x & 63u) == 0u;     // (lane 0 of a wave that owns a slot)
    if (__ballot(may) == 0ull) {                                         // wave-uniform: nearly every wave
        if constexpr (SENSE) { if (row_owner) X.mask[rel >> 6] = 0u; }
        return;
    }
    bool hit = false;
    float4 vi = make_float4(0.f, 0.f, 0.f, 0.f);
    [[maybe_unused]] double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    [[maybe_unused]] bool kicked = false;
    if (may) {
        vi = velr[slot];
        for (int it = 0; it < SPH_OBSTACLE_PUSH_ITERATIONS; it++) {
            if (it > 0 && !ob_locate_at<POSED>(A, X, pi.x, pi.y, pi.z, ci, cf, d)) break;
            float phi, nx, ny, nz;
            ob_sample_cell(A, ci, cf, phi, nx, ny, nz);
            if (!(phi < eps)) break;
            if constexpr (SENSE && !POSED) { d[0] = pi.x - A.off[0]; d[1] = pi.y - A.off[1]; d[2] = pi.z - A.off[2]; }
            float us0 = A.u[0], us1 = A.u[1], us2 = A.u[2];
            if constexpr (POSED) {
                ob_world_normal(X, nx, ny, nz);
                us0 = A.u[0] + (X.omega[1] * d[2] - X.omega[2] * d[1]);
                us1 = A.u[1] + (X.omega[2] * d[0] - X.omega[0] * d[2]);
                us2 = A.u[2] + (X.omega[0] * d[1] - X.omega[1] * d[0]);
            }
            const float wn = ((vi.x - us0) * nx + (vi.y - us1) * ny) + (vi.z - us2) * nz;
            if (wn < 0.f) {
                const float k = (ph.wall_damping - 1.f) * wn;
                if constexpr (!SENSE) {
                    vi.x = vi.x + k * nx; vi.y = vi.y + k * ny; vi.z = vi.z + k * nz;
                } else {
                    const float kx = k * nx, ky = k * ny, kz = k * nz;
                    vi.x = vi.x + kx; vi.y = vi.y + ky; vi.z = vi.z + kz;
                    const float t0 = -(ph.mass * kx), t1 = -(ph.mass * ky), t2 = -(ph.mass * kz);
                    acc[0] = acc[0] + (double)t0; acc[1] = acc[1] + (double)t1; acc[2] = acc[2] + (double)t2;
                    acc[3] = acc[3] + ((double)d[1] * (double)t2 - (double)d[2] * (double)t1);
                    acc[4] = acc[4] + ((double)d[2] * (double)t0 - (double)d[0] * (double)t2);
                    acc[5] = acc[5] + ((double)d[0] * (double)t1 - (double)d[1] * (double)t0);
                    kicked = true;
                }
            }
            const float t = eps - phi;
            pi.x = pi.x + t * nx; pi.y = pi.y + t * ny; pi.z = pi.z + t * nz;
            hit = true;
        }
    }
    if constexpr (SENSE) {
        const uint64_t km = __ballot(kicked);
        if (km != 0ull) {                                                // wave-uniform
            double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (uint64_t m = km; m != 0ull; m &= m - 1ull) {
                const uint32_t l = (uint32_t)__builtin_ctzll(m);
#pragma unroll
                for (int a = 0; a < 6; a++) sum[a] = sum[a] + lane_value_f64(acc[a], l);
            }
            if (row_owner) {
                double* row = X.rows + (size_t)(rel >> 6) * 6u;
#pragma unroll
                for (int a = 0; a < 6; a++) row[a] = sum[a];
            }
        }
        if (row_owner) X.mask[rel >> 6] = km != 0ull ? 1u : 0u;
    }
    bool moved = false;
    if (hit) {
        wall(pi.x, vi.x, ph.box_min[0], ph.box_max[0], eps, ph.wall_damping);
        wall(pi.y, vi.y, ph.box_min[1], ph.box_max[1], eps, ph.wall_damping);
        wall(pi.z, vi.z, ph.box_min[2], ph.box_max[2], eps, ph.wall_damping);
        posi[slot] = pi;
        velr[slot] = vi;
        pos_by_index[__float_as_uint(pi.w)] = make_float4(pi.x, pi.y, pi.z, 1.0f);
        if (keys_out) {
            const uint32_t key = cell_key(g, pi.x, pi.y, pi.z);
            keys_out[rel] = key;
            moved = key != keyS[slot];
        }
    }
    if (mm_mask) {
        const uint64_t hm = __ballot(hit);
        if (hm != 0ull) {                                                // wave-uniform
            const uint64_t mv = __ballot(moved);                         // (a subset of hm)
            if ((threadIdx.x & 63u) == 0u) {                             // (lane 0 of a wave that got here owns a slot)
                const uint32_t chunk = rel >> 6;
                const uint64_t old = mm_mask[chunk], now = (old & ~hm) | mv;
                if (now != old) {
                    mm_mask[chunk] = now;
                    atomicAdd(&mm_tile_cnt[chunk / MM_TILE_CHUNKS], (uint32_t)__popcll(now) - (uint32_t)__popcll(old));
                }
            }
        }
    }
}

// ---- the push of a set of slots ---------------------------------------------------------------------------------------------------
// Every installed set but {slot 0}: ONE launch, the installed slots in ascending order on each owned particle, slot j on what
// slot j - 1 left (include/sph_hip.h: SEVERAL OBSTACLES).  The slots travel by value in one kernel argument and are only ever
// indexed by the constant of an unrolled loop, so they stay in scalar registers and never reach scratch.
//   * a lane reads its position once and one brick word per installed slot; one ballot over "any slot may touch" lets a wave that
//     is near nothing leave after 16 + 4 K bytes per lane, a 0 mask word stored for each sensing slot;
//   * otherwise the lane loads its velocity once and goes through the slots; a slot no lane can touch is skipped wave-uniformly;
//   * a lane that an earlier slot moved takes the later slot's guard from where it is NOW (its first look-up is stale);
//   * posed or not is a wave-uniform branch per slot, each side the arithmetic of k_obstacle_push<POSED> (the identity pose is
//     not the unposed rule); the wall rule runs behind the iterations of every slot that hit, as in a pass of its own;
//   * a sensing slot's six lane sums are reduced in ascending lane order and stored right behind its iterations;
//   * position, velocity, by-index row, key and the marks' fix-up (with the union of the hits) are stored once, at the end.
//   * BODY (a set in which some slot has a body; an instantiation of its own, so that every other set runs the code it ran
//     before): a slot with OB_SLOT_BODY takes the overlay at kernel entry, a kernel-uniform branch per slot, scalar loads.
constexpr uint32_t OB_SLOT_INSTALLED = 1u, OB_SLOT_POSED = 2u, OB_SLOT_SENSE = 4u, OB_SLOT_BODY = 8u;
struct ObstacleSlot {
    ObstacleArgs A;
    ObstaclePose X;
    uint32_t flags;
};
struct ObstacleSet { ObstacleSlot s[SPH_MAX_OBSTACLES]; };
struct ObstacleSetBody {               // the BODY instantiations' argument: the set, and the blocks of its OB_SLOT_BODY slots
    ObstacleSet set;
    const ObstacleBodyBlock* blk[SPH_MAX_OBSTACLES];
};
static_assert(sizeof(ObstacleSetBody) <= 1024, "the slots are one kernel argument");
template <bool BODY> using SetArg = std::conditional_t<BODY, ObstacleSetBody, ObstacleSet>;
__device__ __forceinline__ ObstacleSet& set_of(ObstacleSet& S) { return S; }
__device__ __forceinline__ ObstacleSet& set_of(ObstacleSetBody& S) { return S.set; }

__device__ __forceinline__ void ob_set_overlay(ObstacleSet&) {}
__device__ __forceinline__ void ob_set_overlay(ObstacleSetBody& S) {
#pragma unroll
    for (int k = 0; k < SPH_MAX_OBSTACLES; k++)
        if (S.set.s[k].flags & OB_SLOT_BODY) ob_overlay(S.set.s[k].A, S.set.s[k].X, S.blk[k]);      // kernel-uniform
}

// the guard of one slot at (x, y, z): inside the grid and the brick's minimum under eps + 0.25 s
template <bool POSED>
__device__ __forceinline__ bool ob_slot_may(const ObstacleSlot& S, float guard, float x, float y, float z) {
    uint32_t ci[3];
    float cf[3], d[3];
    if (!ob_locate_at<POSED>(S.A, S.X, x, y, z, ci, cf, d)) return false;
    const uint32_t b = ((ci[2] >> OBSTACLE_BRICK_SH) * S.A.nb[1] + (ci[1] >> OBSTACLE_BRICK_SH)) * S.A.nb[0] + (ci[0] >> OBSTACLE_BRICK_SH);
    return S.A.brick[b] < guard;
}

// the iterations of one slot on the lanes with `may`, as k_obstacle_push<POSED, .> writes them (its first iteration reuses the
// guard's cell; locating again at the same position gives the same cell).  true: the slot hit the lane
template <bool POSED, bool SENSE>
__device__ __forceinline__ bool ob_slot_iterate(const ObstacleSlot& S, const Phys& ph, bool may, bool sense, float4& pi, float4& vi,
                                                double acc[6], bool& kicked) {
#pragma clang fp contract(off)
    const ObstacleArgs& A = S.A;
    const ObstaclePose& X = S.X;
    const float eps = ph.wall_eps;
    bool hit = false;
    if (may) {
        for (int it = 0; it < SPH_OBSTACLE_PUSH_ITERATIONS; it++) {
            uint32_t ci[3];
            float cf[3], d[3];
            if (!ob_locate_at<POSED>(A, X, pi.x, pi.y, pi.z, ci, cf, d)) break;
            float phi, nx, ny, nz;
            ob_sample_cell(A, ci, cf, phi, nx, ny, nz);
            if (!(phi < eps)) break;
            if constexpr (SENSE && !POSED) { d[0] = pi.x - A.off[0]; d[1] = pi.y - A.off[1]; d[2] = pi.z - A.off[2]; }
            float us0 = A.u[0], us1 = A.u[1], us2 = A.u[2];
            if constexpr (POSED) {
                ob_world_normal(X, nx, ny, nz);
                us0 = A.u[0] + (X.omega[1] * d[2] - X.omega[2] * d[1]);
                us1 = A.u[1] + (X.omega[2] * d[0] - X.omega[0] * d[2]);
                us2 = A.u[2] + (X.omega[0] * d[1] - X.omega[1] * d[0]);
            }
            const float wn = ((vi.x - us0) * nx + (vi.y - us1) * ny) + (vi.z - us2) * nz;
            if (wn < 0.f) {
                const float k = (ph.wall_damping - 1.f) * wn;
                const float kx = k * nx, ky = k * ny, kz = k * nz;
                vi.x = vi.x + kx; vi.y = vi.y + ky; vi.z = vi.z + kz;
                if constexpr (SENSE) {
                    if (sense) {                                         // wave-uniform
                        const float t0 = -(ph.mass * kx), t1 = -(ph.mass * ky), t2 = -(ph.mass * kz);
                        acc[0] = acc[0] + (double)t0; acc[1] = acc[1] + (double)t1; acc[2] = acc[2] + (double)t2;
                        acc[3] = acc[3] + ((double)d[1] * (double)t2 - (double)d[2] * (double)t1);
                        acc[4] = acc[4] + ((double)d[2] * (double)t0 - (double)d[0] * (double)t2);
                        acc[5] = acc[5] + ((double)d[0] * (double)t1 - (double)d[1] * (double)t0);
                        kicked = true;
                    }
                }
            }
            const float t = eps - phi;
            pi.x = pi.x + t * nx; pi.y = pi.y + t * ny; pi.z = pi.z + t * nz;
            hit = true;
        }
    }
    return hit;
}

template <bool SENSE, bool BODY = false>
__global__ __launch_bounds__(OBSTACLE_THREADS) void k_obstacle_push_set(float4* __restrict__ posi, float4* __restrict__ velr,
                                                                        float4* __restrict__ pos_by_index,
                                                                        uint32_t* __restrict__ keys_out,
                                                                        const uint32_t* __restrict__ keyS,
                                                                        uint64_t* __restrict__ mm_mask,
                                                                        uint32_t* __restrict__ mm_tile_cnt, uint32_t lo, uint32_t n,
                                                                        GridDesc g, Phys ph, SetArg<BODY> seta) {
#pragma clang fp contract(off)
    static_assert(!BODY || SENSE, "a body slot is sensing");
    ob_set_overlay(seta);                              // (nothing for a set without a body)
    ObstacleSet& set = set_of(seta);
    const uint32_t rel = blockIdx.x * OBSTACLE_THREADS + threadIdx.x;
    const bool active = rel < n;
    const uint32_t slot = lo + (active ? rel : n - 1u);
    float4 pi = posi[slot];
    const float eps = ph.wall_eps;
    bool may[SPH_MAX_OBSTACLES];
    bool any = false;
#pragma unroll
    for (int k = 0; k < SPH_MAX_OBSTACLES; k++) {
        const ObstacleSlot& S = set.s[k];
        may[k] = false;
        if (S.flags & OB_SLOT_INSTALLED) {                               // kernel-uniform
            const float guard = eps + 0.25f * S.A.s;
            if (active)
                may[k] = (S.flags & OB_SLOT_POSED) ? ob_slot_may<true>(S, guard, pi.x, pi.y, pi.z)
                                                   : ob_slot_may<false>(S, guard, pi.x, pi.y, pi.z);
        }
        any = any || may[k];
    }
    [[maybe_unused]] const bool row_owner = active && (threadIdx.x & 63u) == 0u;     // (lane 0 of a wave that owns a slot)
    if (__ballot(any) == 0ull) {                                         // wave-uniform: nearly every wave
        if constexpr (SENSE) {
            if (row_owner) {
#pragma unroll
                for (int k = 0; k < SPH_MAX_OBSTACLES; k++)
                    if ((set.s[k].flags & (OB_SLOT_INSTALLED | OB_SLOT_SENSE)) == (OB_SLOT_INSTALLED | OB_SLOT_SENSE))
                        set.s[k].X.mask[rel >> 6] = 0u;
            }
        }
        return;
    }
    float4 vi = make_float4(0.f, 0.f, 0.f, 0.f);
    if (any) vi = velr[slot];
    bool hit = false;                                                    // the union over the slots: the lane has moved
#pragma unroll
    for (int k = 0; k < SPH_MAX_OBSTACLES; k++) {
        const ObstacleSlot& S = set.s[k];
        if (!(S.flags & OB_SLOT_INSTALLED)) continue;                    // kernel-uniform
        const bool posed = (S.flags & OB_SLOT_POSED) != 0u;
        [[maybe_unused]] const bool sense = (S.flags & OB_SLOT_SENSE) != 0u;
        bool m = may[k];
        if (hit) {                                                       // moved by an earlier slot: the guard from where it is now
            const float guard = eps + 0.25f * S.A.s;
            m = posed ? ob_slot_may<true>(S, guard, pi.x, pi.y, pi.z) : ob_slot_may<false>(S, guard, pi.x, pi.y, pi.z);
        }
        if (__ballot(m) == 0ull) {                                       // wave-uniform: no lane can touch this slot
            if constexpr (SENSE) { if (sense && row_owner) S.X.mask[rel >> 6] = 0u; }
            continue;
        }
        [[maybe_unused]] double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        [[maybe_unused]] bool kicked = false;
        const bool h = posed ? ob_slot_iterate<true, SENSE>(S, ph, m, sense, pi, vi, acc, kicked)
                             : ob_slot_iterate<false, SENSE>(S, ph, m, sense, pi, vi, acc, kicked);
        if constexpr (SENSE) {
            if (sense) {                                                 // kernel-uniform
                const uint64_t km = __ballot(kicked);
                if (km != 0ull) {                                        // wave-uniform
                    double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                    for (uint64_t q = km; q != 0ull; q &= q - 1ull) {
                        const uint32_t l = (uint32_t)__builtin_ctzll(q);
#pragma unroll
                        for (int a = 0; a < 6; a++) sum[a] = sum[a] + lane_value_f64(acc[a], l);
                    }
                    if (row_owner) {
                        double* row = S.X.rows + (size_t)(rel >> 6) * 6u;
#pragma unroll
                        for (int a = 0; a < 6; a++) row[a] = sum[a];
                    }
                }
                if (row_owner) S.X.mask[rel >> 6] = km != 0ull ? 1u : 0u;
            }
        }
        if (h) {
            wall(pi.x, vi.x, ph.box_min[0], ph.box_max[0], eps, ph.wall_damping);
            wall(pi.y, vi.y, ph.box_min[1], ph.box_max[1], eps, ph.wall_damping);
            wall(pi.z, vi.z, ph.box_min[2], ph.box_max[2], eps, ph.wall_damping);
            hit = true;
        }
    }
    bool moved = false;
    if (hit) {
        posi[slot] = pi;
        velr[slot] = vi;
        pos_by_index[__float_as_uint(pi.w)] = make_float4(pi.x, pi.y, pi.z, 1.0f);
        if (keys_out) {
            const uint32_t key = cell_key(g, pi.x, pi.y, pi.z);
            keys_out[rel] = key;
            moved = key != keyS[slot];
        }
    }
    if (mm_mask) {
        const uint64_t hm = __ballot(hit);
        if (hm != 0ull) {                                                // wave-uniform
            const uint64_t mv = __ballot(moved);                         // (a subset of hm)
            if ((threadIdx.x & 63u) == 0u) {                             // (lane 0 of a wave that got here owns a slot)
                const uint32_t chunk = rel >> 6;
                const uint64_t old = mm_mask[chunk], now = (old & ~hm) | mv;
                if (now != old) {
                    mm_mask[chunk] = now;
                    atomicAdd(&mm_tile_cnt[chunk / MM_TILE_CHUNKS], (uint32_t)__popcll(now) - (uint32_t)__popcll(old));
                }
            }
        }
    }
}

// ---- the load: the waves' rows added in a fixed order (sph_obstacle_get_load) ----------------------------------------------------
// One block, once per integrate of a sensing context, behind the push.  The order is k_spheres_step's (sph_pairs.hip): thread t
// takes the waves [t K, (t + 1) K), K = ceil(waves / 256) rounded up to a multiple of 4, and adds the rows the masks point to
// in ascending wave order; the threads that found a row are then added in ascending thread order.  It is a twin and not a
// function shared with k_spheres_step: that kernel selects 3-column pieces of a 24-column row by the bits of its mask word
// and goes on to the body update from its shared sums, this one takes whole rows of 6, and a shared body would have to carry
// both as parameters through a kernel whose bits tests/test_gpu_collider_sums.py pins.
constexpr uint32_t OBSTACLE_LOAD_THREADS = 256;
struct ObstacleAbout { float P[3]; };
struct ObstacleAboutBody { const ObstacleBodyBlock* blk; };      // BODY: the host's P is stale, the block's is that of the push
__device__ __forceinline__ float about_of(const ObstacleAbout& a, uint32_t k) { return a.P[k]; }
__device__ __forceinline__ float about_of(const ObstacleAboutBody& a, uint32_t k) { return a.blk->P[k]; }
template <bool BODY>
__global__ __launch_bounds__(OBSTACLE_LOAD_THREADS) void k_obstacle_load(const double* __restrict__ rows, const uint32_t* __restrict__ mask,
                                                                         uint32_t n_waves, double* out,
                                                                         std::conditional_t<BODY, ObstacleAboutBody, ObstacleAbout> about) {
#pragma clang fp contract(off)
    constexpr uint32_t T = OBSTACLE_LOAD_THREADS, NJ = 6;
    __shared__ double s_acc[T][NJ];
    __shared__ uint64_t s_found[T / 64];
    const uint32_t t = threadIdx.x;
    const uint32_t K = ((n_waves + T - 1u) / T + 3u) & ~3u;
    const uint32_t w0 = t * K, w1 = min(w0 + K, n_waves);
    double acc[NJ] = {};
    bool found = false;
    for (uint32_t q = w0; q < w1; q += 4u) {
        const uint4 m4 = *reinterpret_cast<const uint4*>(mask + q);          // (the buffer is padded to whole quads)
        const uint32_t mm[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
        for (uint32_t e = 0; e < 4u; e++) {
            if (q + e < w1 && mm[e] != 0u) {
                found = true;
                const double* row = rows + (size_t)(q + e) * NJ;
#pragma unroll
                for (uint32_t a = 0; a < NJ; a++) acc[a] = acc[a] + row[a];
            }
        }
    }
    const uint64_t fb = __ballot(found);
    if ((t & 63u) == 0u) s_found[t >> 6] = fb;
    if (found) {
#pragma unroll
        for (uint32_t a = 0; a < NJ; a++) s_acc[t][a] = acc[a];
    }
    __syncthreads();
    if (t < NJ) {
        double sum = 0.0;
        for (uint32_t w = 0; w < T / 64u; w++)
            for (uint64_t m = s_found[w]; m != 0ull; m &= m - 1ull) sum = sum + s_acc[w * 64u + (uint32_t)__builtin_ctzll(m)][t];
        out[t] = sum;
    }
    if (t == NJ) reinterpret_cast<unsigned long long*>(out)[NJ] += 1ull;     // integrates since the obstacle was installed
    if (t > NJ && t <= NJ + 3u) reinterpret_cast<float*>(out + NJ + 1u)[t - NJ - 1u] = about_of(about, t - NJ - 1u);
}

// ---- the body step (sph_obstacle_set_body; THE BODY STEP of include/sph_hip.h) ---------------------------------------------------
// One thread, once per integrate and body slot, behind that slot's k_obstacle_load, whose J and L it reads: the block moves on
// by dt.  Float64 with each operation rounded; the division and the square root are the correctly rounded ones, so that
// tests/obstacle_body_model.py repeats it bit for bit.  It is a kernel of its own and not a tail of k_obstacle_load: that
// kernel's last sums leave six different threads, and a block-wide wait more would only be the same dependence written
// differently, in a kernel whose bits tests/test_gpu_obstacle_pose.py pins.
struct ObstacleBodyArgs {
    double e[3];           // HINGE: the unit axis
    uint32_t dof;
    float mass, inertia[3], accel[3], torque[3], lo[3], hi[3];
    float damp, dt;
};

// the nine float64 expressions of rot before their rounding (ob_rot_of below rounds the same expressions)
__host__ __device__ inline void ob_rot_exact(const double q[4], double R[9]) {
#pragma clang fp contract(off)
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z); R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y); R[7] = 2.0 * (y * z + w * x); R[8] = 1.0 - 2.0 * (x * x + y * y);
}

__global__ __launch_bounds__(WAVE) void k_obstacle_body(ObstacleBodyBlock* __restrict__ blk, const double* __restrict__ load,
                                                        ObstacleBodyArgs B) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0u) return;
    ObstacleBodyBlock s = *blk;
    const float dt = B.dt;
    const double ddt = (double)dt;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (B.dof & (1u << a)) {
            s.u[a] = (float)(((double)s.u[a] + __ddiv_rn(load[a], (double)B.mass)) + ddt * (double)B.accel[a]);
            wall(s.off[a], s.u[a], B.lo[a], B.hi[a], 0.f, B.damp);
        }
        s.off[a] = s.off[a] + dt * s.u[a];
    }
    const double T0 = load[3] + ddt * (double)B.torque[0], T1 = load[4] + ddt * (double)B.torque[1],
                 T2 = load[5] + ddt * (double)B.torque[2];
    const double w0 = (double)s.omega[0], w1 = (double)s.omega[1], w2 = (double)s.omega[2];
    if (B.dof & SPH_BODY_HINGE) {
        const double e0 = B.e[0], e1 = B.e[1], e2 = B.e[2];
        const double sc = ((w0 * e0 + w1 * e1) + w2 * e2) + __ddiv_rn((T0 * e0 + T1 * e1) + T2 * e2, (double)B.inertia[0]);
        s.omega[0] = (float)(sc * e0); s.omega[1] = (float)(sc * e1); s.omega[2] = (float)(sc * e2);
    } else if (B.dof & SPH_BODY_SPIN) {
        double R[9];
        ob_rot_exact(s.quat, R);
        const double I0 = (double)B.inertia[0], I1 = (double)B.inertia[1], I2 = (double)B.inertia[2];
        const double b0 = (R[0] * w0 + R[3] * w1) + R[6] * w2, b1 = (R[1] * w0 + R[4] * w1) + R[7] * w2,
                     b2 = (R[2] * w0 + R[5] * w1) + R[8] * w2;
        const double t0 = (R[0] * T0 + R[3] * T1) + R[6] * T2, t1 = (R[1] * T0 + R[4] * T1) + R[7] * T2,
                     t2 = (R[2] * T0 + R[5] * T1) + R[8] * T2;
        const double h0 = I0 * b0, h1 = I1 * b1, h2 = I2 * b2;
        const double g0 = b1 * h2 - b2 * h1, g1 = b2 * h0 - b0 * h2, g2 = b0 * h1 - b1 * h0;
        const double n0 = b0 + __ddiv_rn(t0 - ddt * g0, I0), n1 = b1 + __ddiv_rn(t1 - ddt * g1, I1),
                     n2 = b2 + __ddiv_rn(t2 - ddt * g2, I2);
        s.omega[0] = (float)((R[0] * n0 + R[1] * n1) + R[2] * n2);
        s.omega[1] = (float)((R[3] * n0 + R[4] * n1) + R[5] * n2);
        s.omega[2] = (float)((R[6] * n0 + R[7] * n1) + R[8] * n2);
    }
    {                                                   // the Cayley step of THE POSE, as advance_obstacle writes it
        const double w = s.quat[0], x = s.quat[1], y = s.quat[2], z = s.quat[3];
        const double h = 0.5 * ddt;
        const double a0 = h * (double)s.omega[0], a1 = h * (double)s.omega[1], a2 = h * (double)s.omega[2];
        const double q[4] = {((w - a0 * x) - a1 * y) - a2 * z, ((x + a0 * w) + a1 * z) - a2 * y, ((y + a1 * w) + a2 * x) - a0 * z,
                             ((z + a2 * w) + a0 * y) - a1 * x};
        const double n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
        if (n2 > 0.0 && n2 < (double)INFINITY) {        // (otherwise the pose stays, as on the host)
            const double len = __dsqrt_rn(n2);
#pragma unroll
            for (int k = 0; k < 4; k++) s.quat[k] = __ddiv_rn(q[k], len);
        }
    }
    double R[9];
    ob_rot_exact(s.quat, R);
#pragma unroll
    for (int k = 0; k < 9; k++) s.rot[k] = (float)R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) s.P[k] = s.pivot[k] + s.off[k];
    *blk = s;
}

// What the host writes into the block: the values travel by value (k_spheres_install of sph_pairs.hip is the pattern), so no
// host buffer has to outlive the call and the host does not wait.  P follows from whatever pivot and off the block then holds.
constexpr uint32_t OB_PUT_OFF = 1u, OB_PUT_U = 2u, OB_PUT_POSE = 4u;
__global__ __launch_bounds__(WAVE) void k_obstacle_body_put(ObstacleBodyBlock* __restrict__ blk, ObstacleBodyBlock v, uint32_t what) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0u) return;
    ObstacleBodyBlock s = *blk;
    for (int k = 0; k < 3; k++) {
        if (what & OB_PUT_OFF) s.off[k] = v.off[k];
        if (what & OB_PUT_U) s.u[k] = v.u[k];
        if (what & OB_PUT_POSE) { s.pivot[k] = v.pivot[k]; s.omega[k] = v.omega[k]; }
    }
    if (what & OB_PUT_POSE) {
        for (int k = 0; k < 4; k++) s.quat[k] = v.quat[k];
        for (int k = 0; k < 9; k++) s.rot[k] = v.rot[k];
    }
    for (int k = 0; k < 3; k++) s.P[k] = s.pivot[k] + s.off[k];
    *blk = s;
}

// ---- the sample rule for caller points ----------------------------------------------------------------------------------------
// POSED: x is a world point, the normal comes back in world axes, by the push's arithmetic
template <bool POSED, bool BODY = false>
__global__ __launch_bounds__(OBSTACLE_THREADS) void k_obstacle_sample(const float* __restrict__ pos, uint32_t n, ObstacleArgs A,
                                                                      float* __restrict__ phi_out, float* __restrict__ nrm_out,
                                                                      uint8_t* __restrict__ in_out, PoseArg<BODY> Xa) {
    ObstaclePose& X = pose_of(Xa);
    if constexpr (BODY) ob_overlay(A, X, block_of(Xa));
    const uint32_t t = blockIdx.x * OBSTACLE_THREADS + threadIdx.x;
    if (t >= n) return;
    uint32_t ci[3];
    float cf[3], d[3];
    float phi = INFINITY, nx = 0.f, ny = 0.f, nz = 0.f;
    const bool in = ob_locate_at<POSED>(A, X, pos[3u * t], pos[3u * t + 1u], pos[3u * t + 2u], ci, cf, d);
    if (in) {
        ob_sample_cell(A, ci, cf, phi, nx, ny, nz);
        if constexpr (POSED) ob_world_normal(X, nx, ny, nz);
    }
    phi_out[t] = phi;
    nrm_out[3u * t] = nx; nrm_out[3u * t + 1u] = ny; nrm_out[3u * t + 2u] = nz;
    in_out[t] = in ? 1 : 0;
}

// ---- the solids as a picture (sph_render_set_solids; THE RULE of include/sph_hip.h) -----------------------------------------------
// One pixel per lane; a wave is an 8 x 8 tile of pixels and a block of SOLID_THREADS lanes a 16 x 16 one, so that the rays of a
// wave walk the same bricks and their eight-node gathers share cache lines.  The slots travel by value like the push's; posed or
// not is a wave-uniform branch per slot.  The loop bound is each lane's own: neighbouring rays need similar step counts, and a
// lane that has left only waits for its tile.  No LDS, no atomics.  Every sample is ob_locate_at + ob_sample_cell: the bits of
// sph_obstacle_sample.  The brick minima are NOT used: the length of a step depends on phi itself, so no sample whose value
// decides the next one can be skipped with the outcome known.
constexpr uint32_t SOLID_THREADS = 256, SOLID_TILE = 16;

// CLIP, MARCH and REFINE of one slot along the ray O + z D.  zstop: a hit at or behind it cannot win (the fluid's depth, an
// earlier slot's hit), so the march leaves at the first free sample there -- every later crossing has z_s >= za >= zstop.
// true: a crossing; zs and the WORLD normal n are then set
template <bool POSED>
__device__ __forceinline__ bool solid_march_slot(const ObstacleSlot& S, bool open, const float O[3], const float D[3], float le,
                                                 float near_z, float far_z, float zstop, float& zs, float n[3]) {
#pragma clang fp contract(off)
    const ObstacleArgs& A = S.A;
    const ObstaclePose& X = S.X;
    float Ob[3], Db[3];
    if constexpr (POSED) {
        const float d0 = O[0] - X.P[0], d1 = O[1] - X.P[1], d2 = O[2] - X.P[2];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            Ob[k] = ((X.rot[k] * d0 + X.rot[3 + k] * d1) + X.rot[6 + k] * d2) + X.pivot[k];
            Db[k] = (X.rot[k] * D[0] + X.rot[3 + k] * D[1]) + X.rot[6 + k] * D[2];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) { Ob[k] = O[k] - A.off[k]; Db[k] = D[k]; }
    }
    float t0 = near_z, t1 = far_z;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float lo = A.origin[k], hi = A.origin[k] + A.nm1[k] * A.s;
        const float inv = 1.0f / Db[k];
        const float ta = (lo - Ob[k]) * inv, tb = (hi - Ob[k]) * inv;
        t0 = fmaxf(t0, fminf(ta, tb));
        t1 = fminf(t1, fmaxf(ta, tb));
    }
    if (!(t0 <= t1)) return false;
    const float qs = 0.25f * A.s;
    float z = t0, za = t0, zb = t0;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f;             // the body normal of the sample that last set zb
    bool open_run = open, cross = false;
    uint32_t ci[3];
    float cf[3], d[3], phi, nx, ny, nz;
    for (int it = 0; it < SPH_SOLID_MAX_STEPS; it++) {
        if (!(z <= t1)) break;
        float a = qs;
        if (ob_locate_at<POSED>(A, X, O[0] + z * D[0], O[1] + z * D[1], O[2] + z * D[2], ci, cf, d)) {
            ob_sample_cell(A, ci, cf, phi, nx, ny, nz);
            if (phi < 0.f) {
                if (!open_run) { zb = z; b0 = nx; b1 = ny; b2 = nz; cross = true; break; }
                a = fmaxf(0.5f * (-phi), qs);
            } else {
                open_run = false;
                a = fmaxf(0.5f * phi, qs);
            }
        }
        za = z;
        if (za >= zstop) break;
        z = z + a / le;
    }
    if (!cross) return false;
    for (int it = 0; it < SPH_SOLID_BISECTIONS; it++) {
        const float zm = 0.5f * (za + zb);
        bool solid = false;
        if (ob_locate_at<POSED>(A, X, O[0] + zm * D[0], O[1] + zm * D[1], O[2] + zm * D[2], ci, cf, d)) {
            ob_sample_cell(A, ci, cf, phi, nx, ny, nz);
            solid = phi < 0.f;
        }
        if (solid) { zb = zm; b0 = nx; b1 = ny; b2 = nz; }
        else za = zm;
    }
    if constexpr (POSED) ob_world_normal(X, b0, b1, b2);
    zs = zb;
    n[0] = b0; n[1] = b1; n[2] = b2;
    return true;
}

// DIRECT (sph_render): depth holds the fluid's d (+inf on background); a pixel whose nearest hit lies strictly in front of it
// takes the solid's RGBA, id and depth, every other pixel is left alone.  Else (sph_render_surface): the nearest hit of every
// pixel -- depth (+inf: none), slot, eye-space normal -- goes to the so_ planes, and k_surface_shade composes.
// `set` holds the DRAWN slots only (flags 0 elsewhere).
template <bool DIRECT, bool BODY = false>
__global__ __launch_bounds__(SOLID_THREADS) void k_solid_march(SolidCam C, SolidLooks K, SetArg<BODY> seta, uint32_t* __restrict__ rgba,
                                                               uint32_t* __restrict__ id, float* __restrict__ depth,
                                                               float* __restrict__ so_depth, uint32_t* __restrict__ so_slot,
                                                               float* __restrict__ so_normal) {
#pragma clang fp contract(off)
    ob_set_overlay(seta);                              // a drawn BODY slot is where its block says (sph_obstacle_set_body)
    ObstacleSet& set = set_of(seta);
    const uint32_t wave = threadIdx.x >> 6, l = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * SOLID_TILE + (wave & 1u) * 8u + (l & 7u);
    const uint32_t j = blockIdx.y * SOLID_TILE + (wave >> 1) * 8u + (l >> 3);
    if (i >= C.width || j >= C.height) return;
    const size_t pix = (size_t)j * C.width + i;
    const float ex = (((float)i + 0.5f) - C.half_w) / C.focal;
    const float ey = (C.half_h - ((float)j + 0.5f)) / C.focal;
    const float le = sqrtf((ex * ex + ey * ey) + 1.0f);
    float O[3], D[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        O[k] = -((C.rot[k] * C.trans[0] + C.rot[3 + k] * C.trans[1]) + C.rot[6 + k] * C.trans[2]);
        D[k] = (C.rot[k] * ex + C.rot[3 + k] * ey) + C.rot[6 + k];
    }
    float best = DIRECT ? depth[pix] : INFINITY;       // what a hit has to beat, strictly: the lowest slot wins among equals
    uint32_t slot = 0;
    bool hit = false;
    float n[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (uint32_t s = 0; s < (uint32_t)SPH_MAX_OBSTACLES; s++) {
        const ObstacleSlot& S = set.s[s];
        if (!(S.flags & OB_SLOT_INSTALLED)) continue;                               // wave-uniform, as the next
        float zs, ns[3];
        const bool got = (S.flags & OB_SLOT_POSED)
            ? solid_march_slot<true>(S, K.open[s] != 0, O, D, le, C.near_z, C.far_z, best, zs, ns)
            : solid_march_slot<false>(S, K.open[s] != 0, O, D, le, C.near_z, C.far_z, best, zs, ns);
        if (got && zs < best) { best = zs; slot = s; hit = true; n[0] = ns[0]; n[1] = ns[1]; n[2] = ns[2]; }
    }
    float ne[3] = {0.f, 0.f, 0.f};
    if (hit) {
#pragma unroll
        for (int k = 0; k < 3; k++) ne[k] = (C.rot[3 * k] * n[0] + C.rot[3 * k + 1] * n[1]) + C.rot[3 * k + 2] * n[2];
    }
    if constexpr (DIRECT) {
        if (!hit) return;
        float c[3];
        solid_color(K, slot, ne, c);
        rgba[pix] = solid_rgba(c);
        id[pix] = SPH_RENDER_ID_SOLID + slot;
        depth[pix] = best;
    } else {
        so_depth[pix] = hit ? best : INFINITY;
        so_slot[pix] = slot;
        so_normal[3 * pix] = ne[0]; so_normal[3 * pix + 1] = ne[1]; so_normal[3 * pix + 2] = ne[2];
    }
}

// ---- installation ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ob_shape_phi(const sph_shape& S, float px, float py, float pz) {
#pragma clang fp contract(off)
    float phi;
    if (S.kind == SPH_SHAPE_SPHERE) {
        const float dx = px - S.a[0], dy = py - S.a[1], dz = pz - S.a[2];
        phi = sqrtf((dx * dx + dy * dy) + dz * dz) - S.r;
    } else if (S.kind == SPH_SHAPE_BOX) {
        const float qx = fabsf(px - S.a[0]) - S.b[0], qy = fabsf(py - S.a[1]) - S.b[1], qz = fabsf(pz - S.a[2]) - S.b[2];
        const float ox = fmaxf(qx, 0.f), oy = fmaxf(qy, 0.f), oz = fmaxf(qz, 0.f);
        phi = (sqrtf((ox * ox + oy * oy) + oz * oz) + fminf(fmaxf(qx, fmaxf(qy, qz)), 0.f)) - S.r;
    } else if (S.kind == SPH_SHAPE_CAPSULE) {
        const float pax = px - S.a[0], pay = py - S.a[1], paz = pz - S.a[2];
        const float bax = S.b[0] - S.a[0], bay = S.b[1] - S.a[1], baz = S.b[2] - S.a[2];
        float t = ((pax * bax + pay * bay) + paz * baz) / ((bax * bax + bay * bay) + baz * baz);
        t = fminf(fmaxf(t, 0.f), 1.f);
        const float dx = pax - t * bax, dy = pay - t * bay, dz = paz - t * baz;
        phi = sqrtf((dx * dx + dy * dy) + dz * dz) - S.r;
    } else {
        phi = ((px - S.a[0]) * S.b[0] + (py - S.a[1]) * S.b[1]) + (pz - S.a[2]) * S.b[2];
    }
    return S.invert ? -phi : phi;
}

__global__ __launch_bounds__(OBSTACLE_THREADS) void k_obstacle_raster(float* __restrict__ phi, uint32_t nodes, ObstacleArgs A, Shapes sh,
                                                                      float D) {
#pragma clang fp contract(off)
    const uint32_t t = blockIdx.x * OBSTACLE_THREADS + threadIdx.x;
    if (t >= nodes) return;
    const uint32_t i = t % A.n[0], jk = t / A.n[0], j = jk % A.n[1], k = jk / A.n[1];
    const float px = A.origin[0] + (float)i * A.s, py = A.origin[1] + (float)j * A.s, pz = A.origin[2] + (float)k * A.s;
    float v = ob_shape_phi(sh.s[0], px, py, pz);
    for (uint32_t q = 1; q < sh.n; q++) v = fminf(v, ob_shape_phi(sh.s[q], px, py, pz));
    phi[t] = fminf(fmaxf(v, -D), D);
}

__global__ __launch_bounds__(OBSTACLE_THREADS) void k_obstacle_clamp(float* __restrict__ phi, uint32_t nodes, float D) {
    const uint32_t t = blockIdx.x * OBSTACLE_THREADS + threadIdx.x;
    if (t < nodes) phi[t] = fminf(fmaxf(phi[t], -D), D);
}

// brick (bx, by, bz) covers the cells [4 b, 4 b + 4) of each axis, i.e. the nodes [4 b, 4 b + 4] (clipped to the lattice)
__global__ __launch_bounds__(OBSTACLE_THREADS) void k_obstacle_bricks(ObstacleArgs A, float* __restrict__ brick, uint32_t bricks) {
    const uint32_t t = blockIdx.x * OBSTACLE_THREADS + threadIdx.x;
    if (t >= bricks) return;
    const uint32_t bx = t % A.nb[0], r = t / A.nb[0], by = r % A.nb[1], bz = r / A.nb[1];
    const uint32_t x0 = bx * OBSTACLE_BRICK, y0 = by * OBSTACLE_BRICK, z0 = bz * OBSTACLE_BRICK;
    const uint32_t x1 = min(x0 + OBSTACLE_BRICK, A.n[0] - 1u), y1 = min(y0 + OBSTACLE_BRICK, A.n[1] - 1u), z1 = min(z0 + OBSTACLE_BRICK, A.n[2] - 1u);
    float m = INFINITY;
    for (uint32_t z = z0; z <= z1; z++)
        for (uint32_t y = y0; y <= y1; y++) {
            const float* __restrict__ row = A.phi + ((size_t)z * A.n[1] + y) * A.n[0];
            for (uint32_t x = x0; x <= x1; x++) m = fminf(m, row[x]);
        }
    brick[t] = m;
}

// ---- the host side --------------------------------------------------------------------------------------------------------------

static uint32_t ob_bricks_axis(uint32_t n) { return ceil_div(n - 1u, OBSTACLE_BRICK); }

static ObstacleArgs obstacle_args(const Obstacle& o) {
    ObstacleArgs A{};
    A.phi = o.phi;
    A.brick = o.brick;
    A.s = o.grid.spacing;
    for (int k = 0; k < 3; k++) {
        A.origin[k] = o.grid.origin[k];
        A.n[k] = o.grid.dims[k];
        A.nm1[k] = (float)(A.n[k] - 1u);
        A.nb[k] = ob_bricks_axis(A.n[k]);
        A.off[k] = o.off[k];
        A.u[k] = o.vel[k];
    }
    return A;
}

float ob_clamp_distance(const sph_obstacle_grid& G) {
#pragma clang fp contract(off)
    return G.spacing * (float)(G.dims[0] + G.dims[1] + G.dims[2]);
}

// rot of the header from the unit quaternion: float64, each entry rounded once
void ob_rot_of(const double q[4], float rot[9]) {
#pragma clang fp contract(off)
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    rot[0] = (float)(1.0 - 2.0 * (y * y + z * z)); rot[1] = (float)(2.0 * (x * y - w * z)); rot[2] = (float)(2.0 * (x * z + w * y));
    rot[3] = (float)(2.0 * (x * y + w * z)); rot[4] = (float)(1.0 - 2.0 * (x * x + z * z)); rot[5] = (float)(2.0 * (y * z - w * x));
    rot[6] = (float)(2.0 * (x * z - w * y)); rot[7] = (float)(2.0 * (y * z + w * x)); rot[8] = (float)(1.0 - 2.0 * (x * x + y * y));
}

// q / |q| with the header's sum; false: the squared norm is 0 or not finite
static bool ob_quat_unit(const double in[4], double out[4]) {
#pragma clang fp contract(off)
    const double n2 = ((in[0] * in[0] + in[1] * in[1]) + in[2] * in[2]) + in[3] * in[3];
    if (!(n2 > 0.0) || !std::isfinite(n2)) return false;
    const double len = std::sqrt(n2);
    for (int k = 0; k < 4; k++) out[k] = in[k] / len;
    return true;
}

static ObstaclePose obstacle_pose(const Obstacle& o) {
#pragma clang fp contract(off)
    ObstaclePose X{};
    if (o.posed) ob_rot_of(o.quat, X.rot);
    for (int k = 0; k < 3; k++) {
        X.pivot[k] = o.posed ? o.pivot[k] : 0.f;
        X.P[k] = o.posed ? o.pivot[k] + o.off[k] : o.off[k];
        X.omega[k] = o.posed ? o.omega[k] : 0.f;
    }
    X.rows = o.rows;
    X.mask = o.wmask;
    return X;
}

static ObstacleSet obstacle_set(const sph_ctx* c) {
    ObstacleSet S{};
    for (uint32_t k = 0; k < (uint32_t)SPH_MAX_OBSTACLES; k++) {
        const Obstacle& o = c->ob[k];
        if (!o.installed()) continue;
        S.s[k].A = obstacle_args(o);
        S.s[k].X = obstacle_pose(o);
        S.s[k].flags = OB_SLOT_INSTALLED | (o.posed ? OB_SLOT_POSED : 0u) | (o.sense && o.load ? OB_SLOT_SENSE : 0u) |
                       (o.body ? OB_SLOT_BODY : 0u);
    }
    return S;
}

// the BODY instantiations' argument of the slots S (flags as the caller left them); false: no slot of S has a body
static bool obstacle_set_body(const sph_ctx* c, const ObstacleSet& S, ObstacleSetBody* out) {
    bool any = false;
    out->set = S;
    for (uint32_t k = 0; k < (uint32_t)SPH_MAX_OBSTACLES; k++) {
        const bool b = (S.s[k].flags & OB_SLOT_BODY) != 0u;
        out->blk[k] = b ? c->ob[k].blk : nullptr;
        any = any || b;
    }
    return any;
}

// ---- the body's host side: the block is the state, the host's copies are stale while `body` -------------------------------------
static ObstacleBodyArgs body_args(const sph_ctx* c, const Obstacle& o, float dt) {
    ObstacleBodyArgs B{};
    const sph_obstacle_body& b = o.bd;
    B.dof = b.dof;
    B.mass = b.mass;
    for (int k = 0; k < 3; k++) {
        B.e[k] = o.axis[k];
        B.inertia[k] = b.inertia[k]; B.accel[k] = b.accel[k]; B.torque[k] = b.torque[k]; B.lo[k] = b.lo[k]; B.hi[k] = b.hi[k];
    }
    B.damp = c->phys.wall_damping;
    B.dt = dt;
    return B;
}

// the block a kinematic slot would be: the host's state, rot and P as obstacle_pose makes them for the next launch
static ObstacleBodyBlock body_block_of(const Obstacle& o) {
    ObstacleBodyBlock v{};
    const ObstaclePose X = obstacle_pose(o);
    for (int k = 0; k < 4; k++) v.quat[k] = o.quat[k];
    for (int k = 0; k < 3; k++) { v.off[k] = o.off[k]; v.u[k] = o.vel[k]; v.pivot[k] = X.pivot[k]; v.omega[k] = X.omega[k]; v.P[k] = X.P[k]; }
    for (int k = 0; k < 9; k++) v.rot[k] = X.rot[k];
    return v;
}

static int body_put(sph_ctx* c, const Obstacle& o, const ObstacleBodyBlock& v, uint32_t what) {
    SPH_HIP(hipSetDevice(c->device));
    hipLaunchKernelGGL(k_obstacle_body_put, dim3(1), dim3(WAVE), 0, c->stream, o.blk, v, what);
    SPH_HIP(hipGetLastError());
    return SPH_OK;
}

// synchronises: the block as the last queued step left it
static int body_fetch(const sph_ctx* c, const Obstacle& o, ObstacleBodyBlock* out) {
    SPH_HIP(hipSetDevice(c->device));
    SPH_HIP(hipMemcpyAsync(out, o.blk, sizeof(*out), hipMemcpyDeviceToHost, c->stream));
    SPH_HIP(hipStreamSynchronize(c->stream));
    return SPH_OK;
}

bool solids_drawn(const sph_ctx* c) {
    if (!c->rd_solids) return false;
    for (uint32_t k = 0; k < (uint32_t)SPH_MAX_OBSTACLES; k++)
        if (c->ob[k].installed() && c->rd_solid_style.slot[k].draw != 0) return true;
    return false;
}

int launch_solid_march(sph_ctx* c, const SolidCam& cam, const SolidLooks& looks, uint32_t* rgba, uint32_t* id, float* depth,
                       float* so_depth, uint32_t* so_slot, float* so_normal) {
    ObstacleSet S = obstacle_set(c);                 // the offset and the pose the next push would see
    for (uint32_t k = 0; k < (uint32_t)SPH_MAX_OBSTACLES; k++)
        if (c->rd_solid_style.slot[k].draw == 0) S.s[k].flags = 0u;
    const dim3 grid(ceil_div(cam.width, SOLID_TILE), ceil_div(cam.height, SOLID_TILE));
    ObstacleSetBody SB;
    if (obstacle_set_body(c, S, &SB)) {              // a drawn slot has a body: the instantiations that read the blocks
        if (so_depth)
            hipLaunchKernelGGL((k_solid_march<false, true>), grid, dim3(SOLID_THREADS), 0, c->stream, cam, looks, SB, rgba, id, depth,
                               so_depth, so_slot, so_normal);
        else
            hipLaunchKernelGGL((k_solid_march<true, true>), grid, dim3(SOLID_THREADS), 0, c->stream, cam, looks, SB, rgba, id, depth,
                               so_depth, so_slot, so_normal);
    } else if (so_depth)
        hipLaunchKernelGGL(k_solid_march<false>, grid, dim3(SOLID_THREADS), 0, c->stream, cam, looks, S, rgba, id, depth, so_depth,
                           so_slot, so_normal);
    else
        hipLaunchKernelGGL(k_solid_march<true>, grid, dim3(SOLID_THREADS), 0, c->stream, cam, looks, S, rgba, id, depth, so_depth,
                           so_slot, so_normal);
    SPH_HIP(hipGetLastError());
    return SPH_OK;
}

// The installed set {slot 0} is the library of one obstacle: k_obstacle_push with its arguments.  Every other set: one launch of
// k_obstacle_push_set.
int launch_obstacle_push(sph_ctx* c, bool fused, bool mark) {
    if (c->n == 0) return SPH_OK;
    bool others = false, any_sense = false;
    for (uint32_t k = 0; k < (uint32_t)SPH_MAX_OBSTACLES; k++) {
        const Obstacle& o = c->ob[k];
        if (!o.installed()) continue;
        others = others || k != 0u;
        any_sense = any_sense || (o.sense && o.load);
    }
#define SPH_PUSH_ARGS                                                                                                            \
    fused ? c->posi2 : c->posi, fused ? c->velr2 : c->velr, c->pos_out, fused ? c->k0 : nullptr, c->keyS,                          \
        fused && mark ? c->mm_mask : nullptr, c->mm_tile_cnt, c->own_off, c->n
    if (others) {
        const ObstacleSet S = obstacle_set(c);
        ObstacleSetBody SB;
        if (obstacle_set_body(c, S, &SB))              // (a body slot senses: sph_obstacle_set_body)
            hipLaunchKernelGGL((k_obstacle_push_set<true, true>), dim3(ceil_div(c->n, OBSTACLE_THREADS)), dim3(OBSTACLE_THREADS), 0,
                               c->stream, SPH_PUSH_ARGS, c->grid, c->phys, SB);
        else if (any_sense)
            hipLaunchKernelGGL(k_obstacle_push_set<true>, dim3(ceil_div(c->n, OBSTACLE_THREADS)), dim3(OBSTACLE_THREADS), 0, c->stream,
                               SPH_PUSH_ARGS, c->grid, c->phys, S);
        else
            hipLaunchKernelGGL(k_obstacle_push_set<false>, dim3(ceil_div(c->n, OBSTACLE_THREADS)), dim3(OBSTACLE_THREADS), 0, c->stream,
                               SPH_PUSH_ARGS, c->grid, c->phys, S);
        SPH_HIP(hipGetLastError());
        return SPH_OK;
    }
    const Obstacle& o = c->ob[0];
#define SPH_LAUNCH_PUSH(P, S)                                                                                                    \
    hipLaunchKernelGGL((k_obstacle_push<P, S>), dim3(ceil_div(c->n, OBSTACLE_THREADS)), dim3(OBSTACLE_THREADS), 0, c->stream,      \
                       SPH_PUSH_ARGS, obstacle_args(o), c->grid, c->phys, obstacle_pose(o))
    if (o.body)                                         // (posed and sensing, its buffers there: sph_obstacle_set_body)
        hipLaunchKernelGGL((k_obstacle_push<true, true, true>), dim3(ceil_div(c->n, OBSTACLE_THREADS)), dim3(OBSTACLE_THREADS), 0,
                           c->stream, SPH_PUSH_ARGS, obstacle_args(o), c->grid, c->phys, ObstaclePoseBody{obstacle_pose(o), o.blk});
    else if (o.posed) { if (any_sense) SPH_LAUNCH_PUSH(true, true); else SPH_LAUNCH_PUSH(true, false); }
    else { if (any_sense) SPH_LAUNCH_PUSH(false, true); else SPH_LAUNCH_PUSH(false, false); }
#undef SPH_LAUNCH_PUSH
#undef SPH_PUSH_ARGS
    SPH_HIP(hipGetLastError());
    return SPH_OK;
}

// Once per integrate, behind the push (sph_pairs.hip: advance_colliders), slot by slot.  A sensing slot queues its load's sum
// first -- with the P the push just used, and also without particles (no push ran: zeros) --, then its offset and pose move on
// by dt.
int advance_obstacle(sph_ctx* c, float dt) {
#pragma clang fp contract(off)
    for (Obstacle& o : c->ob) {
        if (!o.installed()) continue;
        if (o.body) {                                   // the load about the block's P, then the body step: all on the device
            hipLaunchKernelGGL(k_obstacle_load<true>, dim3(1), dim3(OBSTACLE_LOAD_THREADS), 0, c->stream, o.rows, o.wmask,
                               ceil_div(c->n, (uint32_t)WAVE), o.load, ObstacleAboutBody{o.blk});
            SPH_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_obstacle_body, dim3(1), dim3(WAVE), 0, c->stream, o.blk, o.load, body_args(c, o, dt));
            SPH_HIP(hipGetLastError());
            continue;
        }
        if (o.sense && o.load) {
            const ObstaclePose X = obstacle_pose(o);
            hipLaunchKernelGGL(k_obstacle_load<false>, dim3(1), dim3(OBSTACLE_LOAD_THREADS), 0, c->stream, o.rows, o.wmask,
                               ceil_div(c->n, (uint32_t)WAVE), o.load, ObstacleAbout{{X.P[0], X.P[1], X.P[2]}});
            SPH_HIP(hipGetLastError());
        }
        for (int k = 0; k < 3; k++) o.off[k] = o.off[k] + dt * o.vel[k];
        if (o.posed) {                                  // the Cayley step of the header, float64
            const double w = o.quat[0], x = o.quat[1], y = o.quat[2], z = o.quat[3];
            const double h = 0.5 * (double)dt;
            const double a0 = h * (double)o.omega[0], a1 = h * (double)o.omega[1], a2 = h * (double)o.omega[2];
            const double q[4] = {((w - a0 * x) - a1 * y) - a2 * z, ((x + a0 * w) + a1 * z) - a2 * y, ((y + a1 * w) + a2 * x) - a0 * z,
                                 ((z + a2 * w) + a0 * y) - a1 * x};
            ob_quat_unit(q, o.quat);                    // (|q'|^2 = 1 + |a|^2 >= 1; if it is not finite the pose stays)
        }
    }
    return SPH_OK;
}

static void pose_reset(Obstacle& o) {
    o.posed = false;
    for (int k = 0; k < 3; k++) o.pivot[k] = o.omega[k] = 0.f;
    o.quat[0] = 1.0; o.quat[1] = o.quat[2] = o.quat[3] = 0.0;
}

// The sensor's buffers, by capacity (the first sph_obstacle_set_sensor(on)): one row of six sums and one mask word per wave of
// the owned slots, the masks padded as tracked_buffers_alloc (sph_pairs.hip) pads the spheres' -- k_obstacle_load reads them in
// quads --, and the 72 bytes of the result.  Rows and masks are not cleared: every wave a sum reads was stored by the push in
// front of it.  All three or none: ob_load doubles as "the buffers are there".
constexpr size_t OBSTACLE_LOAD_WORDS = 9;        // J[3], L[3], the count, about[3] (fp32) + a pad word: 72 bytes
constexpr size_t OBSTACLE_MASK_QUAD = 4;
static int sensor_buffers_alloc(sph_ctx* c, Obstacle& o) {
    Buffers& m = c->mem;
    const size_t waves = ceil_div(c->cap, (uint32_t)WAVE);
    int rc = m.alloc(&o.rows, waves * 6, false);
    if (!rc) rc = m.alloc(&o.wmask, ((waves + OBSTACLE_MASK_QUAD - 1) & ~(OBSTACLE_MASK_QUAD - 1)) + OBSTACLE_MASK_QUAD, false);
    if (!rc) rc = m.alloc(&o.load, OBSTACLE_LOAD_WORDS, true);
    if (rc) { m.release(&o.load); m.release(&o.wmask); m.release(&o.rows); }
    return rc;
}

void release_obstacle(sph_ctx* c) {
    Obstacle& o = selected_obstacle(c);
    c->mem.release(&o.mesh_marks);
    c->mem.release(&o.mesh_work);
    c->mem.release(&o.brick);
    c->mem.release(&o.phi);
    o.grid = sph_obstacle_grid{};
}

static int check_grid(const sph_obstacle_grid& G) {
    double nodes = 1.0;
    for (int k = 0; k < 3; k++) {
        SPH_REQUIRE(G.dims[k] >= 2u, SPH_E_INVALID, "obstacle grid: %u nodes on axis %d, at least 2", G.dims[k], k);
        SPH_REQUIRE(G.dims[k] <= (uint32_t)SPH_OBSTACLE_MAX_DIM, SPH_E_CAPACITY, "obstacle grid: %u nodes on axis %d, at most %d",
                    G.dims[k], k, SPH_OBSTACLE_MAX_DIM);
        SPH_REQUIRE(std::isfinite(G.origin[k]), SPH_E_INVALID, "obstacle grid: the origin is not finite");
        nodes *= (double)G.dims[k];
    }
    SPH_REQUIRE(nodes <= (double)SPH_OBSTACLE_MAX_NODES, SPH_E_CAPACITY, "obstacle grid: %u x %u x %u nodes, at most 2^27", G.dims[0],
                G.dims[1], G.dims[2]);
    SPH_REQUIRE(std::isfinite(G.spacing) && G.spacing > 0.f && std::isfinite(ob_clamp_distance(G)), SPH_E_INVALID,
                "obstacle grid: spacing %g is not a positive finite number", (double)G.spacing);
    return SPH_OK;
}

// The lattice of a build: checks only, allocates nothing.
int lattice_resolve(const sph_ctx* c, float spacing, const float* lo, const float* hi, sph_obstacle_grid* G) {
#pragma clang fp contract(off)
    SPH_REQUIRE(std::isfinite(spacing) && spacing >= 0.f, SPH_E_INVALID, "obstacle spacing %g: finite and >= 0 (0: the particle diameter)",
                (double)spacing);
    SPH_REQUIRE((lo == nullptr) == (hi == nullptr), SPH_E_INVALID, "obstacle bounds: give both corners or neither");
    const float s = spacing > 0.f ? spacing : (float)(2.0 * (double)c->params.particle_radius);
    SPH_REQUIRE(std::isfinite(s) && s > 0.f, SPH_E_INVALID, "obstacle spacing %g is not a positive finite number", (double)s);
    sph_obstacle_grid R{};
    R.spacing = s;
    for (int k = 0; k < 3; k++) {
        const float l = lo ? lo[k] : c->params.box_min[k], h = hi ? hi[k] : c->params.box_max[k];
        SPH_REQUIRE(std::isfinite(l) && std::isfinite(h) && h >= l, SPH_E_INVALID, "obstacle bounds: axis %d is [%g, %g]", k, (double)l,
                    (double)h);
        const double nk = std::ceil(((double)h - (double)l) / (double)s) + 3.0;
        SPH_REQUIRE(nk <= (double)SPH_OBSTACLE_MAX_DIM, SPH_E_CAPACITY, "obstacle lattice: %.0f nodes on axis %d, at most %d (a wider "
                    "spacing, or bounds around the solid?)", nk, k, SPH_OBSTACLE_MAX_DIM);
        R.dims[k] = (uint32_t)nk;
        R.origin[k] = l - s;
    }
    if (int e = check_grid(R)) return e;
    *G = R;
    return SPH_OK;
}

static int check_shapes(uint32_t n, const sph_shape* shapes, Shapes* out) {
#pragma clang fp contract(off)
    SPH_REQUIRE(n >= 1u && n <= (uint32_t)SPH_MAX_SHAPES, SPH_E_INVALID, "%u shapes: 1..%d", n, SPH_MAX_SHAPES);
    SPH_REQUIRE(shapes, SPH_E_INVALID, "null shapes");
    out->n = n;
    for (uint32_t j = 0; j < n; j++) {
        sph_shape S = shapes[j];
        SPH_REQUIRE(S.kind >= SPH_SHAPE_SPHERE && S.kind <= SPH_SHAPE_HALFSPACE, SPH_E_INVALID, "shape %u: unknown kind %d", j, S.kind);
        const bool uses_b = S.kind != SPH_SHAPE_SPHERE, uses_r = S.kind != SPH_SHAPE_HALFSPACE;
        for (int k = 0; k < 3; k++)
            SPH_REQUIRE(std::isfinite(S.a[k]) && (!uses_b || std::isfinite(S.b[k])), SPH_E_INVALID, "shape %u: a field is not finite", j);
        SPH_REQUIRE(!uses_r || std::isfinite(S.r), SPH_E_INVALID, "shape %u: r is not finite", j);
        if (S.kind == SPH_SHAPE_SPHERE || S.kind == SPH_SHAPE_CAPSULE)
            SPH_REQUIRE(S.r > 0.f, SPH_E_INVALID, "shape %u: radius %g is not positive", j, (double)S.r);
        if (S.kind == SPH_SHAPE_BOX) {
            SPH_REQUIRE(S.r >= 0.f, SPH_E_INVALID, "shape %u: rounding %g is negative", j, (double)S.r);
            SPH_REQUIRE(S.b[0] > 0.f && S.b[1] > 0.f && S.b[2] > 0.f, SPH_E_INVALID, "shape %u: a half extent is not positive", j);
        }
        if (S.kind == SPH_SHAPE_CAPSULE) {
            const float bx = S.b[0] - S.a[0], by = S.b[1] - S.a[1], bz = S.b[2] - S.a[2];
            const float bb = (bx * bx + by * by) + bz * bz;
            SPH_REQUIRE(std::isfinite(bb) && bb > 0.f, SPH_E_INVALID, "shape %u: the capsule's ends coincide", j);
        }
        if (S.kind == SPH_SHAPE_HALFSPACE) {
            const double len = std::sqrt((double)S.b[0] * S.b[0] + (double)S.b[1] * S.b[1] + (double)S.b[2] * S.b[2]);
            SPH_REQUIRE(len > 0.0 && std::isfinite(len), SPH_E_INVALID, "shape %u: the normal is zero", j);
            for (int k = 0; k < 3; k++) S.b[k] = (float)((double)S.b[k] / len);
            S.r = 0.f;
        }
        if (S.kind == SPH_SHAPE_SPHERE) S.b[0] = S.b[1] = S.b[2] = 0.f;
        out->s[j] = S;
    }
    return SPH_OK;
}

int obstacle_ctx(const sph_ctx* c, const char* who) {
    SPH_REQUIRE(c, SPH_E_INVALID, "null context");
    SPH_REQUIRE(!c->slab, SPH_E_STATE, "%s is not supported on a slab context (its step makes several force launches with holes, "
                "and ghosts arrive integrated)", who);
    return SPH_OK;
}

// The checked grid G becomes the context's: the old obstacle leaves (once the stream is idle), the two buffers are allocated.
// On failure there is no obstacle.
int install_begin(sph_ctx* c, const sph_obstacle_grid& G) {
    SPH_HIP(hipSetDevice(c->device));
    Obstacle& o = selected_obstacle(c);
    if (o.installed()) {
        SPH_HIP(hipStreamSynchronize(c->stream));          // (a push of the old grid may still be running)
        release_obstacle(c);
    }
    const size_t nodes = (size_t)G.dims[0] * G.dims[1] * G.dims[2];
    const size_t bricks = (size_t)ob_bricks_axis(G.dims[0]) * ob_bricks_axis(G.dims[1]) * ob_bricks_axis(G.dims[2]);
    int rc = c->mem.alloc(&o.phi, nodes, false);
    if (!rc) rc = c->mem.alloc(&o.brick, bricks, false);
    if (rc) { release_obstacle(c); return rc; }
    o.grid = G;
    return SPH_OK;
}

int install_finish(sph_ctx* c) {
    const Obstacle& o = selected_obstacle(c);
    const ObstacleArgs A = obstacle_args(o);
    const uint32_t bricks = A.nb[0] * A.nb[1] * A.nb[2];
    hipLaunchKernelGGL(k_obstacle_bricks, dim3(ceil_div(bricks, OBSTACLE_THREADS)), dim3(OBSTACLE_THREADS), 0, c->stream, A, o.brick,
                       bricks);
    SPH_HIP(hipGetLastError());
    return SPH_OK;
}

}  // namespace sph

using namespace sph;

extern "C" {

int sph_obstacle_lattice(const sph_ctx* c, float spacing, const float lo[3], const float hi[3], sph_obstacle_grid* out) {
    SPH_REQUIRE(c && out, SPH_E_INVALID, "null argument");
    return lattice_resolve(c, spacing, lo, hi, out);
}

int sph_obstacle_build(sph_ctx* c, float spacing, const float lo[3], const float hi[3], uint32_t n, const sph_shape* shapes) {
    if (int e = obstacle_ctx(c, "sph_obstacle_build")) return e;
    sph_obstacle_grid G;
    Shapes sh{};
    if (int e = lattice_resolve(c, spacing, lo, hi, &G)) return e;
    if (int e = check_shapes(n, shapes, &sh)) return e;
    if (int e = install_begin(c, G)) return e;
    const uint32_t nodes = G.dims[0] * G.dims[1] * G.dims[2];
    const Obstacle& o = selected_obstacle(c);
    hipLaunchKernelGGL(k_obstacle_raster, dim3(ceil_div(nodes, OBSTACLE_THREADS)), dim3(OBSTACLE_THREADS), 0, c->stream, o.phi, nodes,
                       obstacle_args(o), sh, ob_clamp_distance(G));
    SPH_HIP(hipGetLastError());
    return install_finish(c);
}

int sph_obstacle_set_grid(sph_ctx* c, const sph_obstacle_grid* grid, const float* phi) {
    if (int e = obstacle_ctx(c, "sph_obstacle_set_grid")) return e;
    SPH_REQUIRE(grid && phi, SPH_E_INVALID, "null argument");
    const sph_obstacle_grid G = *grid;
    if (int e = check_grid(G)) return e;
    const size_t nodes = (size_t)G.dims[0] * G.dims[1] * G.dims[2];
    for (size_t i = 0; i < nodes; i++)
        SPH_REQUIRE(std::isfinite(phi[i]), SPH_E_INVALID, "obstacle grid: phi[%zu] is not finite", i);
    if (int e = install_begin(c, G)) return e;
    Obstacle& o = selected_obstacle(c);
    hipError_t he = hipMemcpyAsync(o.phi, phi, nodes * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(k_obstacle_clamp, dim3(ceil_div((uint32_t)nodes, OBSTACLE_THREADS)), dim3(OBSTACLE_THREADS), 0, c->stream,
                           o.phi, (uint32_t)nodes, ob_clamp_distance(G));
        he = hipGetLastError();
    }
    int rc = he == hipSuccess ? install_finish(c) : hip_fail(he, "obstacle upload", __FILE__, __LINE__);
    if (!rc) {
        he = hipStreamSynchronize(c->stream);              // (the caller's array is free again)
        if (he != hipSuccess) rc = hip_fail(he, "hipStreamSynchronize", __FILE__, __LINE__);
    }
    if (rc) release_obstacle(c);
    return rc;
}

int sph_obstacle_clear(sph_ctx* c) {
    if (int e = obstacle_ctx(c, "sph_obstacle_clear")) return e;
    Obstacle& o = selected_obstacle(c);
    if (o.installed()) {                                   // (only then: the other slots' pushes do not read this one)
        SPH_HIP(hipSetDevice(c->device));
        SPH_HIP(hipStreamSynchronize(c->stream));
        release_obstacle(c);
    }
    for (int k = 0; k < 3; k++) o.off[k] = o.vel[k] = 0.f;
    pose_reset(o);
    o.body = false;                                        // (the block stays for the slot's next body, as the sensor's buffers do)
    if (o.load) {                                       // (the sensor's switch stays; its sums and the integrate count start again)
        SPH_HIP(hipSetDevice(c->device));
        SPH_HIP(hipMemsetAsync(o.load, 0, OBSTACLE_LOAD_WORDS * sizeof(double), c->stream));
    }
    return SPH_OK;
}

int sph_obstacle_set_pose(sph_ctx* c, const sph_obstacle_pose* pose) {
    if (int e = obstacle_ctx(c, "sph_obstacle_set_pose")) return e;
    Obstacle& o = selected_obstacle(c);
    SPH_REQUIRE(pose || !o.body, SPH_E_STATE, "sph_obstacle_set_pose(NULL): the slot has a body, which needs a pose "
                "(sph_obstacle_set_body(NULL) first)");
    if (!pose) { pose_reset(o); return SPH_OK; }
    const sph_obstacle_pose p = *pose;
    for (int k = 0; k < 3; k++)
        SPH_REQUIRE(std::isfinite(p.pivot[k]) && std::isfinite(p.omega[k]), SPH_E_INVALID, "obstacle pose: pivot or omega is not finite");
    for (int k = 0; k < 4; k++) SPH_REQUIRE(std::isfinite(p.quat[k]), SPH_E_INVALID, "obstacle pose: the quaternion is not finite");
    const double q[4] = {(double)p.quat[0], (double)p.quat[1], (double)p.quat[2], (double)p.quat[3]};
    double unit[4];
    SPH_REQUIRE(ob_quat_unit(q, unit), SPH_E_INVALID, "obstacle pose: the quaternion's squared norm is 0 or not finite");
    if (o.body) {                                          // the block is the state: written on the stream, no host wait
        ObstacleBodyBlock v{};
        for (int k = 0; k < 3; k++) { v.pivot[k] = p.pivot[k]; v.omega[k] = p.omega[k]; }
        for (int k = 0; k < 4; k++) v.quat[k] = unit[k];
        ob_rot_of(unit, v.rot);
        return body_put(c, o, v, OB_PUT_POSE);
    }
    o.posed = true;
    for (int k = 0; k < 3; k++) { o.pivot[k] = p.pivot[k]; o.omega[k] = p.omega[k]; }
    for (int k = 0; k < 4; k++) o.quat[k] = unit[k];
    return SPH_OK;
}

int sph_obstacle_get_pose(const sph_ctx* c, int* posed, float pivot[3], double quat[4], float omega[3], float rot[9]) {
    SPH_REQUIRE(c, SPH_E_INVALID, "null context");
    const Obstacle& o = selected_obstacle(c);
    if (o.body) {                                          // the host's copy is stale: synchronises
        ObstacleBodyBlock b;
        if (int e = body_fetch(c, o, &b)) return e;
        if (posed) *posed = 1;
        for (int k = 0; k < 3; k++) {
            if (pivot) pivot[k] = b.pivot[k];
            if (omega) omega[k] = b.omega[k];
        }
        if (quat) for (int k = 0; k < 4; k++) quat[k] = b.quat[k];
        if (rot) for (int k = 0; k < 9; k++) rot[k] = b.rot[k];
        return SPH_OK;
    }
    if (posed) *posed = o.posed ? 1 : 0;
    for (int k = 0; k < 3; k++) {
        if (pivot) pivot[k] = o.pivot[k];
        if (omega) omega[k] = o.omega[k];
    }
    if (quat) for (int k = 0; k < 4; k++) quat[k] = o.quat[k];
    if (rot) ob_rot_of(o.quat, rot);
    return SPH_OK;
}

int sph_obstacle_set_sensor(sph_ctx* c, int on) {
    if (int e = obstacle_ctx(c, "sph_obstacle_set_sensor")) return e;
    Obstacle& o = selected_obstacle(c);
    SPH_REQUIRE(on || !o.body, SPH_E_STATE, "sph_obstacle_set_sensor(0): the slot has a body, which the load drives "
                "(sph_obstacle_set_body(NULL) first)");
    if (on && !o.load) {
        SPH_HIP(hipSetDevice(c->device));
        if (int rc = sensor_buffers_alloc(c, o)) return rc;
    }
    o.sense = on != 0;
    return SPH_OK;
}

int sph_obstacle_get_load(sph_ctx* c, double J[3], double L[3], float about[3], uint64_t* steps) {
    if (int e = obstacle_ctx(c, "sph_obstacle_get_load")) return e;
    const Obstacle& o = selected_obstacle(c);
    double host[OBSTACLE_LOAD_WORDS] = {};
    if (o.load) {
        SPH_HIP(hipSetDevice(c->device));
        SPH_HIP(hipMemcpyAsync(host, o.load, sizeof(host), hipMemcpyDeviceToHost, c->stream));
        SPH_HIP(hipStreamSynchronize(c->stream));
    }
    for (int k = 0; k < 3; k++) {
        if (J) J[k] = host[k];
        if (L) L[k] = host[3 + k];
    }
    if (steps) std::memcpy(steps, &host[6], sizeof(uint64_t));
    if (about) std::memcpy(about, &host[7], 3 * sizeof(float));
    return SPH_OK;
}

int sph_obstacle_set_body(sph_ctx* c, const sph_obstacle_body* body) {
    if (int e = obstacle_ctx(c, "sph_obstacle_set_body")) return e;
    Obstacle& o = selected_obstacle(c);
    if (!body) {                                           // the slot goes on kinematic from where it is
        if (!o.body) return SPH_OK;
        ObstacleBodyBlock b;
        if (int e = body_fetch(c, o, &b)) return e;
        for (int k = 0; k < 3; k++) { o.off[k] = b.off[k]; o.vel[k] = b.u[k]; o.pivot[k] = b.pivot[k]; o.omega[k] = b.omega[k]; }
        for (int k = 0; k < 4; k++) o.quat[k] = b.quat[k];
        o.body = false;
        return SPH_OK;
    }
    const sph_obstacle_body b = *body;
    constexpr uint32_t FREE = SPH_BODY_FREE_X | SPH_BODY_FREE_Y | SPH_BODY_FREE_Z;
    SPH_REQUIRE((b.dof & ~(FREE | SPH_BODY_SPIN | SPH_BODY_HINGE)) == 0u, SPH_E_INVALID, "obstacle body: dof %u has unknown bits", b.dof);
    SPH_REQUIRE(!((b.dof & SPH_BODY_SPIN) && (b.dof & SPH_BODY_HINGE)), SPH_E_INVALID, "obstacle body: SPIN and HINGE exclude each other");
    if (b.dof & FREE)
        SPH_REQUIRE(std::isfinite(b.mass) && b.mass > 0.f, SPH_E_INVALID, "obstacle body: mass %g is not a positive finite number",
                    (double)b.mass);
    for (int k = 0; k < 3; k++) {
        SPH_REQUIRE(std::isfinite(b.accel[k]) && std::isfinite(b.torque[k]), SPH_E_INVALID, "obstacle body: accel or torque is not finite");
        if (b.dof & (1u << k))
            SPH_REQUIRE(std::isfinite(b.lo[k]) && std::isfinite(b.hi[k]) && b.lo[k] <= b.hi[k], SPH_E_INVALID,
                        "obstacle body: the offset's bounds on axis %d are [%g, %g]", k, (double)b.lo[k], (double)b.hi[k]);
        if ((b.dof & SPH_BODY_SPIN) || ((b.dof & SPH_BODY_HINGE) && k == 0))
            SPH_REQUIRE(std::isfinite(b.inertia[k]) && b.inertia[k] > 0.f, SPH_E_INVALID,
                        "obstacle body: moment %d is %g, not a positive finite number", k, (double)b.inertia[k]);
    }
    double axis[3] = {0.0, 0.0, 0.0};
    if (b.dof & SPH_BODY_HINGE) {
#pragma clang fp contract(off)
        const double x = (double)b.axis[0], y = (double)b.axis[1], z = (double)b.axis[2];
        const double n2 = (x * x + y * y) + z * z;
        SPH_REQUIRE(std::isfinite(n2) && n2 > 0.0, SPH_E_INVALID, "obstacle body: the hinge's axis is zero or not finite");
        const double len = std::sqrt(n2);
        axis[0] = x / len; axis[1] = y / len; axis[2] = z / len;
    }
    SPH_REQUIRE(o.posed, SPH_E_STATE, "sph_obstacle_set_body: the slot has no pose (sph_obstacle_set_pose first; the identity "
                "quaternion will do)");
    SPH_HIP(hipSetDevice(c->device));
    const bool had_load = o.load != nullptr;
    if (!had_load)
        if (int rc = sensor_buffers_alloc(c, o)) return rc;
    if (!o.blk) {
        if (int rc = c->mem.alloc(&o.blk, 1, true)) {
            if (!had_load) { c->mem.release(&o.load); c->mem.release(&o.wmask); c->mem.release(&o.rows); }
            return rc;
        }
    }
    if (!o.body) {                                         // the state moves to the device: what a kinematic slot would launch with
        if (int rc = body_put(c, o, body_block_of(o), OB_PUT_OFF | OB_PUT_U | OB_PUT_POSE)) return rc;
    }
    o.bd = b;
    for (int k = 0; k < 3; k++) o.axis[k] = axis[k];
    o.sense = true;
    o.body = true;
    return SPH_OK;
}

int sph_obstacle_get_body(const sph_ctx* c, int* has_body, sph_obstacle_body* out) {
    SPH_REQUIRE(c, SPH_E_INVALID, "null context");
    const Obstacle& o = selected_obstacle(c);
    if (has_body) *has_body = o.body ? 1 : 0;
    if (out) *out = o.body ? o.bd : sph_obstacle_body{};
    return SPH_OK;
}

int sph_obstacle_set_motion(sph_ctx* c, const float offset[3], const float velocity[3]) {
    if (int e = obstacle_ctx(c, "sph_obstacle_set_motion")) return e;
    Obstacle& o = selected_obstacle(c);
    for (int k = 0; k < 3; k++)
        SPH_REQUIRE((!offset || std::isfinite(offset[k])) && (!velocity || std::isfinite(velocity[k])), SPH_E_INVALID,
                    "obstacle motion: offset or velocity is not finite");
    if (o.body) {                                          // the block is the state: written on the stream, no host wait
        if (!offset && !velocity) return SPH_OK;
        ObstacleBodyBlock v{};
        for (int k = 0; k < 3; k++) { v.off[k] = offset ? offset[k] : 0.f; v.u[k] = velocity ? velocity[k] : 0.f; }
        return body_put(c, o, v, (offset ? OB_PUT_OFF : 0u) | (velocity ? OB_PUT_U : 0u));
    }
    for (int k = 0; k < 3; k++) {
        if (offset) o.off[k] = offset[k];
        if (velocity) o.vel[k] = velocity[k];
    }
    return SPH_OK;
}

int sph_obstacle_get(const sph_ctx* c, sph_obstacle_grid* grid, float offset[3], float velocity[3]) {
    SPH_REQUIRE(c, SPH_E_INVALID, "null context");
    const Obstacle& o = selected_obstacle(c);
    if (grid) *grid = o.grid;
    if (o.body && (offset || velocity)) {                  // the host's copy is stale: synchronises
        ObstacleBodyBlock b;
        if (int e = body_fetch(c, o, &b)) return e;
        for (int k = 0; k < 3; k++) {
            if (offset) offset[k] = b.off[k];
            if (velocity) velocity[k] = b.u[k];
        }
        return SPH_OK;
    }
    for (int k = 0; k < 3; k++) {
        if (offset) offset[k] = o.off[k];
        if (velocity) velocity[k] = o.vel[k];
    }
    return SPH_OK;
}

int sph_obstacle_read(sph_ctx* c, float* phi) {
    SPH_REQUIRE(c && phi, SPH_E_INVALID, "null argument");
    const Obstacle& o = selected_obstacle(c);
    SPH_REQUIRE(o.installed(), SPH_E_STATE, "sph_obstacle_read: no obstacle is installed");
    SPH_HIP(hipSetDevice(c->device));
    const size_t nodes = (size_t)o.grid.dims[0] * o.grid.dims[1] * o.grid.dims[2];
    SPH_HIP(hipMemcpyAsync(phi, o.phi, nodes * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SPH_HIP(hipStreamSynchronize(c->stream));
    return SPH_OK;
}

int sph_obstacle_sample(sph_ctx* c, uint32_t n, const float* pos_xyz, float* phi, float* normal_xyz, uint8_t* inside_grid) {
    SPH_REQUIRE(c, SPH_E_INVALID, "null context");
    const Obstacle& o = selected_obstacle(c);
    SPH_REQUIRE(o.installed(), SPH_E_STATE, "sph_obstacle_sample: no obstacle is installed");
    SPH_REQUIRE(n == 0 || pos_xyz, SPH_E_INVALID, "null positions");
    if (n == 0) return SPH_OK;
    SPH_HIP(hipSetDevice(c->device));
    Buffers tmp;                                   // the call's temporaries: points in, three planes out
    float* d_pos = nullptr; float* d_phi = nullptr; float* d_nrm = nullptr; uint8_t* d_in = nullptr;
    int rc = tmp.alloc(&d_pos, (size_t)n * 3, false);
    if (!rc) rc = tmp.alloc(&d_phi, n, false);
    if (!rc) rc = tmp.alloc(&d_nrm, (size_t)n * 3, false);
    if (!rc) rc = tmp.alloc(&d_in, n, false);
    auto hip = [&](hipError_t e, const char* what) { if (!rc && e != hipSuccess) rc = hip_fail(e, what, __FILE__, __LINE__); };
    if (!rc) {
        hip(hipMemcpyAsync(d_pos, pos_xyz, (size_t)n * 12, hipMemcpyHostToDevice, c->stream), "copy of the points");
        if (!rc) {
            if (o.body)
                hipLaunchKernelGGL((k_obstacle_sample<true, true>), dim3(ceil_div(n, OBSTACLE_THREADS)), dim3(OBSTACLE_THREADS), 0,
                                   c->stream, d_pos, n, obstacle_args(o), d_phi, d_nrm, d_in, ObstaclePoseBody{obstacle_pose(o), o.blk});
            else if (o.posed)
                hipLaunchKernelGGL(k_obstacle_sample<true>, dim3(ceil_div(n, OBSTACLE_THREADS)), dim3(OBSTACLE_THREADS), 0, c->stream,
                                   d_pos, n, obstacle_args(o), d_phi, d_nrm, d_in, obstacle_pose(o));
            else
                hipLaunchKernelGGL(k_obstacle_sample<false>, dim3(ceil_div(n, OBSTACLE_THREADS)), dim3(OBSTACLE_THREADS), 0, c->stream,
                                   d_pos, n, obstacle_args(o), d_phi, d_nrm, d_in, obstacle_pose(o));
            hip(hipGetLastError(), "k_obstacle_sample");
        }
        if (!rc && phi) hip(hipMemcpyAsync(phi, d_phi, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream), "copy of phi");
        if (!rc && normal_xyz) hip(hipMemcpyAsync(normal_xyz, d_nrm, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream), "copy of the normals");
        if (!rc && inside_grid) hip(hipMemcpyAsync(inside_grid, d_in, n, hipMemcpyDeviceToHost, c->stream), "copy of the flags");
        hipError_t e = hipStreamSynchronize(c->stream);    // (also on an error: the temporaries are about to go)
        hip(e, "hipStreamSynchronize");
    }
    tmp.free_all();
    return rc;
}

int sph_obstacle_select(sph_ctx* c, uint32_t slot) {
    if (int e = obstacle_ctx(c, "sph_obstacle_select")) return e;
    SPH_REQUIRE(slot < (uint32_t)SPH_MAX_OBSTACLES, SPH_E_INVALID, "obstacle slot %u: 0..%d", slot, SPH_MAX_OBSTACLES - 1);
    c->ob_sel = slot;
    return SPH_OK;
}

uint32_t sph_obstacle_selected(const sph_ctx* c) { return c ? c->ob_sel : 0u; }

uint32_t sph_obstacle_installed(const sph_ctx* c, uint32_t* mask) {
    uint32_t count = 0, m = 0;
    if (c)
        for (uint32_t k = 0; k < (uint32_t)SPH_MAX_OBSTACLES; k++)
            if (c->ob[k].installed()) { count++; m |= 1u << k; }
    if (mask) *mask = m;
    return count;
}

int sph_obstacle_clear_all(sph_ctx* c) {
    if (int e = obstacle_ctx(c, "sph_obstacle_clear_all")) return e;
    int rc = SPH_OK;
    for (uint32_t k = 0; k < (uint32_t)SPH_MAX_OBSTACLES; k++) {
        c->ob_sel = k;
        const int e = sph_obstacle_clear(c);
        if (e && !rc) rc = e;
    }
    c->ob_sel = 0;
    return rc;
}

}  // extern "C"

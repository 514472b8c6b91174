// sph_common.hpp -- shared declarations of libsph_hip.so (host side + device helpers).
// MI355X / gfx950 only: wave64, no portability layer.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sph_hip.h"

namespace sph {

constexpr int WAVE = 64;
#ifndef SPH_SORT_KPT
#define SPH_SORT_KPT 16
#endif
constexpr uint32_t SORT_TILE_KEYS = 256 * SPH_SORT_KPT;   // keys per radix-sort tile (sph_sort.hip)
#ifndef SPH_PAIR_SMALL_SLOTS_DEFAULT
#define SPH_PAIR_SMALL_SLOTS_DEFAULT 524288u
#endif
constexpr uint32_t MM_TILE_CHUNKS = 256;   // merge sort: 64-slot chunks per scan tile (sph_sort.hip)
constexpr uint32_t SCRATCH_WORDS = 64;     // words of a context's d_scratch / h_scratch pair (counts; the answers of sph_halo.hip's lower bounds)

// Grid description passed by value to kernels (replaces the device-resident SimParams*
// every reference kernel dereferences, particleSystem.cu:93-103,127-130).
struct GridDesc {
    float box_min[3];
    float box_dims[3];     // box_max - box_min
    float inv_dims[3];     // 1 / box_dims where that is a power of two (the division is then an exact scaling), else 0
    uint32_t g[3];         // global cells per axis
    float gf[3];           // (float)g
    int32_t z_off;         // local z layer = global z layer - z_off (slab: z_lo - ghost layers; whole domain: 0)
    uint32_t zl;           // local z layers (slab: owned + 2 x ghost layers; whole domain: g[2])
    uint32_t ncells;       // g[0]*g[1]*zl
};

struct Phys {
    float h, h2;
    float mass;
    float rest_density, gas_constant;
    float poly6_mass;      // MASS * 315/(65*pi*h^9)        (particleSystem.cu:30,35)
    float spiky_half_mass; // MASS * 45/(pi*h^6) / 2         (particleSystem.cu:41,47; sign folded)
    float visc_coef;       // VISC * MASS * 45/(pi*h^6)      (particleSystem.cu:42,48)
    float cp_scale;        // spiky_half_mass / visc_coef: the pressure coefficient relative to the viscous one (sph_pairs.hip)
    float gravity_y;
    float wall_eps, wall_damping;
    float coll_dist2;      // (COLLISION_PARAM * 2 * radius)^2 (particleSystem.cu:61)
    float coll_mass;       // MASS * (1 + RESTITUTION)        (particleSystem.cu:62)
    float box_min[3], box_max[3];
    float visc_on;         // 1, or 0 for viscosity = 0: visc_coef is then folded with viscosity 1 (cp_scale stays finite) and k_force
                           // multiplies its viscous sum by this (by 1.0f: not a bit changes)
};

// The sphere colliders of a context (sph_set_colliders) as the collider instantiations of k_force / k_integrate take them: a
// kernel argument by value -- a 256-byte table and its count -- so that they cost no dispatch and no copy of their own.
struct Spheres {
    float4 c[SPH_MAX_COLLIDERS];   // centre, R + wall_eps
    float4 u[SPH_MAX_COLLIDERS];   // velocity, (R + wall_eps)^2
    uint32_t n;
};

// The same table for a TRACKED context (sph_set_collider_bodies): it lives in device memory, where k_spheres_step moves the
// spheres once per step, and the tracked instantiations of k_force / k_integrate take a pointer to it plus the per-step outputs.
// Every wave of a tracked launch stores one mask word -- which spheres it wrote a row of partial sums for -- so that nothing
// has to be cleared between steps.
struct SpheresTracked {
    const Spheres* table;     // device
    double* partial;          // [wave][SPH_MAX_COLLIDERS][3]: the wave's sum of -(mass * (k * nrm)) for sphere j
    uint32_t* mask;           // [wave]: bit j = partial[wave][j] was written by this launch
    uint32_t rel;             // the lane's slot relative to the first owned slot (filled in by the kernel: wave = rel / 64)
};

// The bodies of a tracked context as k_spheres_step takes them: by value.
struct SphereBodies {
    float4 am[SPH_MAX_COLLIDERS];    // accel, mass (0: kinematic)
    float radius[SPH_MAX_COLLIDERS]; // R (the wall rule's eps of a free body)
};

constexpr uint32_t SPHERES_STEP_THREADS = 256;   // k_spheres_step: one block (sph_pairs.hip)

void set_error(const char* fmt, ...);

// ---- device and pinned memory: one owner per object ----
// A Buffers allocates, remembers and frees: sph_ctx, sph_slab, the compat seam's scratch and every call with temporaries hold one.
// free_all frees what is left in reverse order of allocation -- the owner's destroy calls it; there is no destructor, so that
// nothing is freed while the process exits -- and release frees one buffer early (an image that changes size, a table that
// grows).  The four HIP allocation calls appear nowhere else in the library.
inline std::atomic<uint64_t> g_mem_stats[3];   // live device bytes, live pinned bytes, live buffers (sph_memory_stats)
inline std::atomic<uint32_t> g_fail_alloc{0};  // [test hook] sph_test_fail_alloc: the k-th allocation from now fails, once
// [test hook] sph_test_guard: while g_guard_band is not 0, every allocation gets a band of that many bytes in front of the
// caller's range and another behind it, both filled with guard_word; with g_guard_fill the range itself gets the pattern too
// unless it is zeroed.  sph_test_guard_check compares the bands of every guarded buffer (sph_capi.hip has the registry).
inline std::atomic<uint32_t> g_guard_band{0};
inline std::atomic<uint32_t> g_guard_fill{0};
// word `w` of a guarded allocation, counted from its base pointer (the trailing band starts at the next word boundary behind the
// caller's bytes): 1 .. 511, a subnormal as fp32, and no two words a small distance apart hold the same sequence
__host__ __device__ inline uint32_t guard_word(uint64_t w) { return 1u + (uint32_t)((w + 7u * (w >> 8)) % 511u); }
int guard_adopt(void* base, size_t bytes, uint32_t band, bool pinned, bool fill);   // fills, registers; nonzero: HIP failed
void guard_retire(void* user, size_t bytes, uint32_t band, bool pinned);            // checks the bands, latches, unregisters

struct Buffers {
    struct Rec { void* p; size_t bytes; bool pinned; uint32_t band; };   // band: guard bytes on either side of p (0: none)
    std::vector<Rec> live;
    Buffers() = default;
    Buffers(const Buffers&) = delete;
    Buffers& operator=(const Buffers&) = delete;
    // `count` elements of device memory (0: one element), as zeros if `zero`
    template <class T> int alloc(T** p, size_t count, bool zero) {
        const size_t bytes = (count ? count : 1) * sizeof(T);
        int rc = take((void**)p, bytes, false, false, !zero);
        if (rc || !zero || hipMemset((void*)*p, 0, bytes) == hipSuccess) return rc;
        release(p);
        set_error("hipMemset of %zu bytes failed", bytes);
        return SPH_E_DEVICE;
    }
    // pinned host memory; with `dev_view` it is mapped, and *dev_view is the device's pointer to it
    template <class T> int alloc_host(T** p, size_t count, T** dev_view = nullptr) {
        int rc = take((void**)p, count * sizeof(T), true, dev_view != nullptr, true);
        if (rc || !dev_view || hipHostGetDevicePointer((void**)dev_view, (void*)*p, 0) == hipSuccess) return rc;
        release(p);
        set_error("hipHostGetDevicePointer failed");
        return SPH_E_NOMEM;
    }
    template <class T> void release(T** p) {
        for (size_t k = live.size(); k-- > 0;)
            if (live[k].p == (void*)*p) { drop(live[k]); live.erase(live.begin() + k); break; }
        *p = nullptr;
    }
    void free_all() {
        while (!live.empty()) { drop(live.back()); live.pop_back(); }
    }

private:
    // `unzeroed`: the caller does not clear the range (what the guard mode's second flag fills with the pattern)
    int take(void** p, size_t bytes, bool pinned, bool mapped, bool unzeroed) {
        const char* fn = !pinned ? "hipMalloc" : mapped ? "hipHostMalloc(mapped)" : "hipHostMalloc";
        *p = nullptr;
        uint32_t k = g_fail_alloc.load();
        while (k && !g_fail_alloc.compare_exchange_weak(k, k - 1)) {}
        const uint32_t band = g_guard_band.load();
        const size_t total = band ? ((bytes + 3) & ~(size_t)3) + 2 * (size_t)band : bytes;
        const hipError_t e = k == 1 ? hipErrorOutOfMemory
                           : pinned ? hipHostMalloc(p, total, mapped ? hipHostMallocMapped : hipHostMallocDefault) : hipMalloc(p, total);
        if (e != hipSuccess) {
            *p = nullptr;
            set_error("%s of %zu bytes failed: %s", fn, bytes, hipGetErrorString(e));
            return SPH_E_NOMEM;
        }
        if (band) {
            if (guard_adopt(*p, bytes, band, pinned, unzeroed && g_guard_fill.load())) {
                if (pinned) hipHostFree(*p); else hipFree(*p);
                *p = nullptr;
                set_error("the guard bands of %zu bytes could not be written", bytes);
                return SPH_E_DEVICE;
            }
            *p = (char*)*p + band;
        }
        live.push_back(Rec{*p, bytes, pinned, band});
        g_mem_stats[pinned] += bytes; g_mem_stats[2] += 1;
        return SPH_OK;
    }
    static void drop(const Rec& r) {
        void* base = r.p;
        if (r.band) { guard_retire(r.p, r.bytes, r.band, r.pinned); base = (char*)r.p - r.band; }
        if (r.pinned) hipHostFree(base); else hipFree(base);
        g_mem_stats[r.pinned] -= r.bytes; g_mem_stats[2] -= 1;
    }
};

// What sph_hash leaves of the old cell table to the sort that follows it.  It lives in the context because the two are
// separate public calls; launch_sort takes it (table_take_left), and clearing or forgetting the table resets it.
enum class TableLeft : uint8_t {
    NOTHING,            // the hash cleared the table (or there was none)
    OWNED,              // the table of the owned slots stays live for a merging sort, which clears only the cells the movers leave
    OWNED_AND_GHOSTS    // ... and the cells of the old ghosts are still in it (the slab step: spare blocks of the sort's
                        // k_mm_compact clear them, ~6 us less than a kernel of their own at the head of every rank's step)
};

// The cell table and what the host knows of it.  Everybody reads it (table_covers); it is written only by the operations next
// to the launch_cells_* launchers (sph_pairs.hip) and by table_set below.
struct CellTable {
    uint2* cells = nullptr;        // = base + 1
    uint2* base = nullptr;         // the allocation: ncells + one zero guard entry on either side
    uint32_t alloc = 0;            // cells the allocation holds (a slab whose layer range grows gets a bigger table: set_slab_range)
    uint32_t lo = 0, hi = 0;       // slot range the table was built from
    bool valid = false;
    TableLeft left = TableLeft::NOTHING;
};

// The movers the fused integrate epilogue marked for the next sort, and the count of them the host may look at.  Owned by
// sph_sort.hip (mm_set_marks, mm_scan_marks, mm_drop_marks, launch_merge_count).
struct MoverMarks {
    bool marked = false;           // mm_mask / mm_tile_cnt hold the marks of the slots [off, off + n)
    bool scanned = false;          // ... and the scan that counts them is already queued (mm_scan_marks)
    uint32_t off = 0, n = 0;
    uint32_t scan_seq = 0;         // mover counts queued so far (k_mm_tilescan; k_mm_compact when it counts itself)
    bool counted_valid = false;    // the last count queued (scan_seq) is that of the CURRENT marks
};

// The words of the mapped host block mm_count_host, which the device writes and the host only looks at (sph_ctx below).
enum HostWord : uint32_t {
    HW_MOVERS = 0,     // the last known mover count (a hint)
    HW_FIRST_KEY,      // the keys of the first / last owned slot after the last table build (block_order's estimate):
    HW_LAST_KEY,       // the two words cells_build_thread writes through `ends`
    HW_BUILD_SEQ,      // the number of the last sort whose table build has started (sort_throttle)
    HW_COUNT_SEQ,      // the number of the last mover count, stored AFTER the count itself (launch_sort's skip)
    HW_WORDS = 8
};

// One obstacle slot of a whole-domain context (sph_obstacle.hip): the clamped signed distances, 4 bytes per node, and the minimum
// of every brick of OBSTACLE_BRICK^3 cells; grid.dims = 0, 0, 0 and null pointers while there is none.  Allocated by the call
// that installs a grid, freed by sph_obstacle_clear; never by a caller who sets no obstacle.  The offset advances on the host
// once per step, next to the spheres' centres (sph_pairs.hip: advance_colliders).
// The state of a BODY slot (sph_obstacle_set_body), which lives on the device while the body is set: the push, the sample and
// the solids' march read it at kernel entry, k_obstacle_body moves it on once per integrate.  rot and P are what the next launch
// uses: rot from quat, each entry rounded once, and P = pivot + off.
struct ObstacleBodyBlock {
    double quat[4];
    float off[3], u[3], pivot[3], omega[3];
    float rot[9], P[3];
};

struct Obstacle {
    sph_obstacle_grid grid{};
    float* phi = nullptr;
    float* brick = nullptr;
    float off[3] = {0.f, 0.f, 0.f}, vel[3] = {0.f, 0.f, 0.f};
    // the rigid pose (sph_obstacle_set_pose): while `posed`, the grid's coordinates are a body frame turned by the unit
    // quaternion quat (w, x, y, z; double) about pivot, and omega is the angular velocity in world axes.  It belongs to the
    // slot like the motion and advances where the offset does (advance_obstacle).
    bool posed = false;
    float pivot[3] = {0.f, 0.f, 0.f}, omega[3] = {0.f, 0.f, 0.f};
    double quat[4] = {1.0, 0.0, 0.0, 0.0};
    // the load sensor (sph_obstacle_set_sensor): while `sense`, every push leaves one row of six float64 sums and one mask
    // word per wave, and k_obstacle_load adds them once per integrate.  Allocated when the slot's sensor is first switched on.
    bool sense = false;
    double* rows = nullptr;             // ceil(cap / 64) rows of 6: J, L
    uint32_t* wmask = nullptr;          // ceil(cap / 64) words, padded to whole quads plus one
    double* load = nullptr;             // J[3], L[3], the integrate count (uint64), about[3] (fp32) and a pad word: 72 bytes
    // the body (sph_obstacle_set_body): while `body`, off, vel, pivot, omega and quat above are STALE -- the block on the device
    // holds them, as trk_table holds the spheres of a tracked context -- and the slot is posed and sensing.  The block is
    // allocated at the slot's first set_body and freed by sph_destroy.
    bool body = false;
    sph_obstacle_body bd{};             // as the caller gave it
    double axis[3] = {0.0, 0.0, 0.0};   // HINGE: bd.axis normalised in double
    ObstacleBodyBlock* blk = nullptr;
    // an obstacle voxelised from a triangle mesh (sph_obstacle_mesh.hip) keeps the scratch of its build -- the work list with the
    // four counters in front, and the parity marks of the columns -- until the next installation, sph_obstacle_clear or
    // sph_destroy; both null for every other obstacle, and sph_obstacle_mesh_stats reads the counters
    uint64_t* mesh_work = nullptr;
    uint32_t* mesh_marks = nullptr;
    bool installed() const { return phi != nullptr; }
};

}  // namespace sph

// The opaque context of include/sph_hip.h.
struct sph_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    sph::Buffers mem;        // every device and pinned buffer below (sph_destroy frees them all)
    sph_params params{};
    int precision = SPH_PRECISION_F32;   // sph_set_precision
    sph::GridDesc grid{};
    sph::Phys phys{};

    uint32_t cap = 0;        // owned capacity
    uint32_t gcap = 0;       // ghost capacity per side (0: whole-domain context)
    uint32_t tot = 0;        // gcap + cap + gcap
    bool slab = false;
    uint32_t z_lo = 0, z_hi = 0;   // owned global cell layers
    // ghost cell layers a slab context keeps on either side of its owned layers: 1 (the three-message step: the neighbours'
    // boundary layers, whose densities arrive in a message of their own) or 2 (the one-message step: two layers of the
    // neighbour's particles, the densities of the inner one recomputed here) -- sph_create_slab_layers
    uint32_t ghost_layers = 1;

    // counts
    uint32_t n = 0;          // owned particles
    uint32_t own_off = 0;    // offset of the owned range inside posi/velr (gcap after a sort)
    uint32_t n_glo = 0, n_ghi = 0;   // ghosts installed below / above
    uint32_t halo_n[2] = {0, 0};     // boundary-layer counts of the last halo pack
    bool halo_n_valid = false;

    // sorted SoA state, `tot` entries each; the owned range starts at own_off
    float4* posi = nullptr;   // x, y, z, creation index (bits)
    float4* velr = nullptr;   // vx, vy, vz, unused
    float4* posi2 = nullptr;  // ping-pong targets of reorder / integrate
    float4* velr2 = nullptr;
    uint32_t* keyS = nullptr; // cell key per slot (same indexing as posi)
    uint32_t* keyS2 = nullptr;// ping-pong target of the sort
    float2* dp = nullptr;     // density, pressure
    float2* cw = nullptr;     // what the force pass needs of a NEIGHBOUR: cp_j = cp_scale * p_j, w_j = visc_coef / rho_j (0 where
                              // rho_j = 0: padding), written by the density pass next to dp (neighbour_terms, sph_device.hpp)
    float4* fpress = nullptr; // phase API outputs
    float4* fvisc = nullptr;
    float4* dvel = nullptr;   // delta_velocity xyz, collision count
    float4* pos_out = nullptr;// (x,y,z,1) by creation index: the gl_pos analogue
    uint32_t pos_out_cap = 0;
    // the creation index sph_emit hands out next when the caller gives none: one past the highest index uploaded, generated,
    // loaded or emitted so far (sph_upload and sph_reset_lattice start it again from the set they install; sph_edit.hip)
    uint32_t next_index = 0;

    // sphere colliders (sph_set_colliders): every integrate pushes the particles out of them, the centres advance on the host
    // once per step (sph_pairs.hip: push_out_of_spheres, advance_colliders); none by default
    uint32_t n_colliders = 0;
    sph_collider colliders[SPH_MAX_COLLIDERS] = {};
    // bodies (sph_set_collider_bodies): while `tracked`, the table trk_table on the device holds the centres and velocities
    // (`colliders` above keeps the radii and is otherwise stale), the tracked kernel instantiations run, and k_spheres_step
    // sums the impulses and moves the spheres once per step.  The buffers are allocated when tracking is first switched on.
    bool tracked = false;
    sph::SphereBodies bodies{};
    sph::Spheres* trk_table = nullptr;
    double* trk_partial = nullptr;      // ceil(cap / 64) rows of SPH_MAX_COLLIDERS x 3
    uint32_t* trk_mask = nullptr;       // ceil(cap / 64) words, padded to a multiple of 4
    double* trk_J = nullptr;            // SPH_MAX_COLLIDERS x 3 doubles of the last integrate, then the step count (uint64)

    // the obstacles (sph_obstacle.hip): SPH_MAX_OBSTACLES slots, each what `struct Obstacle` (above) holds, and the slot the
    // sph_obstacle_* calls address (sph_obstacle_select).  The installed slots act in ascending order behind every integrate.
    sph::Obstacle ob[SPH_MAX_OBSTACLES];
    uint32_t ob_sel = 0;

    // the image of the last sph_render (sph_render.hip): per pixel a 64-bit key (depth bits << 32 | slot) and the resolved
    // RGBA8, creation index and depth.  Allocated at the first render, again when the image size changes; never by a caller
    // who does not render.
    uint64_t* rd_keys = nullptr;
    uint32_t* rd_rgba = nullptr;
    uint32_t* rd_id = nullptr;
    float* rd_depth = nullptr;
    uint32_t rd_alloc_w = 0, rd_alloc_h = 0;    // what the buffers were allocated for
    uint32_t rd_w = 0, rd_h = 0;                // the last image
    bool rd_valid = false;
    unsigned long long* rd_counts = nullptr;    // fragment counters of the measuring build (SPH_RENDER_STATS); else never allocated
    // the extra planes of sph_render_surface, of the size of the image above: the raw sphere depth, the second plane of the
    // filter's ping-pong (the first is rd_depth), the thickness counts and the normals (4 + 4 + 4 + 12 bytes per pixel).
    // Allocated at the first surface render only, freed with the image.
    float* rd_sf_raw = nullptr;
    float* rd_sf_pong = nullptr;
    uint32_t* rd_sf_thick = nullptr;
    float* rd_sf_normal = nullptr;
    bool rd_surface = false;                    // the last render was a surface render (sph_render_surface_read)
    bool rd_sf_thick_on = false;                // ... and its thickness pass ran
    // the solids in the picture (sph_render_set_solids): the style as the caller gave it, and the planes the march leaves for
    // the surface's shading -- the nearest hit's depth (+inf: none), slot and eye-space normal (4 + 4 + 12 bytes per pixel).
    // Allocated at the first surface render with solids on, freed with the image; never while the style is off.
    bool rd_solids = false;
    sph_solid_style rd_solid_style{};
    float* rd_so_depth = nullptr;
    uint32_t* rd_so_slot = nullptr;
    float* rd_so_normal = nullptr;

    // the mesh of the last sph_mesh_extract (sph_mesh.hip): the lattice's counts and vertex bases (4 + 4 bytes per node), the
    // scans' block sums with the two totals and the case table in front (mesh_aux), and the vertices, normals and triangles.
    // Allocated at the first extraction or when one must grow; never by a caller who does not mesh.
    uint32_t* mesh_field = nullptr;
    uint32_t* mesh_vbase = nullptr;
    uint32_t* mesh_aux = nullptr;
    float* mesh_vpos = nullptr;
    float* mesh_vnrm = nullptr;
    uint32_t* mesh_tri = nullptr;
    uint32_t mesh_nodes_cap = 0, mesh_v_cap = 0, mesh_t_cap = 0;   // what the buffers hold: nodes, vertices, triangles
    uint32_t mesh_dims[3] = {0, 0, 0};          // the lattice of the last extraction
    uint32_t mesh_nv = 0, mesh_nt = 0;
    bool mesh_valid = false;

    // pair kernels: a (dz, dy) row whose staged hull would exceed this many slots is read straight from global memory
    // by every lane instead (sph_pairs.hip: traverse; sph_set_direct_hull)
    uint32_t direct_hull = 512;
    // pair kernels: a context with fewer owned particles than this launches blocks of 128 threads instead of 256 (sph_pairs.hip:
    // SMALL_THREADS_PAIR; same results bit for bit; sph_set_pair_small_launch)
    uint32_t pair_small_slots = SPH_PAIR_SMALL_SLOTS_DEFAULT;
    // pair kernels: the r < h cut of the hot launches as the fma's clamp modifier while h <= 1 (sph_pairs.hip: pair_clamp; same
    // results bit for bit); false (SPH_PAIR_CLAMP=0 at create time) keeps the v_max_f32 form at every h
    bool pair_clamp = true;
    // block order of the pair kernels (sph_device.hpp: BlockOrder; sph_set_block_order): every XCD walks a contiguous eighth
    // of the slots; the fused force pass also walks strips of 2^order_strip_sh blocks through the z layers of that eighth
    bool order_xcd = true, order_ztile = true;
    bool order_ztile_dens = true, order_xrot = true;        // (SPH_BLOCK_ORDER fields 4 and 5: the strips for the density pass too; XCD x starts at strip x * strips / 8)
    uint32_t order_strip_sh = 4;

    // cell table: {start, end} per local cell, zero = empty (sph::CellTable above; changed only by the operations at the head
    // of sph_pairs.hip)
    sph::CellTable table;
    bool keys_fresh = false;   // k0 already holds the keys of the current positions (written by the integrate epilogue)

    // radix sort scratch
    uint32_t* k0 = nullptr; uint32_t* v0 = nullptr;
    uint32_t* k1 = nullptr; uint32_t* v1 = nullptr;
    uint32_t* os_hist = nullptr;    // [group][4 passes][512 digits]: digit counts per group of 16 tiles
    uint32_t* os_base = nullptr;    // same shape: first output position of a (group, digit)
    uint32_t* os_tickets = nullptr; // one per pass (re-armed by k_os_scan)
    uint32_t* os_tot = nullptr;     // [4 passes][512 digits]: keys per digit
    uint32_t os_groups_cap = 0;
    unsigned long long* os_status = nullptr;   // (tile, digit) look-back words {epoch << 1 | is_prefix, count} (one-group sorts)
    uint32_t* os_status32 = nullptr;           // (tile, digit) words {epoch:19, count:13} (grouped sorts)
    uint32_t os_epoch = 0;          // changes with every pass of every sort: the status table is never cleared
    uint32_t* os_err_host = nullptr;           // pinned, mapped: set by a look-back that timed out
    uint32_t* os_err_dev = nullptr;
    uint32_t sort_blocks_cap = 0;
    uint32_t key_bits = 0;
    const uint32_t* last_perm = nullptr;   // v0 or v1: the permutation of the last sort; null = identity / not kept
    bool keep_perm = false;         // the merge path also writes the permutation (only the compat seam needs it)
    // the sort as a merge (sph_sort.hip: launch_sort_merge)
    bool sort_merge = true;         // SPH_SORT_MERGE=0 in the environment at create time turns it off
    bool sort_merge_always = false; // sph_set_sort_mode(c, 2): merge whatever the mover count (tests)
    bool order_valid = false;       // [own_off, own_off+n) is still in the order of the last sort, keyS = its keys
    bool last_sort_skipped = false;
    // A slab context is stepped by sph_slab_step, whose host waits for the device once per step: the host cannot run
    // ahead, so its run-ahead needs no bound.
    bool host_paced = false;
    // What the host learns from the device about the sorts WITHOUT events (every event recorded on a stream costs the device
    // ~5.5 us of idle at its next dispatch; rounds 1-5 recorded two per step in a whole-domain context: 11 us of a 92 us step
    // at 131,072 particles, profiles/r06base_headless_n131072_kernel_stats.csv): the kernels echo sequence numbers into the
    // mapped host block mm_count_host -- HW_BUILD_SEQ the number of the last sort whose table build has started (bounds the host's
    // run-ahead to four sorts), HW_COUNT_SEQ the number of the last mover count, stored AFTER the count HW_MOVERS (the skip of a sort with
    // nothing to do needs the count of the CURRENT marks: it is looked at, never waited for).
    uint32_t sort_seq_issued = 0;   // sorts that queued a table build so far
    uint64_t sort_merges = 0, sort_calls = 0, sort_skips = 0;   // skips: merges with no mover at all (nothing done)
    // A whole-domain context picks ONE form of the movers' sort from a count up to four steps old (radix_sort_bits).  A flow
    // changes that count slowly; the caller can change it at once (new positions or velocities for everybody: an upload, a
    // kick through sph_set_by_index, another box): for the sorts up to this call number both forms are launched again, or
    // a count that went from 0 to millions would go through the one-block sort's tile-by-tile fallback (~8 ms per sort at
    // 2 M movers, four times).
    uint64_t sort_form_both_until = 0;
    uint64_t sort_forms[3] = {0, 0, 0};   // movers' sorts launched as: both forms / the one-block sort alone / the multi-block passes alone
    uint64_t* mm_mask = nullptr;    // one bit per slot: key changed since the last sort
    uint32_t* mm_M64 = nullptr;     // movers before each 64-slot chunk
    uint32_t* mm_tile_cnt = nullptr; uint32_t* mm_tile_off = nullptr;
    uint32_t* mm_k0 = nullptr; uint32_t* mm_k1 = nullptr; uint32_t* mm_v1 = nullptr;   // mover (key, slot) ping-pong (+ v0)
    uint32_t* mm_count = nullptr;           // movers of the current sort (device)
    uint32_t* mm_count_host = nullptr;      // pinned, written by the device: the HW_WORDS words of sph::HostWord above
    uint32_t* mm_count_host_dev = nullptr;  // device view of the same word
    unsigned long long* mm_total = nullptr; // movers of all sorts so far (device; sph_sort_stats)
    sph::MoverMarks marks;          // the fused integrate epilogue already wrote mm_mask / mm_tile_cnt for a range
    uint32_t* mm_tileL = nullptr;   // coarse mover ranks per 4096 slots (k_mm_tile_rank)
    uint32_t* mm_tileA = nullptr;   // first key of every 4096-slot tile of the old order (k_mm_tile_rank)
    uint32_t* d_scratch = nullptr;  // small device scratch (counts)
    uint32_t* h_scratch = nullptr;  // pinned host mirror

    // state machine for the phase API
    enum Stage { ST_LOADED = 0, ST_HASHED, ST_SORTED, ST_CELLS } stage = ST_LOADED;
    bool have_force = false, have_coll = false, have_dens = false;

    // device timing
    bool timing = false;
    std::vector<hipEvent_t> events;   // triples: start event, stop event, phase id (see PhaseTimer)
    double ph_ms[SPH_PH_COUNT] = {0};
    uint32_t timed_steps = 0;
};

namespace sph {

void mm_set_marks(sph_ctx* c);      // sph_sort.hip: the integrate epilogue has marked the movers of the owned range
void mm_scan_marks(sph_ctx* c);     // ... count them now if the next sort could be skipped
void mm_drop_marks(sph_ctx* c, bool counted = false);     // ... forget them
int hip_fail(hipError_t e, const char* what, const char* file, int line);

#define SPH_HIP(call)                                                        \
    do {                                                                     \
        hipError_t e__ = (call);                                             \
        if (e__ != hipSuccess) return sph::hip_fail(e__, #call, __FILE__, __LINE__); \
    } while (0)

#define SPH_REQUIRE(cond, code, ...)          \
    do {                                      \
        if (!(cond)) {                        \
            sph::set_error(__VA_ARGS__);      \
            return (code);                    \
        }                                     \
    } while (0)

// kernel launchers (defined in the .hip files)
int launch_hash(sph_ctx* c);
int launch_reset_lattice(sph_ctx* c, const uint32_t lattice[3], int jitter, const float jitter_dims[3], uint64_t start,
                         uint32_t count);
// radix sort of (k0,v0)[0,n) + reorder into posi2/velr2/keyS, or the merge, or nothing (at rest); `owned_build_pending`: step_sort
int launch_sort(sph_ctx* c, bool* owned_build_pending = nullptr);
int launch_merge_arrivals(sph_ctx* c, uint32_t n_in, uint32_t n_front = 0);   // particles appended behind the sorted range join it
// the cell table (sph_pairs.hip): the first six keep c->table's description, the *_range / *_2ranges launchers only touch entries
int launch_cells_clear(sph_ctx* c);                   // clears the entries of the built range and forgets it (table_forget)
void table_forget(sph_ctx* c);                        // no table any more, nothing left to a sort (the entries are the caller's business)
int table_drop_ends(sph_ctx* c, uint32_t m_lo, uint32_t m_hi);   // a table over the owned slots loses the first m_lo and the last m_hi of them
int table_drop_ghosts(sph_ctx* c);                    // a table over the owned slots and the ghosts shrinks to the owned slots
int table_leave_to_sort(sph_ctx* c, bool ghosts_too); // sph_hash: the table stays live for a merging sort (TableLeft)
TableLeft table_take_left(sph_ctx* c);                // launch_sort: what the hash left, if the table is still there; taken once
int launch_cells_clear_range(sph_ctx* c, uint32_t lo, uint32_t hi);
// (`seq`: what a build over the whole owned range echoes into mm_count_host[HW_BUILD_SEQ] -- the sort's number, sort_throttle)
int launch_cells_build_range(sph_ctx* c, uint32_t lo, uint32_t hi, uint32_t seq = 0);
int launch_cells_clear_2ranges(sph_ctx* c, uint32_t lo0, uint32_t hi0, uint32_t lo1, uint32_t hi1);
int launch_cells_build_2ranges(sph_ctx* c, uint32_t lo0, uint32_t hi0, uint32_t lo1, uint32_t hi1);
int launch_cells_build(sph_ctx* c);
constexpr uint32_t CELLS_SPT = 4;                     // slots per thread of the table build (sph_device.hpp: cells_build_thread)
inline uint32_t cells_build_blocks(uint32_t count) { return (count + 256u * CELLS_SPT - 1u) / (256u * CELLS_SPT); }
int launch_density(sph_ctx* c);
int launch_force(sph_ctx* c, bool force, bool collide, bool integrate, float dt);
// sub-range forms for the slab driver (interior first, boundary layers once the ghosts are in)
int launch_density_range(sph_ctx* c, uint32_t lo, uint32_t hi);
int launch_density_hole(sph_ctx* c, uint32_t lo, uint32_t hi, uint32_t hole_lo, uint32_t hole_hi);   // [lo, hi) minus the hole
int launch_density_dev_range(sph_ctx* c, const uint32_t* range_dev, uint32_t max_count);            // range in device memory
int launch_force_dev_range(sph_ctx* c, const uint32_t* range_dev, uint32_t max_count, float dt);   // fused pass, range in device memory
int launch_force_hole(sph_ctx* c, uint32_t lo, uint32_t hi, uint32_t hole_lo, uint32_t hole_hi, bool force, bool collide,
                      bool integrate, float dt, bool mark);
bool force_begin(sph_ctx* c, bool integrate);
int launch_force_range(sph_ctx* c, uint32_t lo, uint32_t hi, bool force, bool collide, bool integrate, float dt, bool mark);
int force_finish(sph_ctx* c, bool integrate, bool mark, float dt);   // also advances the colliders' centres by dt (a tracked context: queues k_spheres_step)
// phase bodies of sph_capi.hip (with their bookkeeping), for the slab driver
int set_slab_range(sph_ctx* c, uint32_t z_lo, uint32_t z_hi);   // sph_capi.hip: a slab context takes over another layer range (its table must be clear)
// `ghosts_to_sort`: the cells of the old ghosts are cleared by the sort that the caller runs next, not by a kernel of their own
int step_hash(sph_ctx* c, bool ghosts_to_sort = false);
// non-null `owned_build_pending`: the caller builds the table of the owned slots itself (the slab step: inside
// k_slab_bounds_pack, one dispatch less on every rank's critical path); set to whether a build is owed (not after a skipped sort)
int step_sort(sph_ctx* c, bool* owned_build_pending = nullptr);
int step_cells(sph_ctx* c);
int launch_integrate(sph_ctx* c, float dt);
// the obstacle (sph_obstacle.hip): push the owned particles an integrate just wrote out of the solid.  `fused`: the launch wrote
// posi2 / velr2 and the next keys k0, and, with `mark`, the movers' marks, which the pass keeps right; else posi / velr alone
inline bool have_obstacle(const sph_ctx* c) {        // any slot installed
    for (const Obstacle& o : c->ob) if (o.installed()) return true;
    return false;
}
inline Obstacle& selected_obstacle(sph_ctx* c) { return c->ob[c->ob_sel]; }
inline const Obstacle& selected_obstacle(const sph_ctx* c) { return c->ob[c->ob_sel]; }
int launch_obstacle_push(sph_ctx* c, bool fused, bool mark);
int advance_obstacle(sph_ctx* c, float dt);   // once per integrate, behind the push: queues the load's sum while sensing, then offset and pose move on
// the solids as a picture (k_solid_march, sph_obstacle.hip; THE RULE of sph_render_set_solids): the camera and the looks as the
// kernels take them, by value
struct SolidCam {
    uint32_t width, height;
    float rot[9], trans[3];
    float focal, near_z, far_z;
    float half_w, half_h;
};
struct SolidLooks {
    int32_t open[SPH_MAX_OBSTACLES];
    float color[SPH_MAX_OBSTACLES][3];
    float L[3];              // the light, normalised
    float ambient;
};
// SHADE of the rule: the colour c of slot `slot` under the eye-space normal ne (the slot picked by selects: a by-value table
// indexed by a lane's value would go to scratch)
__device__ __forceinline__ void solid_color(const SolidLooks& K, uint32_t slot, const float ne[3], float c[3]) {
#pragma clang fp contract(off)
    const float ndl = fmaxf(0.0f, (ne[0] * K.L[0] + ne[1] * K.L[1]) + ne[2] * K.L[2]);
    const float g = K.ambient + (1.0f - K.ambient) * ndl;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float col = K.color[0][k];
#pragma unroll
        for (uint32_t q = 1; q < (uint32_t)SPH_MAX_OBSTACLES; q++)
            if (slot == q) col = K.color[q][k];
        c[k] = fminf(fmaxf(col * g, 0.0f), 1.0f);
    }
}
__device__ __forceinline__ uint32_t solid_rgba(const float c[3]) {
#pragma clang fp contract(off)
    uint32_t out = 0xFF000000u;
#pragma unroll
    for (int k = 0; k < 3; k++) out |= (uint32_t)(c[k] * 255.0f + 0.5f) << (8 * k);
    return out;
}
// whether the style is set and some installed slot has draw != 0: else a render is the one without solids, launch for launch
bool solids_drawn(const sph_ctx* c);
// One march of every drawn slot over the image.  so_depth null: composed straight into sph_render's resolved planes (depth
// holds the fluid's d, +inf on background); else the nearest hit of every pixel goes to the three planes for k_surface_shade
int launch_solid_march(sph_ctx* c, const SolidCam& cam, const SolidLooks& looks, uint32_t* rgba, uint32_t* id, float* depth,
                       float* so_depth, uint32_t* so_slot, float* so_normal);
// the installation helpers of sph_obstacle.hip, for the mesh voxeliser (sph_obstacle_mesh.hip): the context check, the lattice
// of a build (checks only), the clamp distance D, the exchange of the context's grid (on failure: no obstacle) and the bricks
int obstacle_ctx(const sph_ctx* c, const char* who);
int lattice_resolve(const sph_ctx* c, float spacing, const float* lo, const float* hi, sph_obstacle_grid* G);
float ob_clamp_distance(const sph_obstacle_grid& G);
int install_begin(sph_ctx* c, const sph_obstacle_grid& G);
int install_finish(sph_ctx* c);
void release_obstacle(sph_ctx* c);
// tracked contexts (sph_pairs.hip): write the host's sphere set into trk_table and zero J and the step count; refresh R + eps
int launch_spheres_install(sph_ctx* c);
int launch_spheres_radii(sph_ctx* c);
// the kernels of a slab's messages (sph_halo.hip), shared by the phase API there and the slab step (sph_slab.hip), which queues them
// on the context's stream, its comm stream or whichever of the two packs: the stream is the caller's.  No launch for no work.
// One side of a message: n records (put_record / get_record, sph_device.hpp) and the slots they are packed from or unpacked to
struct RecSide { float4* rec; float4* posi; float4* velr; uint32_t* key; uint32_t n; };
int launch_pack_records(hipStream_t st, const RecSide& lo, const RecSide& hi);      // (key: not used)
// records -> slots; with a key pointer also their cell keys; with `err_word` a record whose cell is not in an owned layer of `g` --
// the local layers [G, zl - G) -- sets that mapped host word to 1
int launch_unpack_records(hipStream_t st, const RecSide& lo, const RecSide& hi, const GridDesc& g, uint32_t G, volatile uint32_t* err_word);
// (rho, p) of n_lo + n_hi ghosts <- a message, with the neighbour terms the force pass reads of them
int launch_unpack_dp(hipStream_t st, const float2* src_lo, float2* dp_lo, float2* cw_lo, uint32_t n_lo, const float2* src_hi, float2* dp_hi,
                     float2* cw_hi, uint32_t n_hi, const Phys& ph);
// out[k] = the first slot of the sorted keys[0, n) whose key is >= v[k], for k < m: to device words and, where given, mapped host words
constexpr uint32_t LB_MAX = 32;
struct LbTargets { uint32_t v[LB_MAX]; uint32_t m; };
int launch_lower_bounds(hipStream_t st, const uint32_t* keys, uint32_t n, const LbTargets& tg, uint32_t* out, volatile uint32_t* out_host);
// The bounds a slab step looks up in its sorted owned keys (k_slab_bounds_pack, sph_slab.hip): the first slot whose key lies in
// local layer bound_layer(b, G, zl) or above.  G ghost layers per side: the owned layers are the local layers [G, zl - G);
// "layer k" counts from the first owned layer = 1 on the low side, "layer zl-k" mirrors it on the high side.
enum Bound {
    B_OWN_BEGIN, B_FIRST_END,       // the first four in ascending order: the start of the owned layers (what lies in front leaves
    B_LAST_BEGIN, B_OWN_END,        // downwards), the end of the first one, the start of the last one, their end (the rest leaves upwards)
    B_DEEP_LO, B_DEEP_HI,           // the deep interior, layers [4, zl-4): at least three layers from either cut
    B_NEAR_LO, B_NEAR_HI,           // the start of layer 3 / of layer zl-3: the layers next to the deep interior
    B_EARLY_LO, B_EARLY_HI,         // layers [6, zl-6): their force pass reads densities of the deep launch only
    B_LAYER5,                       // the start of layer 5, to check exactly that
    B_COUNT
};
__host__ __device__ inline uint32_t bound_layer(uint32_t b, uint32_t G, uint32_t zl) {
    // thin slabs: a range that does not exist is empty (its end clamped to its start), every target a layer of the grid
    // (a constant table indexed HERE becomes a chain of selects in the kernel; one returned by value went to LDS, 44 bytes a thread)
    const uint32_t d0 = min(G + 3u, zl - 1u), d1 = zl >= 2u * G + 6u ? zl - G - 3u : d0;
    const uint32_t e0 = min(G + 2u, zl - 1u), e1 = zl >= 2u * G + 4u ? zl - G - 2u : e0;
    const uint32_t f0 = min(G + 5u, zl - 1u), f1 = zl >= 2u * G + 11u ? zl - G - 5u : f0;
    const uint32_t d_end = max(d1, d0), e_end = max(e1, e0), f_end = max(f1, f0), layer5 = min(G + 4u, zl - 1u);
    const uint32_t z[B_COUNT] = {G, G + 1u, zl - G - 1u, zl - G,    // B_OWN_BEGIN, B_FIRST_END, B_LAST_BEGIN, B_OWN_END
                                 d0, d_end, e0, e_end,              // B_DEEP_LO, B_DEEP_HI, B_NEAR_LO, B_NEAR_HI
                                 f0, f_end, layer5};                // B_EARLY_LO, B_EARLY_HI, B_LAYER5
    return z[b];
}
// the ends of a slab's boundary layers in its sorted keys, in ascending order: first ghost | first owned layer | ... | last | ghost
inline LbTargets layer_bound_targets(const sph_ctx* c) {
    const uint32_t layer = c->grid.g[0] * c->grid.g[1], G = c->ghost_layers, zl = c->grid.zl;
    return LbTargets{{bound_layer(B_OWN_BEGIN, G, zl) * layer, bound_layer(B_FIRST_END, G, zl) * layer,
                      bound_layer(B_LAST_BEGIN, G, zl) * layer, bound_layer(B_OWN_END, G, zl) * layer}, 4u};
}
// record 0 of both send buffers (a message's header)
int launch_headers(hipStream_t st, float4* out_lo, float4* out_hi, float4 lo, float4 hi);
// what each subsystem allocates in the context's owner, sized next to the kernels that index it
int sort_buffers_alloc(sph_ctx* c);       // sph_sort.hip: the sorts' scratch and the mapped word block (create_impl)
int tracked_buffers_alloc(sph_ctx* c);    // sph_pairs.hip: the table, partial sums and masks of a tracked context (first tracking)

inline uint32_t ceil_div(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// ---- the host-side state of a context: the events its entry points compose (DESIGN.md section 2 has the table) ----
// results stale: density, forces and collision terms describe particles that have changed since
inline void results_stale(sph_ctx* c) { c->have_dens = c->have_force = c->have_coll = false; }
// mover count unknown: the count the device last reported says nothing about these particles (both sort forms for a while)
inline void mover_count_unknown(sph_ctx* c) { c->sort_form_both_until = c->sort_calls + 5; }
// positions moved under the keys: k0 is stale, the step starts again at the hash
inline void positions_moved(sph_ctx* c) { c->keys_fresh = false; c->stage = sph_ctx::ST_LOADED; }
// order lost: positions moved, and the slots no longer follow the last sort (the next sort is the full, stable one)
inline void order_lost(sph_ctx* c) { positions_moved(c); c->order_valid = false; }
// ping-pong: what a kernel wrote into posi2 / velr2 is the state now; `keys`: a sort or a compaction wrote keyS2 as well, and
// put the owned range at its canonical offset
inline void swap_state(sph_ctx* c, bool keys) {
    std::swap(c->posi, c->posi2);
    std::swap(c->velr, c->velr2);
    if (keys) { std::swap(c->keyS, c->keyS2); c->own_off = c->gcap; }
}
// the cell table is live and was built from exactly the slots [lo, hi)
inline bool table_covers(const sph_ctx* c, uint32_t lo, uint32_t hi) { return c->table.valid && c->table.lo == lo && c->table.hi == hi; }
// the allocation of `alloc` cells at `base`, all zero, is the table now (create; a slab that takes over more layers)
inline void table_init(sph_ctx* c, uint2* base, uint32_t alloc) { c->table.base = base; c->table.cells = base + 1; c->table.alloc = alloc; }
// a table build over the slots [lo, hi) has been queued
inline void table_set(sph_ctx* c, uint32_t lo, uint32_t hi) { c->table.lo = lo; c->table.hi = hi; c->table.valid = true; }
// the slots that hold particles: the owned range and the ghosts installed on either side of it
struct SlotRange { uint32_t lo, hi; };
inline SlotRange live_slots(const sph_ctx* c) { return SlotRange{c->own_off - c->n_glo, c->own_off + c->n + c->n_ghi}; }

// the records of posi / velr as sph_upload, sph_emit and a snapshot hold them: (x, y, z, creation index bits), (vx, vy, vz, 0);
// particle i gets index[i], or first + i without an index array
inline void pack_records(uint32_t n, const float* pos, const float* vel, const uint32_t* index, uint32_t first, float4* hp, float4* hv) {
    for (size_t i = 0; i < n; i++) {
        const uint32_t idx = index ? index[i] : first + (uint32_t)i;
        float w;
        memcpy(&w, &idx, 4);
        hp[i] = make_float4(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], w);
        hv[i] = vel ? make_float4(vel[3 * i], vel[3 * i + 1], vel[3 * i + 2], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// ---- device timing: a pair of HIP events on the context's stream around a phase (only while sph_timing_enable) ----
struct PhaseTimer {
    sph_ctx* c; int phase; hipEvent_t a = nullptr, b = nullptr;
    PhaseTimer(sph_ctx* c_, int ph) : c(c_), phase(ph) {
        if (!c->timing) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
        hipEventRecord(a, c->stream);
    }
    ~PhaseTimer() {
        if (!a || !b) return;
        hipEventRecord(b, c->stream);
        c->events.push_back(a);
        c->events.push_back(b);
        c->events.push_back((hipEvent_t)(intptr_t)phase);   // tag
    }
};
void timing_collect(sph_ctx* c);      // sph_capi.hip: waits for the recorded events and adds them up per phase

}  // namespace sph

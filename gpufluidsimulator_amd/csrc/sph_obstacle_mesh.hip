// sph_obstacle_mesh.hip -- an obstacle from a triangle mesh: the mesh is voxelised on the device into the truncated signed
// distances the obstacle pass reads (sph_obstacle_build_mesh, _build_mesh_dev, _build_obj, sph_obstacle_mesh_stats of
// include/sph_hip.h, which states the rule; tests/mesh_obstacle_model.py is the same arithmetic in numpy).  The installation
// itself -- the lattice, the two buffers, the bricks -- is sph_obstacle.hip's.  The reference has no counterpart.
//
//   k_obmesh_count     one triangle per lane: is it usable, and how many TILES of the distance pass and of the crossing pass its
//                      index boxes give; the in-block scan of both and the block's sums
//   k_obmesh_scan      ONE workgroup: the exclusive scan of the block sums (64-bit) and the two totals (scan_array_one_block,
//                      sph_device.hpp)
//   k_obmesh_distance  one wave per tile, found by binary search in the scanned counts: 64 consecutive x nodes times up to
//                      OBMESH_TILE_ROWS rows; per node one unsigned atomic min on the bits of the squared distance
//   k_obmesh_cross     one wave per tile of (j, k) columns: 64 consecutive j times up to OBMESH_TILE_ROWS k; per crossing one atomic
//                      XOR of a parity mark
//   k_obmesh_finish    one node per lane: sqrt, the band, the sign from the prefix parity of its column, invert, the clamp; the odd
//                      columns are counted
//
// Work is dealt out by tiles and not by triangles, so that twelve triangles on a large lattice and a million small ones both fill
// the device; the launches have a fixed size and walk the tiles with a stride, because the number of tiles stays on the device
// (the build makes no host wait).  A tile's triangle is loaded once per wave, uniformly.  Minimum and XOR do not depend on the
// order of arrival: two builds of one mesh give the same bits.  No floating-point atomic.
#include "sph_device.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

namespace sph {

constexpr uint32_t OBMESH_THREADS = 256;
constexpr uint32_t OBMESH_WAVES = OBMESH_THREADS / WAVE;
constexpr uint32_t OBMESH_TILE_ROWS = 128;       // rows of a tile (tests/mesh_obstacle_model.py: TILE_ROWS)
constexpr uint32_t OBMESH_SCAN2 = 1024;          // block sums the second level scans at a time
constexpr uint32_t OBMESH_MAX_BLOCKS = 2048;     // of the two tile kernels: 8192 waves walk the tiles
constexpr uint32_t OBMESH_HEAD = 4;              // 64-bit words in front of the work list: the two totals, the four counters
static_assert(WAVE == 64, "a tile is 64 consecutive nodes");

// the lattice of the build as the kernels take it: by value
struct ObMeshLattice {
    float origin[3];
    float s;
    uint32_t n[3];
    float nm1[3];          // (float)(n - 1)
    float W;               // (float)band * s
    uint32_t words;        // parity marks of a column: ceil((n_x + 1) / 32) words
};

struct ObMeshTri {
    float a[3], b[3], c[3];
};

// the work list behind the head: the scanned block sums of both passes (64-bit), then every triangle's offset inside its block
struct ObMeshWork {
    uint64_t* head;        // [0] tiles of the distance pass, [1] of the crossing pass, [2..3] the four counters
    uint64_t* blk_d;
    uint64_t* blk_x;
    uint32_t* off_d;
    uint32_t* off_x;
    uint32_t* cnt;         // used, skipped, lost crossings, odd columns
};

static ObMeshWork obmesh_work(uint64_t* work, uint32_t nt) {
    const uint32_t nb = ceil_div(nt, OBMESH_THREADS);
    ObMeshWork w;
    w.head = work;
    w.cnt = (uint32_t*)(work + 2);
    w.blk_d = work + OBMESH_HEAD;
    w.blk_x = w.blk_d + nb;
    w.off_d = (uint32_t*)(w.blk_x + nb);
    w.off_x = w.off_d + nt;
    return w;
}
static size_t obmesh_work_words(uint32_t nt) { return (size_t)OBMESH_HEAD + 2 * (size_t)ceil_div(nt, OBMESH_THREADS) + (size_t)nt; }

// a triangle whose indices are below nv and whose vertices are finite; anything else is skipped (and counted)
__device__ __forceinline__ bool obmesh_load(const float* __restrict__ pos, const uint32_t* __restrict__ tri, uint32_t nv, uint32_t t,
                                            ObMeshTri& T) {
    const uint32_t ia = tri[3 * (size_t)t], ib = tri[3 * (size_t)t + 1], ic = tri[3 * (size_t)t + 2];
    if (ia >= nv || ib >= nv || ic >= nv) return false;
    bool fin = true;
    for (int k = 0; k < 3; k++) {
        T.a[k] = pos[3 * (size_t)ia + k]; T.b[k] = pos[3 * (size_t)ib + k]; T.c[k] = pos[3 * (size_t)ic + k];
        fin = fin && fabsf(T.a[k]) < INFINITY && fabsf(T.b[k]) < INFINITY && fabsf(T.c[k]) < INFINITY;
    }
    return fin;
}

// the index range of one axis: floorf((lo - origin) / s) .. ceilf((hi - origin) / s), each clamped as a float to [0, n - 1]
__device__ __forceinline__ void obmesh_range(float lo, float hi, float origin, float s, float nm1, uint32_t& a, uint32_t& b) {
#pragma clang fp contract(off)
    const float fa = floorf((lo - origin) / s), fb = ceilf((hi - origin) / s);
    a = (uint32_t)fminf(fmaxf(fa, 0.f), nm1);
    b = (uint32_t)fminf(fmaxf(fb, 0.f), nm1);
}

// the index box of the distance pass (band W around the triangle's extent) or of the crossing pass (axes 1 and 2, no band)
__device__ __forceinline__ void obmesh_box(const ObMeshLattice& L, const ObMeshTri& T, bool banded, uint32_t lo[3], uint32_t hi[3]) {
#pragma clang fp contract(off)
    for (int k = 0; k < 3; k++) {
        const float l = fminf(fminf(T.a[k], T.b[k]), T.c[k]), h = fmaxf(fmaxf(T.a[k], T.b[k]), T.c[k]);
        if (banded) obmesh_range(l - L.W, h + L.W, L.origin[k], L.s, L.nm1[k], lo[k], hi[k]);
        else obmesh_range(l, h, L.origin[k], L.s, L.nm1[k], lo[k], hi[k]);
    }
}

__device__ __forceinline__ uint32_t obmesh_tiles(uint32_t across, uint32_t rows) {
    return ((across + WAVE - 1u) / WAVE) * ((rows + OBMESH_TILE_ROWS - 1u) / OBMESH_TILE_ROWS);
}

__global__ __launch_bounds__(OBMESH_THREADS) void k_obmesh_count(const float* __restrict__ pos, const uint32_t* __restrict__ tri,
                                                                 uint32_t nv, uint32_t nt, ObMeshLattice L, ObMeshWork w) {
    __shared__ uint32_t lds[OBMESH_WAVES];
    const uint32_t t = blockIdx.x * OBMESH_THREADS + threadIdx.x;
    uint32_t td = 0, tx = 0;
    bool used = false;
    if (t < nt) {
        ObMeshTri T;
        used = obmesh_load(pos, tri, nv, t, T);
        if (used) {
            uint32_t lo[3], hi[3];
            obmesh_box(L, T, true, lo, hi);
            td = obmesh_tiles(hi[0] - lo[0] + 1u, (hi[1] - lo[1] + 1u) * (hi[2] - lo[2] + 1u));
            obmesh_box(L, T, false, lo, hi);
            tx = obmesh_tiles(hi[1] - lo[1] + 1u, hi[2] - lo[2] + 1u);
        }
    }
    uint32_t sum_d, sum_x;
    const uint32_t ed = block_scan_excl<OBMESH_WAVES>(td, lds, sum_d);
    const uint32_t ex = block_scan_excl<OBMESH_WAVES>(tx, lds, sum_x);
    if (t < nt) { w.off_d[t] = ed; w.off_x[t] = ex; }
    if (threadIdx.x == 0) { w.blk_d[blockIdx.x] = sum_d; w.blk_x[blockIdx.x] = sum_x; }
    const uint64_t um = __ballot(used), sm = __ballot(t < nt && !used);
    if (lane_id() == 0u) {
        if (um) atomicAdd(&w.cnt[0], (uint32_t)__popcll(um));
        if (sm) atomicAdd(&w.cnt[1], (uint32_t)__popcll(sm));
    }
}

// sums -> exclusive bases, in place, one row after the other; head[0], head[1] = the totals.  One workgroup (scan_array_one_block,
// sph_device.hpp), 64-bit: a work list may hold more than 2^32 tiles.
__global__ __launch_bounds__(OBMESH_SCAN2) void k_obmesh_scan(ObMeshWork w, uint32_t nb) {
    __shared__ uint64_t lds[OBMESH_SCAN2 / 64];
    uint64_t* const rows[2] = {w.blk_d, w.blk_x};
    for (uint32_t r = 0; r < 2; r++) {
        uint64_t* const row = rows[r];
        const uint64_t sum = scan_array_one_block<OBMESH_SCAN2>(nb, lds, [&](uint32_t b) { return row[b]; },
                                                                [&](uint32_t b, uint64_t before) { row[b] = before; });
        if (threadIdx.x == 0) w.head[r] = sum;
    }
}

// tile `tile` of a pass -> its triangle and the tile's number inside the triangle: the last block whose base is <= tile, then the
// last triangle of that block whose offset is <= the rest (triangles without tiles share their successor's offset and lose)
__device__ __forceinline__ uint32_t obmesh_find(const uint64_t* __restrict__ blk, const uint32_t* __restrict__ off, uint32_t nt,
                                                uint64_t tile, uint32_t& local) {
    // (both searches start one past their first entry: blk[0] = 0 <= tile and a block's first offset 0 <= rest hold without a
    // probe, and "the first beyond, minus one" then never goes below the range.  nt >= 1: the caller has tile < the pass's total.
    // Among equal entries the first beyond them all is found, so the LAST of them wins, as the comment above asks.)
    const uint32_t nb = (nt + OBMESH_THREADS - 1u) / OBMESH_THREADS;
    const uint32_t b = first_not(1u, nb, [&](uint32_t i) { return blk[i] <= tile; }) - 1u;
    const uint32_t rest = (uint32_t)(tile - blk[b]);
    const uint32_t t0 = b * OBMESH_THREADS;
    const uint32_t a = first_not(t0 + 1u, min(nt, t0 + OBMESH_THREADS), [&](uint32_t i) { return off[i] <= rest; }) - 1u;
    local = rest - off[a];
    return a;
}

// squared distance of p to the segment from a along ba (bb = ba.ba; ok: bb is a positive finite number): the capsule's arithmetic
__device__ __forceinline__ float obmesh_seg(float px, float py, float pz, const float a[3], const float ba[3], float bb, bool ok) {
#pragma clang fp contract(off)
    const float pax = px - a[0], pay = py - a[1], paz = pz - a[2];
    float t = ((pax * ba[0] + pay * ba[1]) + paz * ba[2]) / bb;
    t = fminf(fmaxf(t, 0.f), 1.f);
    if (!ok) t = 0.f;
    const float dx = pax - t * ba[0], dy = pay - t * ba[1], dz = paz - t * ba[2];
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ void obmesh_cross3(const float u[3], const float v[3], float out[3]) {
#pragma clang fp contract(off)
    out[0] = u[1] * v[2] - u[2] * v[1];
    out[1] = u[2] * v[0] - u[0] * v[2];
    out[2] = u[0] * v[1] - u[1] * v[0];
}

__global__ __launch_bounds__(OBMESH_THREADS) void k_obmesh_distance(const float* __restrict__ pos, const uint32_t* __restrict__ tri,
                                                                    uint32_t nv, uint32_t nt, ObMeshLattice L, ObMeshWork w,
                                                                    uint32_t* __restrict__ d2_bits) {
#pragma clang fp contract(off)
    const uint32_t lane = lane_id();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t total = w.head[0], stride = (uint64_t)gridDim.x * OBMESH_WAVES;
    for (uint64_t tile = (uint64_t)blockIdx.x * OBMESH_WAVES + wave; tile < total; tile += stride) {
        uint32_t local;
        const uint32_t t = obmesh_find(w.blk_d, w.off_d, nt, tile, local);
        ObMeshTri T;
        if (!obmesh_load(pos, tri, nv, t, T)) continue;                  // (wave-uniform; a skipped triangle has no tile)
        uint32_t lo[3], hi[3];
        obmesh_box(L, T, true, lo, hi);
        const uint32_t nj = hi[1] - lo[1] + 1u, rows = nj * (hi[2] - lo[2] + 1u);
        const uint32_t chunks = (hi[0] - lo[0] + WAVE) / WAVE;
        const uint32_t chunk = local % chunks, r0 = (local / chunks) * OBMESH_TILE_ROWS;
        if (r0 >= rows) continue;                                        // (cannot happen: the count kernel saw the same box)
        const uint32_t r1 = min(rows, r0 + OBMESH_TILE_ROWS);
        // the triangle's constants, once per wave
        float ab[3], bc[3], ca[3], ac[3], n[3], cab[3], cbc[3], cca[3];
        for (int k = 0; k < 3; k++) { ab[k] = T.b[k] - T.a[k]; bc[k] = T.c[k] - T.b[k]; ca[k] = T.a[k] - T.c[k]; ac[k] = T.c[k] - T.a[k]; }
        const float bb_ab = (ab[0] * ab[0] + ab[1] * ab[1]) + ab[2] * ab[2];
        const float bb_bc = (bc[0] * bc[0] + bc[1] * bc[1]) + bc[2] * bc[2];
        const float bb_ca = (ca[0] * ca[0] + ca[1] * ca[1]) + ca[2] * ca[2];
        const bool ok_ab = bb_ab > 0.f && bb_ab < INFINITY, ok_bc = bb_bc > 0.f && bb_bc < INFINITY, ok_ca = bb_ca > 0.f && bb_ca < INFINITY;
        obmesh_cross3(ab, ac, n);
        const float nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
        const bool plane = nn > 0.f && nn < INFINITY;
        obmesh_cross3(ab, n, cab);
        obmesh_cross3(bc, n, cbc);
        obmesh_cross3(ca, n, cca);
        const uint32_t i = lo[0] + chunk * WAVE + lane;
        const bool active = i <= hi[0];
        const float px = L.origin[0] + (float)i * L.s;
        if (!active) continue;                                           // (nothing below is a wave-wide operation)
        for (uint32_t r = r0; r < r1; r++) {
            const uint32_t j = lo[1] + r % nj, k = lo[2] + r / nj;
            const float py = L.origin[1] + (float)j * L.s, pz = L.origin[2] + (float)k * L.s;
            float cand = fminf(fminf(obmesh_seg(px, py, pz, T.a, ab, bb_ab, ok_ab), obmesh_seg(px, py, pz, T.b, bc, bb_bc, ok_bc)),
                               obmesh_seg(px, py, pz, T.c, ca, bb_ca, ok_ca));
            if (plane) {
                const float ax = px - T.a[0], ay = py - T.a[1], az = pz - T.a[2];
                const float bx = px - T.b[0], by = py - T.b[1], bz = pz - T.b[2];
                const float cx = px - T.c[0], cy = py - T.c[1], cz = pz - T.c[2];
                const float v0 = (ax * cab[0] + ay * cab[1]) + az * cab[2];
                const float v1 = (bx * cbc[0] + by * cbc[1]) + bz * cbc[2];
                const float v2 = (cx * cca[0] + cy * cca[1]) + cz * cca[2];
                if (v0 <= 0.f && v1 <= 0.f && v2 <= 0.f) {
                    const float h = (ax * n[0] + ay * n[1]) + az * n[2];
                    cand = fminf(cand, (h * h) / nn);
                }
            }
            uint32_t* at = d2_bits + ((size_t)k * L.n[1] + j) * L.n[0] + i;
            const uint32_t bits = __float_as_uint(cand);
            // (a plain look first: the word only ever falls, so a stale value costs an atomic that changes nothing, never one left out)
            if (bits < __atomic_load_n(at, __ATOMIC_RELAXED)) atomicMin(at, bits);
        }
    }
}

__global__ __launch_bounds__(OBMESH_THREADS) void k_obmesh_cross(const float* __restrict__ pos, const uint32_t* __restrict__ tri,
                                                                 uint32_t nv, uint32_t nt, ObMeshLattice L, ObMeshWork w,
                                                                 uint32_t* __restrict__ marks) {
#pragma clang fp contract(off)
    const uint32_t lane = lane_id();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t total = w.head[1], stride = (uint64_t)gridDim.x * OBMESH_WAVES;
    for (uint64_t tile = (uint64_t)blockIdx.x * OBMESH_WAVES + wave; tile < total; tile += stride) {
        uint32_t local;
        const uint32_t t = obmesh_find(w.blk_x, w.off_x, nt, tile, local);
        ObMeshTri T;
        if (!obmesh_load(pos, tri, nv, t, T)) continue;
        uint32_t lo[3], hi[3];
        obmesh_box(L, T, false, lo, hi);
        const uint32_t chunks = (hi[1] - lo[1] + WAVE) / WAVE, nk = hi[2] - lo[2] + 1u;
        const uint32_t chunk = local % chunks, r0 = (local / chunks) * OBMESH_TILE_ROWS;
        if (r0 >= nk) continue;
        const uint32_t r1 = min(nk, r0 + OBMESH_TILE_ROWS);
        // the three edges with their ends in canonical order (smaller z first, on equal z smaller y first): l, and u - l
        float ly[3], lz[3], uz[3], dy[3], dz[3];
        const float* ends[4] = {T.a, T.b, T.c, T.a};
        for (int e = 0; e < 3; e++) {
            const float* p = ends[e];
            const float* q = ends[e + 1];
            const bool swap = q[2] < p[2] || (q[2] == p[2] && q[1] < p[1]);
            const float* l = swap ? q : p;
            const float* u = swap ? p : q;
            ly[e] = l[1]; lz[e] = l[2]; uz[e] = u[2];
            dy[e] = u[1] - l[1]; dz[e] = u[2] - l[2];
        }
        float ab[3], ac[3], n[3];
        for (int k = 0; k < 3; k++) { ab[k] = T.b[k] - T.a[k]; ac[k] = T.c[k] - T.a[k]; }
        obmesh_cross3(ab, ac, n);
        const uint32_t j = lo[1] + chunk * WAVE + lane;
        const bool active = j <= hi[1];
        const float qy = L.origin[1] + (float)j * L.s;
        for (uint32_t r = r0; r < r1; r++) {
            const uint32_t k = lo[2] + r;
            const float qz = L.origin[2] + (float)k * L.s;
            bool odd = false, lost = false;
            if (active) {
                for (int e = 0; e < 3; e++) {
                    const bool straddle = lz[e] <= qz && !(uz[e] <= qz);
                    const float E = dy[e] * (qz - lz[e]) - dz[e] * (qy - ly[e]);
                    odd ^= straddle && E > 0.f;
                }
                if (odd) {
                    const float xc = T.a[0] + ((n[1] * (T.a[1] - qy)) + n[2] * (T.a[2] - qz)) / n[0];
                    const float g = (xc - L.origin[0]) / L.s;
                    lost = !(fabsf(g) < INFINITY);
                    if (!lost) {
                        const uint32_t i0 = g <= 0.f ? 0u : (g > L.nm1[0] ? L.n[0] : (uint32_t)ceilf(g));
                        atomicXor(&marks[((size_t)k * L.n[1] + j) * L.words + (i0 >> 5)], 1u << (i0 & 31u));
                    }
                }
            }
            const uint64_t lm = __ballot(lost);
            if (lm != 0ull && lane == 0u) atomicAdd(&w.cnt[2], (uint32_t)__popcll(lm));
        }
    }
}

// in place: the bits of d2 become phi = +-min(sqrtf(d2), W), negative where the prefix parity of the node's column is odd
__global__ __launch_bounds__(OBMESH_THREADS) void k_obmesh_finish(float* __restrict__ phi, uint32_t nodes, ObMeshLattice L,
                                                                  const uint32_t* __restrict__ marks, uint32_t* __restrict__ cnt,
                                                                  int invert, float D) {
#pragma clang fp contract(off)
    const uint32_t t = blockIdx.x * OBMESH_THREADS + threadIdx.x;
    if (t >= nodes) return;
    const uint32_t i = t % L.n[0], col = t / L.n[0];
    const uint32_t* __restrict__ m = marks + (size_t)col * L.words;
    uint32_t x = 0;
    for (uint32_t q = 0; q < (i >> 5); q++) x ^= m[q];
    x ^= m[i >> 5] & (0xFFFFFFFFu >> (31u - (i & 31u)));
    const bool inside = (__popc(x) & 1) != 0;
    if (i == 0u) {                                   // the column's first node also looks at the whole column
        uint32_t all = 0;
        for (uint32_t q = 0; q < L.words; q++) all ^= m[q];
        if (__popc(all) & 1) atomicAdd(&cnt[3], 1u);
    }
    float v = fminf(sqrtf(phi[t]), L.W);
    if (inside) v = -v;
    if (invert) v = -v;
    phi[t] = fminf(fmaxf(v, -D), D);
}

// ---- the host side --------------------------------------------------------------------------------------------------------------

// what every form checks before anything is allocated: the context, the parameters, the counts and the lattice
static int obmesh_check(const sph_ctx* c, const char* who, const sph_obstacle_mesh_params* p, const float* lo, const float* hi,
                        uint32_t nv, uint32_t nt, sph_obstacle_grid* G, uint32_t* band, int* invert) {
    if (int e = obstacle_ctx(c, who)) return e;
    const sph_obstacle_mesh_params P = p ? *p : sph_obstacle_mesh_params{};
    SPH_REQUIRE(P.band <= (uint32_t)SPH_OBSTACLE_MESH_MAX_BAND, SPH_E_INVALID, "%s: a band of %u nodes, at most %d (0: %d)", who, P.band,
                SPH_OBSTACLE_MESH_MAX_BAND, SPH_OBSTACLE_MESH_DEFAULT_BAND);
    SPH_REQUIRE(nv >= 1u && nt >= 1u, SPH_E_INVALID, "%s: %u vertices and %u triangles, at least one of each", who, nv, nt);
    SPH_REQUIRE(nt <= (uint32_t)SPH_OBSTACLE_MESH_MAX_TRIANGLES, SPH_E_CAPACITY, "%s: %u triangles, at most 2^28", who, nt);
    if (int e = lattice_resolve(c, P.spacing, lo, hi, G)) return e;
    *band = P.band ? P.band : (uint32_t)SPH_OBSTACLE_MESH_DEFAULT_BAND;
    *invert = P.invert != 0;
    return SPH_OK;
}

// the checked build: the grid is exchanged, the scratch allocated, the kernels queued.  On failure there is no obstacle.
static int obmesh_build_dev(sph_ctx* c, const sph_obstacle_grid& G, uint32_t band, int invert, uint32_t nv, const float* pos_dev,
                            uint32_t nt, const uint32_t* tri_dev) {
#pragma clang fp contract(off)
    if (int e = install_begin(c, G)) return e;
    Obstacle& o = selected_obstacle(c);
    ObMeshLattice L{};
    L.s = G.spacing;
    for (int k = 0; k < 3; k++) { L.origin[k] = G.origin[k]; L.n[k] = G.dims[k]; L.nm1[k] = (float)(G.dims[k] - 1u); }
    L.W = (float)band * G.spacing;
    L.words = ceil_div(G.dims[0] + 1u, 32u);
    const uint32_t nodes = G.dims[0] * G.dims[1] * G.dims[2];
    const size_t mark_words = (size_t)G.dims[1] * G.dims[2] * L.words;
    int rc = c->mem.alloc(&o.mesh_work, obmesh_work_words(nt), false);
    if (!rc) rc = c->mem.alloc(&o.mesh_marks, mark_words, false);
    if (rc) { release_obstacle(c); return rc; }
    const ObMeshWork w = obmesh_work(o.mesh_work, nt);
    const uint32_t nb = ceil_div(nt, OBMESH_THREADS);
    // no more workgroups than there can be tiles: a triangle's box has at most this many
    const uint64_t most = (uint64_t)nt * ceil_div(G.dims[0], WAVE) * ceil_div(G.dims[1] * G.dims[2], OBMESH_TILE_ROWS);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(OBMESH_MAX_BLOCKS, (most + OBMESH_WAVES - 1u) / OBMESH_WAVES);
    hipError_t he = hipMemsetD32Async((hipDeviceptr_t)o.phi, 0x7F800000, nodes, c->stream);      // the bits of +inf
    if (he == hipSuccess) he = hipMemsetAsync(o.mesh_marks, 0, mark_words * sizeof(uint32_t), c->stream);
    if (he == hipSuccess) he = hipMemsetAsync(o.mesh_work, 0, OBMESH_HEAD * sizeof(uint64_t), c->stream);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(k_obmesh_count, dim3(nb), dim3(OBMESH_THREADS), 0, c->stream, pos_dev, tri_dev, nv, nt, L, w);
        hipLaunchKernelGGL(k_obmesh_scan, dim3(1), dim3(OBMESH_SCAN2), 0, c->stream, w, nb);
        hipLaunchKernelGGL(k_obmesh_distance, dim3(blocks), dim3(OBMESH_THREADS), 0, c->stream, pos_dev, tri_dev, nv, nt, L, w,
                           (uint32_t*)o.phi);
        hipLaunchKernelGGL(k_obmesh_cross, dim3(blocks), dim3(OBMESH_THREADS), 0, c->stream, pos_dev, tri_dev, nv, nt, L, w,
                           o.mesh_marks);
        hipLaunchKernelGGL(k_obmesh_finish, dim3(ceil_div(nodes, OBMESH_THREADS)), dim3(OBMESH_THREADS), 0, c->stream, o.phi, nodes, L,
                           o.mesh_marks, w.cnt, invert, ob_clamp_distance(G));
        he = hipGetLastError();
    }
    rc = he == hipSuccess ? install_finish(c) : hip_fail(he, "mesh voxeliser", __FILE__, __LINE__);
    if (rc) {
        hipStreamSynchronize(c->stream);                   // (what was queued may still be writing)
        release_obstacle(c);
    }
    return rc;
}

// one vertex reference of an OBJ face: a, a/b, a//c or a/b/c; 1-based, negative = relative to the vertices read so far
static uint32_t obj_index(const char* tok, size_t nv) {
    char* end = nullptr;
    const long long v = strtoll(tok, &end, 10);
    if (end == tok || (*end != '\0' && *end != '/')) return 0xFFFFFFFFu;
    if (v > 0 && (unsigned long long)v <= nv) return (uint32_t)(v - 1);
    if (v < 0 && (unsigned long long)(-v) <= nv) return (uint32_t)(nv - (size_t)(-v));
    return 0xFFFFFFFFu;                                    // refused later: no vertex has this index
}

static int obj_read(const char* path, std::vector<float>* pos, std::vector<uint32_t>* tri) {
    std::ifstream f(path);
    SPH_REQUIRE(f.good(), SPH_E_INVALID, "sph_obstacle_build_obj: cannot read %s", path);
    std::string line;
    std::vector<uint32_t> face;
    while (std::getline(f, line)) {
        const char* s = line.c_str();
        while (*s == ' ' || *s == '\t') s++;
        if (s[0] == 'v' && (s[1] == ' ' || s[1] == '\t')) {
            char* end = nullptr;
            const char* at = s + 1;
            float v[3];
            for (int k = 0; k < 3; k++) {
                v[k] = strtof(at, &end);
                SPH_REQUIRE(end != at, SPH_E_INVALID, "sph_obstacle_build_obj: %s: a `v` line without three numbers", path);
                at = end;
            }
            pos->insert(pos->end(), v, v + 3);
        } else if (s[0] == 'f' && (s[1] == ' ' || s[1] == '\t')) {
            face.clear();
            const char* at = s + 1;
            for (;;) {
                while (*at == ' ' || *at == '\t' || *at == '\r') at++;
                if (!*at) break;
                const char* tok_end = at;
                while (*tok_end && *tok_end != ' ' && *tok_end != '\t' && *tok_end != '\r') tok_end++;
                const std::string tok(at, tok_end);
                face.push_back(obj_index(tok.c_str(), pos->size() / 3));
                at = tok_end;
            }
            SPH_REQUIRE(face.size() >= 3, SPH_E_INVALID, "sph_obstacle_build_obj: %s: a face with %zu vertices", path, face.size());
            for (size_t k = 1; k + 1 < face.size(); k++) {         // a fan from the first vertex
                tri->push_back(face[0]); tri->push_back(face[k]); tri->push_back(face[k + 1]);
            }
        }
    }
    SPH_REQUIRE(!tri->empty(), SPH_E_INVALID, "sph_obstacle_build_obj: %s holds no face", path);
    SPH_REQUIRE(tri->size() / 3 <= 0xFFFFFFFFull && pos->size() / 3 <= 0xFFFFFFFFull, SPH_E_CAPACITY,
                "sph_obstacle_build_obj: %s is too large", path);
    return SPH_OK;
}

}  // namespace sph

using namespace sph;

extern "C" {

int sph_obstacle_build_mesh_dev(sph_ctx* c, const sph_obstacle_mesh_params* p, const float lo[3], const float hi[3], uint32_t n_vertices,
                                const void* pos_dev, uint32_t n_triangles, const void* tri_dev) {
    sph_obstacle_grid G;
    uint32_t band;
    int invert;
    if (int e = obmesh_check(c, "sph_obstacle_build_mesh_dev", p, lo, hi, n_vertices, n_triangles, &G, &band, &invert)) return e;
    SPH_REQUIRE(pos_dev && tri_dev, SPH_E_INVALID, "null argument");
    return obmesh_build_dev(c, G, band, invert, n_vertices, (const float*)pos_dev, n_triangles, (const uint32_t*)tri_dev);
}

int sph_obstacle_build_mesh(sph_ctx* c, const sph_obstacle_mesh_params* p, const float lo[3], const float hi[3], uint32_t n_vertices,
                            const float* pos_xyz, uint32_t n_triangles, const uint32_t* tri) {
    sph_obstacle_grid G;
    uint32_t band;
    int invert;
    if (int e = obmesh_check(c, "sph_obstacle_build_mesh", p, lo, hi, n_vertices, n_triangles, &G, &band, &invert)) return e;
    SPH_REQUIRE(pos_xyz && tri, SPH_E_INVALID, "null argument");
    for (size_t k = 0; k < (size_t)n_vertices * 3; k++)
        SPH_REQUIRE(std::isfinite(pos_xyz[k]), SPH_E_INVALID, "sph_obstacle_build_mesh: vertex %zu is not finite", k / 3);
    for (size_t k = 0; k < (size_t)n_triangles * 3; k++)
        SPH_REQUIRE(tri[k] < n_vertices, SPH_E_INVALID, "sph_obstacle_build_mesh: triangle %zu names vertex %u of %u", k / 3, tri[k],
                    n_vertices);
    SPH_HIP(hipSetDevice(c->device));
    Buffers tmp;                                           // the call's temporaries: the mesh on the device
    float* d_pos = nullptr;
    uint32_t* d_tri = nullptr;
    int rc = tmp.alloc(&d_pos, (size_t)n_vertices * 3, false);
    if (!rc) rc = tmp.alloc(&d_tri, (size_t)n_triangles * 3, false);
    auto hip = [&](hipError_t e, const char* what) { if (!rc && e != hipSuccess) rc = hip_fail(e, what, __FILE__, __LINE__); };
    if (!rc) hip(hipMemcpyAsync(d_pos, pos_xyz, (size_t)n_vertices * 12, hipMemcpyHostToDevice, c->stream), "copy of the vertices");
    if (!rc) hip(hipMemcpyAsync(d_tri, tri, (size_t)n_triangles * 12, hipMemcpyHostToDevice, c->stream), "copy of the triangles");
    if (!rc) rc = obmesh_build_dev(c, G, band, invert, n_vertices, d_pos, n_triangles, d_tri);
    hipError_t e = hipStreamSynchronize(c->stream);        // (the caller's arrays are free again; the temporaries are about to go)
    hip(e, "hipStreamSynchronize");
    if (rc) release_obstacle(c);                           // a failed call leaves NO obstacle (the stream is idle)
    tmp.free_all();
    return rc;
}

int sph_obstacle_build_obj(sph_ctx* c, const sph_obstacle_mesh_params* p, const float lo[3], const float hi[3], const char* path) {
    if (int e = obstacle_ctx(c, "sph_obstacle_build_obj")) return e;
    SPH_REQUIRE(path, SPH_E_INVALID, "null argument");
    std::vector<float> pos;
    std::vector<uint32_t> tri;
    if (int e = obj_read(path, &pos, &tri)) return e;
    return sph_obstacle_build_mesh(c, p, lo, hi, (uint32_t)(pos.size() / 3), pos.data(), (uint32_t)(tri.size() / 3), tri.data());
}

int sph_obstacle_mesh_stats(sph_ctx* c, uint64_t out[4]) {
    SPH_REQUIRE(c && out, SPH_E_INVALID, "null argument");
    const Obstacle& o = selected_obstacle(c);
    SPH_REQUIRE(o.installed() && o.mesh_work, SPH_E_STATE, "sph_obstacle_mesh_stats: the obstacle was not built from a mesh");
    SPH_HIP(hipSetDevice(c->device));
    uint32_t h[4] = {0, 0, 0, 0};
    SPH_HIP(hipMemcpyAsync(h, o.mesh_work + 2, sizeof h, hipMemcpyDeviceToHost, c->stream));
    SPH_HIP(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 4; k++) out[k] = h[k];
    return SPH_OK;
}

}  // extern "C"

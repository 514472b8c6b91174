// sph_mesh.hip -- the fluid's surface as a triangle mesh, on the device (sph_mesh_defaults, sph_mesh_lattice, sph_mesh_extract,
// sph_mesh_read, sph_mesh_dev, sph_mesh_save_obj, sph_mesh_field_dims, sph_mesh_field_read of include/sph_hip.h, which states the rule).  The
// reference has no counterpart: it draws into a GL window.  One pass over posi, then passes over a lattice of 8 bytes per node.
//
//   (memset)          the counts = 0
//   k_mesh_splat      one owned particle per lane: walk the nodes within reach of it and add the quantised weight to each node's
//                     count with a 32-bit integer atomic add (no return value).  The sum does not depend on the order of
//                     arrival: the field is the same bits in every run, with no float atomic.  The hot kernel: a workgroup
//                     sums in an LDS tile where the nodes its particles reach fit one, and sends each word to the field once.
//   k_mesh_count      one node per lane, MESH_BLOCK nodes per workgroup: the inside flags of the node's cube -> how many of its
//                     seven edges carry a vertex (kept per node for the scan) and how many triangles its cube gives; the
//                     workgroup's two sums
//   k_mesh_scan_sums  ONE workgroup: the exclusive scans of the two rows of sums and the totals (scan_array_one_block, sph_device.hpp)
//   k_mesh_vbase      the in-block scan of the vertex counts + the block's base: the vertex base of every node (4 B per node;
//                     a vertex's number is base[node] + popcount(mask & ((1 << (d-1)) - 1)), the mask recomputed from the counts)
//   -- the host reads the two totals here: the call's one wait --
//   k_mesh_generate   one node per lane: the vertices and normals of the edges it owns; the triangles of its cube, at the block's
//                     triangle base + the in-block scan redone here (per cube nothing is stored)
//
// The 6 x 16 case table (which edges, in which order) is built on the host from the midpoint geometry (build_case_table), not
// typed in; tests/mesh_model.py derives its own.  Everything of the rule is fp32 with each operation rounded (fp contract off).
#include "sph_device.hpp"

#include <cmath>
#include <cstring>

namespace sph {

constexpr uint32_t MESH_THREADS = 256;
constexpr uint32_t MESH_BLOCK = 256;        // nodes per workgroup of the lattice kernels = entries of one first-level scan block
constexpr uint32_t MESH_SCAN2 = 1024;       // block sums the second level scans at a time (its workgroup's size)
constexpr uint32_t MESH_TILE_NODES = 8192;  // words of LDS a workgroup of the splat sums in (32 KiB + the box: four workgroups per CU)
constexpr uint32_t MESH_CASES = 6 * 16;     // words of the case table
constexpr uint32_t MESH_AUX_HEAD = 2 + MESH_CASES;   // mesh_aux: the two totals, the case table, then the two rows of block sums
static_assert(MESH_BLOCK == MESH_THREADS, "one node per lane");

// the lattice and the level of one extraction as the kernels take them: by value
struct MeshArgs {
    float origin[3];
    float s, r2;
    uint32_t n[3];
    uint32_t nodes;          // n[0]*n[1]*n[2]
    int32_t reach;           // ceil(r / s)
    uint32_t iso_q;
};

// ---- the field ------------------------------------------------------------------------------------------------------------------

// The nodes of one axis a particle can reach: those of [c - reach - 1, c + reach + 2), c = floor((p - origin) / s), clamped to
// the lattice as floats (p may be anywhere, or NaN: then nothing), narrowed to those whose own squared distance is below r2 -- a
// node that fails on one axis fails the sum, because fp32 addition of non-negative terms never goes below a term.
__device__ __forceinline__ bool mesh_axis_range(const MeshArgs& A, int k, float p, uint32_t& lo, uint32_t& hi) {
#pragma clang fp contract(off)
    const float c = floorf((p - A.origin[k]) / A.s), nf = (float)A.n[k], R = (float)A.reach;
    const float f0 = fminf(fmaxf(c - (R + 1.0f), 0.0f), nf), f1 = fminf(fmaxf(c + (R + 2.0f), 0.0f), nf);
    if (!(f0 < f1)) return false;
    uint32_t a = (uint32_t)f0, b = (uint32_t)f1;
    while (a < b) {
        const float d = (A.origin[k] + (float)a * A.s) - p;
        if (d * d < A.r2) break;
        a++;
    }
    while (b > a) {
        const float d = (A.origin[k] + (float)(b - 1) * A.s) - p;
        if (d * d < A.r2) break;
        b--;
    }
    lo = a; hi = b;
    return a < b;
}

// TILED: the workgroup first agrees on the box of nodes its 256 particles reach -- the slots are cell-sorted, so that is a short
// stick of the lattice -- and, where the box fits MESH_TILE_NODES words of LDS, sums there (ds_add_u32, no return value) and
// sends every non-zero word to the field once: consecutive lanes, consecutive nodes.  Where it does not fit (particles in upload
// order, a fine lattice) every lane adds to the field directly: the plain form, which the measuring build SPH_MESH_PLAIN_SPLAT
// launches alone (profiles/scripts/mesh_time.py).  Integer sums: the same bits either way.
template <bool TILED>
__global__ __launch_bounds__(MESH_THREADS) void k_mesh_splat(const float4* __restrict__ posi, uint32_t n, MeshArgs A,
                                                             uint32_t* __restrict__ field) {
#pragma clang fp contract(off)
    __shared__ uint32_t tile[TILED ? MESH_TILE_NODES : 1];
    __shared__ uint32_t box[6];                        // min of i0, j0, k0; max of i1, j1, k1 over the workgroup
    const uint32_t slot = blockIdx.x * MESH_THREADS + threadIdx.x;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t i0 = 0, i1 = 0, j0 = 0, j1 = 0, k0 = 0, k1 = 0;
    bool has = slot < n;
    if (has) {
        p = posi[slot];
        has = mesh_axis_range(A, 0, p.x, i0, i1) && mesh_axis_range(A, 1, p.y, j0, j1) && mesh_axis_range(A, 2, p.z, k0, k1);
    }
    bool tiled = false;
    uint32_t b0 = 0, b1 = 0, b2 = 0, tx = 0, ty = 0, tz = 0;
    if (TILED) {                                       // (no lane leaves before the last barrier)
        if (threadIdx.x < 3) box[threadIdx.x] = 0xFFFFFFFFu;
        else if (threadIdx.x < 6) box[threadIdx.x] = 0u;
        __syncthreads();
        if (has) {
            __hip_atomic_fetch_min(&box[0], i0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_min(&box[1], j0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_min(&box[2], k0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_max(&box[3], i1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_max(&box[4], j1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_max(&box[5], k1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();
        b0 = box[0]; b1 = box[1]; b2 = box[2];
        if (box[3] <= b0) return;                      // nobody reaches a node (the same for every lane)
        tx = box[3] - b0; ty = box[4] - b1; tz = box[5] - b2;        // each at most SPH_MESH_MAX_DIM: the product fits 2^33
        const uint64_t size = (uint64_t)tx * ty * tz;
        tiled = size <= (uint64_t)MESH_TILE_NODES;
        if (tiled) {
            for (uint32_t t = threadIdx.x; t < (uint32_t)size; t += MESH_THREADS) tile[t] = 0u;
            __syncthreads();
        }
    }
    if (has) {
        for (uint32_t k = k0; k < k1; k++) {
            const float dz = (A.origin[2] + (float)k * A.s) - p.z;
            for (uint32_t j = j0; j < j1; j++) {
                const float dy = (A.origin[1] + (float)j * A.s) - p.y;
                uint32_t* row = field + ((size_t)k * A.n[1] + j) * A.n[0];      // (i1 <= n[0], j1 <= n[1], k1 <= n[2]: inside the lattice)
                const uint32_t trow = ((k - b2) * ty + (j - b1)) * tx - b0;      // (b0 <= i0, i1 <= b0 + tx, likewise j, k: inside the tile)
                for (uint32_t i = i0; i < i1; i++) {
                    const float dx = (A.origin[0] + (float)i * A.s) - p.x;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    if (!(d2 < A.r2)) continue;
                    const float t = 1.0f - d2 / A.r2;
                    const float w = (t * t) * t;
                    const uint32_t q = (uint32_t)(w * 4096.0f + 0.5f);
                    if (!q) continue;
                    if (TILED && tiled) __hip_atomic_fetch_add(&tile[trow + i], q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    else __hip_atomic_fetch_add(row + i, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (result unused: no return)
                }
            }
        }
    }
    if (TILED && tiled) {
        __syncthreads();
        const uint32_t size = tx * ty * tz;
        for (uint32_t t = threadIdx.x; t < size; t += MESH_THREADS) {
            const uint32_t v = tile[t];
            if (!v) continue;
            const uint32_t rowt = t / tx, i = t - rowt * tx, k = rowt / ty, j = rowt - k * ty;
            __hip_atomic_fetch_add(field + ((size_t)(b2 + k) * A.n[1] + (b1 + j)) * A.n[0] + (b0 + i), v, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- the cases ------------------------------------------------------------------------------------------------------------------

// corner t of tetrahedron m of a cube: (0, e_a, e_a | e_b, 7) for the axis orders xyz, xzy, yxz, yzx, zxy, zyx
__host__ __device__ __forceinline__ uint32_t tet_corner(uint32_t m, uint32_t t) {
    const uint32_t a = m >> 1;
    const uint32_t b = (m & 1u) ? (a == 2u ? 1u : 2u) : (a == 0u ? 1u : 0u);
    return t == 0u ? 0u : t == 1u ? (1u << a) : t == 2u ? ((1u << a) | (1u << b)) : 7u;
}

// A word of the case table: bits 0-1 the number of triangles, then 4 bits per triangle vertex (t*3 + v): the tetrahedron's
// corners (p << 2 | q), p < q, of the edge that carries it.
static void build_case_table(uint32_t T[MESH_CASES]) {
    for (uint32_t m = 0; m < 6; m++) {
        double P[4][3];
        for (uint32_t t = 0; t < 4; t++)
            for (int k = 0; k < 3; k++) P[t][k] = (double)((tet_corner(m, t) >> k) & 1u);
        for (uint32_t cs = 0; cs < 16; cs++) {
            uint32_t in[4], out[4], ni = 0, no = 0;
            for (uint32_t t = 0; t < 4; t++) {
                if ((cs >> t) & 1u) in[ni++] = t; else out[no++] = t;
            }
            uint32_t tri[2][3][2], nt = 0;      // [triangle][vertex][the edge's two corners]
            auto edge = [](uint32_t e[2], uint32_t x, uint32_t y) { e[0] = x < y ? x : y; e[1] = x < y ? y : x; };
            if (ni == 1 || no == 1) {
                const uint32_t A = ni == 1 ? in[0] : out[0];
                const uint32_t* o = ni == 1 ? out : in;
                for (int v = 0; v < 3; v++) edge(tri[0][v], A, o[v]);
                nt = 1;
            } else if (ni == 2) {
                const uint32_t A = in[0], B = in[1], C = out[0], D = out[1];
                edge(tri[0][0], A, C); edge(tri[0][1], A, D); edge(tri[0][2], B, D);
                edge(tri[1][0], A, C); edge(tri[1][1], B, D); edge(tri[1][2], B, C);
                nt = 2;
            }
            double dir[3] = {0, 0, 0};          // centroid of the outside corners - centroid of the inside corners
            for (int k = 0; k < 3; k++) {
                for (uint32_t q = 0; q < no; q++) dir[k] += P[out[q]][k] / (double)(no ? no : 1);
                for (uint32_t q = 0; q < ni; q++) dir[k] -= P[in[q]][k] / (double)(ni ? ni : 1);
            }
            uint32_t word = nt;
            for (uint32_t t = 0; t < nt; t++) {
                double mid[3][3];
                for (int v = 0; v < 3; v++)
                    for (int k = 0; k < 3; k++) mid[v][k] = 0.5 * (P[tri[t][v][0]][k] + P[tri[t][v][1]][k]);
                double u[3], w[3];
                for (int k = 0; k < 3; k++) { u[k] = mid[1][k] - mid[0][k]; w[k] = mid[2][k] - mid[0][k]; }
                const double sign = (u[1] * w[2] - u[2] * w[1]) * dir[0] + (u[2] * w[0] - u[0] * w[2]) * dir[1] +
                                    (u[0] * w[1] - u[1] * w[0]) * dir[2];
                if (sign < 0.0) { std::swap(tri[t][1][0], tri[t][2][0]); std::swap(tri[t][1][1], tri[t][2][1]); }
                for (uint32_t v = 0; v < 3; v++) word |= ((tri[t][v][0] << 2) | tri[t][v][1]) << (2 + (t * 3 + v) * 4);
            }
            T[m * 16 + cs] = word;
        }
    }
}

static const uint32_t* case_table() {
    static const struct Table { uint32_t w[MESH_CASES]; Table() { build_case_table(w); } } table;     // (its address never changes)
    return table.w;
}

// ---- the lattice kernels --------------------------------------------------------------------------------------------------------

__device__ __forceinline__ void mesh_coords(const MeshArgs& A, uint32_t node, uint32_t& i, uint32_t& j, uint32_t& k) {
    const uint32_t row = node / A.n[0];
    i = node - row * A.n[0];
    k = row / A.n[1];
    j = row - k * A.n[1];
}

// The cube at (i, j, k): bit c of `lat` = corner c is a node of the lattice, bit c of the result = it is inside.
__device__ __forceinline__ uint32_t mesh_cube(const MeshArgs& A, const uint32_t* __restrict__ field, uint32_t i, uint32_t j, uint32_t k,
                                              uint32_t& lat) {
    uint32_t in = 0;
    lat = 0;
#pragma unroll
    for (uint32_t c = 0; c < 8; c++) {
        const uint32_t x = i + (c & 1u), y = j + ((c >> 1) & 1u), z = k + (c >> 2);
        if (x < A.n[0] && y < A.n[1] && z < A.n[2]) {
            lat |= 1u << c;
            if (field[((size_t)z * A.n[1] + y) * A.n[0] + x] >= A.iso_q) in |= 1u << c;
        }
    }
    return in;
}

// bit d-1: the edge from corner 0 in direction d carries a vertex (the far node exists and differs in inside-ness)
__device__ __forceinline__ uint32_t mesh_edge_mask(uint32_t in, uint32_t lat) {
    const uint32_t differs = (in & 1u) ? ~in : in;
    return ((differs & lat) >> 1) & 0x7Fu;
}

// triangles of a whole cube: one per tetrahedron with 1 or 3 corners inside, two with 2
__device__ __forceinline__ uint32_t mesh_cube_triangles(uint32_t in, uint32_t lat) {
    if (lat != 0xFFu || in == 0u || in == 0xFFu) return 0;
    uint32_t nt = 0;
#pragma unroll
    for (uint32_t m = 0; m < 6; m++) {
        const uint32_t inside = (in & 1u) + ((in >> tet_corner(m, 1)) & 1u) + ((in >> tet_corner(m, 2)) & 1u) + ((in >> 7) & 1u);
        nt += inside == 2u ? 2u : (inside == 1u || inside == 3u) ? 1u : 0u;
    }
    return nt;
}

__global__ __launch_bounds__(MESH_THREADS) void k_mesh_count(const uint32_t* __restrict__ field, MeshArgs A, uint32_t* __restrict__ vcount,
                                                             uint32_t* __restrict__ blk_v, uint32_t* __restrict__ blk_t) {
    __shared__ uint32_t lds[MESH_THREADS / 64];
    const uint32_t node = blockIdx.x * MESH_BLOCK + threadIdx.x;
    uint32_t nv = 0, nt = 0;
    if (node < A.nodes) {
        uint32_t i, j, k, lat;
        mesh_coords(A, node, i, j, k);
        const uint32_t in = mesh_cube(A, field, i, j, k, lat);
        nv = __popc(mesh_edge_mask(in, lat));
        nt = mesh_cube_triangles(in, lat);
        vcount[node] = nv;
    }
    uint32_t tv, tt;
    block_scan_excl<MESH_THREADS / 64>(nv, lds, tv);
    block_scan_excl<MESH_THREADS / 64>(nt, lds, tt);
    if (threadIdx.x == 0) { blk_v[blockIdx.x] = tv; blk_t[blockIdx.x] = tt; }
}

// sums -> exclusive bases, in place, one row after the other; tot[0], tot[1] = the totals.  One workgroup (scan_array_one_block,
// sph_device.hpp).
__global__ __launch_bounds__(MESH_SCAN2) void k_mesh_scan_sums(uint32_t* __restrict__ blk_v, uint32_t* __restrict__ blk_t, uint32_t nb,
                                                               uint32_t* __restrict__ tot) {
    __shared__ uint32_t lds[MESH_SCAN2 / 64];
    uint32_t* const rows[2] = {blk_v, blk_t};
    for (uint32_t r = 0; r < 2; r++) {
        uint32_t* const row = rows[r];
        const uint32_t sum = scan_array_one_block<MESH_SCAN2>(nb, lds, [&](uint32_t b) { return row[b]; },
                                                              [&](uint32_t b, uint32_t before) { row[b] = before; });
        if (threadIdx.x == 0) tot[r] = sum;
    }
}

__global__ __launch_bounds__(MESH_THREADS) void k_mesh_vbase(uint32_t* __restrict__ vbase, uint32_t nodes, const uint32_t* __restrict__ blk_v) {
    __shared__ uint32_t lds[MESH_THREADS / 64];
    const uint32_t node = blockIdx.x * MESH_BLOCK + threadIdx.x;
    const uint32_t v = node < nodes ? vbase[node] : 0u;
    uint32_t total;
    const uint32_t e = block_scan_excl<MESH_THREADS / 64>(v, lds, total);
    if (node < nodes) vbase[node] = blk_v[blockIdx.x] + e;
}

// G of the header at node (i, j, k): central differences of the counts, a neighbour outside the lattice counting 0
__device__ __forceinline__ void mesh_gradient(const MeshArgs& A, const uint32_t* __restrict__ field, uint32_t i, uint32_t j, uint32_t k,
                                              float G[3]) {
    const size_t sy = A.n[0], sz = (size_t)A.n[0] * A.n[1];
    const uint32_t* at = field + (size_t)k * sz + (size_t)j * sy + i;
    const int64_t xp = i + 1 < A.n[0] ? at[1] : 0u, xm = i > 0 ? at[-1] : 0u;
    const int64_t yp = j + 1 < A.n[1] ? at[sy] : 0u, ym = j > 0 ? *(at - sy) : 0u;
    const int64_t zp = k + 1 < A.n[2] ? at[sz] : 0u, zm = k > 0 ? *(at - sz) : 0u;
    G[0] = (float)(xp - xm);
    G[1] = (float)(yp - ym);
    G[2] = (float)(zp - zm);
}

__global__ __launch_bounds__(MESH_THREADS) void k_mesh_generate(const uint32_t* __restrict__ field, MeshArgs A,
                                                                const uint32_t* __restrict__ vbase, const uint32_t* __restrict__ blk_t,
                                                                const uint32_t* __restrict__ cases, float* __restrict__ vpos,
                                                                float* __restrict__ vnrm, uint32_t* __restrict__ tri) {
#pragma clang fp contract(off)
    __shared__ uint32_t lds[MESH_THREADS / 64];
    __shared__ uint32_t T[MESH_CASES];
    if (threadIdx.x < MESH_CASES) T[threadIdx.x] = cases[threadIdx.x];
    const uint32_t node = blockIdx.x * MESH_BLOCK + threadIdx.x;
    const bool live = node < A.nodes;
    uint32_t i = 0, j = 0, k = 0, lat = 0, in = 0, ntri = 0;
    if (live) {
        mesh_coords(A, node, i, j, k);
        in = mesh_cube(A, field, i, j, k, lat);
        ntri = mesh_cube_triangles(in, lat);
    }
    uint32_t total;
    uint32_t tb = block_scan_excl<MESH_THREADS / 64>(ntri, lds, total);      // (its barriers also publish T)
    if (!live) return;
    const uint32_t mask = mesh_edge_mask(in, lat);
    if (mask) {                                                              // the vertices of the edges this node owns
        const float Ca = (float)field[node];
        const float level = (float)A.iso_q;
        const float Xa[3] = {A.origin[0] + (float)i * A.s, A.origin[1] + (float)j * A.s, A.origin[2] + (float)k * A.s};
        float Ga[3];
        mesh_gradient(A, field, i, j, k, Ga);
        size_t v = vbase[node];
        for (uint32_t d = 1; d < 8; d++) {
            if (!((mask >> (d - 1)) & 1u)) continue;
            const uint32_t bi = i + (d & 1u), bj = j + ((d >> 1) & 1u), bk = k + (d >> 2);
            const float Cb = (float)field[((size_t)bk * A.n[1] + bj) * A.n[0] + bi];
            const float t = (level - Ca) / (Cb - Ca);
            const float Xb[3] = {A.origin[0] + (float)bi * A.s, A.origin[1] + (float)bj * A.s, A.origin[2] + (float)bk * A.s};
            float Gb[3], g[3];
            mesh_gradient(A, field, bi, bj, bk, Gb);
#pragma unroll
            for (int q = 0; q < 3; q++) {
                vpos[3 * v + q] = Xa[q] + t * (Xb[q] - Xa[q]);
                g[q] = Ga[q] + t * (Gb[q] - Ga[q]);
            }
            const float len2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
            const bool ok = len2 > 0.0f && len2 < __uint_as_float(0x7F800000u);
            const float len = sqrtf(len2);
#pragma unroll
            for (int q = 0; q < 3; q++) vnrm[3 * v + q] = ok ? (-g[q]) / len : 0.0f;
            v++;
        }
    }
    if (!ntri) return;
    // The triangles of this cube.  A vertex on the edge (corner cu, direction d) belongs to the node at cu, whose mask needs that
    // node's own cube: the inside flags of the 27 nodes (i..i+2, j..j+2, k..k+2), bit (z*3 + y)*3 + x.
    uint32_t in27 = 0, lat27 = 0;
    for (uint32_t z = 0; z < 3; z++)
        for (uint32_t y = 0; y < 3; y++)
            for (uint32_t x = 0; x < 3; x++) {
                if (i + x < A.n[0] && j + y < A.n[1] && k + z < A.n[2]) {
                    const uint32_t bit = 1u << ((z * 3 + y) * 3 + x);
                    lat27 |= bit;
                    if (field[((size_t)(k + z) * A.n[1] + (j + y)) * A.n[0] + (i + x)] >= A.iso_q) in27 |= bit;
                }
            }
    tb += blk_t[blockIdx.x];
    for (uint32_t m = 0; m < 6; m++) {
        uint32_t corner[4], cs = 0;
#pragma unroll
        for (uint32_t t = 0; t < 4; t++) {
            corner[t] = tet_corner(m, t);
            cs |= ((in >> corner[t]) & 1u) << t;
        }
        const uint32_t word = T[m * 16 + cs], nt = word & 3u;
        for (uint32_t t = 0; t < nt; t++) {
            for (uint32_t v = 0; v < 3; v++) {
                const uint32_t code = (word >> (2 + (t * 3 + v) * 4)) & 15u;
                const uint32_t cu = corner[code >> 2], cv = corner[code & 3u], d = cu ^ cv;
                const uint32_t ax = cu & 1u, ay = (cu >> 1) & 1u, az = cu >> 2;
                // the mask of the node at cu, from the 27 flags
                const uint32_t self = (in27 >> ((az * 3 + ay) * 3 + ax)) & 1u;
                uint32_t below = 0;                                           // vertices of that node on directions below d
                for (uint32_t e = 1; e < d; e++) {
                    const uint32_t bit = ((az + (e >> 2)) * 3 + (ay + ((e >> 1) & 1u))) * 3 + (ax + (e & 1u));
                    below += ((lat27 >> bit) & 1u) & (((in27 >> bit) & 1u) ^ self);
                }
                const size_t at = ((size_t)(k + az) * A.n[1] + (j + ay)) * A.n[0] + (i + ax);
                tri[3 * (size_t)tb + v] = vbase[at] + below;
            }
            tb++;
        }
    }
}

// ---- the host side --------------------------------------------------------------------------------------------------------------

// the mesh leaves the context's owner before the context does: a failed allocation
static void release_mesh(sph_ctx* c) {
    Buffers& m = c->mem;
    m.release(&c->mesh_tri); m.release(&c->mesh_vnrm); m.release(&c->mesh_vpos);
    m.release(&c->mesh_aux); m.release(&c->mesh_vbase); m.release(&c->mesh_field);
    c->mesh_nodes_cap = c->mesh_v_cap = c->mesh_t_cap = 0;
    c->mesh_nv = c->mesh_nt = 0;
    c->mesh_valid = false;
}

// The parameters resolved and checked, and the lattice they give in the context's box: what sph_mesh_lattice and
// sph_mesh_extract share.  Allocates nothing.
static int mesh_resolve(const sph_ctx* c, const sph_mesh_params* p, MeshArgs* A) {
    sph_mesh_params d{0.f, 0.f, 0.f};
    if (p) d = *p;
    SPH_REQUIRE(std::isfinite(d.spacing) && d.spacing >= 0.f, SPH_E_INVALID, "mesh spacing %g: finite and >= 0 (0: the particle radius)",
                (double)d.spacing);
    SPH_REQUIRE(std::isfinite(d.radius) && d.radius >= 0.f, SPH_E_INVALID, "mesh radius %g: finite and >= 0 (0: three spacings)",
                (double)d.radius);
    SPH_REQUIRE(std::isfinite(d.iso) && d.iso >= 0.f, SPH_E_INVALID, "mesh iso %g: finite and >= 0 (0: 0.5)", (double)d.iso);
    const float s = d.spacing > 0.f ? d.spacing : c->params.particle_radius;
    const float r = d.radius > 0.f ? d.radius : 3.0f * s;
    const float iso = d.iso > 0.f ? d.iso : 0.5f;
    const float r2 = r * r;
    SPH_REQUIRE(s > 0.f && std::isfinite(r) && std::isfinite(r2) && r2 > 0.f, SPH_E_INVALID, "mesh spacing %g, radius %g: r * r must "
                "be a positive fp32", (double)s, (double)r);
    const double reach = std::ceil((double)r / (double)s);
    SPH_REQUIRE(reach <= (double)SPH_MESH_MAX_REACH, SPH_E_INVALID, "mesh radius %g is %g spacings: at most %d", (double)r,
                (double)r / (double)s, SPH_MESH_MAX_REACH);
    const double pad = reach + 1.0;
    double nodes = 1.0;
    for (int k = 0; k < 3; k++) {
        const double nk = std::ceil(((double)c->params.box_max[k] - (double)c->params.box_min[k]) / (double)s) + 1.0 + 2.0 * pad;
        SPH_REQUIRE(nk <= (double)SPH_MESH_MAX_DIM, SPH_E_CAPACITY, "mesh lattice: %.0f nodes on axis %d, at most %d (a wider spacing?)",
                    nk, k, SPH_MESH_MAX_DIM);
        A->n[k] = (uint32_t)nk;
        A->origin[k] = c->params.box_min[k] - (float)pad * s;
        SPH_REQUIRE(std::isfinite(A->origin[k]), SPH_E_INVALID, "mesh lattice: the origin does not fit fp32");
        nodes *= nk;
    }
    SPH_REQUIRE(nodes <= (double)SPH_MESH_MAX_NODES, SPH_E_CAPACITY, "mesh lattice: %u x %u x %u nodes, at most 2^27 (a wider spacing?)",
                A->n[0], A->n[1], A->n[2]);
    A->nodes = A->n[0] * A->n[1] * A->n[2];
    A->s = s;
    A->r2 = r2;
    A->reach = (int32_t)reach;
    const float v = iso * 4096.0f + 0.5f;
    const uint32_t q = v < 4294967296.0f ? (uint32_t)v : 0xFFFFFFFFu;
    A->iso_q = q > 1u ? q : 1u;
    return SPH_OK;
}

static int mesh_have(const sph_ctx* c, const char* who) {
    SPH_REQUIRE(c, SPH_E_INVALID, "null context");
    SPH_REQUIRE(c->mesh_valid, SPH_E_STATE, "%s: no mesh was extracted yet", who);
    return SPH_OK;
}

}  // namespace sph

using namespace sph;

extern "C" {

void sph_mesh_defaults(sph_mesh_params* p) {
    if (!p) return;
    p->spacing = 0.f;
    p->radius = 0.f;
    p->iso = 0.f;
}

int sph_mesh_lattice(const sph_ctx* c, const sph_mesh_params* p, uint32_t dims[3], float origin[3]) {
    SPH_REQUIRE(c && dims && origin, SPH_E_INVALID, "null argument");
    MeshArgs A;
    if (int e = mesh_resolve(c, p, &A)) return e;
    for (int k = 0; k < 3; k++) { dims[k] = A.n[k]; origin[k] = A.origin[k]; }
    return SPH_OK;
}

int sph_mesh_extract(sph_ctx* c, const sph_mesh_params* p, uint32_t* n_vertices, uint32_t* n_triangles) {
    SPH_REQUIRE(c, SPH_E_INVALID, "null context");
    SPH_REQUIRE(!c->slab, SPH_E_STATE, "sph_mesh_extract is not supported on a slab context (the ranks would have to share a "
                "lattice seam)");
    MeshArgs A;
    if (int e = mesh_resolve(c, p, &A)) return e;
    SPH_HIP(hipSetDevice(c->device));
    const uint32_t nb = ceil_div(A.nodes, MESH_BLOCK);
    if (A.nodes > c->mesh_nodes_cap) {                   // the first extraction, or a bigger lattice
        SPH_HIP(hipStreamSynchronize(c->stream));        // (a consumer of the old mesh on this stream has finished)
        release_mesh(c);
        int rc = c->mem.alloc(&c->mesh_field, A.nodes, false);
        if (!rc) rc = c->mem.alloc(&c->mesh_vbase, A.nodes, false);
        if (!rc) rc = c->mem.alloc(&c->mesh_aux, (size_t)MESH_AUX_HEAD + 2 * (size_t)nb, false);
        if (rc) { release_mesh(c); return rc; }
        c->mesh_nodes_cap = A.nodes;
        SPH_HIP(hipMemcpyAsync(c->mesh_aux + 2, case_table(), MESH_CASES * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    }
    c->mesh_valid = false;
    uint32_t* tot = c->mesh_aux;
    const uint32_t* cases = c->mesh_aux + 2;
    uint32_t* blk_v = c->mesh_aux + MESH_AUX_HEAD;
    uint32_t* blk_t = blk_v + nb;
    SPH_HIP(hipMemsetAsync(c->mesh_field, 0, (size_t)A.nodes * sizeof(uint32_t), c->stream));
    if (c->n)
#ifdef SPH_MESH_PLAIN_SPLAT      // measuring builds only: every add goes to the field (profiles/scripts/mesh_time.py)
        hipLaunchKernelGGL(k_mesh_splat<false>, dim3(ceil_div(c->n, MESH_THREADS)), dim3(MESH_THREADS), 0, c->stream,
                           c->posi + c->own_off, c->n, A, c->mesh_field);
#else
        hipLaunchKernelGGL(k_mesh_splat<true>, dim3(ceil_div(c->n, MESH_THREADS)), dim3(MESH_THREADS), 0, c->stream,
                           c->posi + c->own_off, c->n, A, c->mesh_field);
#endif
    hipLaunchKernelGGL(k_mesh_count, dim3(nb), dim3(MESH_THREADS), 0, c->stream, c->mesh_field, A, c->mesh_vbase, blk_v, blk_t);
    hipLaunchKernelGGL(k_mesh_scan_sums, dim3(1), dim3(MESH_SCAN2), 0, c->stream, blk_v, blk_t, nb, tot);
    hipLaunchKernelGGL(k_mesh_vbase, dim3(nb), dim3(MESH_THREADS), 0, c->stream, c->mesh_vbase, A.nodes, blk_v);
    SPH_HIP(hipGetLastError());
    uint32_t h[2] = {0, 0};
    SPH_HIP(hipMemcpyAsync(h, tot, sizeof h, hipMemcpyDeviceToHost, c->stream));
    SPH_HIP(hipStreamSynchronize(c->stream));            // the call's one wait
    const uint32_t nv = h[0], nt = h[1];
    if (nv > c->mesh_v_cap || nt > c->mesh_t_cap) {      // (the stream is idle: nothing reads the old buffers)
        int rc = SPH_OK;
        if (nv > c->mesh_v_cap) {
            c->mem.release(&c->mesh_vnrm); c->mem.release(&c->mesh_vpos);
            c->mesh_v_cap = 0;
            rc = c->mem.alloc(&c->mesh_vpos, (size_t)nv * 3, false);
            if (!rc) rc = c->mem.alloc(&c->mesh_vnrm, (size_t)nv * 3, false);
            if (!rc) c->mesh_v_cap = nv;
        }
        if (!rc && nt > c->mesh_t_cap) {
            c->mem.release(&c->mesh_tri);
            c->mesh_t_cap = 0;
            rc = c->mem.alloc(&c->mesh_tri, (size_t)nt * 3, false);
            if (!rc) c->mesh_t_cap = nt;
        }
        if (rc) { release_mesh(c); return rc; }
    }
    if (nv)      // (no vertex: no triangle either)
        hipLaunchKernelGGL(k_mesh_generate, dim3(nb), dim3(MESH_THREADS), 0, c->stream, c->mesh_field, A, c->mesh_vbase, blk_t, cases,
                           c->mesh_vpos, c->mesh_vnrm, c->mesh_tri);
    SPH_HIP(hipGetLastError());
    for (int k = 0; k < 3; k++) c->mesh_dims[k] = A.n[k];
    c->mesh_nv = nv;
    c->mesh_nt = nt;
    c->mesh_valid = true;
    if (n_vertices) *n_vertices = nv;
    if (n_triangles) *n_triangles = nt;
    return SPH_OK;
}

int sph_mesh_read(sph_ctx* c, float* pos_xyz, float* normal_xyz, uint32_t* tri) {
    if (int e = mesh_have(c, "sph_mesh_read")) return e;
    SPH_HIP(hipSetDevice(c->device));
    const size_t nv = c->mesh_nv, nt = c->mesh_nt;
    if (pos_xyz && nv) SPH_HIP(hipMemcpyAsync(pos_xyz, c->mesh_vpos, nv * 12, hipMemcpyDeviceToHost, c->stream));
    if (normal_xyz && nv) SPH_HIP(hipMemcpyAsync(normal_xyz, c->mesh_vnrm, nv * 12, hipMemcpyDeviceToHost, c->stream));
    if (tri && nt) SPH_HIP(hipMemcpyAsync(tri, c->mesh_tri, nt * 12, hipMemcpyDeviceToHost, c->stream));
    SPH_HIP(hipStreamSynchronize(c->stream));
    return SPH_OK;
}

int sph_mesh_dev(sph_ctx* c, void** pos_dev, void** normal_dev, void** tri_dev, uint32_t* n_vertices, uint32_t* n_triangles) {
    if (int e = mesh_have(c, "sph_mesh_dev")) return e;
    if (pos_dev) *pos_dev = c->mesh_vpos;
    if (normal_dev) *normal_dev = c->mesh_vnrm;
    if (tri_dev) *tri_dev = c->mesh_tri;
    if (n_vertices) *n_vertices = c->mesh_nv;
    if (n_triangles) *n_triangles = c->mesh_nt;
    return SPH_OK;
}

int sph_mesh_field_dims(sph_ctx* c, uint32_t dims[3]) {
    if (int e = mesh_have(c, "sph_mesh_field_dims")) return e;
    SPH_REQUIRE(dims, SPH_E_INVALID, "null argument");
    for (int k = 0; k < 3; k++) dims[k] = c->mesh_dims[k];
    return SPH_OK;
}

int sph_mesh_field_read(sph_ctx* c, uint32_t* counts) {
    if (int e = mesh_have(c, "sph_mesh_field_read")) return e;
    SPH_REQUIRE(counts, SPH_E_INVALID, "null argument");
    SPH_HIP(hipSetDevice(c->device));
    const size_t nodes = (size_t)c->mesh_dims[0] * c->mesh_dims[1] * c->mesh_dims[2];
    SPH_HIP(hipMemcpyAsync(counts, c->mesh_field, nodes * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    SPH_HIP(hipStreamSynchronize(c->stream));
    return SPH_OK;
}

int sph_mesh_save_obj(sph_ctx* c, const char* path) {
    if (int e = mesh_have(c, "sph_mesh_save_obj")) return e;
    SPH_REQUIRE(path, SPH_E_INVALID, "null argument");
    const size_t nv = c->mesh_nv, nt = c->mesh_nt;
    std::vector<float> pos(nv * 3), nrm(nv * 3);
    std::vector<uint32_t> tri(nt * 3);
    if (int e = sph_mesh_read(c, pos.data(), nrm.data(), tri.data())) return e;
    FILE* f = fopen(path, "w");
    SPH_REQUIRE(f, SPH_E_INVALID, "sph_mesh_save_obj: cannot open %s for writing", path);
    fprintf(f, "# %zu vertices, %zu triangles\n", nv, nt);
    for (size_t v = 0; v < nv; v++) fprintf(f, "v %.9g %.9g %.9g\n", (double)pos[3 * v], (double)pos[3 * v + 1], (double)pos[3 * v + 2]);
    for (size_t v = 0; v < nv; v++) fprintf(f, "vn %.9g %.9g %.9g\n", (double)nrm[3 * v], (double)nrm[3 * v + 1], (double)nrm[3 * v + 2]);
    for (size_t t = 0; t < nt; t++) {
        const unsigned a = tri[3 * t] + 1u, b = tri[3 * t + 1] + 1u, d = tri[3 * t + 2] + 1u;
        fprintf(f, "f %u//%u %u//%u %u//%u\n", a, a, b, b, d, d);
    }
    const bool bad = ferror(f) != 0;
    SPH_REQUIRE(fclose(f) == 0 && !bad, SPH_E_INVALID, "sph_mesh_save_obj: writing %s failed", path);
    return SPH_OK;
}

}  // extern "C"

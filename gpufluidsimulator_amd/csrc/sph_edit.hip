// sph_edit.hip -- particles enter and leave a running whole-domain context: sph_emit, sph_remove, sph_count_in_regions
// (include/sph_hip.h).  The one hot path is the removal: a stable, in-order compaction of the sorted arrays
// posi / velr / keyS into their ping-pong twins -- the survivors keep their relative slot order, so the range stays sorted by
// the keys of the last sort and the next sort may merge.  No atomic decides an order; every run gives the same slots.
//
//   k_edit_count    one pass over posi: the region predicate per slot, a ballot per wave, one count per 2048-slot tile
//   k_edit_scan     one block: exclusive scan of the tile counts, and their total (scan_array_one_block, sph_device.hpp)
//   k_edit_compact  the predicate again (same arithmetic, same answer), ranks from the ballot masks; survivors stream to
//                   slot - (selected particles in front of it) with 16-byte loads and stores, the selected ones leave their
//                   creation index in slot order and their row of the by-index position buffer is zeroed
//
// The tile counts and offsets live in the movers' ping-pong scratch of the sort (edit_tiles below) and the removed indices in k0:
// all three are dead between two steps, so a call that selects nothing leaves every bit of the context as it was.
#include "sph_device.hpp"

#include <cmath>
#include <cstring>

namespace sph {

constexpr uint32_t EDIT_THREADS = 256;
constexpr uint32_t EDIT_ROUNDS = 8;                              // 64-slot chunks per wave
constexpr uint32_t EDIT_WAVE_SLOTS = EDIT_ROUNDS * 64u;          // a wave owns 512 consecutive slots
constexpr uint32_t EDIT_TILE = (EDIT_THREADS / 64u) * EDIT_WAVE_SLOTS;   // a block owns 2048

// the regions of one call as the kernels take them: a kernel argument by value, like Spheres
struct Regions {
    sph_region r[SPH_MAX_REGIONS];
    uint32_t n;
};

// Membership as include/sph_hip.h states it: fp32, every operation rounded (no multiply-add fusion), sums left to right --
// tests/region_model.py decides every particle identically in numpy.
__device__ __forceinline__ bool in_regions(const Regions& R, float x, float y, float z) {
#pragma clang fp contract(off)
    bool in = false;
    for (uint32_t j = 0; j < R.n; j++) {
        const sph_region& g = R.r[j];
        if (g.kind == SPH_REGION_SPHERE) {
            const float dx = x - g.a[0], dy = y - g.a[1], dz = z - g.a[2];
            in |= dx * dx + dy * dy + dz * dz < g.r * g.r;
        } else if (g.kind == SPH_REGION_BOX) {
            in |= g.a[0] <= x && x < g.b[0] && g.a[1] <= y && y < g.b[1] && g.a[2] <= z && z < g.b[2];
        } else {
            in |= (x - g.a[0]) * g.b[0] + (y - g.a[1]) * g.b[1] + (z - g.a[2]) * g.b[2] < 0.f;
        }
    }
    return in;
}

// the wave's 8 chunks: positions (all loads in flight before the first is used) and the ballot of the predicate per chunk
__device__ __forceinline__ uint32_t edit_masks(const float4* __restrict__ posi, uint32_t n, const Regions& R, uint32_t base,
                                               uint32_t lane, float4 (&p)[EDIT_ROUNDS], uint64_t (&m)[EDIT_ROUNDS]) {
#pragma unroll
    for (uint32_t j = 0; j < EDIT_ROUNDS; j++) {
        const uint32_t s = base + j * 64u + lane;
        p[j] = s < n ? posi[s] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t j = 0; j < EDIT_ROUNDS; j++) {
        const uint32_t s = base + j * 64u + lane;
        m[j] = __ballot(s < n && in_regions(R, p[j].x, p[j].y, p[j].z));
        cnt += (uint32_t)__popcll(m[j]);
    }
    return cnt;
}

__global__ __launch_bounds__(EDIT_THREADS) void k_edit_count(const float4* __restrict__ posi, uint32_t n, Regions R,
                                                             uint32_t* __restrict__ tile_cnt) {
    __shared__ uint32_t wsum[EDIT_THREADS / 64u];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    float4 p[EDIT_ROUNDS];
    uint64_t m[EDIT_ROUNDS];
    const uint32_t cnt = edit_masks(posi, n, R, blockIdx.x * EDIT_TILE + w * EDIT_WAVE_SLOTS, lane, p, m);
    if (lane == 0u) wsum[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0u) tile_cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one block: exclusive scan of the tile counts (scan_array_one_block, sph_device.hpp; the counts are left as they are)
__global__ __launch_bounds__(1024) void k_edit_scan(const uint32_t* __restrict__ tile_cnt, uint32_t nt,
                                                    uint32_t* __restrict__ tile_off, uint32_t* __restrict__ total) {
    __shared__ uint32_t lds[1024 / 64];
    const uint32_t sum = scan_array_one_block<1024>(nt, lds, [&](uint32_t t) { return tile_cnt[t]; },
                                                    [&](uint32_t t, uint32_t before) { tile_off[t] = before; });
    if (threadIdx.x == 1023u) *total = sum;
}

__global__ __launch_bounds__(EDIT_THREADS) void k_edit_compact(const float4* __restrict__ posi, const float4* __restrict__ velr,
                                                               const uint32_t* __restrict__ key, uint32_t n, Regions R,
                                                               const uint32_t* __restrict__ tile_off,
                                                               float4* __restrict__ posi_out, float4* __restrict__ velr_out,
                                                               uint32_t* __restrict__ key_out, uint32_t* __restrict__ removed,
                                                               uint32_t max_removed, float4* __restrict__ pos_by_index,
                                                               uint32_t pos_cap) {
    __shared__ uint32_t wsum[EDIT_THREADS / 64u];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t base = blockIdx.x * EDIT_TILE + w * EDIT_WAVE_SLOTS;
    float4 p[EDIT_ROUNDS];
    uint64_t m[EDIT_ROUNDS];
    const uint32_t cnt = edit_masks(posi, n, R, base, lane, p, m);
    if (lane == 0u) wsum[w] = cnt;
    __syncthreads();
    uint32_t before = tile_off[blockIdx.x];                  // selected particles in front of this wave's first slot
    for (uint32_t k = 0; k < w; k++) before += wsum[k];
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (uint32_t j = 0; j < EDIT_ROUNDS; j++) {
        const uint32_t s = base + j * 64u + lane;
        const uint32_t rank = before + (uint32_t)__popcll(m[j] & below);     // selected particles in front of slot s
        if (s < n) {
            if ((m[j] >> lane) & 1ull) {
                const uint32_t idx = __float_as_uint(p[j].w);
                if (rank < max_removed) removed[rank] = idx;
                if (pos_by_index && idx < pos_cap) pos_by_index[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                const uint32_t d = s - rank;
                posi_out[d] = p[j];
                velr_out[d] = velr[s];
                key_out[d] = key[s];
            }
        }
        before += (uint32_t)__popcll(m[j]);
    }
}

// the by-index position rows of freshly appended particles: (x, y, z, 1), as sph_upload writes them
__global__ __launch_bounds__(256) void k_emit_positions(const float4* __restrict__ posi, uint32_t n,
                                                        float4* __restrict__ pos_by_index, uint32_t pos_cap) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 p = posi[i];
    const uint32_t idx = __float_as_uint(p.w);
    if (idx < pos_cap) pos_by_index[idx] = make_float4(p.x, p.y, p.z, 1.0f);
}

static int check_regions(const sph_ctx* c, uint32_t n_regions, const sph_region* regions, Regions& R, const char* who) {
    SPH_REQUIRE(c, SPH_E_INVALID, "null context");
    SPH_REQUIRE(!c->slab, SPH_E_STATE, "%s is not supported on a slab context (the slab step sizes its messages from the "
                "previous step's counts)", who);
    SPH_REQUIRE(n_regions >= 1u && n_regions <= (uint32_t)SPH_MAX_REGIONS, SPH_E_INVALID, "%s: %u regions (1..%d)", who, n_regions,
                SPH_MAX_REGIONS);
    SPH_REQUIRE(regions, SPH_E_INVALID, "null regions");
    memset(&R, 0, sizeof(R));
    for (uint32_t j = 0; j < n_regions; j++) {
        const sph_region& g = regions[j];
        SPH_REQUIRE(g.kind == SPH_REGION_SPHERE || g.kind == SPH_REGION_BOX || g.kind == SPH_REGION_HALFSPACE, SPH_E_INVALID,
                    "region %u: unknown kind %d", j, (int)g.kind);
        bool finite = std::isfinite(g.a[0]) && std::isfinite(g.a[1]) && std::isfinite(g.a[2]);
        if (g.kind == SPH_REGION_SPHERE) finite = finite && std::isfinite(g.r);
        else finite = finite && std::isfinite(g.b[0]) && std::isfinite(g.b[1]) && std::isfinite(g.b[2]);
        SPH_REQUIRE(finite, SPH_E_INVALID, "region %u: a field its kind uses is not finite", j);
        R.r[j].kind = g.kind;                                  // (the fields a kind does not use stay 0)
        for (int a = 0; a < 3; a++) R.r[j].a[a] = g.a[a];
        if (g.kind == SPH_REGION_SPHERE) R.r[j].r = g.r;
        else for (int a = 0; a < 3; a++) R.r[j].b[a] = g.b[a];
    }
    R.n = n_regions;
    return SPH_OK;
}

// The tile counts and offsets of a selection borrow the movers' ping-pong of the sort: `cap` words each (sort_buffers_alloc),
// dead between two steps.
struct EditTiles { uint32_t* cnt; uint32_t* off; };
static EditTiles edit_tiles(sph_ctx* c) { return EditTiles{c->mm_k1, c->mm_v1}; }

// the selection of the owned range: tile counts and their offsets into edit_tiles, the total to the host (synchronises)
static int count_selected(sph_ctx* c, const Regions& R, uint32_t* total) {
    *total = 0;
    if (c->n == 0) return SPH_OK;
    const uint32_t nt = ceil_div(c->n, EDIT_TILE);
    SPH_REQUIRE(nt <= c->cap, SPH_E_CAPACITY, "%u selection tiles > the %u words of the scratch they borrow", nt, c->cap);
    const EditTiles t = edit_tiles(c);
    hipLaunchKernelGGL(k_edit_count, dim3(nt), dim3(EDIT_THREADS), 0, c->stream, c->posi + c->own_off, c->n, R, t.cnt);
    hipLaunchKernelGGL(k_edit_scan, dim3(1), dim3(1024), 0, c->stream, t.cnt, nt, t.off, c->d_scratch);
    SPH_HIP(hipGetLastError());
    SPH_HIP(hipMemcpyAsync(c->h_scratch, c->d_scratch, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    SPH_HIP(hipStreamSynchronize(c->stream));
    *total = c->h_scratch[0];
    return SPH_OK;
}

}  // namespace sph

using namespace sph;

extern "C" {

int sph_count_in_regions(sph_ctx* c, uint32_t n_regions, const sph_region* regions, uint32_t* count) {
    Regions R;
    int rc = check_regions(c, n_regions, regions, R, "sph_count_in_regions");
    if (rc) return rc;
    SPH_REQUIRE(count, SPH_E_INVALID, "null argument");
    SPH_HIP(hipSetDevice(c->device));
    return count_selected(c, R, count);
}

int sph_remove(sph_ctx* c, uint32_t n_regions, const sph_region* regions, uint32_t* n_removed, uint32_t* removed_index,
               uint32_t max_out) {
    Regions R;
    int rc = check_regions(c, n_regions, regions, R, "sph_remove");
    if (rc) return rc;
    if (n_removed) *n_removed = 0;
    SPH_HIP(hipSetDevice(c->device));
    uint32_t total = 0;
    rc = count_selected(c, R, &total);
    if (rc) return rc;
    if (total == 0) return SPH_OK;            // nothing selected: no bit of the state and no flag has changed
    SPH_REQUIRE(total <= c->n, SPH_E_DEVICE, "sph_remove: the device counted %u of %u particles", total, c->n);
    // the table of the last sort describes slots that are about to move: clear it from the OLD keys while they are in place
    rc = launch_cells_clear(c);
    if (rc) return rc;
    mm_drop_marks(c);                         // per-slot marks of the integrate epilogue: the slots are renumbered
    const uint32_t n = c->n, take = removed_index ? (max_out < total ? max_out : total) : 0u;
    hipLaunchKernelGGL(k_edit_compact, dim3(ceil_div(n, EDIT_TILE)), dim3(EDIT_THREADS), 0, c->stream, c->posi + c->own_off,
                       c->velr + c->own_off, c->keyS + c->own_off, n, R, edit_tiles(c).off, c->posi2 + c->gcap, c->velr2 + c->gcap,
                       c->keyS2 + c->gcap, c->k0, take, c->pos_out, c->pos_out_cap);
    SPH_HIP(hipGetLastError());
    // dp / cw are not compacted (the next step rewrites them): what a slot holds now belongs to another particle, so the
    // survivors' rows read 0 until then, like those of an emitted particle -- sph_download never hands out a neighbour's density
    if (n > total) {
        SPH_HIP(hipMemsetAsync(c->dp + c->gcap, 0, (size_t)(n - total) * sizeof(float2), c->stream));
        SPH_HIP(hipMemsetAsync(c->cw + c->gcap, 0, (size_t)(n - total) * sizeof(float2), c->stream));
    }
    if (take) SPH_HIP(hipMemcpyAsync(removed_index, c->k0, (size_t)take * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    SPH_HIP(hipStreamSynchronize(c->stream));
    swap_state(c, true);
    c->n = n - total;
    // order_valid stays as it was: the survivors follow the last sort, keyS holds its keys.  Everything derived from the
    // old slot numbers is stale -- the treatment of sph_set_by_index, plus the table (cleared above).
    positions_moved(c);                       // k0 held the keys of the old slots (and now the removed indices)
    c->last_perm = nullptr;
    mover_count_unknown(c);
    results_stale(c);
    if (n_removed) *n_removed = total;
    return SPH_OK;
}

int sph_emit(sph_ctx* c, uint32_t n, const float* pos_xyz, const float* vel_xyz, const uint32_t* index,
             uint32_t* first_index_out) {
    SPH_REQUIRE(c, SPH_E_INVALID, "null context");
    SPH_REQUIRE(!c->slab, SPH_E_STATE, "sph_emit is not supported on a slab context (the slab step sizes its messages from the "
                "previous step's counts)");
    SPH_REQUIRE(n == 0 || pos_xyz, SPH_E_INVALID, "null positions");
    SPH_REQUIRE((uint64_t)c->n + n <= c->cap, SPH_E_CAPACITY, "%u + %u particles exceed the capacity %u", c->n, n, c->cap);
    const uint32_t first = c->next_index;
    if (!index)
        SPH_REQUIRE((uint64_t)first + n <= c->pos_out_cap, SPH_E_CAPACITY, "creation indices [%u, +%u) reach the capacity %u: "
                    "pass the indices sph_remove returned", first, n, c->pos_out_cap);
    uint32_t next = index ? c->next_index : first + n;
    for (uint32_t i = 0; i < n; i++) {
        for (int a = 0; a < 3; a++) {
            const float x = pos_xyz[3 * (size_t)i + a];
            SPH_REQUIRE(std::isfinite(x) && x >= c->params.box_min[a] && x <= c->params.box_max[a], SPH_E_INVALID,
                        "particle %u: position %g on axis %d is not inside the box", i, (double)x, a);
            SPH_REQUIRE(!vel_xyz || std::isfinite(vel_xyz[3 * (size_t)i + a]), SPH_E_INVALID, "particle %u: velocity is not finite", i);
        }
        if (index) {
            SPH_REQUIRE(index[i] < c->pos_out_cap, SPH_E_INVALID, "creation index %u >= capacity %u", index[i], c->pos_out_cap);
            if (index[i] >= next) next = index[i] + 1u;
        }
    }
    if (first_index_out) *first_index_out = index ? (n ? index[0] : first) : first;
    if (n == 0) return SPH_OK;
    SPH_HIP(hipSetDevice(c->device));
    std::vector<float4> hp(n), hv(n);
    pack_records(n, pos_xyz, vel_xyz, index, first, hp.data(), hv.data());
    const uint32_t at = c->own_off + c->n;                   // behind the owned range, as sph_migrants_append does
    SPH_HIP(hipMemcpyAsync(c->posi + at, hp.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    SPH_HIP(hipMemcpyAsync(c->velr + at, hv.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    SPH_HIP(hipMemsetAsync(c->dp + at, 0, (size_t)n * sizeof(float2), c->stream));
    SPH_HIP(hipMemsetAsync(c->cw + at, 0, (size_t)n * sizeof(float2), c->stream));
    hipLaunchKernelGGL(k_emit_positions, dim3(ceil_div(n, 256u)), dim3(256), 0, c->stream, c->posi + at, n, c->pos_out,
                       c->pos_out_cap);
    SPH_HIP(hipGetLastError());
    SPH_HIP(hipStreamSynchronize(c->stream));                // the host staging goes away now
    c->n += n;
    c->next_index = next;
    order_lost(c);
    mover_count_unknown(c);
    results_stale(c);
    return SPH_OK;
}

}  // extern "C"

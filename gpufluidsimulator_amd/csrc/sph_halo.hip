// sph_halo.hip -- z-slab support: migrants, ghost layers, layer histogram (multi-GPU).
//
// No counterpart in the reference (single GPU).  A rank owns the cell layers [z_lo, z_hi) of the
// global grid; cell keys are slab-local with z slowest, so after the sort
//   * particles that left the slab sit at the two ENDS of the owned range (local layer 0 / zl-1),
//   * the boundary layers a neighbour needs as ghosts are the first / last layer of what is left,
// i.e. both are contiguous slices of the sorted SoA arrays.  The library packs those slices into
// caller-provided device buffers (the caller moves them with RCCL send/recv via torch.distributed)
// and installs received records: ghosts go directly in front of / behind the owned range, already
// in key order, so no re-sort is needed for ghosts.
//
// This file also OWNS the small kernels of a slab's messages -- record pack and unpack, the ghosts' (rho, p) unpack, the lower
// bounds of a few targets in the sorted keys, the header writer -- one of each, two-sided; the native one-call step
// (sph_slab.hip) launches them on its own streams through the launch_* functions declared in sph_common.hpp.
#include "sph_device.hpp"

namespace sph {

// ---- the kernels of the messages: ONE of each, two-sided (a one-sided caller passes n = 0 for the other side).  The slab step
//      (sph_slab.hip) reaches them through the launchers below, declared in sph_common.hpp ------------------------------------------
__global__ __launch_bounds__(256) void k_pack_records(RecSide lo, RecSide hi) {
    const SideSplit s = side_split(blockIdx.x * 256u + threadIdx.x, lo.n, hi.n);
    if (!s.live) return;
    const RecSide& a = s.hi ? hi : lo;
    put_record(a.rec, s.i, a.posi[s.i], a.velr[s.i]);
}

__global__ __launch_bounds__(256) void k_unpack_records(RecSide lo, RecSide hi, GridDesc g, uint32_t G, volatile uint32_t* err_word) {
    const SideSplit s = side_split(blockIdx.x * 256u + threadIdx.x, lo.n, hi.n);
    if (!s.live) return;
    const RecSide& a = s.hi ? hi : lo;
    float4 p, v;
    get_record(a.rec, s.i, p, v);
    a.posi[s.i] = p;
    a.velr[s.i] = v;
    if (!a.key && !err_word) return;
    const uint32_t k = cell_key(g, p.x, p.y, p.z);
    if (a.key) a.key[s.i] = k;
    // a particle that is not inside this slab at all cannot be represented (its key is clamped into a ghost layer)
    const uint32_t lz = k / (g.g[0] * g.g[1]);
    if (err_word && (lz < G || lz + G >= g.zl)) *err_word = 1u;
}

__global__ __launch_bounds__(256) void k_unpack_dp(const float2* __restrict__ src_lo, float2* __restrict__ dp_lo, float2* __restrict__ cw_lo,
                                                   uint32_t n_lo, const float2* __restrict__ src_hi, float2* __restrict__ dp_hi,
                                                   float2* __restrict__ cw_hi, uint32_t n_hi, Phys ph) {
    const SideSplit s = side_split(blockIdx.x * 256u + threadIdx.x, n_lo, n_hi);
    if (!s.live) return;
    const float2 v = (s.hi ? src_hi : src_lo)[s.i];
    (s.hi ? dp_hi : dp_lo)[s.i] = v;
    (s.hi ? cw_hi : cw_lo)[s.i] = neighbour_terms(ph, v.x, v.y);
}

__global__ __launch_bounds__(64) void k_lower_bounds(const uint32_t* __restrict__ keys, uint32_t n, LbTargets tg, uint32_t* __restrict__ out,
                                                     volatile uint32_t* __restrict__ out_host) {
    const uint32_t t = threadIdx.x;
    if (t >= tg.m) return;
    const uint32_t v = tg.v[t];
    const uint32_t r = first_not(0u, n, [&](uint32_t i) { return keys[i] < v; });
    out[t] = r;
    if (out_host) out_host[t] = r;
}

__global__ __launch_bounds__(64) void k_headers(float4* __restrict__ out_lo, float4* __restrict__ out_hi, float4 lo, float4 hi) {
    if (threadIdx.x == 0) out_lo[0] = lo;
    if (threadIdx.x == 1) out_hi[0] = hi;
}

int launch_pack_records(hipStream_t st, const RecSide& lo, const RecSide& hi) {
    if (lo.n + hi.n) hipLaunchKernelGGL(k_pack_records, dim3(ceil_div(lo.n + hi.n, 256u)), dim3(256), 0, st, lo, hi);
    SPH_HIP(hipGetLastError());
    return SPH_OK;
}

int launch_unpack_records(hipStream_t st, const RecSide& lo, const RecSide& hi, const GridDesc& g, uint32_t G, volatile uint32_t* err_word) {
    if (lo.n + hi.n) hipLaunchKernelGGL(k_unpack_records, dim3(ceil_div(lo.n + hi.n, 256u)), dim3(256), 0, st, lo, hi, g, G, err_word);
    SPH_HIP(hipGetLastError());
    return SPH_OK;
}

int launch_unpack_dp(hipStream_t st, const float2* src_lo, float2* dp_lo, float2* cw_lo, uint32_t n_lo, const float2* src_hi, float2* dp_hi,
                     float2* cw_hi, uint32_t n_hi, const Phys& ph) {
    if (n_lo + n_hi)
        hipLaunchKernelGGL(k_unpack_dp, dim3(ceil_div(n_lo + n_hi, 256u)), dim3(256), 0, st, src_lo, dp_lo, cw_lo, n_lo, src_hi, dp_hi, cw_hi,
                           n_hi, ph);
    SPH_HIP(hipGetLastError());
    return SPH_OK;
}

int launch_lower_bounds(hipStream_t st, const uint32_t* keys, uint32_t n, const LbTargets& tg, uint32_t* out, volatile uint32_t* out_host) {
    SPH_REQUIRE(tg.m <= LB_MAX, SPH_E_INVALID, "too many targets");
    if (tg.m) hipLaunchKernelGGL(k_lower_bounds, dim3(1), dim3(64), 0, st, keys, n, tg, out, out_host);
    SPH_HIP(hipGetLastError());
    return SPH_OK;
}

int launch_headers(hipStream_t st, float4* out_lo, float4* out_hi, float4 lo, float4 hi) {
    hipLaunchKernelGGL(k_headers, dim3(1), dim3(64), 0, st, out_lo, out_hi, lo, hi);
    SPH_HIP(hipGetLastError());
    return SPH_OK;
}

// lower bounds of a few key targets in the owned sorted keys, returned through the context's scratch pair
static int lower_bounds(sph_ctx* c, LbTargets tg, uint32_t* out) {
    SPH_HIP(hipSetDevice(c->device));
    const int rc = launch_lower_bounds(c->stream, c->keyS + c->own_off, c->n, tg, c->d_scratch, nullptr);
    if (rc) return rc;
    SPH_HIP(hipMemcpyAsync(c->h_scratch, c->d_scratch, tg.m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    SPH_HIP(hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < tg.m; k++) out[k] = c->h_scratch[k];
    return SPH_OK;
}

// the first m[0] and the last m[1] slots of the sorted owned range -> the caller's two buffers
static int pack_ends(sph_ctx* c, const uint32_t m[2], void* buf_dev[2], uint32_t capacity) {
    for (int side = 0; side < 2; side++) {
        SPH_REQUIRE(m[side] <= capacity, SPH_E_CAPACITY, "halo slice of %u records > buffer capacity %u", m[side], capacity);
        SPH_REQUIRE(!m[side] || buf_dev[side], SPH_E_INVALID, "null halo buffer");
    }
    const uint32_t hi0 = c->own_off + c->n - m[1];
    return launch_pack_records(c->stream, RecSide{(float4*)buf_dev[0], c->posi + c->own_off, c->velr + c->own_off, nullptr, m[0]},
                               RecSide{(float4*)buf_dev[1], c->posi + hi0, c->velr + hi0, nullptr, m[1]});
}

}  // namespace sph

using namespace sph;

extern "C" {

int sph_migrants_count(sph_ctx* c, uint32_t count[2]) {
    SPH_REQUIRE(c && count, SPH_E_INVALID, "null argument");
    SPH_REQUIRE(c->stage == sph_ctx::ST_SORTED, SPH_E_STATE, "sph_migrants_count needs sph_sort first");
    const uint32_t layer = c->grid.g[0] * c->grid.g[1];
    const uint32_t G = c->ghost_layers;
    uint32_t lb[2];
    int rc = lower_bounds(c, LbTargets{{G * layer, (c->grid.zl - G) * layer}, 2u}, lb);
    if (rc) return rc;
    count[0] = lb[0];
    count[1] = c->n - lb[1];
    return SPH_OK;
}

int sph_slab_counts(sph_ctx* c, uint32_t count[4]) {
    SPH_REQUIRE(c && count, SPH_E_INVALID, "null argument");
    SPH_REQUIRE(c->stage == sph_ctx::ST_SORTED, SPH_E_STATE, "sph_slab_counts needs sph_sort first");
    uint32_t lb[4];
    int rc = lower_bounds(c, layer_bound_targets(c), lb);
    if (rc) return rc;
    count[0] = lb[0];
    count[1] = lb[1] - lb[0];
    count[2] = lb[3] - lb[2];
    count[3] = c->n - lb[3];
    return SPH_OK;
}

int sph_migrants_pack(sph_ctx* c, void* buf_dev[2], uint32_t capacity) {
    SPH_REQUIRE(c && buf_dev, SPH_E_INVALID, "null argument");
    uint32_t m[2];
    int rc = sph_migrants_count(c, m);
    if (rc) return rc;
    rc = pack_ends(c, m, buf_dev, capacity);
    if (rc) return rc;
    rc = table_drop_ends(c, m[0], m[1]);      // the cells of the particles that leave
    if (rc) return rc;
    c->own_off += m[0];
    c->n -= m[0] + m[1];
    return SPH_OK;
}

int sph_migrants_append(sph_ctx* c, const void* buf_dev, uint32_t n_in) {
    SPH_REQUIRE(c, SPH_E_INVALID, "null context");
    if (n_in == 0) return SPH_OK;
    SPH_REQUIRE(buf_dev, SPH_E_INVALID, "null buffer");
    SPH_REQUIRE(c->n + n_in <= c->cap && c->own_off + c->n + n_in <= c->tot, SPH_E_CAPACITY,
                "%u + %u particles exceed the capacity %u", c->n, n_in, c->cap);
    SPH_HIP(hipSetDevice(c->device));
    const uint32_t at = c->own_off + c->n;
    const int rc = launch_unpack_records(c->stream, RecSide{(float4*)buf_dev, c->posi + at, c->velr + at, nullptr, n_in}, RecSide{}, c->grid, 0u,
                                         nullptr);
    if (rc) return rc;
    c->n += n_in;
    order_lost(c);              // hash + sort again
    // (no results_stale: kept as found.  The sort that must follow calls it; only a caller that asks for forces or packs
    // densities BEFORE that sort is served those of the old slots.  No mover_count_unknown: that sort is the full one, and the
    // slab step is host-paced and never reads it)
    return SPH_OK;
}

int sph_halo_count(sph_ctx* c, uint32_t count[2]) {
    SPH_REQUIRE(c && count, SPH_E_INVALID, "null argument");
    SPH_REQUIRE(c->stage >= sph_ctx::ST_SORTED, SPH_E_STATE, "sph_halo_count needs sph_sort first");
    const uint32_t layer = c->grid.g[0] * c->grid.g[1];
    const uint32_t G = c->ghost_layers;
    uint32_t lb[2];
    int rc = lower_bounds(c, LbTargets{{(G + 1) * layer, (c->grid.zl - G - 1) * layer}, 2u}, lb);
    if (rc) return rc;
    count[0] = lb[0];
    count[1] = c->n - lb[1];
    return SPH_OK;
}

int sph_halo_pack_counts(sph_ctx* c, void* buf_dev[2], uint32_t capacity, const uint32_t count[2]) {
    SPH_REQUIRE(c && buf_dev, SPH_E_INVALID, "null argument");
    SPH_REQUIRE(c->stage >= sph_ctx::ST_SORTED, SPH_E_STATE, "sph_halo_pack needs sph_sort first");
    uint32_t m[2];
    if (count) {
        m[0] = count[0]; m[1] = count[1];
        SPH_REQUIRE(m[0] <= c->n && m[1] <= c->n, SPH_E_INVALID, "halo counts exceed the owned particles");
    } else {
        int rc = sph_halo_count(c, m);
        if (rc) return rc;
    }
    SPH_HIP(hipSetDevice(c->device));
    int rc = pack_ends(c, m, buf_dev, capacity);
    if (rc) return rc;
    c->halo_n[0] = m[0]; c->halo_n[1] = m[1]; c->halo_n_valid = true;
    return SPH_OK;
}

int sph_halo_pack(sph_ctx* c, void* buf_dev[2], uint32_t capacity) { return sph_halo_pack_counts(c, buf_dev, capacity, nullptr); }

int sph_halo_unpack(sph_ctx* c, const void* lo_dev, uint32_t n_lo, const void* hi_dev, uint32_t n_hi) {
    SPH_REQUIRE(c, SPH_E_INVALID, "null context");
    SPH_REQUIRE(c->stage >= sph_ctx::ST_SORTED, SPH_E_STATE, "sph_halo_unpack needs sph_sort first");
    SPH_REQUIRE(n_lo <= c->own_off && c->own_off + c->n + n_hi <= c->tot && n_lo <= c->gcap && n_hi <= c->gcap,
                SPH_E_CAPACITY, "ghost layers of %u / %u records exceed the ghost capacity %u", n_lo, n_hi, c->gcap);
    SPH_HIP(hipSetDevice(c->device));
    if (!table_covers(c, c->own_off, c->own_off + c->n)) {
        int rc = launch_cells_clear(c);   // a table that includes old ghosts; one over just the owned slots is kept
        if (rc) return rc;
    }
    SPH_REQUIRE((!n_lo || lo_dev) && (!n_hi || hi_dev), SPH_E_INVALID, "null buffer");
    const uint32_t at_lo = c->own_off - n_lo, at_hi = c->own_off + c->n;       // with their cell keys: already in key order
    const int rc = launch_unpack_records(c->stream, RecSide{(float4*)lo_dev, c->posi + at_lo, c->velr + at_lo, c->keyS + at_lo, n_lo},
                                         RecSide{(float4*)hi_dev, c->posi + at_hi, c->velr + at_hi, c->keyS + at_hi, n_hi}, c->grid, 0u, nullptr);
    if (rc) return rc;
    c->n_glo = n_lo;
    c->n_ghi = n_hi;
    c->stage = sph_ctx::ST_SORTED;
    return SPH_OK;
}

int sph_halo_pack_density(sph_ctx* c, void* buf_dev[2], uint32_t capacity) {
    SPH_REQUIRE(c && buf_dev, SPH_E_INVALID, "null argument");
    SPH_REQUIRE(c->have_dens, SPH_E_STATE, "sph_halo_pack_density needs sph_density first");
    uint32_t m[2];
    if (c->halo_n_valid) {          // same particles, same order as the position halo of this step
        m[0] = c->halo_n[0]; m[1] = c->halo_n[1];
    } else {
        int rc = sph_halo_count(c, m);
        if (rc) return rc;
    }
    SPH_HIP(hipSetDevice(c->device));
    SPH_REQUIRE(m[0] <= capacity && m[1] <= capacity, SPH_E_CAPACITY, "halo slice > buffer capacity %u", capacity);
    if (m[0]) SPH_HIP(hipMemcpyAsync(buf_dev[0], c->dp + c->own_off, m[0] * sizeof(float2), hipMemcpyDeviceToDevice, c->stream));
    if (m[1]) SPH_HIP(hipMemcpyAsync(buf_dev[1], c->dp + c->own_off + c->n - m[1], m[1] * sizeof(float2), hipMemcpyDeviceToDevice, c->stream));
    return SPH_OK;
}

int sph_halo_unpack_density(sph_ctx* c, const void* lo_dev, const void* hi_dev) {
    SPH_REQUIRE(c, SPH_E_INVALID, "null context");
    SPH_HIP(hipSetDevice(c->device));
    SPH_REQUIRE((!c->n_glo || lo_dev) && (!c->n_ghi || hi_dev), SPH_E_INVALID, "null buffer");
    const uint32_t at_lo = c->own_off - c->n_glo, at_hi = c->own_off + c->n;
    return launch_unpack_dp(c->stream, (const float2*)lo_dev, c->dp + at_lo, c->cw + at_lo, c->n_glo, (const float2*)hi_dev, c->dp + at_hi,
                            c->cw + at_hi, c->n_ghi, c->phys);
}

int sph_layer_histogram(sph_ctx* c, uint32_t* hist, uint32_t n_layers) {
    SPH_REQUIRE(c && hist, SPH_E_INVALID, "null argument");
    SPH_REQUIRE(c->stage >= sph_ctx::ST_SORTED, SPH_E_STATE, "sph_layer_histogram needs sph_sort first");
    SPH_REQUIRE(n_layers == c->grid.g[2], SPH_E_INVALID, "n_layers must be the global z grid size %u", c->grid.g[2]);
    const uint32_t layer = c->grid.g[0] * c->grid.g[1];
    for (uint32_t l = 0; l < n_layers; l++) hist[l] = 0;
    // local layer l holds global layer l + z_off
    uint32_t prev = 0;
    for (uint32_t ll0 = 0; ll0 < c->grid.zl; ll0 += 30) {
        uint32_t m = c->grid.zl - ll0 < 30 ? c->grid.zl - ll0 : 30, lb[LB_MAX];
        LbTargets tg{{}, m};
        for (uint32_t k = 0; k < m; k++) tg.v[k] = (ll0 + k + 1) * layer;
        int rc = lower_bounds(c, tg, lb);
        if (rc) return rc;
        for (uint32_t k = 0; k < m; k++) {
            int64_t gl = (int64_t)c->grid.z_off + ll0 + k;
            if (gl >= 0 && gl < (int64_t)n_layers) hist[gl] = lb[k] - prev;
            prev = lb[k];
        }
    }
    return SPH_OK;
}

}  // extern "C"

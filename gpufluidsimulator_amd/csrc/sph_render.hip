// sph_render.hip -- the fluid as a picture, on the device: depth-tested sphere sprites (sph_camera_look_at, sph_render,
// sph_render_read, sph_render_image_dev of include/sph_hip.h).  Stands in for the reference's OpenGL point-sprite renderer
// (SPH/render_particles.cpp, SPH/shaders.cpp: gl_PointSize = R * scale / dist, `if (mag > 1.0) discard`, a diffuse light on
// the sprite's sphere normal, colours from colorRamp by creation index) without a GL context and without a copy of the state
// to the host: one pass over posi.
//
//   k_render_clear    every pixel's 64-bit key = ~0
//   k_render_splat    one owned particle per lane: project it (sprite_of), walk the pixels of its sprite's bounding square and,
//                     where the pixel centre lies in the disc, atomicMin the key (depth bits << 32 | slot).  Depth is a
//                     positive fp32, so its bits order as the float does; min does not depend on arrival order: the image is
//                     the same bits in every run, with no float atomic.  A plain load of the key goes first and the atomic is
//                     skipped when the fragment cannot win: the key only decreases, so a stale read costs one atomic that
//                     loses, never a winner.  In a dense fluid nearly every fragment is occluded.
//   k_render_resolve  one pixel per lane: the winner's slot -> its particle, the SAME sprite_of (same bits), the shading, and
//                     RGBA8 + creation index + depth.
//
// Everything of the rule is fp32 with each operation rounded (fp contract off), sums left to right, IEEE division and square
// root: tests/render_model.py is the same arithmetic in numpy and gives the same id and depth images bit for bit.
//
// The fluid as a surface (sph_surface_defaults, sph_render_surface, sph_render_surface_read): the same camera, sprites, walk and
// key image, and an image-space half behind them.
//
//   k_render_clear    as above; the thickness words are cleared by a memset node on the stream
//   k_surface_splat   the walk of k_render_splat; per covered pixel the SPHERE's depth d - R*sqrt(1 - mag) goes into the key, and
//                     (THICK) every fragment, occluded or not, adds its quantised chord to the pixel's 32-bit thickness word: an
//                     integer atomic add, so the plane does not depend on the order of arrival
//   k_surface_depth   one pixel per lane: the key's depth bits -> the raw depth plane Z_0 (+inf on background)
//   k_surface_filter  the hot kernel, K launches: a 32 x 8 tile of pixels per workgroup, the tile and its halo of r pixels staged
//                     in LDS (+inf outside the image), (2r+1)^2 taps per pixel in the header's order; ping-pong between rd_depth
//                     and rd_sf_pong, arranged so that Z_K lands in rd_depth and Z_0 stays readable
//   k_surface_shade   one pixel per lane: normals from Z_K and its four neighbours, the front particle's colour, the thickness,
//                     the shading; RGBA8 + creation index + normals
// tests/surface_model.py is its arithmetic in numpy; every plane is compared bit for bit.
//
// The solids (sph_render_set_solids): while a style is set and a drawn slot is installed, k_solid_march (sph_obstacle.hip, next
// to the sample rule it repeats) runs behind k_render_resolve and stores straight into the resolved planes; in a surface render
// it runs in front of k_surface_shade<true>, which composes, and k_solid_depth puts the winners' depth into Z_K afterwards.
// tests/solid_render_model.py is the arithmetic in numpy.
#include "sph_common.hpp"

#include <cmath>
#include <cstring>

namespace sph {

constexpr uint32_t RENDER_THREADS = 256;
constexpr uint64_t RENDER_EMPTY = ~0ull;

// the camera and the style of one call as the kernels take them: by value
struct RenderArgs {
    uint32_t width, height;
    float rot[9], trans[3];
    float focal, near_z, far_z;
    float radius;            // world units, resolved (style.radius or params.particle_radius)
    float half_w, half_h;    // 0.5f * width, 0.5f * height (exact)
    int32_t mode;
    float lo, span;          // SPEED / DENSITY: t = (value - lo) / span, span = hi - lo rounded to fp32
    float index_count;       // INDEX: t = (float)index / index_count
    uint32_t background;     // RGBA8, r in the low byte
};

struct Sprite {
    float cx, cy, rp, d;
    bool visible;
};

// The rule of include/sph_hip.h, used by the splat and by the resolve so that their bits agree.
__device__ __forceinline__ Sprite sprite_of(const RenderArgs& A, float x, float y, float z) {
#pragma clang fp contract(off)
    Sprite s;
    const float e0 = ((A.rot[0] * x + A.rot[1] * y) + A.rot[2] * z) + A.trans[0];
    const float e1 = ((A.rot[3] * x + A.rot[4] * y) + A.rot[5] * z) + A.trans[1];
    const float d = ((A.rot[6] * x + A.rot[7] * y) + A.rot[8] * z) + A.trans[2];
    s.d = d;
    s.visible = d >= A.near_z && d <= A.far_z;
    float rp = (A.radius * A.focal) / d;
    rp = fminf(rp, (float)SPH_RENDER_MAX_RADIUS_PX);
    rp = fmaxf(rp, 0.75f);
    s.rp = rp;
    s.cx = A.half_w + (A.focal * e0) / d;
    s.cy = A.half_h - (A.focal * e1) / d;
    return s;
}

__device__ __forceinline__ float sprite_mag(const Sprite& s, uint32_t i, uint32_t j, float& u, float& v) {
#pragma clang fp contract(off)
    u = (((float)i + 0.5f) - s.cx) / s.rp;
    v = (((float)j + 0.5f) - s.cy) / s.rp;
    return u * u + v * v;
}

__global__ __launch_bounds__(RENDER_THREADS) void k_render_clear(uint64_t* __restrict__ keys, uint32_t npix) {
    const uint32_t p = blockIdx.x * RENDER_THREADS + threadIdx.x;
    if (p < npix) keys[p] = RENDER_EMPTY;
}

// The walk: a superset of the covered pixels -- |(i + 0.5) - cx| <= rp up to rounding -- with one pixel of margin on either
// side (tests/render_model.py: walk_bounds, held against the whole image in tests/test_render_model_cpu.py); clamped to the
// image as floats, before the conversion (cx may be far outside): no pixel outside the image is ever addressed.  A tighter
// walk (a quarter of the pixel tests for the smallest sprites) was measured and is SLOWER in a dense scene: the pass is
// bound by the atomics on hot pixels, and lanes that arrive faster read staler words.
// false: nothing to walk (also for a NaN centre); else [i0, i1) x [j0, j1), within the image.
__device__ __forceinline__ bool sprite_walk(const RenderArgs& A, const Sprite& s, uint32_t& i0, uint32_t& i1, uint32_t& j0, uint32_t& j1) {
    const float wf = (float)A.width, hf = (float)A.height;
    const float x0 = fminf(fmaxf(floorf(s.cx - s.rp) - 1.0f, 0.0f), wf), x1 = fminf(fmaxf(ceilf(s.cx + s.rp) + 1.0f, 0.0f), wf);
    const float y0 = fminf(fmaxf(floorf(s.cy - s.rp) - 1.0f, 0.0f), hf), y1 = fminf(fmaxf(ceilf(s.cy + s.rp) + 1.0f, 0.0f), hf);
    if (!(x0 < x1 && y0 < y1)) return false;
    i0 = (uint32_t)x0; i1 = (uint32_t)x1; j0 = (uint32_t)y0; j1 = (uint32_t)y1;
    return true;
}

// COUNT: the measuring build (SPH_RENDER_STATS) also counts the covered fragments [0] and those that reached the atomic [1]
template <bool COUNT>
__global__ __launch_bounds__(RENDER_THREADS) void k_render_splat(const float4* __restrict__ posi, uint32_t n, RenderArgs A,
                                                                 uint64_t* __restrict__ keys,
                                                                 unsigned long long* __restrict__ counts) {
    const uint32_t slot = blockIdx.x * RENDER_THREADS + threadIdx.x;
    if (slot >= n) return;
    const float4 p = posi[slot];
    const Sprite s = sprite_of(A, p.x, p.y, p.z);
    if (!s.visible) return;
    uint32_t i0, i1, j0, j1;
    if (!sprite_walk(A, s, i0, i1, j0, j1)) return;
    const uint64_t key = ((uint64_t)__float_as_uint(s.d) << 32) | (uint64_t)slot;
    uint32_t covered = 0, sent = 0;
    for (uint32_t j = j0; j < j1; j++) {
        uint64_t* row = keys + (size_t)j * A.width;
        for (uint32_t i = i0; i < i1; i++) {
            float u, v;
            if (!(sprite_mag(s, i, j, u, v) <= 1.0f)) continue;
            if (COUNT) covered++;
#ifdef SPH_RENDER_FRESH_LOAD      // measuring builds only: the early-out reads past the caches (profiles/scripts/render_time.py)
            const uint64_t seen = __hip_atomic_load(row + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
            const uint64_t seen = row[i];
#endif
            if (key < seen) {
                __hip_atomic_fetch_min(row + i, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (COUNT) sent++;
            }
        }
    }
    if (COUNT) {
        atomicAdd(counts, (unsigned long long)covered);
        atomicAdd(counts + 1, (unsigned long long)sent);
    }
}

// the seven colours of the reference's colorRamp (SPH/particleSystem.cpp), rows of r, g, b
__device__ __forceinline__ void ramp(float t, float c[3]) {
#pragma clang fp contract(off)
    const float R[7][3] = {{1.0f, 0.0f, 0.0f}, {1.0f, 0.5f, 0.0f}, {1.0f, 1.0f, 0.0f}, {0.0f, 1.0f, 0.0f},
                           {0.0f, 1.0f, 1.0f}, {0.0f, 0.0f, 1.0f}, {1.0f, 0.0f, 1.0f}};
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    const float s = t * 6.0f;
    int i = (int)s;
    i = i < 5 ? i : 5;
    const float f = s - (float)i;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float a = R[0][k], b = R[1][k];
#pragma unroll
        for (int q = 1; q < 6; q++)
            if (i == q) { a = R[q][k]; b = R[q + 1][k]; }
        c[k] = a + f * (b - a);
    }
}

// the ramp's argument of the particle in `slot` under the style's colour mode
__device__ __forceinline__ float ramp_t(const RenderArgs& A, uint32_t slot, uint32_t index, const float4* __restrict__ velr,
                                        const float2* __restrict__ dp) {
#pragma clang fp contract(off)
    if (A.mode == SPH_COLOR_INDEX) return (float)index / A.index_count;
    if (A.mode == SPH_COLOR_SPEED) {
        const float4 w = velr[slot];
        return (sqrtf((w.x * w.x + w.y * w.y) + w.z * w.z) - A.lo) / A.span;
    }
    return (dp[slot].x - A.lo) / A.span;
}

__global__ __launch_bounds__(RENDER_THREADS) void k_render_resolve(const uint64_t* __restrict__ keys, const float4* __restrict__ posi,
                                                                   const float4* __restrict__ velr, const float2* __restrict__ dp,
                                                                   uint32_t n, RenderArgs A, uint32_t* __restrict__ rgba,
                                                                   uint32_t* __restrict__ id, float* __restrict__ depth) {
#pragma clang fp contract(off)
    const uint32_t pix = blockIdx.x * RENDER_THREADS + threadIdx.x;
    if (pix >= A.width * A.height) return;
    const uint64_t key = keys[pix];
    const uint32_t slot = (uint32_t)key;
    if (key == RENDER_EMPTY || slot >= n) {      // (slot >= n cannot happen: the splat only writes slots below n)
        rgba[pix] = A.background;
        id[pix] = 0xFFFFFFFFu;
        depth[pix] = __uint_as_float(0x7F800000u);
        return;
    }
    const float4 p = posi[slot];
    const Sprite s = sprite_of(A, p.x, p.y, p.z);
    float u, v;
    const float mag = sprite_mag(s, pix % A.width, pix / A.width, u, v);
    const float nz = sqrtf(1.0f - mag);
    const float diffuse = fmaxf(0.0f, (0.577f * u + 0.577f * (-v)) + 0.577f * nz);
    const uint32_t index = __float_as_uint(p.w);
    float c[3];
    ramp(ramp_t(A, slot, index, velr, dp), c);
    uint32_t out = 0xFF000000u;
#pragma unroll
    for (int k = 0; k < 3; k++) out |= (uint32_t)(fminf(c[k] * diffuse, 1.0f) * 255.0f + 0.5f) << (8 * k);
    rgba[pix] = out;
    id[pix] = index;
    depth[pix] = __uint_as_float((uint32_t)(key >> 32));
}

// ---- the surface (sph_render_surface) -----------------------------------------------------------------------------------------------

constexpr uint32_t SF_TX = 32, SF_TY = 8;             // the filter's tile of pixels: one workgroup of RENDER_THREADS lanes
constexpr uint32_t SF_MAX_R = SPH_SURFACE_MAX_RADIUS_PX;
constexpr uint32_t SF_TILE_MAX = (SF_TX + 2 * SF_MAX_R) * (SF_TY + 2 * SF_MAX_R);      // 64 x 40 floats = 10 KiB
static_assert(SF_TX * SF_TY == RENDER_THREADS, "one pixel per lane");

// the surface style of one call as the kernels take it: by value
struct SurfaceArgs {
    uint32_t r;
    float tau;
    float S[SF_MAX_R + 1];       // the filter's weights, from the host
    int32_t flat, thick;         // thick: the thickness pass ran
    float tint[3], absorb[3], L[3];
    float specular;
    float thick_unit;            // R * 0.125f: world thickness of one count
    float bg[3];                 // (float)background[k] / 255.0f
};

#define SF_INF __uint_as_float(0x7F800000u)
__device__ __forceinline__ bool sf_finite(float z) { return fabsf(z) < SF_INF; }

// MIN: the depth key; THICK: the thickness word.  One launch does both; the measuring build SPH_SURFACE_SPLIT_WALK launches
// them as two walks (profiles/scripts/surface_time.py).
template <bool MIN, bool THICK>
__global__ __launch_bounds__(RENDER_THREADS) void k_surface_splat(const float4* __restrict__ posi, uint32_t n, RenderArgs A,
                                                                  uint64_t* __restrict__ keys, uint32_t* __restrict__ thick) {
#pragma clang fp contract(off)
    const uint32_t slot = blockIdx.x * RENDER_THREADS + threadIdx.x;
    if (slot >= n) return;
    const float4 p = posi[slot];
    const Sprite s = sprite_of(A, p.x, p.y, p.z);
    if (!(s.d - A.radius >= A.near_z && s.d <= A.far_z)) return;      // (also a NaN depth)
    uint32_t i0, i1, j0, j1;
    if (!sprite_walk(A, s, i0, i1, j0, j1)) return;
    for (uint32_t j = j0; j < j1; j++) {
        const size_t row = (size_t)j * A.width;
        for (uint32_t i = i0; i < i1; i++) {
            float u, v;
            const float mag = sprite_mag(s, i, j, u, v);
            if (!(mag <= 1.0f)) continue;
            const float nz = sqrtf(1.0f - mag);
            if (THICK) {
                const uint32_t q = (uint32_t)(nz * 16.0f + 0.5f);
                if (q) __hip_atomic_fetch_add(thick + row + i, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (result unused: no return)
            }
            if (MIN) {
                const float dz = s.d - A.radius * nz;
                const uint64_t key = ((uint64_t)__float_as_uint(dz) << 32) | (uint64_t)slot;
                const uint64_t seen = keys[row + i];
                if (key < seen) __hip_atomic_fetch_min(keys + row + i, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// raw: Z_0.  also: a second copy where nothing is smoothed (Z_K = Z_0), else null
__global__ __launch_bounds__(RENDER_THREADS) void k_surface_depth(const uint64_t* __restrict__ keys, uint32_t npix,
                                                                  float* __restrict__ raw, float* __restrict__ also) {
    const uint32_t pix = blockIdx.x * RENDER_THREADS + threadIdx.x;
    if (pix >= npix) return;
    const uint64_t key = keys[pix];
    const float z = key == RENDER_EMPTY ? SF_INF : __uint_as_float((uint32_t)(key >> 32));
    raw[pix] = z;
    if (also) also[pix] = z;
}

// One iteration Z_{it-1} (src) -> Z_it (dst).  Lanes 0..31 of a wave hold one row of the tile and lanes 32..63 the next: every
// LDS read of a half wave is 32 consecutive floats, free of bank conflicts whatever r.  The weights come by value and are put in
// LDS once, so that |di| can index them.
__global__ __launch_bounds__(RENDER_THREADS) void k_surface_filter(const float* __restrict__ src, float* __restrict__ dst, uint32_t w,
                                                                   uint32_t h, SurfaceArgs F) {
#pragma clang fp contract(off)
    __shared__ float tile[SF_TILE_MAX];
    __shared__ float wS[SF_MAX_R + 1];
    const uint32_t r = F.r, tw = SF_TX + 2 * r, th = SF_TY + 2 * r;
    const uint32_t tid = threadIdx.y * SF_TX + threadIdx.x;
#pragma unroll
    for (uint32_t k = 0; k <= SF_MAX_R; k++)
        if (tid == k) wS[k] = F.S[k];
    const int x0 = (int)(blockIdx.x * SF_TX) - (int)r, y0 = (int)(blockIdx.y * SF_TY) - (int)r;
    for (uint32_t t = tid; t < tw * th; t += RENDER_THREADS) {          // tw * th <= SF_TILE_MAX because r <= SF_MAX_R
        const uint32_t ly = t / tw, lx = t - ly * tw;
        const int gx = x0 + (int)lx, gy = y0 + (int)ly;
        const bool in = gx >= 0 && gx < (int)w && gy >= 0 && gy < (int)h;
        tile[t] = in ? src[(size_t)gy * w + (uint32_t)gx] : SF_INF;
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * SF_TX + threadIdx.x, j = blockIdx.y * SF_TY + threadIdx.y;
    if (i >= w || j >= h) return;
    const float zc = tile[(threadIdx.y + r) * tw + threadIdx.x + r];
    float out = zc;                                                      // a background pixel stays background
    if (sf_finite(zc)) {
        float num = 0.0f, den = 0.0f;
        for (uint32_t dj = 0; dj <= 2 * r; dj++) {
            const float sj = wS[dj < r ? r - dj : dj - r];
            const float* row = tile + (threadIdx.y + dj) * tw + threadIdx.x;
            for (uint32_t di = 0; di <= 2 * r; di++) {
                const float zn = row[di];
                if (!sf_finite(zn)) continue;
                const float e = (zn - zc) / F.tau;
                const float q = 1.0f - e * e;
                if (q > 0.0f) {
                    const float wt = (wS[di < r ? r - di : di - r] * sj) * (q * q);
                    num = num + wt * zn;
                    den = den + wt;
                }
            }
        }
        out = num / den;
    }
    dst[(size_t)j * w + i] = out;
}

// P(i, j) of the header
__device__ __forceinline__ void eye_point(const RenderArgs& A, uint32_t i, uint32_t j, float z, float P[3]) {
#pragma clang fp contract(off)
    P[0] = ((((float)i + 0.5f) - A.half_w) * z) / A.focal;
    P[1] = ((A.half_h - ((float)j + 0.5f)) * z) / A.focal;
    P[2] = z;
}

// ddx / ddy of the header: Pf the forward neighbour's point (has_f: it is inside the image and surface), Pb the backward one's
__device__ __forceinline__ void slope(const float P[3], bool has_f, const float Pf[3], bool has_b, const float Pb[3], float d[3]) {
#pragma clang fp contract(off)
    float f[3], b[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { f[k] = Pf[k] - P[k]; b[k] = P[k] - Pb[k]; }
    const bool use_f = has_f && (!has_b || fabsf(f[2]) <= fabsf(b[2]));
#pragma unroll
    for (int k = 0; k < 3; k++) d[k] = use_f ? f[k] : b[k];          // (neither: the caller's default)
}

__device__ __forceinline__ float dot3(const float a[3], const float b[3]) {
#pragma clang fp contract(off)
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// SOLID (a solid style is set, sph_render_set_solids): the so_ planes hold every pixel's nearest solid hit (k_solid_march).  A
// pixel whose hit lies in front of the fluid, or that has no fluid, takes the solid's colour, id and normal (its depth follows
// in k_solid_depth: the neighbours' normals read Z here); a fluid pixel with a hit behind it shades over the solid's colour
// instead of the background's.  <false> is the kernel without solids, operation for operation.
template <bool SOLID>
__global__ __launch_bounds__(RENDER_THREADS) void k_surface_shade(const uint64_t* __restrict__ keys, const float* __restrict__ Z,
                                                                  const uint32_t* __restrict__ thick, const float4* __restrict__ posi,
                                                                  const float4* __restrict__ velr, const float2* __restrict__ dp,
                                                                  uint32_t n, RenderArgs A, SurfaceArgs F, uint32_t* __restrict__ rgba,
                                                                  uint32_t* __restrict__ id, float* __restrict__ normal, SolidLooks K,
                                                                  const float* __restrict__ so_depth, const uint32_t* __restrict__ so_slot,
                                                                  const float* __restrict__ so_normal) {
#pragma clang fp contract(off)
    const uint32_t pix = blockIdx.x * RENDER_THREADS + threadIdx.x;
    if (pix >= A.width * A.height) return;
    const uint64_t key = keys[pix];
    const uint32_t slot = (uint32_t)key;
    float behind[3] = {F.bg[0], F.bg[1], F.bg[2]};      // what shows through the fluid
    if constexpr (SOLID) {
        const float zs = so_depth[pix];
        if (sf_finite(zs)) {
            const uint32_t ss = so_slot[pix];
            const float ne[3] = {so_normal[3 * (size_t)pix], so_normal[3 * (size_t)pix + 1], so_normal[3 * (size_t)pix + 2]};
            solid_color(K, ss, ne, behind);
            if (key == RENDER_EMPTY || slot >= n || zs < Z[pix]) {
                rgba[pix] = solid_rgba(behind);
                id[pix] = SPH_RENDER_ID_SOLID + ss;
                normal[3 * (size_t)pix] = ne[0]; normal[3 * (size_t)pix + 1] = ne[1]; normal[3 * (size_t)pix + 2] = ne[2];
                return;
            }
        }
    }
    if (key == RENDER_EMPTY || slot >= n) {      // (slot >= n cannot happen: the splat only writes slots below n)
        rgba[pix] = A.background;
        id[pix] = 0xFFFFFFFFu;
        normal[3 * (size_t)pix] = 0.0f; normal[3 * (size_t)pix + 1] = 0.0f; normal[3 * (size_t)pix + 2] = 0.0f;
        return;
    }
    const uint32_t i = pix % A.width, j = pix / A.width;
    const float z = Z[pix];
    float P[3], Pf[3] = {0.0f, 0.0f, 0.0f}, Pb[3] = {0.0f, 0.0f, 0.0f}, ddx[3], ddy[3];
    eye_point(A, i, j, z, P);
    {   // ddx: forward is column i + 1
        const float zf = i + 1 < A.width ? Z[pix + 1] : SF_INF, zb = i > 0 ? Z[pix - 1] : SF_INF;
        const bool hf = sf_finite(zf), hb = sf_finite(zb);
        if (hf) eye_point(A, i + 1, j, zf, Pf);
        if (hb) eye_point(A, i - 1, j, zb, Pb);
        slope(P, hf, Pf, hb, Pb, ddx);
        if (!hf && !hb) { ddx[0] = z / A.focal; ddx[1] = 0.0f; ddx[2] = 0.0f; }
    }
    {   // ddy: forward is row j - 1 (+y in eye space)
        const float zf = j > 0 ? Z[pix - A.width] : SF_INF, zb = j + 1 < A.height ? Z[pix + A.width] : SF_INF;
        const bool hf = sf_finite(zf), hb = sf_finite(zb);
        if (hf) eye_point(A, i, j - 1, zf, Pf);
        if (hb) eye_point(A, i, j + 1, zb, Pb);
        slope(P, hf, Pf, hb, Pb, ddy);
        if (!hf && !hb) { ddy[0] = 0.0f; ddy[1] = z / A.focal; ddy[2] = 0.0f; }
    }
    float nv[3];
    nv[0] = ddy[1] * ddx[2] - ddy[2] * ddx[1];
    nv[1] = ddy[2] * ddx[0] - ddy[0] * ddx[2];
    nv[2] = ddy[0] * ddx[1] - ddy[1] * ddx[0];
    const float len2 = dot3(nv, nv);
    if (len2 > 0.0f && sf_finite(len2)) {
        const float len = sqrtf(len2);
#pragma unroll
        for (int k = 0; k < 3; k++) nv[k] = nv[k] / len;
    } else {
        nv[0] = 0.0f; nv[1] = 0.0f; nv[2] = -1.0f;
    }
    const float pl = sqrtf(dot3(P, P));
    float V[3], H[3];
#pragma unroll
    for (int k = 0; k < 3; k++) V[k] = (-P[k]) / pl;
    const float ndl = fmaxf(0.0f, dot3(nv, F.L));
#pragma unroll
    for (int k = 0; k < 3; k++) H[k] = F.L[k] + V[k];
    const float hl = sqrtf(dot3(H, H));
#pragma unroll
    for (int k = 0; k < 3; k++) H[k] = hl > 0.0f ? H[k] / hl : nv[k];
    float spec = fmaxf(0.0f, dot3(nv, H));
#pragma unroll
    for (int k = 0; k < 5; k++) spec = spec * spec;
    const float ndv = fminf(fmaxf(dot3(nv, V), 0.0f), 1.0f);
    const float m = 1.0f - ndv;
    const float fres = 0.02f + 0.98f * (((m * m) * (m * m)) * m);
    const float lit = 0.25f + 0.75f * ndl;
    const float4 p = posi[slot];
    const uint32_t index = __float_as_uint(p.w);
    float c[3] = {1.0f, 1.0f, 1.0f};
    if (!F.flat) ramp(ramp_t(A, slot, index, velr, dp), c);
    const float T = F.thick ? (float)thick[pix] * F.thick_unit : 0.0f;
    uint32_t out = 0xFF000000u;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float base = F.flat ? F.tint[k] : F.tint[k] * c[k];
        const float tr = F.thick ? 1.0f / (1.0f + F.absorb[k] * T) : 0.0f;
        const float body = (base * lit) * (1.0f - tr) + (SOLID ? behind[k] : F.bg[k]) * tr;
        const float o = (body * (1.0f - fres) + fres) + F.specular * spec;
        out |= (uint32_t)(fminf(fmaxf(o, 0.0f), 1.0f) * 255.0f + 0.5f) << (8 * k);
    }
    rgba[pix] = out;
    id[pix] = index;
#pragma unroll
    for (int k = 0; k < 3; k++) normal[3 * (size_t)pix + k] = nv[k];
}

// behind k_surface_shade<true>: the depth plane of the pixels the solid won (the shade's own test)
__global__ __launch_bounds__(RENDER_THREADS) void k_solid_depth(const uint64_t* __restrict__ keys, uint32_t n, uint32_t npix,
                                                                const float* __restrict__ so_depth, float* __restrict__ Z) {
    const uint32_t pix = blockIdx.x * RENDER_THREADS + threadIdx.x;
    if (pix >= npix) return;
    const float zs = so_depth[pix];
    if (!sf_finite(zs)) return;
    const uint64_t key = keys[pix];
    if (key == RENDER_EMPTY || (uint32_t)key >= n || zs < Z[pix]) Z[pix] = zs;
}

// the image and its surface planes leave the context's owner before the context does: another image size, a failed allocation
static void release_image(sph_ctx* c) {
    Buffers& m = c->mem;
    m.release(&c->rd_so_normal); m.release(&c->rd_so_slot); m.release(&c->rd_so_depth);
    m.release(&c->rd_sf_normal); m.release(&c->rd_sf_thick); m.release(&c->rd_sf_pong); m.release(&c->rd_sf_raw);
    m.release(&c->rd_depth); m.release(&c->rd_id); m.release(&c->rd_rgba); m.release(&c->rd_keys);
    c->rd_alloc_w = c->rd_alloc_h = 0;
    c->rd_valid = false;
}

static bool finite3(const float* v, int n) {
    for (int k = 0; k < n; k++) if (!std::isfinite(v[k])) return false;
    return true;
}

}  // namespace sph

using namespace sph;

extern "C" {

int sph_camera_look_at(sph_camera* out, uint32_t width, uint32_t height, const float eye[3], const float target[3],
                       const float up[3], float fovy_deg, float near_z, float far_z) {
    SPH_REQUIRE(out && eye && target && up, SPH_E_INVALID, "null argument");
    SPH_REQUIRE(width >= 1u && width <= (uint32_t)SPH_RENDER_MAX_SIZE && height >= 1u && height <= (uint32_t)SPH_RENDER_MAX_SIZE,
                SPH_E_INVALID, "image %u x %u: 1..%d each", width, height, SPH_RENDER_MAX_SIZE);
    SPH_REQUIRE(finite3(eye, 3) && finite3(target, 3) && finite3(up, 3) && std::isfinite(fovy_deg) && std::isfinite(near_z) &&
                std::isfinite(far_z), SPH_E_INVALID, "sph_camera_look_at: an argument is not finite");
    SPH_REQUIRE(fovy_deg > 0.f && fovy_deg < 180.f, SPH_E_INVALID, "fovy %g: between 0 and 180 degrees", (double)fovy_deg);
    SPH_REQUIRE(near_z > 0.f && far_z > near_z, SPH_E_INVALID, "0 < near_z < far_z");
    double f[3], r[3], u[3];
    for (int k = 0; k < 3; k++) f[k] = (double)target[k] - (double)eye[k];
    const double fl = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    SPH_REQUIRE(fl > 0.0 && std::isfinite(fl), SPH_E_INVALID, "sph_camera_look_at: eye and target coincide");
    for (int k = 0; k < 3; k++) f[k] /= fl;
    const double ul = std::sqrt((double)up[0] * up[0] + (double)up[1] * up[1] + (double)up[2] * up[2]);
    SPH_REQUIRE(ul > 0.0 && std::isfinite(ul), SPH_E_INVALID, "sph_camera_look_at: up has no direction");
    const double w[3] = {up[0] / ul, up[1] / ul, up[2] / ul};
    r[0] = f[1] * w[2] - f[2] * w[1];              // right = forward x up
    r[1] = f[2] * w[0] - f[0] * w[2];
    r[2] = f[0] * w[1] - f[1] * w[0];
    const double rl = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    SPH_REQUIRE(rl > 1e-12, SPH_E_INVALID, "sph_camera_look_at: up is parallel to the view direction");
    for (int k = 0; k < 3; k++) r[k] /= rl;
    u[0] = r[1] * f[2] - r[2] * f[1];              // the camera's up = right x forward
    u[1] = r[2] * f[0] - r[0] * f[2];
    u[2] = r[0] * f[1] - r[1] * f[0];
    const double* rows[3] = {r, u, f};             // eye space: +x right, +y up, +z forward
    sph_camera cam;
    cam.width = width;
    cam.height = height;
    for (int k = 0; k < 3; k++) {
        double t = 0.0;
        for (int a = 0; a < 3; a++) {
            cam.rot[3 * k + a] = (float)(rows[k][a] + 0.0);      // (+ 0.0: a -0 becomes +0)
            t += rows[k][a] * (double)eye[a];
        }
        cam.trans[k] = (float)(-t + 0.0);
    }
    const double kPi = 3.14159265358979323846;
    cam.focal_px = (float)(0.5 * (double)height / std::tan(0.5 * (double)fovy_deg * kPi / 180.0));
    cam.near_z = near_z;
    cam.far_z = far_z;
    SPH_REQUIRE(finite3(cam.rot, 9) && finite3(cam.trans, 3) && std::isfinite(cam.focal_px) && cam.focal_px > 0.f, SPH_E_INVALID,
                "sph_camera_look_at: the camera does not fit fp32");
    *out = cam;
    return SPH_OK;
}

// What sph_render and sph_render_surface check alike; `who` names the entry point in the messages.
static int check_render(sph_ctx* c, const sph_camera* cam, const sph_render_style* style, const char* who) {
    SPH_REQUIRE(c && cam && style, SPH_E_INVALID, "null argument");
    SPH_REQUIRE(!c->slab, SPH_E_STATE, "%s is not supported on a slab context (the ranks would have to composite "
                "their images)", who);
    SPH_REQUIRE(cam->width >= 1u && cam->width <= (uint32_t)SPH_RENDER_MAX_SIZE && cam->height >= 1u &&
                cam->height <= (uint32_t)SPH_RENDER_MAX_SIZE, SPH_E_INVALID, "image %u x %u: 1..%d each", cam->width, cam->height,
                SPH_RENDER_MAX_SIZE);
    SPH_REQUIRE(finite3(cam->rot, 9) && finite3(cam->trans, 3) && std::isfinite(cam->focal_px) && std::isfinite(cam->near_z) &&
                std::isfinite(cam->far_z), SPH_E_INVALID, "%s: a camera field is not finite", who);
    SPH_REQUIRE(cam->focal_px > 0.f, SPH_E_INVALID, "focal_px %g: must be positive", (double)cam->focal_px);
    SPH_REQUIRE(cam->near_z > 0.f && cam->far_z > cam->near_z, SPH_E_INVALID, "0 < near_z < far_z");
    SPH_REQUIRE(style->color_mode == SPH_COLOR_INDEX || style->color_mode == SPH_COLOR_SPEED || style->color_mode == SPH_COLOR_DENSITY,
                SPH_E_INVALID, "unknown colour mode %d", (int)style->color_mode);
    if (style->color_mode != SPH_COLOR_INDEX)
        SPH_REQUIRE(std::isfinite(style->lo) && std::isfinite(style->hi) && style->hi != style->lo &&
                    std::isfinite(style->hi - style->lo), SPH_E_INVALID, "colour range [%g, %g]: finite, and hi != lo",
                    (double)style->lo, (double)style->hi);
    SPH_REQUIRE(std::isfinite(style->radius) && style->radius >= 0.f, SPH_E_INVALID, "sprite radius %g: finite and >= 0 (0: the particle radius)",
                (double)style->radius);
    return SPH_OK;
}

// The image buffers for w x h: kept when they have that size, else (first call, or another image size) allocated anew.
static int ensure_image(sph_ctx* c, uint32_t w, uint32_t h) {
    if (w == c->rd_alloc_w && h == c->rd_alloc_h) return SPH_OK;
    const uint32_t npix = w * h;
    SPH_HIP(hipStreamSynchronize(c->stream));        // (a consumer of the old image on this stream has finished)
    release_image(c);
    int rc = c->mem.alloc(&c->rd_keys, npix, false);     // (every plane is written by the render before anything reads it)
    if (!rc) rc = c->mem.alloc(&c->rd_rgba, npix, false);
    if (!rc) rc = c->mem.alloc(&c->rd_id, npix, false);
    if (!rc) rc = c->mem.alloc(&c->rd_depth, npix, false);
    if (rc) { release_image(c); return rc; }
    c->rd_alloc_w = w;
    c->rd_alloc_h = h;
    return SPH_OK;
}

static RenderArgs render_args(const sph_ctx* c, const sph_camera* cam, const sph_render_style* style) {
    RenderArgs A;
    memset(&A, 0, sizeof(A));
    A.width = cam->width;
    A.height = cam->height;
    for (int k = 0; k < 9; k++) A.rot[k] = cam->rot[k];
    for (int k = 0; k < 3; k++) A.trans[k] = cam->trans[k];
    A.focal = cam->focal_px;
    A.near_z = cam->near_z;
    A.far_z = cam->far_z;
    A.radius = style->radius > 0.f ? style->radius : c->params.particle_radius;
    A.half_w = 0.5f * (float)cam->width;
    A.half_h = 0.5f * (float)cam->height;
    A.mode = style->color_mode;
    A.lo = style->lo;
    A.span = style->hi - style->lo;
    A.index_count = (float)(style->index_count ? style->index_count : c->n);
    memcpy(&A.background, style->background, 4);
    return A;
}

// the camera and the context's solid style as k_solid_march takes them
static SolidCam solid_cam(const RenderArgs& A) {
    SolidCam C;
    memset(&C, 0, sizeof(C));
    C.width = A.width;
    C.height = A.height;
    for (int k = 0; k < 9; k++) C.rot[k] = A.rot[k];
    for (int k = 0; k < 3; k++) C.trans[k] = A.trans[k];
    C.focal = A.focal;
    C.near_z = A.near_z;
    C.far_z = A.far_z;
    C.half_w = A.half_w;
    C.half_h = A.half_h;
    return C;
}

static SolidLooks solid_looks(const sph_ctx* c) {
    const sph_solid_style& s = c->rd_solid_style;
    SolidLooks K;
    memset(&K, 0, sizeof(K));
    const double ll = std::sqrt((double)s.light[0] * s.light[0] + (double)s.light[1] * s.light[1] + (double)s.light[2] * s.light[2]);
    for (int q = 0; q < SPH_MAX_OBSTACLES; q++) {
        K.open[q] = s.slot[q].open;
        for (int k = 0; k < 3; k++) K.color[q][k] = s.slot[q].color[k];
    }
    for (int k = 0; k < 3; k++) K.L[k] = (float)((double)s.light[k] / ll);
    K.ambient = s.ambient;
    return K;
}

int sph_render(sph_ctx* c, const sph_camera* cam, const sph_render_style* style) {
    if (int e = check_render(c, cam, style, "sph_render")) return e;
    SPH_HIP(hipSetDevice(c->device));
    const uint32_t w = cam->width, h = cam->height, npix = w * h;
    if (int e = ensure_image(c, w, h)) return e;
    const RenderArgs A = render_args(c, cam, style);
    const uint32_t pix_blocks = ceil_div(npix, RENDER_THREADS);
    hipLaunchKernelGGL(k_render_clear, dim3(pix_blocks), dim3(RENDER_THREADS), 0, c->stream, c->rd_keys, npix);
    if (c->n) {
#ifdef SPH_RENDER_STATS
        if (!c->rd_counts) {
            if (int e = c->mem.alloc(&c->rd_counts, 2, false)) return e;
            SPH_HIP(hipMemsetAsync(c->rd_counts, 0, 2 * sizeof(unsigned long long), c->stream));
        }
        hipLaunchKernelGGL(k_render_splat<true>, dim3(ceil_div(c->n, RENDER_THREADS)), dim3(RENDER_THREADS), 0, c->stream,
                           c->posi + c->own_off, c->n, A, c->rd_keys, c->rd_counts);
#else
        hipLaunchKernelGGL(k_render_splat<false>, dim3(ceil_div(c->n, RENDER_THREADS)), dim3(RENDER_THREADS), 0, c->stream,
                           c->posi + c->own_off, c->n, A, c->rd_keys, (unsigned long long*)nullptr);
#endif
    }
    hipLaunchKernelGGL(k_render_resolve, dim3(pix_blocks), dim3(RENDER_THREADS), 0, c->stream, c->rd_keys, c->posi + c->own_off,
                       c->velr + c->own_off, c->dp + c->own_off, c->n, A, c->rd_rgba, c->rd_id, c->rd_depth);
    SPH_HIP(hipGetLastError());
    if (solids_drawn(c))
        if (int e = launch_solid_march(c, solid_cam(A), solid_looks(c), c->rd_rgba, c->rd_id, c->rd_depth, nullptr, nullptr, nullptr))
            return e;
    c->rd_w = w;
    c->rd_h = h;
    c->rd_valid = true;
    c->rd_surface = false;
    return SPH_OK;
}

void sph_surface_defaults(sph_surface_style* s) {
    if (!s) return;
    memset(s, 0, sizeof *s);
    s->smooth_radius_px = 5;
    s->smooth_iterations = 2;
    s->depth_falloff = 0.0f;
    s->flat_color = 1;
    s->tint[0] = 0.25f; s->tint[1] = 0.55f; s->tint[2] = 0.95f;
    s->absorb[0] = 6.0f; s->absorb[1] = 2.0f; s->absorb[2] = 0.5f;
    s->light[0] = 1.0f; s->light[1] = 1.0f; s->light[2] = -1.0f;
    s->specular = 0.6f;
}

int sph_render_surface(sph_ctx* c, const sph_camera* cam, const sph_render_style* style, const sph_surface_style* sf) {
    if (int e = check_render(c, cam, style, "sph_render_surface")) return e;
    SPH_REQUIRE(sf, SPH_E_INVALID, "null argument");
    SPH_REQUIRE(sf->smooth_radius_px <= (uint32_t)SPH_SURFACE_MAX_RADIUS_PX, SPH_E_INVALID, "smooth_radius_px %u: 0..%d",
                sf->smooth_radius_px, SPH_SURFACE_MAX_RADIUS_PX);
    SPH_REQUIRE(sf->smooth_iterations <= (uint32_t)SPH_SURFACE_MAX_ITERATIONS, SPH_E_INVALID, "smooth_iterations %u: 0..%d",
                sf->smooth_iterations, SPH_SURFACE_MAX_ITERATIONS);
    SPH_REQUIRE(std::isfinite(sf->depth_falloff) && sf->depth_falloff >= 0.f, SPH_E_INVALID, "depth_falloff %g: finite and >= 0 "
                "(0: four sprite radii)", (double)sf->depth_falloff);
    for (int k = 0; k < 3; k++)
        SPH_REQUIRE(std::isfinite(sf->tint[k]) && sf->tint[k] >= 0.f && std::isfinite(sf->absorb[k]) && sf->absorb[k] >= 0.f,
                    SPH_E_INVALID, "tint / absorb channel %d: finite and >= 0", k);
    SPH_REQUIRE(std::isfinite(sf->specular) && sf->specular >= 0.f, SPH_E_INVALID, "specular %g: finite and >= 0", (double)sf->specular);
    const double ll = std::sqrt((double)sf->light[0] * sf->light[0] + (double)sf->light[1] * sf->light[1] +
                                (double)sf->light[2] * sf->light[2]);
    SPH_REQUIRE(finite3(sf->light, 3) && ll > 0.0, SPH_E_INVALID, "light: a finite vector that is not zero");
    SPH_REQUIRE(c->n < (1u << 28), SPH_E_CAPACITY, "sph_render_surface: %u particles: the thickness word holds fewer than 2^28", c->n);
    SPH_HIP(hipSetDevice(c->device));
    const uint32_t w = cam->width, h = cam->height, npix = w * h;
    if (int e = ensure_image(c, w, h)) return e;
    if (!c->rd_sf_raw) {                                  // the first surface render of an image of this size
        int rc = c->mem.alloc(&c->rd_sf_raw, npix, false);
        if (!rc) rc = c->mem.alloc(&c->rd_sf_pong, npix, false);
        if (!rc) rc = c->mem.alloc(&c->rd_sf_thick, npix, false);
        if (!rc) rc = c->mem.alloc(&c->rd_sf_normal, (size_t)npix * 3, false);
        if (rc) {
            SPH_HIP(hipStreamSynchronize(c->stream));
            release_image(c);
            return rc;
        }
    }
    const bool solids = solids_drawn(c);
    if (solids && !c->rd_so_depth) {                      // the first surface render with solids of an image of this size
        int rc = c->mem.alloc(&c->rd_so_depth, npix, false);
        if (!rc) rc = c->mem.alloc(&c->rd_so_slot, npix, false);
        if (!rc) rc = c->mem.alloc(&c->rd_so_normal, (size_t)npix * 3, false);
        if (rc) {
            SPH_HIP(hipStreamSynchronize(c->stream));
            release_image(c);
            return rc;
        }
    }
    const RenderArgs A = render_args(c, cam, style);
    SurfaceArgs F;
    memset(&F, 0, sizeof(F));
    const uint32_t K = sf->smooth_radius_px ? sf->smooth_iterations : 0;
    F.r = K ? sf->smooth_radius_px : 0;
    F.tau = sf->depth_falloff > 0.f ? sf->depth_falloff : 4.0f * A.radius;
    for (uint32_t k = 0; k <= F.r; k++) {
        const double sigma = 0.5 * (double)F.r;
        F.S[k] = (float)std::exp(-((double)k * (double)k) / (2.0 * sigma * sigma));
    }
    F.flat = sf->flat_color ? 1 : 0;
    F.thick = (sf->absorb[0] > 0.f || sf->absorb[1] > 0.f || sf->absorb[2] > 0.f) ? 1 : 0;
    for (int k = 0; k < 3; k++) {
        F.tint[k] = sf->tint[k];
        F.absorb[k] = sf->absorb[k];
        F.L[k] = (float)((double)sf->light[k] / ll);
        F.bg[k] = (float)style->background[k] / 255.0f;
    }
    F.specular = sf->specular;
    F.thick_unit = A.radius * 0.125f;
    const uint32_t pix_blocks = ceil_div(npix, RENDER_THREADS), part_blocks = ceil_div(c->n, RENDER_THREADS);
    hipLaunchKernelGGL(k_render_clear, dim3(pix_blocks), dim3(RENDER_THREADS), 0, c->stream, c->rd_keys, npix);
    if (F.thick) SPH_HIP(hipMemsetAsync(c->rd_sf_thick, 0, (size_t)npix * 4, c->stream));
    if (c->n) {
        const float4* posi = c->posi + c->own_off;
#ifdef SPH_SURFACE_SPLIT_WALK      // measuring builds only: the thickness in a walk of its own (profiles/scripts/surface_time.py)
        hipLaunchKernelGGL((k_surface_splat<true, false>), dim3(part_blocks), dim3(RENDER_THREADS), 0, c->stream, posi, c->n, A, c->rd_keys, c->rd_sf_thick);
        if (F.thick)
            hipLaunchKernelGGL((k_surface_splat<false, true>), dim3(part_blocks), dim3(RENDER_THREADS), 0, c->stream, posi, c->n, A, c->rd_keys, c->rd_sf_thick);
#else
        if (F.thick)
            hipLaunchKernelGGL((k_surface_splat<true, true>), dim3(part_blocks), dim3(RENDER_THREADS), 0, c->stream, posi, c->n, A, c->rd_keys, c->rd_sf_thick);
        else
            hipLaunchKernelGGL((k_surface_splat<true, false>), dim3(part_blocks), dim3(RENDER_THREADS), 0, c->stream, posi, c->n, A, c->rd_keys, c->rd_sf_thick);
#endif
    }
    hipLaunchKernelGGL(k_surface_depth, dim3(pix_blocks), dim3(RENDER_THREADS), 0, c->stream, c->rd_keys, npix, c->rd_sf_raw,
                       K ? (float*)nullptr : c->rd_depth);
    // Z_0 = rd_sf_raw stays; the iterations alternate between rd_depth and rd_sf_pong so that the last one writes rd_depth
    const float* src = c->rd_sf_raw;
    for (uint32_t it = 1; it <= K; it++) {
        float* dst = (K - it) % 2 == 0 ? c->rd_depth : c->rd_sf_pong;
        hipLaunchKernelGGL(k_surface_filter, dim3(ceil_div(w, SF_TX), ceil_div(h, SF_TY)), dim3(SF_TX, SF_TY), 0, c->stream, src, dst, w, h, F);
        src = dst;
    }
    if (solids) {
        const SolidLooks K = solid_looks(c);
        if (int e = launch_solid_march(c, solid_cam(A), K, nullptr, nullptr, nullptr, c->rd_so_depth, c->rd_so_slot, c->rd_so_normal))
            return e;
        hipLaunchKernelGGL(k_surface_shade<true>, dim3(pix_blocks), dim3(RENDER_THREADS), 0, c->stream, c->rd_keys, c->rd_depth,
                           c->rd_sf_thick, c->posi + c->own_off, c->velr + c->own_off, c->dp + c->own_off, c->n, A, F, c->rd_rgba,
                           c->rd_id, c->rd_sf_normal, K, c->rd_so_depth, c->rd_so_slot, c->rd_so_normal);
        hipLaunchKernelGGL(k_solid_depth, dim3(pix_blocks), dim3(RENDER_THREADS), 0, c->stream, c->rd_keys, c->n, npix, c->rd_so_depth,
                           c->rd_depth);
    } else {
        hipLaunchKernelGGL(k_surface_shade<false>, dim3(pix_blocks), dim3(RENDER_THREADS), 0, c->stream, c->rd_keys, c->rd_depth,
                           c->rd_sf_thick, c->posi + c->own_off, c->velr + c->own_off, c->dp + c->own_off, c->n, A, F, c->rd_rgba,
                           c->rd_id, c->rd_sf_normal, SolidLooks{}, (const float*)nullptr, (const uint32_t*)nullptr,
                           (const float*)nullptr);
    }
    SPH_HIP(hipGetLastError());
    c->rd_w = w;
    c->rd_h = h;
    c->rd_valid = true;
    c->rd_surface = true;
    c->rd_sf_thick_on = F.thick != 0;
    return SPH_OK;
}

void sph_solid_defaults(sph_solid_style* s) {
    if (!s) return;
    memset(s, 0, sizeof *s);
    for (int q = 0; q < SPH_MAX_OBSTACLES; q++) {
        s->slot[q].draw = 1;
        s->slot[q].open = 0;
        s->slot[q].color[0] = 0.72f; s->slot[q].color[1] = 0.72f; s->slot[q].color[2] = 0.75f;
    }
    s->light[0] = 1.0f; s->light[1] = 1.0f; s->light[2] = -1.0f;
    s->ambient = 0.25f;
}

int sph_render_set_solids(sph_ctx* c, const sph_solid_style* s) {
    SPH_REQUIRE(c, SPH_E_INVALID, "null context");
    SPH_REQUIRE(!c->slab, SPH_E_STATE, "sph_render_set_solids is not supported on a slab context (it does not render)");
    if (!s) {
        c->rd_solids = false;
        return SPH_OK;
    }
    for (int q = 0; q < SPH_MAX_OBSTACLES; q++)
        for (int k = 0; k < 3; k++)
            SPH_REQUIRE(std::isfinite(s->slot[q].color[k]) && s->slot[q].color[k] >= 0.f && s->slot[q].color[k] <= 1.f, SPH_E_INVALID,
                        "solid style: slot %d colour channel %d: finite and in [0, 1]", q, k);
    SPH_REQUIRE(std::isfinite(s->ambient) && s->ambient >= 0.f && s->ambient <= 1.f, SPH_E_INVALID, "solid style: ambient %g: finite "
                "and in [0, 1]", (double)s->ambient);
    const double ll = std::sqrt((double)s->light[0] * s->light[0] + (double)s->light[1] * s->light[1] +
                                (double)s->light[2] * s->light[2]);
    SPH_REQUIRE(finite3(s->light, 3) && ll > 0.0, SPH_E_INVALID, "solid style: light: a finite vector that is not zero");
    SPH_REQUIRE(c->cap < SPH_RENDER_ID_SOLID, SPH_E_CAPACITY, "sph_render_set_solids: capacity %u: the id plane keeps the ids from "
                "0x%X for the solids", c->cap, SPH_RENDER_ID_SOLID);
    c->rd_solid_style = *s;
    c->rd_solids = true;
    return SPH_OK;
}

int sph_render_get_solids(const sph_ctx* c, int* on, sph_solid_style* out) {
    SPH_REQUIRE(c, SPH_E_INVALID, "null context");
    if (on) *on = c->rd_solids ? 1 : 0;
    if (out && c->rd_solids) *out = c->rd_solid_style;
    return SPH_OK;
}

int sph_render_surface_read(sph_ctx* c, float* raw_depth, uint32_t* thickness_q, float* normal_xyz) {
    SPH_REQUIRE(c, SPH_E_INVALID, "null context");
    SPH_REQUIRE(c->rd_valid && c->rd_surface, SPH_E_STATE, "sph_render_surface_read: the last render was not a surface render");
    SPH_HIP(hipSetDevice(c->device));
    const size_t npix = (size_t)c->rd_w * c->rd_h;
    if (raw_depth) SPH_HIP(hipMemcpyAsync(raw_depth, c->rd_sf_raw, npix * 4, hipMemcpyDeviceToHost, c->stream));
    if (thickness_q) {
        if (c->rd_sf_thick_on) SPH_HIP(hipMemcpyAsync(thickness_q, c->rd_sf_thick, npix * 4, hipMemcpyDeviceToHost, c->stream));
        else memset(thickness_q, 0, npix * 4);
    }
    if (normal_xyz) SPH_HIP(hipMemcpyAsync(normal_xyz, c->rd_sf_normal, npix * 12, hipMemcpyDeviceToHost, c->stream));
    SPH_HIP(hipStreamSynchronize(c->stream));
    return SPH_OK;
}

int sph_render_read(sph_ctx* c, uint8_t* rgba, uint32_t* id, float* depth) {
    SPH_REQUIRE(c, SPH_E_INVALID, "null context");
    SPH_REQUIRE(c->rd_valid, SPH_E_STATE, "sph_render_read: nothing was rendered yet");
    SPH_HIP(hipSetDevice(c->device));
    const size_t npix = (size_t)c->rd_w * c->rd_h;
    if (rgba) SPH_HIP(hipMemcpyAsync(rgba, c->rd_rgba, npix * 4, hipMemcpyDeviceToHost, c->stream));
    if (id) SPH_HIP(hipMemcpyAsync(id, c->rd_id, npix * 4, hipMemcpyDeviceToHost, c->stream));
    if (depth) SPH_HIP(hipMemcpyAsync(depth, c->rd_depth, npix * 4, hipMemcpyDeviceToHost, c->stream));
    SPH_HIP(hipStreamSynchronize(c->stream));
    return SPH_OK;
}

int sph_render_image_dev(sph_ctx* c, void** rgba_dev, uint32_t* width, uint32_t* height) {
    SPH_REQUIRE(c && rgba_dev, SPH_E_INVALID, "null argument");
    SPH_REQUIRE(c->rd_valid, SPH_E_STATE, "sph_render_image_dev: nothing was rendered yet");
    *rgba_dev = c->rd_rgba;
    if (width) *width = c->rd_w;
    if (height) *height = c->rd_h;
    return SPH_OK;
}

#ifdef SPH_RENDER_STATS
// measuring build only (profiles/scripts/render_time.py): covered fragments and those that reached the atomic, summed over
// the renders since the last call; synchronises
int sph_render_stats(sph_ctx* c, uint64_t out[2]) {
    SPH_REQUIRE(c && out, SPH_E_INVALID, "null argument");
    out[0] = out[1] = 0;
    if (!c->rd_counts) return SPH_OK;
    unsigned long long h[2];
    SPH_HIP(hipMemcpyAsync(h, c->rd_counts, sizeof h, hipMemcpyDeviceToHost, c->stream));
    SPH_HIP(hipMemsetAsync(c->rd_counts, 0, sizeof h, c->stream));
    SPH_HIP(hipStreamSynchronize(c->stream));
    out[0] = h[0];
    out[1] = h[1];
    return SPH_OK;
}
#endif

}  // extern "C"

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
    // The walk: a superset of the covered pixels -- |(i + 0.5) - cx| <= rp up to rounding -- with one pixel of margin on either
    // side (tests/render_model.py: walk_bounds, held against the whole image in tests/test_render_model_cpu.py); clamped to the
    // image as floats, before the conversion (cx may be far outside): no pixel outside the image is ever addressed.  A tighter
    // walk (a quarter of the pixel tests for the smallest sprites) was measured and is SLOWER in a dense scene: the pass is
    // bound by the atomics on hot pixels, and lanes that arrive faster read staler words.
    const float wf = (float)A.width, hf = (float)A.height;
    const float x0 = fminf(fmaxf(floorf(s.cx - s.rp) - 1.0f, 0.0f), wf), x1 = fminf(fmaxf(ceilf(s.cx + s.rp) + 1.0f, 0.0f), wf);
    const float y0 = fminf(fmaxf(floorf(s.cy - s.rp) - 1.0f, 0.0f), hf), y1 = fminf(fmaxf(ceilf(s.cy + s.rp) + 1.0f, 0.0f), hf);
    if (!(x0 < x1 && y0 < y1)) return;            // (also a NaN centre: nothing to draw)
    const uint32_t i0 = (uint32_t)x0, i1 = (uint32_t)x1, j0 = (uint32_t)y0, j1 = (uint32_t)y1;   // [i0, i1) x [j0, j1), within the image
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
    float t;
    if (A.mode == SPH_COLOR_INDEX) {
        t = (float)index / A.index_count;
    } else if (A.mode == SPH_COLOR_SPEED) {
        const float4 w = velr[slot];
        t = (sqrtf((w.x * w.x + w.y * w.y) + w.z * w.z) - A.lo) / A.span;
    } else {
        t = (dp[slot].x - A.lo) / A.span;
    }
    float c[3];
    ramp(t, c);
    uint32_t out = 0xFF000000u;
#pragma unroll
    for (int k = 0; k < 3; k++) out |= (uint32_t)(fminf(c[k] * diffuse, 1.0f) * 255.0f + 0.5f) << (8 * k);
    rgba[pix] = out;
    id[pix] = index;
    depth[pix] = __uint_as_float((uint32_t)(key >> 32));
}

static void free_image(sph_ctx* c) {
    hipFree(c->rd_keys); hipFree(c->rd_rgba); hipFree(c->rd_id); hipFree(c->rd_depth);
    c->rd_keys = nullptr; c->rd_rgba = nullptr; c->rd_id = nullptr; c->rd_depth = nullptr;
    c->rd_alloc_w = c->rd_alloc_h = 0;
}

void render_release(sph_ctx* c) {
    free_image(c);
    hipFree(c->rd_counts);
    c->rd_counts = nullptr;
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

int sph_render(sph_ctx* c, const sph_camera* cam, const sph_render_style* style) {
    SPH_REQUIRE(c && cam && style, SPH_E_INVALID, "null argument");
    SPH_REQUIRE(!c->slab, SPH_E_STATE, "sph_render is not supported on a slab context (the ranks would have to composite "
                "their images)");
    SPH_REQUIRE(cam->width >= 1u && cam->width <= (uint32_t)SPH_RENDER_MAX_SIZE && cam->height >= 1u &&
                cam->height <= (uint32_t)SPH_RENDER_MAX_SIZE, SPH_E_INVALID, "image %u x %u: 1..%d each", cam->width, cam->height,
                SPH_RENDER_MAX_SIZE);
    SPH_REQUIRE(finite3(cam->rot, 9) && finite3(cam->trans, 3) && std::isfinite(cam->focal_px) && std::isfinite(cam->near_z) &&
                std::isfinite(cam->far_z), SPH_E_INVALID, "sph_render: a camera field is not finite");
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
    SPH_HIP(hipSetDevice(c->device));
    const uint32_t w = cam->width, h = cam->height, npix = w * h;
    if (w != c->rd_alloc_w || h != c->rd_alloc_h) {      // first call, or another image size
        SPH_HIP(hipStreamSynchronize(c->stream));        // (a consumer of the old image on this stream has finished)
        free_image(c);
        c->rd_valid = false;
        hipError_t e = hipMalloc((void**)&c->rd_keys, (size_t)npix * 8);
        if (e == hipSuccess) e = hipMalloc((void**)&c->rd_rgba, (size_t)npix * 4);
        if (e == hipSuccess) e = hipMalloc((void**)&c->rd_id, (size_t)npix * 4);
        if (e == hipSuccess) e = hipMalloc((void**)&c->rd_depth, (size_t)npix * 4);
        if (e != hipSuccess) {
            free_image(c);
            set_error("sph_render: hipMalloc of a %u x %u image failed: %s", w, h, hipGetErrorString(e));
            return SPH_E_NOMEM;
        }
        c->rd_alloc_w = w;
        c->rd_alloc_h = h;
    }
    RenderArgs A;
    memset(&A, 0, sizeof(A));
    A.width = w;
    A.height = h;
    for (int k = 0; k < 9; k++) A.rot[k] = cam->rot[k];
    for (int k = 0; k < 3; k++) A.trans[k] = cam->trans[k];
    A.focal = cam->focal_px;
    A.near_z = cam->near_z;
    A.far_z = cam->far_z;
    A.radius = style->radius > 0.f ? style->radius : c->params.particle_radius;
    A.half_w = 0.5f * (float)w;
    A.half_h = 0.5f * (float)h;
    A.mode = style->color_mode;
    A.lo = style->lo;
    A.span = style->hi - style->lo;
    A.index_count = (float)(style->index_count ? style->index_count : c->n);
    memcpy(&A.background, style->background, 4);
    const uint32_t pix_blocks = ceil_div(npix, RENDER_THREADS);
    hipLaunchKernelGGL(k_render_clear, dim3(pix_blocks), dim3(RENDER_THREADS), 0, c->stream, c->rd_keys, npix);
    if (c->n) {
#ifdef SPH_RENDER_STATS
        if (!c->rd_counts) {
            SPH_HIP(hipMalloc((void**)&c->rd_counts, 2 * sizeof(unsigned long long)));
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
    c->rd_w = w;
    c->rd_h = h;
    c->rd_valid = true;
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

"""numpy float32 model of the device renderer of include/sph_hip.h (sph_render): every operation rounded to fp32, no
multiply-add fusion, sums left to right, IEEE division and square root -- the arithmetic of sprite_of / sprite_mag /
k_render_resolve in csrc/sph_render.hip, so that model and device give the same id and depth images bit for bit.

The particles are given IN SLOT ORDER (what sph_download_owned returns): the slot breaks ties of equal depth.  The camera is
anything with the fields of `sph_camera` (capi.Camera, or camera(...) below)."""
from types import SimpleNamespace

import numpy as np

f32 = np.float32
MAX_RADIUS_PX = f32(64.0)          # SPH_RENDER_MAX_RADIUS_PX
MIN_RADIUS_PX = f32(0.75)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_ID = np.uint32(0xFFFFFFFF)
MODES = {"index": 0, "speed": 1, "density": 2}
RAMP = np.array([[1, 0, 0], [1, 0.5, 0], [1, 1, 0], [0, 1, 0], [0, 1, 1], [0, 0, 1], [1, 0, 1]], dtype=f32)
_SMALL = 24                        # windows up to this edge go through the vectorised walk


def camera(width, height, rot, trans, focal_px, near_z, far_z):
    return SimpleNamespace(width=int(width), height=int(height), rot=[float(v) for v in rot], trans=[float(v) for v in trans],
                           focal_px=float(focal_px), near_z=float(near_z), far_z=float(far_z))


def _cam(cam):
    return (int(cam.width), int(cam.height), np.array(list(cam.rot), dtype=f32), np.array(list(cam.trans), dtype=f32),
            f32(cam.focal_px), f32(cam.near_z), f32(cam.far_z))


def sprites(pos, cam, radius):
    """(cx, cy, rp, d, visible) per particle: the projection of include/sph_hip.h."""
    w, h, rot, trans, focal, near, far = _cam(cam)
    pos = np.asarray(pos, dtype=f32).reshape(-1, 3)
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    pe = [((rot[3 * k] * x + rot[3 * k + 1] * y) + rot[3 * k + 2] * z) + trans[k] for k in range(3)]
    d = pe[2]
    visible = (d >= near) & (d <= far)
    with np.errstate(all="ignore"):
        rp = (f32(radius) * focal) / d
        rp = np.maximum(np.minimum(rp, MAX_RADIUS_PX), MIN_RADIUS_PX)
        cx = f32(0.5) * f32(w) + (focal * pe[0]) / d
        cy = f32(0.5) * f32(h) - (focal * pe[1]) / d
    return cx.astype(f32), cy.astype(f32), rp.astype(f32), d.astype(f32), visible


def mag_of(cx, cy, rp, i, j):
    """(u, v, mag) of pixel (column i, row j) in the sprite (cx, cy, rp); arrays of one shape."""
    u = ((np.asarray(i).astype(f32) + f32(0.5)) - cx) / rp
    v = ((np.asarray(j).astype(f32) + f32(0.5)) - cy) / rp
    return u, v, u * u + v * v


def ramp(t):
    """The seven-colour ramp: t (n,) -> c (n, 3) float32."""
    t = np.minimum(np.maximum(np.asarray(t, dtype=f32), f32(0.0)), f32(1.0))
    s = t * f32(6.0)
    i = np.minimum(s.astype(np.int32), 5)
    f = s - i.astype(f32)
    a, b = RAMP[i], RAMP[i + 1]
    return a + f[:, None] * (b - a)


def walk_bounds(cx, cy, rp, w, h):
    """The pixel ranges [i0, i1) x [j0, j1) the device's splat walks for a sprite: k_render_splat's fp32 expressions.  A
    superset of the covered pixels inside the image (tests/test_render_model_cpu.py), empty for a sprite off the image."""
    def lo(c, size):
        with np.errstate(all="ignore"):
            v = np.floor(c - rp) - f32(1.0)
        return np.nan_to_num(np.minimum(np.maximum(v, f32(0.0)), f32(size)), nan=0.0).astype(np.int64)

    def hi(c, size):
        with np.errstate(all="ignore"):
            v = np.ceil(c + rp) + f32(1.0)
        return np.nan_to_num(np.minimum(np.maximum(v, f32(0.0)), f32(size)), nan=0.0).astype(np.int64)
    cx, cy, rp = (np.atleast_1d(np.asarray(a, dtype=f32)) for a in (cx, cy, rp))
    return lo(cx, w), hi(cx, w), lo(cy, h), hi(cy, h)


def depth_keys(pos, cam, radius):
    """The per-pixel 64-bit keys (depth bits << 32 | slot), EMPTY where nothing is drawn: what the splat leaves behind."""
    w, h = int(cam.width), int(cam.height)
    cx, cy, rp, d, visible = sprites(pos, cam, radius)
    keys = np.full(w * h, EMPTY, dtype=np.uint64)
    i0, i1, j0, j1 = walk_bounds(cx, cy, rp, w, h)
    slots = np.nonzero(visible)[0]
    i0, i1, j0, j1 = i0[slots], i1[slots], j0[slots], j1[slots]
    on = (i0 < i1) & (j0 < j1)
    slots, i0, i1, j0, j1 = slots[on], i0[on], i1[on], j0[on], j1[on]
    key = (d[slots].view(np.uint32).astype(np.uint64) << np.uint64(32)) | slots.astype(np.uint64)
    small = ((i1 - i0) <= _SMALL) & ((j1 - j0) <= _SMALL)
    # small windows: one vectorised pass over the particles per window offset
    s = np.nonzero(small)[0]
    if s.size:
        a, ky = slots[s], key[s]
        for dj in range(int((j1[s] - j0[s]).max())):
            for di in range(int((i1[s] - i0[s]).max())):
                i, j = i0[s] + di, j0[s] + dj
                m = (i < i1[s]) & (j < j1[s])
                if not m.any():
                    continue
                _, _, mag = mag_of(cx[a[m]], cy[a[m]], rp[a[m]], i[m], j[m])
                c = mag <= f32(1.0)
                np.minimum.at(keys, (j[m] * w + i[m])[c], ky[m][c])
    # large windows: one particle at a time
    for q in np.nonzero(~small)[0]:
        p = slots[q]
        jj, ii = np.meshgrid(np.arange(j0[q], j1[q]), np.arange(i0[q], i1[q]), indexing="ij")
        _, _, mag = mag_of(cx[p], cy[p], rp[p], ii, jj)
        c = mag <= f32(1.0)
        pix = (jj * w + ii)[c]
        keys[pix] = np.minimum(keys[pix], key[q])
    return keys


def render(pos, cam, vel=None, index=None, density=None, color="index", lo=0.0, hi=1.0, radius=1.0 / 64.0, index_count=None,
           background=(0, 0, 0, 255)):
    """(rgba[h, w, 4] uint8, id[h, w] uint32, depth[h, w] float32) of the particles `pos` (n, 3) in slot order."""
    w, h = int(cam.width), int(cam.height)
    pos = np.asarray(pos, dtype=f32).reshape(-1, 3)
    n = pos.shape[0]
    index = np.arange(n, dtype=np.uint32) if index is None else np.asarray(index, dtype=np.uint32)
    keys = depth_keys(pos, cam, radius)
    rgba = np.empty((w * h, 4), dtype=np.uint8)
    rgba[:] = np.asarray(background, dtype=np.uint8)
    ident = np.full(w * h, NO_ID, dtype=np.uint32)
    depth = np.full(w * h, np.inf, dtype=f32)
    pix = np.nonzero(keys != EMPTY)[0]
    if pix.size:
        slot = (keys[pix] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        cx, cy, rp, d, _ = sprites(pos[slot], cam, radius)
        u, v, mag = mag_of(cx, cy, rp, pix % w, pix // w)
        nz = np.sqrt(f32(1.0) - mag)
        diffuse = np.maximum(f32(0.0), (f32(0.577) * u + f32(0.577) * (-v)) + f32(0.577) * nz)
        mode = MODES[color]
        if mode == 0:
            t = index[slot].astype(f32) / f32(n if not index_count else index_count)
        elif mode == 1:
            vv = np.asarray(vel, dtype=f32).reshape(-1, 3)[slot]
            speed = np.sqrt((vv[:, 0] * vv[:, 0] + vv[:, 1] * vv[:, 1]) + vv[:, 2] * vv[:, 2])
            t = (speed - f32(lo)) / (f32(hi) - f32(lo))
        else:
            t = (np.asarray(density, dtype=f32)[slot] - f32(lo)) / (f32(hi) - f32(lo))
        c = ramp(t)
        rgba[pix, :3] = (np.minimum(c * diffuse[:, None], f32(1.0)) * f32(255.0) + f32(0.5)).astype(np.uint8)
        rgba[pix, 3] = 255
        ident[pix] = index[slot]
        depth[pix] = (keys[pix] >> np.uint64(32)).astype(np.uint32).view(f32)
    return rgba.reshape(h, w, 4), ident.reshape(h, w), depth.reshape(h, w)

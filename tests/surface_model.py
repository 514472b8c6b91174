"""numpy float32 model of the surface renderer of include/sph_hip.h (sph_render_surface): every operation rounded to fp32, no
multiply-add fusion, sums left to right, IEEE division and square root -- the arithmetic of k_surface_splat / k_surface_filter /
k_surface_shade in csrc/sph_render.hip, so that model and device give every plane bit for bit.  Sprites, walk bounds and the
colour ramp are render_model's: the projection is sph_render's.

The particles are given IN SLOT ORDER (what sph_download_owned returns): the slot breaks ties of equal depth."""
import math
from types import SimpleNamespace

import numpy as np

import render_model as rm

f32 = np.float32
INF = f32(np.inf)
MAX_RADIUS_PX, MAX_ITERATIONS = 16, 8          # SPH_SURFACE_MAX_RADIUS_PX, SPH_SURFACE_MAX_ITERATIONS
_SMALL = 24


def surface_style(smooth_radius_px=5, smooth_iterations=2, depth_falloff=0.0, flat_color=1, tint=(0.25, 0.55, 0.95),
                  absorb=(6.0, 2.0, 0.5), light=(1.0, 1.0, -1.0), specular=0.6):
    """The fields of `sph_surface_style`, defaults of sph_surface_defaults."""
    return SimpleNamespace(smooth_radius_px=int(smooth_radius_px), smooth_iterations=int(smooth_iterations),
                           depth_falloff=float(depth_falloff), flat_color=int(flat_color), tint=[float(v) for v in tint],
                           absorb=[float(v) for v in absorb], light=[float(v) for v in light], specular=float(specular))


def fragments(pos, cam, radius):
    """Every covered fragment of every drawn particle, in no particular order: (pixel index, slot, mag) arrays."""
    w, h = int(cam.width), int(cam.height)
    R = f32(radius)
    cx, cy, rp, d, _ = rm.sprites(pos, cam, radius)
    with np.errstate(all="ignore"):
        drawn = ((d - R) >= f32(cam.near_z)) & (d <= f32(cam.far_z))
    i0, i1, j0, j1 = rm.walk_bounds(cx, cy, rp, w, h)
    slots = np.nonzero(drawn)[0]
    i0, i1, j0, j1 = i0[slots], i1[slots], j0[slots], j1[slots]
    on = (i0 < i1) & (j0 < j1)
    slots, i0, i1, j0, j1 = slots[on], i0[on], i1[on], j0[on], j1[on]
    out_p, out_s, out_m = [], [], []
    small = ((i1 - i0) <= _SMALL) & ((j1 - j0) <= _SMALL)
    s = np.nonzero(small)[0]
    if s.size:
        a = slots[s]
        for dj in range(int((j1[s] - j0[s]).max())):
            for di in range(int((i1[s] - i0[s]).max())):
                i, j = i0[s] + di, j0[s] + dj
                m = (i < i1[s]) & (j < j1[s])
                if not m.any():
                    continue
                _, _, mag = rm.mag_of(cx[a[m]], cy[a[m]], rp[a[m]], i[m], j[m])
                c = mag <= f32(1.0)
                out_p.append((j[m] * w + i[m])[c]); out_s.append(a[m][c]); out_m.append(mag[c])
    for q in np.nonzero(~small)[0]:
        p = slots[q]
        jj, ii = np.meshgrid(np.arange(j0[q], j1[q]), np.arange(i0[q], i1[q]), indexing="ij")
        _, _, mag = rm.mag_of(cx[p], cy[p], rp[p], ii, jj)
        c = mag <= f32(1.0)
        out_p.append((jj * w + ii)[c]); out_s.append(np.full(int(c.sum()), p, dtype=np.int64)); out_m.append(mag[c])
    if not out_p:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, f32), d
    return np.concatenate(out_p).astype(np.int64), np.concatenate(out_s).astype(np.int64), np.concatenate(out_m).astype(f32), d


def splat(pos, cam, radius):
    """(keys[w*h] uint64: bits(dz) << 32 | slot, EMPTY on background; thickness counts[w*h] uint32)"""
    w, h = int(cam.width), int(cam.height)
    pix, slot, mag, d = fragments(pos, cam, radius)
    keys = np.full(w * h, rm.EMPTY, dtype=np.uint64)
    thick = np.zeros(w * h, dtype=np.uint32)
    if pix.size:
        nz = np.sqrt(f32(1.0) - mag)
        dz = (d[slot] - f32(radius) * nz).astype(f32)
        key = (dz.view(np.uint32).astype(np.uint64) << np.uint64(32)) | slot.astype(np.uint64)
        np.minimum.at(keys, pix, key)
        q = (nz * f32(16.0) + f32(0.5)).astype(np.uint32)
        np.add.at(thick, pix, q)
    return keys, thick


def weights(r):
    """S[0..r]: exp in double, rounded once."""
    sigma = 0.5 * r
    return np.array([math.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(r + 1)], dtype=np.float64).astype(f32)


def smooth(z0, r, K, tau):
    """K iterations of the filter on the plane z0[h, w] (+inf on background)."""
    z = np.array(z0, dtype=f32)
    if r == 0 or K == 0:
        return z
    h, w = z.shape
    S, tau = weights(r), f32(tau)
    for _ in range(K):
        pad = np.full((h + 2 * r, w + 2 * r), INF, dtype=f32)
        pad[r:r + h, r:r + w] = z
        surf = np.isfinite(z)
        zc = np.where(surf, z, f32(0.0))
        num, den = np.zeros((h, w), f32), np.zeros((h, w), f32)
        with np.errstate(all="ignore"):
            for dj in range(-r, r + 1):
                for di in range(-r, r + 1):
                    zn = pad[r + dj:r + dj + h, r + di:r + di + w]
                    fin = np.isfinite(zn)
                    zn = np.where(fin, zn, f32(0.0))
                    e = (zn - zc) / tau
                    q = f32(1.0) - e * e
                    use = fin & (q > 0)
                    wt = (S[abs(di)] * S[abs(dj)]) * (q * q)
                    num = np.where(use, num + wt * zn, num)
                    den = np.where(use, den + wt, den)
            z = np.where(surf, num / den, INF).astype(f32)
    return z


def eye_points(z, cam):
    """P(i, j) for the plane z[h, w]: (x, y, z) planes (garbage where z is not finite)."""
    h, w = z.shape
    focal = f32(cam.focal_px)
    half_w, half_h = f32(0.5) * f32(w), f32(0.5) * f32(h)
    jj, ii = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        x = (((ii.astype(f32) + f32(0.5)) - half_w) * z) / focal
        y = ((half_h - (jj.astype(f32) + f32(0.5))) * z) / focal
    return np.stack([x, y, z], axis=-1).astype(f32)


def _shift(a, dy, dx, fill):
    """b[j, i] = a[j + dy, i + dx], `fill` outside"""
    out = np.full_like(a, fill)
    h, w = a.shape[:2]
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    out[yd, xd] = a[ys, xs]
    return out


def _slope(P, surf, dy, dx, none):
    """forward neighbour at (j + dy, i + dx), backward at (j - dy, i - dx)"""
    with np.errstate(all="ignore"):
        f = _shift(P, dy, dx, f32(0.0)) - P
        b = P - _shift(P, -dy, -dx, f32(0.0))
        hf, hb = _shift(surf, dy, dx, False), _shift(surf, -dy, -dx, False)
        use_f = hf & (~hb | (np.abs(f[..., 2]) <= np.abs(b[..., 2])))
    d = np.where(use_f[..., None], f, b)
    return np.where((hf | hb)[..., None], d, none).astype(f32)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normals(z, cam):
    """Eye-space unit normals[h, w, 3] from the plane z; (0, 0, 0) on background."""
    surf = np.isfinite(z)
    P = eye_points(z, cam)
    with np.errstate(all="ignore"):
        zf = (z / f32(cam.focal_px)).astype(f32)
        zero = np.zeros_like(zf)
        ddx = _slope(P, surf, 0, 1, np.stack([zf, zero, zero], axis=-1))
        ddy = _slope(P, surf, -1, 0, np.stack([zero, zf, zero], axis=-1))
        n = np.stack([ddy[..., 1] * ddx[..., 2] - ddy[..., 2] * ddx[..., 1],
                      ddy[..., 2] * ddx[..., 0] - ddy[..., 0] * ddx[..., 2],
                      ddy[..., 0] * ddx[..., 1] - ddy[..., 1] * ddx[..., 0]], axis=-1).astype(f32)
        len2 = _dot(n, n)
        ok = (len2 > 0) & np.isfinite(len2)
        n = np.where(ok[..., None], n / np.sqrt(len2)[..., None], np.array([0.0, 0.0, -1.0], f32))
    return np.where(surf[..., None], n, f32(0.0)).astype(f32)


def render(pos, cam, surface=None, vel=None, index=None, density=None, color="index", lo=0.0, hi=1.0, radius=1.0 / 64.0,
           index_count=None, background=(0, 0, 0, 255)):
    """All planes of one surface render of the particles `pos` (n, 3) in slot order, as a namespace: rgba[h, w, 4] uint8,
    id[h, w] uint32, depth[h, w] (smoothed), raw[h, w], thick[h, w] uint32 (zeros when the thickness pass is off),
    normal[h, w, 3]."""
    sf = surface or surface_style()
    w, h = int(cam.width), int(cam.height)
    pos = np.asarray(pos, dtype=f32).reshape(-1, 3)
    n = pos.shape[0]
    R = f32(radius)
    index = np.arange(n, dtype=np.uint32) if index is None else np.asarray(index, dtype=np.uint32)
    keys, thick = splat(pos, cam, radius)
    thick_on = any(a > 0 for a in sf.absorb)
    if not thick_on:
        thick[:] = 0
    surf = keys != rm.EMPTY
    raw = np.full(w * h, INF, dtype=f32)
    raw[surf] = (keys[surf] >> np.uint64(32)).astype(np.uint32).view(f32)
    raw = raw.reshape(h, w)
    K = sf.smooth_iterations if sf.smooth_radius_px else 0
    tau = f32(sf.depth_falloff) if sf.depth_falloff > 0 else f32(4.0) * R
    z = smooth(raw, sf.smooth_radius_px if K else 0, K, tau)
    nrm = normals(z, cam)
    rgba = np.empty((h, w, 4), dtype=np.uint8)
    rgba[:] = np.asarray(background, dtype=np.uint8)
    ident = np.full(w * h, rm.NO_ID, dtype=np.uint32)
    surf2 = surf.reshape(h, w)
    if surf.any():
        slot = (keys[surf] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        ident[surf] = index[slot]
        ll = math.sqrt(sum(float(f32(v)) ** 2 for v in sf.light))
        L = np.array([float(f32(v)) / ll for v in sf.light], dtype=np.float64).astype(f32)
        P, nv = eye_points(z, cam)[surf2], nrm[surf2]
        pl = np.sqrt(_dot(P, P))
        V = (-P) / pl[:, None]
        ndl = np.maximum(f32(0.0), _dot(nv, L))
        H = L + V
        hl = np.sqrt(_dot(H, H))
        with np.errstate(all="ignore"):
            H = np.where((hl > 0)[:, None], H / hl[:, None], nv)
        spec = np.maximum(f32(0.0), _dot(nv, H))
        for _ in range(5):
            spec = spec * spec
        ndv = np.minimum(np.maximum(_dot(nv, V), f32(0.0)), f32(1.0))
        m = f32(1.0) - ndv
        F = f32(0.02) + f32(0.98) * (((m * m) * (m * m)) * m)
        lit = f32(0.25) + f32(0.75) * ndl
        if sf.flat_color:
            c = np.ones((slot.size, 3), f32)
        else:
            mode = rm.MODES[color]
            if mode == 0:
                t = index[slot].astype(f32) / f32(n if not index_count else index_count)
            elif mode == 1:
                vv = np.asarray(vel, dtype=f32).reshape(-1, 3)[slot]
                t = (np.sqrt((vv[:, 0] * vv[:, 0] + vv[:, 1] * vv[:, 1]) + vv[:, 2] * vv[:, 2]) - f32(lo)) / (f32(hi) - f32(lo))
            else:
                t = (np.asarray(density, dtype=f32)[slot] - f32(lo)) / (f32(hi) - f32(lo))
            c = rm.ramp(t)
        T = thick[surf].astype(f32) * (R * f32(0.125))
        out = np.empty((slot.size, 3), np.uint8)
        for k in range(3):
            base = f32(sf.tint[k]) * c[:, k] if not sf.flat_color else np.full(slot.size, f32(sf.tint[k]))
            tr = f32(1.0) / (f32(1.0) + f32(sf.absorb[k]) * T) if thick_on else np.zeros(slot.size, f32)
            bg = f32(background[k]) / f32(255.0)
            body = (base * lit) * (f32(1.0) - tr) + bg * tr
            o = (body * (f32(1.0) - F) + F) + f32(sf.specular) * spec
            out[:, k] = (np.minimum(np.maximum(o, f32(0.0)), f32(1.0)) * f32(255.0) + f32(0.5)).astype(np.uint8)
        rgba[surf2, :3] = out
        rgba[surf2, 3] = 255
    return SimpleNamespace(rgba=rgba, id=ident.reshape(h, w), depth=z, raw=raw, thick=thick.reshape(h, w), normal=nrm)

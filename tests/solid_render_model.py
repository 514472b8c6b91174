"""numpy float32 model of the solids in the picture (include/sph_hip.h: sph_render_set_solids, THE RULE): the ray of a pixel, the
clip against a slot's grid in its body frame, the march, the bisection, the shading and the two compositions -- every operation
rounded to fp32, no multiply-add fusion, sums left to right, IEEE division and square root, fmin / fmax that drop a NaN.  A sample
is obstacle_pose_model.sample (posed or not: the rule of sph_obstacle_sample); the fluid's planes are render_model's and
surface_model's.  The model marches EVERY ray to its end: it knows nothing of the fluid's depth that lets the kernel leave early.

A slot is slot(...) below; `slots` maps the slot number to one.  Rays are flattened row by row: pixel (i, j) is ray j * w + i."""
import math
from types import SimpleNamespace

import numpy as np

import obstacle_pose_model as opm
import render_model as rm
import surface_model as sm

f32 = np.float32
INF = f32(np.inf)
ID_SOLID = 0xFFFFFFF0            # SPH_RENDER_ID_SOLID
MAX_STEPS, BISECTIONS = 512, 6   # SPH_SOLID_MAX_STEPS, SPH_SOLID_BISECTIONS
MAX_SLOTS = 4                    # SPH_MAX_OBSTACLES
DEFAULT_COLOR, DEFAULT_LIGHT, DEFAULT_AMBIENT = (0.72, 0.72, 0.75), (1.0, 1.0, -1.0), 0.25


def slot(grid, phi, off=(0.0, 0.0, 0.0), pose=None, draw=1, open=0, color=DEFAULT_COLOR):
    """One slot: the grid ({"dims", "origin", "spacing"}), its field phi (n_z, n_y, n_x), the offset, the pose
    (obstacle_pose_model.pose, None: unposed) and the look."""
    return {"grid": grid, "phi": np.asarray(phi, f32), "off": np.array(off, f32), "pose": pose, "draw": int(draw), "open": int(open),
            "color": np.array(color, f32)}


def rays(cam):
    """(ex, ey, le (n,), O (3 scalars), D (3 arrays (n,))) of every pixel, row by row."""
    w, h, rot, trans, focal, _, _ = rm._cam(cam)
    half_w, half_h = f32(0.5) * f32(w), f32(0.5) * f32(h)
    jj, ii = np.mgrid[0:h, 0:w]
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    ex = ((ii.astype(f32) + f32(0.5)) - half_w) / focal
    ey = (half_h - (jj.astype(f32) + f32(0.5))) / focal
    le = np.sqrt((ex * ex + ey * ey) + f32(1.0))
    O = [-((rot[k] * trans[0] + rot[3 + k] * trans[1]) + rot[6 + k] * trans[2]) for k in range(3)]
    D = [((rot[k] * ex + rot[3 + k] * ey) + rot[6 + k]).astype(f32) for k in range(3)]
    assert all(o.dtype == f32 for o in O) and le.dtype == f32
    return ex, ey, le, O, D


def clip(sl, O, D, near, far):
    """(t0, t1) of every ray against the slot's grid, in its body frame; a ray enters iff t0 <= t1."""
    g, off, ps = sl["grid"], sl["off"], sl["pose"]
    s, origin = f32(g["spacing"]), np.asarray(g["origin"], f32)
    if ps is None:
        Ob = [O[k] - off[k] for k in range(3)]
        Db = D
    else:
        R, piv, P = opm.rot_of(ps["q"]), ps["pivot"], opm.world_pivot(ps, off)
        dO = [O[k] - P[k] for k in range(3)]
        Ob = [((R[0, k] * dO[0] + R[1, k] * dO[1]) + R[2, k] * dO[2]) + piv[k] for k in range(3)]
        Db = [((R[0, k] * D[0] + R[1, k] * D[1]) + R[2, k] * D[2]).astype(f32) for k in range(3)]
    n = D[0].shape[0]
    t0, t1 = np.full(n, f32(near), f32), np.full(n, f32(far), f32)
    with np.errstate(all="ignore"):
        for k in range(3):
            lo, hi = origin[k], origin[k] + f32(g["dims"][k] - 1) * s
            inv = f32(1.0) / Db[k]
            ta, tb = ((lo - Ob[k]) * inv).astype(f32), ((hi - Ob[k]) * inv).astype(f32)
            t0 = np.fmax(t0, np.fmin(ta, tb))
            t1 = np.fmin(t1, np.fmax(ta, tb))
    assert t0.dtype == f32 and t1.dtype == f32
    return t0, t1


def _sample(sl, O, D, z, rays_idx):
    pts = np.stack([O[k] + z * D[k][rays_idx] for k in range(3)], axis=1).astype(f32)
    ph, nw, ins, _ = opm.sample(sl["grid"], sl["phi"], sl["off"], sl["pose"], pts)
    return ph, nw, ins


def march_slot(sl, cam, geometry=None):
    """One slot alone: (hit (n,) bool, z_s (n,) (+inf: miss), world normal (n, 3), stats) -- stats: "entered" (t0 <= t1),
    "exhausted" (the ray used up MAX_STEPS samples), "steps" (samples of the march, without the bisection)."""
    _, _, le, O, D = geometry or rays(cam)
    n = le.shape[0]
    t0, t1 = clip(sl, O, D, cam.near_z, cam.far_z)
    qs = f32(0.25) * f32(sl["grid"]["spacing"])
    entered = t0 <= t1
    z, za, zb = t0.copy(), t0.copy(), np.zeros(n, f32)
    nrm = np.zeros((n, 3), f32)
    open_run = np.full(n, bool(sl["open"]))
    cross, exhausted = np.zeros(n, bool), np.zeros(n, bool)
    steps = np.zeros(n, np.int32)
    act = np.nonzero(entered)[0]
    with np.errstate(all="ignore"):
        for _ in range(MAX_STEPS):
            act = act[z[act] <= t1[act]]
            if act.size == 0:
                break
            steps[act] += 1
            ph, nw, ins = _sample(sl, O, D, z[act], act)
            neg = ins & (ph < 0)
            cr = neg & ~open_run[act]
            zb[act[cr]] = z[act[cr]]
            nrm[act[cr]] = nw[cr]
            cross[act[cr]] = True
            a = np.where(ins, np.where(neg, np.fmax(f32(0.5) * (-ph), qs), np.fmax(f32(0.5) * ph, qs)), qs).astype(f32)
            open_run[act[ins & ~neg]] = False
            go = ~cr
            act, a = act[go], a[go]
            za[act] = z[act]
            z[act] = z[act] + a / le[act]
        else:
            exhausted[act] = True
        j = np.nonzero(cross)[0]
        for _ in range(BISECTIONS):
            if j.size == 0:
                break
            zm = f32(0.5) * (za[j] + zb[j])
            ph, nw, ins = _sample(sl, O, D, zm, j)
            solid = ins & (ph < 0)
            zb[j[solid]] = zm[solid]
            nrm[j[solid]] = nw[solid]
            za[j[~solid]] = zm[~solid]
    zs = np.where(cross, zb, INF).astype(f32)
    assert z.dtype == f32 and zs.dtype == f32 and nrm.dtype == f32
    return cross, zs, nrm, {"entered": entered, "exhausted": exhausted, "steps": steps}


def light_of(light):
    ll = math.sqrt(sum(float(f32(v)) ** 2 for v in light))
    return np.array([float(f32(v)) / ll for v in light], dtype=np.float64).astype(f32)


def march(cam, slots, light=DEFAULT_LIGHT, ambient=DEFAULT_AMBIENT):
    """The nearest hit of every pixel over the drawn slots, as a namespace of planes: hit[h, w] bool, z[h, w] (+inf: none),
    slot[h, w], ne[h, w, 3] (eye-space normal), color[h, w, 3] float32 (c of the rule), rgba[h, w, 4] uint8; stats[k] per slot."""
    w, h, rot = int(cam.width), int(cam.height), np.array(list(cam.rot), f32)
    geo = rays(cam)
    n = w * h
    best, who, nrm, hit, stats = np.full(n, INF, f32), np.zeros(n, np.int64), np.zeros((n, 3), f32), np.zeros(n, bool), {}
    for k in sorted(slots):
        if not slots[k]["draw"]:
            continue
        got, zs, nw, stats[k] = march_slot(slots[k], cam, geo)
        take = got & (zs < best)                         # strictly: the lowest slot wins among equals
        best[take], who[take], nrm[take] = zs[take], k, nw[take]
        hit |= take
    ne = np.stack([(rot[3 * k] * nrm[:, 0] + rot[3 * k + 1] * nrm[:, 1]) + rot[3 * k + 2] * nrm[:, 2] for k in range(3)], axis=1)
    L, amb = light_of(light), f32(ambient)
    ndl = np.fmax(f32(0.0), (ne[:, 0] * L[0] + ne[:, 1] * L[1]) + ne[:, 2] * L[2])
    g = amb + (f32(1.0) - amb) * ndl
    col = np.zeros((n, 3), f32)
    for k in slots:
        col[who == k] = slots[k]["color"]
    c = np.fmin(np.fmax(col * g[:, None], f32(0.0)), f32(1.0)).astype(f32)
    rgba = np.full((n, 4), 255, np.uint8)
    rgba[:, :3] = (c * f32(255.0) + f32(0.5)).astype(np.uint8)
    ne = np.where(hit[:, None], ne, f32(0.0)).astype(f32)
    assert c.dtype == f32 and g.dtype == f32
    return SimpleNamespace(hit=hit.reshape(h, w), z=best.reshape(h, w), slot=who.reshape(h, w), ne=ne.reshape(h, w, 3),
                           color=c.reshape(h, w, 3), rgba=rgba.reshape(h, w, 4), stats=stats)


def compose_render(fluid, sol):
    """sph_render with solids: fluid = (rgba, id, depth) of render_model.render; -> (rgba, id, depth, win[h, w])."""
    rgba, ident, depth = (np.array(a) for a in fluid)
    win = sol.hit & (sol.z < depth)                      # (depth is +inf where no sprite covers the pixel)
    rgba[win] = sol.rgba[win]
    ident[win] = (ID_SOLID + sol.slot[win]).astype(np.uint32)
    depth[win] = sol.z[win]
    return rgba, ident, depth, win


def fluid_rgba(r, cam, sf, behind, color="index", index_count=None, radius=1.0 / 64.0):
    """The shading of surface_model.render for the fluid pixels of its planes r, over the per-pixel colour behind[h, w, 3]
    (float32) in place of the background's: rgba[h, w, 4], r.rgba where there is no fluid."""
    surf = np.isfinite(r.depth)
    out = np.array(r.rgba)
    if not surf.any():
        return out
    R = f32(radius)
    L = light_of(sf.light)
    P, nv = sm.eye_points(r.depth, cam)[surf], r.normal[surf]
    pl = np.sqrt(sm._dot(P, P))
    V = (-P) / pl[:, None]
    ndl = np.maximum(f32(0.0), sm._dot(nv, L))
    H = L + V
    hl = np.sqrt(sm._dot(H, H))
    with np.errstate(all="ignore"):
        H = np.where((hl > 0)[:, None], H / hl[:, None], nv)
    spec = np.maximum(f32(0.0), sm._dot(nv, H))
    for _ in range(5):
        spec = spec * spec
    ndv = np.minimum(np.maximum(sm._dot(nv, V), f32(0.0)), f32(1.0))
    m = f32(1.0) - ndv
    F = f32(0.02) + f32(0.98) * (((m * m) * (m * m)) * m)
    lit = f32(0.25) + f32(0.75) * ndl
    if sf.flat_color:
        c = np.ones((int(surf.sum()), 3), f32)
    else:
        assert color == "index", "the model of the solids shades by tint or by creation index"
        c = rm.ramp(r.id[surf].astype(f32) / f32(index_count))
    thick_on = any(a > 0 for a in sf.absorb)
    T = r.thick[surf].astype(f32) * (R * f32(0.125))
    bg = np.asarray(behind, f32)[surf]
    px = np.empty((c.shape[0], 3), np.uint8)
    for k in range(3):
        base = np.full(c.shape[0], f32(sf.tint[k])) if sf.flat_color else f32(sf.tint[k]) * c[:, k]
        tr = f32(1.0) / (f32(1.0) + f32(sf.absorb[k]) * T) if thick_on else np.zeros(c.shape[0], f32)
        body = (base * lit) * (f32(1.0) - tr) + bg[:, k] * tr
        o = (body * (f32(1.0) - F) + F) + f32(sf.specular) * spec
        assert o.dtype == f32
        px[:, k] = (np.minimum(np.maximum(o, f32(0.0)), f32(1.0)) * f32(255.0) + f32(0.5)).astype(np.uint8)
    out[surf, :3] = px
    out[surf, 3] = 255
    return out


def compose_surface(r, cam, sf, sol, background=(0, 0, 0, 255), **shade):
    """sph_render_surface with solids: r the planes of surface_model.render (the fluid alone) -> a namespace rgba, id, depth,
    normal, win[h, w] (the solid's pixels), through[h, w] (fluid pixels with a hit behind them); raw and thick are r's."""
    h, w = r.depth.shape
    win = sol.hit & (sol.z < r.depth)                    # (r.depth is +inf on background)
    fluid = np.isfinite(r.depth)
    through = fluid & sol.hit & ~win
    behind = np.empty((h, w, 3), f32)
    behind[:] = np.array([f32(background[k]) / f32(255.0) for k in range(3)], f32)
    behind[through] = sol.color[through]
    rgba = fluid_rgba(r, cam, sf, behind, **shade)
    ident, depth, normal = np.array(r.id), np.array(r.depth), np.array(r.normal)
    rgba[win] = sol.rgba[win]
    ident[win] = (ID_SOLID + sol.slot[win]).astype(np.uint32)
    depth[win] = sol.z[win]
    normal[win] = sol.ne[win]
    return SimpleNamespace(rgba=rgba, id=ident, depth=depth, normal=normal, win=win, through=through, raw=r.raw, thick=r.thick)

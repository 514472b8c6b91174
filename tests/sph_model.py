"""float64 model of one SPH step for ANY sph_params -- TEST INFRASTRUCTURE.

The oracle (oracle/sph_oracle.c) restates the reference bit for bit but bakes in the reference's constants.  This model states
the same formulas (SPH/particleSystem.cu:15-65, 375-420) in plain numpy for the physics parameters of a `capi.Params`, one
phase at a time.  Each phase takes its inputs from the caller, so a test can feed it the GPU's own state for that phase and the
comparison measures that phase alone.

Semantics kept from the reference:
  * neighbours are the 27-cell stencil of the float32 cell coordinates (csrc/sph_device.hpp: cell_coord), not a radius
    search: where h exceeds the cell edge, neighbours beyond the stencil are missed, as in the reference;
  * density  m 315 / (65 pi h^9) sum (h^2 - r^2)^3 over r < h, self included (the reference's 65);
  * pressure max(0, k (rho - rho0));
  * force    f_press += r^ m (p_i + p_j) / (2 rho_j) 45/(pi h^6) (h - r)^2 (r_ij = 0 adds nothing),
             f_visc  += visc m (v_j - v_i) / rho_j 45/(pi h^6) (h - r), r < h;
  * collide  j != i with sqrtf(r2) <= COLLISION_PARAM 2 R (compared in double) and r.v < 0, both predicates in float32 in the
             reference's operation order; dv = -sum m (1 + e) (r.v / d^2) r / (m (1 + count)), the magnitudes in float64;
  * integrate a = (f + (0, g rho, 0)) / rho, v += dt a + dv, x += dt v, then the walls per axis (lower wall first), then the
             sphere colliders (tests/collider_model.py).
The wall and sphere tests are discontinuous: a float64 position a few ulps from a threshold may land on either side in float32.
`integrate` therefore returns, next to its result, every outcome such a particle may legally have.
"""
from types import SimpleNamespace

import numpy as np

import collider_model

F = np.float32


def reference_params(box, grid):
    """sph_default_params without the library: the reference's constants for a box centred on the origin
    (include/sph_hip.h, sph_params)."""
    box = np.asarray(box, F).reshape(3)
    return SimpleNamespace(box_min=list(-box / F(2)), box_max=list(box / F(2)), grid=[int(g) for g in grid], h=F(0.1),
                           mass=F(65), rest_density=F(1000), gas_constant=F(2000), viscosity=F(250),
                           gravity_y=F(-9.81) * F(11000), wall_eps=F(1e-5), wall_damping=F(-0.75), restitution=F(0),
                           collision_param=F(1), particle_radius=F(1 / 64))


class Model:
    def __init__(self, params, colliders=None):
        """params: capi.Params (or anything with its fields); colliders: None or (centers, radii, velocities) float32."""
        p = params
        self.box_min = np.array(p.box_min[:], F)
        self.box_max = np.array(p.box_max[:], F)
        self.dims = (self.box_max - self.box_min).astype(F)
        self.grid = np.array(p.grid[:], np.int64)
        self.h = float(F(p.h))
        self.mass = float(F(p.mass))
        self.rest_density = float(F(p.rest_density))
        self.gas_constant = float(F(p.gas_constant))
        self.viscosity = float(F(p.viscosity))
        self.gravity_y = float(F(p.gravity_y))
        self.wall_eps = F(p.wall_eps)
        self.wall_damping = F(p.wall_damping)
        self.restitution = float(F(p.restitution))
        self.coll_dist = float(F(p.collision_param)) * 2.0 * float(F(p.particle_radius))
        self.colliders = colliders

    # ---- neighbours ----------------------------------------------------------------------------------------------------
    def cells(self, pos):
        """float32 cell coordinates, ((p - bmin) / bdim) * gf, floor, clamped (cell_coord)."""
        pos = np.asarray(pos, F)
        q = ((pos - self.box_min) / self.dims) * self.grid.astype(F)
        c = np.floor(q).astype(np.int64)
        return np.clip(c, 0, self.grid - 1)

    def pairs(self, pos):
        """(i, j) of every candidate pair of the 27-cell stencil, self pairs included."""
        c = self.cells(pos)
        gx, gy, gz = (int(v) for v in self.grid)
        key = (c[:, 2] * gy + c[:, 1]) * gx + c[:, 0]
        order = np.argsort(key, kind="stable")
        skey = key[order]
        I, J = [], []
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    nc = c + np.array([dx, dy, dz])
                    ok = np.all((nc >= 0) & (nc < self.grid), axis=1)
                    nk = (nc[:, 2] * gy + nc[:, 1]) * gx + nc[:, 0]
                    lo = np.searchsorted(skey, nk, "left")
                    hi = np.searchsorted(skey, nk, "right")
                    cnt = np.where(ok, hi - lo, 0)
                    i = np.repeat(np.arange(pos.shape[0]), cnt)
                    start = np.repeat(lo - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt)
                    J.append(order[start + np.arange(i.size)])
                    I.append(i)
        return np.concatenate(I), np.concatenate(J)

    # ---- phases --------------------------------------------------------------------------------------------------------
    def density(self, pos, pairs=None):
        """(density, pressure) float64 from float32 positions."""
        i, j = self.pairs(pos) if pairs is None else pairs
        x = np.asarray(pos, np.float64)
        r2 = ((x[i] - x[j]) ** 2).sum(axis=1)
        h2 = self.h * self.h
        w = np.where(r2 < h2, (h2 - r2) ** 3, 0.0)
        rho = self.mass * 315.0 / (65.0 * np.pi * self.h ** 9) * np.bincount(i, w, minlength=x.shape[0])
        return rho, self.pressure(rho)

    def pressure(self, rho):
        return np.maximum(0.0, self.gas_constant * (np.asarray(rho, np.float64) - self.rest_density))

    def forces(self, pos, vel, rho, p, pairs=None):
        """(f_press, f_visc) float64 (n, 3) from the given positions, velocities, densities and pressures."""
        i, j = self.pairs(pos) if pairs is None else pairs
        x, v = np.asarray(pos, np.float64), np.asarray(vel, np.float64)
        rho, p = np.asarray(rho, np.float64), np.asarray(p, np.float64)
        d = x[i] - x[j]
        r = np.sqrt((d * d).sum(axis=1))
        near = r < self.h
        i, j, d, r = i[near], j[near], d[near], r[near]
        lap = 45.0 / (np.pi * self.h ** 6)
        hr = self.h - r
        pos_r = r > 0
        s = np.zeros_like(r)
        s[pos_r] = self.mass * (p[i] + p[j])[pos_r] / (2.0 * rho[j][pos_r]) * lap * hr[pos_r] ** 2 / r[pos_r]
        fv = (self.viscosity * self.mass * lap) * ((v[j] - v[i]) / rho[j][:, None]) * hr[:, None]
        n = x.shape[0]
        fp = np.stack([np.bincount(i, s * d[:, a], minlength=n) for a in range(3)], axis=1)
        fvs = np.stack([np.bincount(i, fv[:, a], minlength=n) for a in range(3)], axis=1)
        return fp, fvs

    def collide(self, pos, vel, pairs=None):
        """(dv float64 (n, 3), count int32 (n,)): the predicates in float32 exactly as the reference evaluates them."""
        i, j = self.pairs(pos) if pairs is None else pairs
        keep = i != j
        i, j = i[keep], j[keep]
        x, v = np.asarray(pos, F), np.asarray(vel, F)
        r = x[i] - x[j]
        u = v[i] - v[j]
        r2 = r[:, 0] * r[:, 0] + (r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2])
        dot = r[:, 0] * u[:, 0] + (r[:, 1] * u[:, 1] + r[:, 2] * u[:, 2])
        hit = (np.sqrt(r2).astype(np.float64) <= self.coll_dist) & (dot < 0)
        i, r, u = i[hit], r[hit].astype(np.float64), u[hit].astype(np.float64)
        s = self.mass * (1.0 + self.restitution) * (r * u).sum(axis=1) / (r * r).sum(axis=1)
        n = x.shape[0]
        count = np.bincount(i, minlength=n).astype(np.int32)
        acc = np.stack([np.bincount(i, s * r[:, a], minlength=n) for a in range(3)], axis=1)
        return -acc / (self.mass * (1.0 + count))[:, None], count

    def integrate(self, pos, vel, rho, force, dv, dt, ulps=4):
        """One integrate from the given state.  Returns (pos, vel, alts): float64 (n, 3) results and the other outcomes a
        particle may legally take where a wall or sphere predicate lies within `ulps` float32 ulps of its threshold:
        alts = {particle: {axis: [(x, v), ...] per wall axis, "sphere": [(pos (3,), vel (3,)), ...]}}."""
        rho = np.asarray(rho, np.float64)
        a = np.asarray(force, np.float64).copy()
        a[:, 1] += self.gravity_y * rho
        a /= rho[:, None]
        v = np.asarray(vel, np.float64) + dt * a + np.asarray(dv, np.float64)
        x = np.asarray(pos, np.float64) + dt * v
        out_x, out_v = x.copy(), v.copy()
        alts = {}
        tol = ulps * np.spacing(np.maximum(np.abs(self.box_min), np.abs(self.box_max)).astype(F)).astype(np.float64)
        damp = float(self.wall_damping)
        for ax in range(3):
            lo, hi, eps = float(self.box_min[ax]), float(self.box_max[ax]), float(self.wall_eps)
            xa, va = x[:, ax], v[:, ax]
            t_lo = xa - eps - lo                                  # lower wall first, then the upper one on the moved x
            x1 = np.where(t_lo < 0, lo + eps, xa)
            v1 = np.where(t_lo < 0, va * damp, va)
            t_hi = x1 + eps - hi
            out_x[:, ax] = np.where(t_hi > 0, hi - eps, x1)
            out_v[:, ax] = np.where(t_hi > 0, v1 * damp, v1)
            amb = (np.abs(t_lo) <= tol[ax]) | (np.abs(t_hi) <= tol[ax]) | (np.abs(xa + eps - hi) <= tol[ax])
            for k in np.nonzero(amb)[0]:
                opts = set()
                for lo_hit in (False, True):
                    for hi_hit in (False, True):
                        xx, vv = float(xa[k]), float(va[k])
                        if lo_hit: xx, vv = lo + eps, vv * damp
                        if hi_hit: xx, vv = hi - eps, vv * damp
                        opts.add((xx, vv))
                alts.setdefault(int(k), {})[ax] = sorted(opts)
        if self.colliders is not None:
            out_x, out_v, alts = self._spheres(out_x, out_v, alts, ulps)
        return out_x, out_v, alts

    def _spheres(self, x, v, alts, ulps):
        centers, radii, vels = self.colliders
        x32, v32 = x.astype(F), v.astype(F)
        px, pv, touched = collider_model.push(x32, v32, centers, radii, vels, self.box_min, self.box_max,
                                              self.wall_eps, self.wall_damping)
        out_x, out_v = x.copy(), v.copy()
        out_x[touched], out_v[touched] = px[touched], pv[touched]
        # near a shell the float32 test r2 < (R + eps)^2 can go either way: such a particle may stay where the walls left
        # it, or be pushed (its position moved just inside every shell it is near, then the sphere rule)
        cs, rps = np.asarray(centers, F).reshape(-1, 3), (np.asarray(radii, F).reshape(-1) + self.wall_eps).astype(F)
        dist = np.sqrt(((x[:, None, :] - cs[None].astype(np.float64)) ** 2).sum(axis=2))         # (n, spheres)
        near = np.abs(dist - rps.astype(np.float64)) <= 64 * ulps * np.spacing(rps).astype(np.float64)
        for k in np.nonzero(near.any(axis=1))[0]:
            xin = x32[k].copy()
            for j in np.nonzero(near[k])[0]:
                xin = (cs[j] + (xin - cs[j]) * F(0.9999)).astype(F)
            qx, qv, _ = collider_model.push_one(xin, v32[k], centers, radii, vels, self.box_min, self.box_max,
                                                self.wall_eps, self.wall_damping)
            alts.setdefault(int(k), {})["sphere"] = [(x[k].copy(), v[k].copy()), (out_x[k].copy(), out_v[k].copy()),
                                                     (qx.astype(np.float64), qv.astype(np.float64))]
        return out_x, out_v, alts


def integrate_mismatch(model_out, pos, vel, pos_tol, vel_tol):
    """Particles whose GPU (pos, vel) matches neither the model's integrate result nor any legal alternative outcome."""
    mx, mv, alts = model_out
    pos, vel = np.asarray(pos, np.float64), np.asarray(vel, np.float64)
    bad = (np.abs(pos - mx) > pos_tol).any(axis=1) | (np.abs(vel - mv) > vel_tol).any(axis=1)
    for k in np.nonzero(bad)[0]:
        a = alts.get(int(k))
        if not a:
            continue
        if "sphere" in a:
            if any(np.all(np.abs(pos[k] - ax) <= pos_tol) and np.all(np.abs(vel[k] - av) <= vel_tol) for ax, av in a["sphere"]):
                bad[k] = False
            continue
        ok = True
        for ax in range(3):
            if abs(pos[k, ax] - mx[k, ax]) <= pos_tol and abs(vel[k, ax] - mv[k, ax]) <= vel_tol:
                continue
            ok &= any(abs(pos[k, ax] - xx) <= pos_tol and abs(vel[k, ax] - vv) <= vel_tol for xx, vv in a.get(ax, ()))
        bad[k] = not ok
    return np.nonzero(bad)[0]

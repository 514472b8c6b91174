"""TEST INFRASTRUCTURE: a CPU stand-in for the per-rank engine of gpufluidsimulator_amd.slab, with the
oracle behind it, so that the slab PROTOCOL (cuts, counts, migrants, ghost layers, density halo) can be
driven by CPU ranks (gloo / in-process).  Never imported by the product package."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from gpufluidsimulator_amd import slab  # noqa: E402
from oracle import oracle  # noqa: E402


def _cell(p, bmin, bdim, g):
    q = ((p.astype(np.float32) - np.float32(bmin)) / np.float32(bdim)) * np.float32(g)
    return np.clip(np.floor(q).astype(np.int64), 0, int(g) - 1)


class OracleEngine:
    GHOST_LAYERS = 1            # OracleEngine2 below: two (the one-message protocol)

    def __init__(self, capacity, ghost_capacity, params, z_lo, z_hi):
        self.grid = tuple(int(v) for v in params.grid)
        self.bmin = np.float32(list(params.box_min))
        self.bdim = np.float32(list(params.box_max)) - self.bmin
        self.box = tuple(float(v) for v in self.bdim)
        self.G = int(self.GHOST_LAYERS)
        self.z_lo, self.z_hi, self.zl = int(z_lo), int(z_hi), int(z_hi - z_lo + 2 * self.G)
        self.layer = self.grid[0] * self.grid[1]
        self.capacity, self.ghost_capacity = capacity, ghost_capacity
        self.pos = np.zeros((0, 3), np.float32); self.vel = np.zeros((0, 3), np.float32)
        self.idx = np.zeros((0,), np.uint32); self.key = np.zeros((0,), np.int64)
        self.rho = np.zeros((0,), np.float32); self.prs = np.zeros((0,), np.float32)
        self._clear_ghosts()
        self.o = None

    def _clear_ghosts(self):
        z3, z1 = np.zeros((0, 3), np.float32), np.zeros((0,), np.float32)
        self.g = [dict(pos=z3, vel=z3, idx=np.zeros((0,), np.uint32), rho=z1, prs=z1) for _ in range(2)]

    # plumbing ------------------------------------------------------------------------------------
    def buffer(self, rows, cols): return torch.zeros((rows, cols), dtype=torch.float32)
    def small(self, values): return torch.tensor(values, dtype=torch.int64)
    @property
    def n(self): return int(self.pos.shape[0])
    def sync(self): pass
    def close(self): pass

    def upload(self, pos, vel, index):
        self.pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3).copy()
        self.vel = np.ascontiguousarray(vel, np.float32).reshape(-1, 3).copy()
        self.idx = np.ascontiguousarray(index, np.uint32).copy()
        assert self.n <= self.capacity
        self.rho = np.zeros(self.n, np.float32); self.prs = np.zeros(self.n, np.float32)

    # grid phases -----------------------------------------------------------------------------------
    def hash(self):
        c = [_cell(self.pos[:, a], self.bmin[a], self.bdim[a], self.grid[a]) for a in range(3)]
        lz = np.clip(c[2] - self.z_lo + self.G, 0, self.zl - 1)
        self.key = (lz * self.grid[1] + c[1]) * self.grid[0] + c[0]

    def sort_skipped(self): return False        # the CPU test engine always sorts

    def sort(self):
        o = np.argsort(self.key, kind="stable")
        self.pos, self.vel, self.idx, self.key = self.pos[o], self.vel[o], self.idx[o], self.key[o]
        self.rho, self.prs = self.rho[o] if self.rho.shape[0] == o.shape[0] else np.zeros(self.n, np.float32), \
            self.prs[o] if self.prs.shape[0] == o.shape[0] else np.zeros(self.n, np.float32)
        self._clear_ghosts()

    def slab_counts(self):
        L, G = self.layer, self.G
        lb = np.searchsorted(self.key, [G * L, (G + 1) * L, (self.zl - G - 1) * L, (self.zl - G) * L], side="left")
        return int(lb[0]), int(lb[1] - lb[0]), int(lb[3] - lb[2]), int(self.n - lb[3])

    # ---- the one-message protocol (slab.SlabSimulation._step_one): two layers per side --------------------------------
    def second_layer_counts(self):
        L, G = self.layer, self.G
        lb = np.searchsorted(self.key, [(G + 1) * L, (G + 2) * L, (self.zl - G - 2) * L, (self.zl - G - 1) * L], side="left")
        return int(lb[1] - lb[0]), int(lb[3] - lb[2])

    def pack_one(self, lo, hi):
        """Rows 1.. of each buffer (row 0 is the caller's header): my leavers towards that side, then the RESIDENTS of the two
        owned layers next to that cut, in slot order; the leavers are dropped from the owned set."""
        m_lo, own_lo, own_hi, m_hi = self.slab_counts()
        n2_lo, n2_hi = self.second_layer_counts()
        n = self.n
        lo.numpy()[1:1 + m_lo] = self._records(slice(0, m_lo))
        lo.numpy()[1 + m_lo:1 + m_lo + own_lo + n2_lo] = self._records(slice(m_lo, m_lo + own_lo + n2_lo))
        hi.numpy()[1:1 + m_hi] = self._records(slice(n - m_hi, n))
        hi.numpy()[1 + m_hi:1 + m_hi + own_hi + n2_hi] = self._records(slice(n - m_hi - own_hi - n2_hi, n - m_hi))
        self._keep(slice(m_lo, n - m_hi))

    def _records(self, sl):
        r = np.zeros((self.pos[sl].shape[0], 8), np.float32)
        r[:, 0:3] = self.pos[sl]
        r[:, 3] = self.idx[sl].view(np.float32)
        r[:, 4:7] = self.vel[sl]
        return r

    def _keep(self, sl):
        self.pos, self.vel, self.idx, self.key = self.pos[sl], self.vel[sl], self.idx[sl], self.key[sl]
        self.rho, self.prs = self.rho[sl], self.prs[sl]

    def migrants_pack(self, lo, hi):
        m_lo, _, _, m_hi = self.slab_counts()
        lo.numpy()[:m_lo] = self._records(slice(0, m_lo))
        hi.numpy()[:m_hi] = self._records(slice(self.n - m_hi, self.n))
        self._keep(slice(m_lo, self.n - m_hi))

    def migrants_append(self, buf, n):
        r = buf.numpy()[:n]
        self.pos = np.concatenate([self.pos, r[:, 0:3]]); self.vel = np.concatenate([self.vel, r[:, 4:7]])
        self.idx = np.concatenate([self.idx, np.ascontiguousarray(r[:, 3]).view(np.uint32)])
        self.rho = np.zeros(self.n, np.float32); self.prs = np.zeros(self.n, np.float32)
        assert self.n <= self.capacity

    def _halo_counts(self):
        L, G = self.layer, self.G
        lb = np.searchsorted(self.key, [G * L, (G + 1) * L, (self.zl - G - 1) * L, (self.zl - G) * L], side="left")
        return int(lb[1] - lb[0]), int(lb[3] - lb[2])

    def halo_pack(self, lo, hi, counts=None):
        h_lo, h_hi = self._halo_counts()
        assert counts is None or tuple(counts) == (h_lo, h_hi), (counts, h_lo, h_hi)
        lo.numpy()[:h_lo] = self._records(slice(0, h_lo))
        hi.numpy()[:h_hi] = self._records(slice(self.n - h_hi, self.n))

    def halo_unpack(self, lo, n_lo, hi, n_hi):
        assert max(n_lo, n_hi) <= self.ghost_capacity
        for side, (buf, m) in enumerate(((lo, n_lo), (hi, n_hi))):
            r = buf.numpy()[:m].copy()
            self.g[side] = dict(pos=r[:, 0:3].copy(), vel=r[:, 4:7].copy(),
                                idx=np.ascontiguousarray(r[:, 3]).view(np.uint32).copy(),
                                rho=np.zeros(m, np.float32), prs=np.zeros(m, np.float32))

    # neighbour passes: the oracle over ghosts + owned ------------------------------------------------------
    def build_cells(self):
        pos = np.concatenate([self.g[0]["pos"], self.pos, self.g[1]["pos"]])
        vel = np.concatenate([self.g[0]["vel"], self.vel, self.g[1]["vel"]])
        self.n_glo = self.g[0]["pos"].shape[0]
        self.o = oracle.Oracle(pos, vel, self.box, self.grid, oracle.CELL_LINEAR)
        self.o.map_zindex(); self.o.sort(); self.o.construct_bgrid()

    def density(self):
        self.o.compute_densities()
        rho, prs = self.o.by_index("density"), self.o.by_index("pressure")
        self.rho = rho[self.n_glo:self.n_glo + self.n].copy()
        self.prs = prs[self.n_glo:self.n_glo + self.n].copy()

    def halo_pack_density(self, lo, hi):
        h_lo, h_hi = self._halo_counts()
        lo.numpy()[:h_lo] = np.stack([self.rho[:h_lo], self.prs[:h_lo]], axis=1)
        hi.numpy()[:h_hi] = np.stack([self.rho[self.n - h_hi:], self.prs[self.n - h_hi:]], axis=1)

    def halo_unpack_density(self, lo, hi):
        p = self.o.particles
        slot = np.empty(p.shape[0], np.int64)
        slot[p["index"]] = np.arange(p.shape[0])
        n_lo, n_hi = self.n_glo, self.g[1]["pos"].shape[0]
        for base, buf, m in ((0, lo, n_lo), (self.n_glo + self.n, hi, n_hi)):
            r = buf.numpy()[:m]
            s = slot[base:base + m]
            p["density"][s] = r[:, 0]
            p["pressure"][s] = r[:, 1]

    def force_collide_integrate(self, dt):
        self.o.compute_forces(); self.o.particle_collisions(); self.o.integrate(dt)
        pos, vel = self.o.by_index("position"), self.o.by_index("velocity")
        self.pos = pos[self.n_glo:self.n_glo + self.n].copy()
        self.vel = vel[self.n_glo:self.n_glo + self.n].copy()
        self.o.close(); self.o = None

    def download_owned(self):
        return self.pos.copy(), self.vel.copy(), self.idx.copy()

    def to_device(self, arr):
        return torch.from_numpy(np.ascontiguousarray(arr))

    def download(self, total):
        out = dict(pos=np.full((total, 3), np.nan, np.float32), vel=np.full((total, 3), np.nan, np.float32),
                   density=np.full(total, np.nan, np.float32), pressure=np.full(total, np.nan, np.float32))
        out["pos"][self.idx] = self.pos; out["vel"][self.idx] = self.vel
        out["density"][self.idx] = self.rho; out["pressure"][self.idx] = self.prs
        return out


class OracleEngine2(OracleEngine):
    """Two ghost layers per side: what the one-message protocol needs (the ghost densities then come out of this engine's own
    density pass over owned + ghosts: the inner ghost layer's neighbourhood is complete)."""
    GHOST_LAYERS = 2


def make_case(name):
    """Small systems that force particles across slab boundaries within a few steps."""
    from gpufluidsimulator_amd import ic
    box, grid = (4.0, 4.0, 4.0), (64, 64, 64)
    if name == "tall_up":           # 24 cell layers: two slabs of 12 layers each have a deep interior (>= 7 layers)
        pos, vel = ic.dam_break_lattice((12, 12, 48), box, jitter=True)
        vel[:, 2] = 4000.0
        return pos, vel, box, grid
    pos, vel = ic.dam_break_lattice((12, 12, 24), box, jitter=True)
    if name == "up":
        vel[:, 2] = 4000.0          # 0.002 per step at dt 5e-7: crosses a cell layer every ~8 steps
    elif name == "down":
        vel[:, 2] = -4000.0         # into the floor: wall clamp + damping, then back up
    elif name == "shear":
        vel[:, 2] = np.where(pos[:, 2] > pos[:, 2].mean(), 4000.0, -2500.0)
    return pos, vel, box, grid


def far_case(direction="up", speed=2.8e5):
    """make_case's block at rest under the cuts [0, 4, 8, 64] of three slabs, except 20 particles that cross more than one
    cell layer per step (2.8e5: 0.14 = 2.24 layers).  "up": of the two lattice layers under the first cut (cell layer 3, the
    top layer of slab 0, at 3.25 and 3.75 cells), flying up into slab 1.  "down": of the two lattice layers above the second
    cut (cell layer 8, the bottom layer of slab 2, at 8.25 and 8.75 cells), flying down into slab 1.  What the oracle makes
    of either at each speed the GPU tests use: tests/test_slab_cpu.py::test_far_case_premises."""
    pos, vel, box, grid = make_case("up")
    vel[:] = 0.0
    iz = np.arange(pos.shape[0]) // (12 * 12)
    near, next_ = {"up": (7, 6), "down": (16, 17)}[direction]
    fast = np.concatenate([np.nonzero(iz == near)[0][::15][:10], np.nonzero(iz == next_)[0][::15][:10]])
    vel[fast, 2] = speed if direction == "up" else -speed
    return pos, vel, box, grid, fast


def one_cap(prev):
    """csrc/sph_slab.hip one_cap: the one-message step's size rule on the previous step's count."""
    return (int(prev) + int(prev) // 16 + 1024 + 63) & ~63


def slab_buffers(per_layer, ghost_factor, migrant_capacity):
    """(gcap, mcap, msg_cap) in records, as slab.SlabSimulation sizes the ghost capacity from the fullest cell layer and
    sph_slab_create the migrant capacity and the message buffers of a context with two ghost layers."""
    gcap = int(ghost_factor * per_layer) + 1024
    mcap = min(int(migrant_capacity) if migrant_capacity else gcap // 2 + 1024, gcap)
    return gcap, mcap, mcap + gcap + 64


# The one-message step at the edge of its buffers (tests/test_slab_cpu.py::test_clamp_case_premises counts what these give,
# tests/test_gpu_slab_limits.py runs them): make_case("tall_up") in three slabs of 8 cell layers of 288 particles, a ghost capacity
# of 1024 and a migrant capacity of 512 -> message buffers of 1600 records.  A link carries 576 records on a usual step (two
# layers), 720 and 432 in its two directions on the steps in which a lattice plane of 144 crosses the cut: the size rule asks for
# 1664, 1792 and 1536.
CLAMP_CASE = dict(case="tall_up", world=3, steps=28, ghost_factor=0.0, migrant_capacity=512)


def clamp_case_counts():
    """CLAMP_CASE stepped by CPU ranks under the one-message protocol (the oracle engine with two ghost layers): per rank and
    step {"tot_s", "tot_r": records either end of each link packed, "m": my leavers per side}, and the fullest cell layer."""
    import threading
    cc = CLAMP_CASE
    pos, vel, box, grid = make_case(cc["case"])
    hub = slab.LocalComm.Hub(cc["world"])
    rows, errors, per_layer = [[] for _ in range(cc["world"])], [], [0]

    class Counting(OracleEngine2):
        def slab_counts(self):
            self.last_counts = super().slab_counts()
            return self.last_counts

    def rank_main(r):
        try:
            sim = slab.SlabSimulation(slab.LocalComm(hub, r), Counting, box, grid, particles=(pos, vel), python_protocol=1)
            per_layer[0] = sim.per_layer
            for _ in range(cc["steps"]):
                sim.step(5e-7)
                m_lo, _, _, m_hi = sim.engine.last_counts           # (a step counts before anything leaves or arrives)
                rows[r].append(dict(tot_s=list(sim._one_prev[0]), tot_r=list(sim._one_prev[1]), m=[m_lo, m_hi]))
        except BaseException as e:     # noqa: BLE001
            errors.append(e)
            hub.bar.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(cc["world"])]
    for t in threads: t.start()
    for t in threads: t.join(timeout=600)
    assert not errors, errors
    return rows, per_layer[0]


def gloo_worker(rank, world, port, case, steps, out_dir, protocol=3):
    """Entry of one CPU rank (torch.multiprocessing.spawn): TorchDistComm over gloo."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pos, vel, box, grid = make_case(case)
        comm = slab.TorchDistComm(torch.device("cpu"))
        sim = slab.SlabSimulation(comm, OracleEngine2 if protocol == 1 else OracleEngine, box, grid, particles=(pos, vel),
                                  python_protocol=protocol)
        sim.run(5e-7, steps)
        st = sim.gather_state()
        if rank == 0:
            np.savez(os.path.join(out_dir, "out.npz"), cuts=np.array(sim.cuts), migrants=sim.stats["migrants"], **st)
        stats = comm.allreduce_sum(np.array([sim.stats["migrants"], sim.stats["resorts"], sim.stats.get("one_steps", 0)], dtype=np.int64))
        if rank == 0:
            np.save(os.path.join(out_dir, "stats.npy"), stats)
    finally:
        dist.destroy_process_group()

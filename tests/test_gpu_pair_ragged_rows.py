"""GPU: ragged candidate rows -- the staged walk's bookkeeping against the direct walk, bit for bit.

Around its candidate loops the staged walk of `k_density` / `k_force` (csrc/sph_pairs.hip) keeps trip counts for the part of a
row every lane has and for the ragged tail, cuts a row into pieces of 128 staged candidates and a lane's part of a piece into
chunks of 32, carries its LDS position from chunk to chunk and from there into the collision drain, and requests the next piece
while the current one is walked.  The direct walk (`sph_set_direct_hull(0)`: every lane gathers its own candidates) runs the same
arithmetic on the same candidates in the same order and uses none of that, so the two must agree in every bit.

The box is built so that rows are ragged in every way that bookkeeping distinguishes: empty cells beside cells of 1, 7, 8, 9,
33, 45, 64 and 70 particles (a lane's row is up to 167 candidates: a second piece, six chunks), range starts of both parities
(the two z-pair copies of `k_density`), a last wave with idle lanes, particles in the grid's first and last cell of every axis,
coincident particles, and -- 70 particles in a cell of two collision ranges' edge -- close pairs with approaching and with
separating velocities in every chunk of the long rows, so lanes leave the tail while others still collect collision bits."""
import numpy as np
import pytest

from conftest import bits
from gpufluidsimulator_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
DT = 5e-7
NEVER = 0xFFFFFFFF
BOX, GRID = (2.0, 2.0, 2.0), (32, 32, 32)
# particles per cell along an x-row (cyclic, rotated from row to row); (cy, cz) of the occupied rows: three clumps of
# neighbouring rows, at the low corner, in the middle and at the high corner of the grid
COUNTS = (0, 1, 7, 8, 9, 33, 70, 64, 8, 0, 45, 9, 1, 0, 0, 7)
ROWS = ((0, 0), (1, 0), (0, 1), (1, 1), (15, 16), (16, 16), (17, 16), (16, 17), (30, 31), (31, 31), (31, 30))
SPHERE = dict(centers=[[-0.35, 0.02, 0.05]], radii=[0.22], velocities=[[40.0, -10.0, 5.0]])


def _ragged_box():
    rng = np.random.default_rng(20261)
    edge = BOX[0] / GRID[0]
    per_cell = np.zeros(GRID[::-1], np.int64)                                  # [cz, cy, cx]
    for i, (cy, cz) in enumerate(ROWS):
        per_cell[cz, cy] = np.roll(np.tile(COUNTS, 2), 3 * i)
    per_cell[0, 0, 0] = max(per_cell[0, 0, 0], 7)                               # the grid's first and last cell
    per_cell[31, 31, 31] = max(per_cell[31, 31, 31], 9)
    if per_cell.sum() % 64 == 0:
        per_cell[16, 16, 3] += 5
    cz, cy, cx = np.nonzero(per_cell)
    rep = per_cell[cz, cy, cx]
    cell = np.repeat(np.stack([cx, cy, cz], 1), rep, axis=0).astype(np.float64)
    pos = -1.0 + (cell + rng.uniform(0.05, 0.95, cell.shape)) * edge
    first = np.concatenate([[0], np.cumsum(rep)[:-1]])
    for s, k in zip(first, rep):                                                # coincident particles: twins in the crowded cells
        if k >= 33:
            pos[s + 5] = pos[s + 2]
            pos[s + k - 1] = pos[s + k - 9]
    vel = rng.uniform(-60.0, 60.0, pos.shape)
    order = rng.permutation(pos.shape[0])                                      # creation order is not slot order
    return pos[order].astype(F), vel[order].astype(F), per_cell


@pytest.fixture(scope="module")
def ragged():
    pos, vel, per_cell = _ragged_box()
    n = pos.shape[0]
    # what the docstring promises, from the construction itself (keys are x-fastest: slot order = flat order of per_cell)
    flat = per_cell.reshape(-1)
    start = np.concatenate([[0], np.cumsum(flat)[:-1]])[flat > 0]
    assert 3000 <= n <= 8000 and n % 64 != 0
    assert {1, 7, 8, 9, 33, 45, 64, 70} <= set(flat.tolist()) and (flat == 0).any()
    assert (start % 2 == 0).any() and (start % 2 == 1).any()
    rows3 = per_cell[:, :, :-2] + per_cell[:, :, 1:-1] + per_cell[:, :, 2:]
    assert rows3.max() > 128 and ((rows3 > 32) & (rows3 <= 128)).any()
    assert per_cell[0, 0, 0] > 0 and per_cell[31, 31, 31] > 0
    return pos, vel


def _run(pos, vel, direct_hull, collider, threads):
    with capi.Context(pos.shape[0], box=BOX, grid=GRID) as c:
        c.set_direct_hull(direct_hull)
        c.set_pair_small_launch(NEVER if threads == 128 else 0)
        if collider != "none":
            c.set_colliders(**SPHERE)
        if collider == "tracked":
            c.set_collider_bodies([0.0])
        c.upload(pos, vel)
        c.hash(); c.sort(); c.build_cells(); c.density(); c.force(); c.collide()
        out = dict(c.download(want=("density", "pressure")), **c.download_forces())
        c.step(DT, 2)
        out.update({k + "_2": v for k, v in c.download().items()})
    return out


def _same(a, b, what):
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])) if a[k].dtype == np.float32 else np.array_equal(a[k], b[k]), (what, k)


_FIRST = {}          # per collider kind: the first staged result of the session; every other form must give its bits


@pytest.mark.parametrize("threads", [128, 256])
@pytest.mark.parametrize("collider", ["none", "sphere", "tracked"])
@pytest.mark.parametrize("clamp", ["clamp", "v_max"])
def test_staged_and_direct_walks_agree_on_ragged_rows(monkeypatch, ragged, clamp, collider, threads):
    pos, vel = ragged
    if clamp == "clamp":
        monkeypatch.delenv("SPH_PAIR_CLAMP", raising=False)
    else:
        monkeypatch.setenv("SPH_PAIR_CLAMP", "0")
    staged = _run(pos, vel, NEVER, collider, threads)
    direct = _run(pos, vel, 0, collider, threads)
    for k, v in staged.items():
        assert np.isfinite(v).all() if v.dtype == np.float32 else (v >= 0).all(), k
    assert staged["count"].max() >= 3 and (staged["count"] == 0).any(), "collisions in some lanes of a wave and none in others"
    assert float(staged["pressure"].max()) > 0 and float(np.abs(staged["fpress"]).max()) > 0
    _same(staged, direct, "staged vs direct")
    # the form of the r < h cut and the workgroup size change no bit either
    _same(staged, _FIRST.setdefault(collider, staged), "against the session's first form")


def test_the_sphere_moves_particles(ragged):
    """The collider cases are not the plain case again: the sphere reaches particles of the middle clump."""
    pos, vel = ragged
    plain = _run(pos, vel, NEVER, "none", 128)
    sphere = _run(pos, vel, NEVER, "sphere", 128)
    assert not np.array_equal(bits(plain["pos_2"]), bits(sphere["pos_2"]))
    _same({k: plain[k] for k in ("density", "pressure", "fpress", "fvisc", "dv", "count")}, sphere, "phases before the first integrate")

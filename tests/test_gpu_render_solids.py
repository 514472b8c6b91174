"""GPU: the solids in the picture (sph_render_set_solids; include/sph_hip.h: THE RULE) against the numpy model of
tests/solid_render_model.py, BIT FOR BIT in every plane: RGBA, id, depth, and for the surface the normals, raw depth and
thickness too.  The model is fed with what the device reports -- each slot's grid, field, advanced offset and pose, and the
particles as sph_download_owned returns them -- so that model and device perform the same IEEE fp32 operations on the same words.
The scenes are tests/solid_render_cases.py's; tests/test_solid_render_model_cpu.py holds them to the step budget."""
import contextlib
import ctypes as C
import gc

import numpy as np
import pytest

import render_model as rm
import solid_render_cases as sc
import solid_render_model as so
import surface_model as sm
from gpufluidsimulator_amd import capi

pytestmark = pytest.mark.gpu
F = np.float32
BG = (10, 20, 30, 255)
E_INVALID, E_STATE = -1, -5
BAND = 65536
SURFACE = dict(smooth_radius_px=3, smooth_iterations=2)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


def _same(got, want, what=""):
    """dicts of planes by name: the same bits in every plane (every count printed before anything is asserted)"""
    assert set(got) == set(want)
    for k in sorted(got):
        assert got[k].shape == want[k].shape, f"{what}: {k}"
        print(f"{what}: {k}: {int((_bits(got[k]) != _bits(want[k])).sum())} of {got[k].size} words differ")
    for k in sorted(got):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), f"{what}: {k}"


def _code(fn, *args, **kw):
    with pytest.raises(capi.SphError) as e:
        fn(*args, **kw)
    return int(str(e.value).split("error ")[1].split(":")[0])


def _ctx(capacity=4096, **kw):
    return capi.Context(capacity, box=sc.BOX, grid=sc.GRID, **kw)


def _shape(sh):
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    return capi.Shape(int(sh["kind"]), int(sh["invert"]), f3(sh["a"]), f3(sh["b"]), float(sh["r"]))


def _install(c, solids):
    for k in sorted(solids, reverse=True):
        sd = solids[k]
        bounds = sd["bounds"] or (sc.BMIN, sc.BMAX)
        if sd["mesh"] is not None:
            v, t, band, invert = sd["mesh"]
            c.build_obstacle_mesh(v, t, sd["spacing"], band, invert, bounds, slot=k)
        else:
            c.build_obstacle([_shape(s) for s in sd["shapes"]], sd["spacing"], bounds, slot=k)
        c.set_obstacle_motion(offset=sd["off"], velocity=sd["u"], slot=k)
        if sd["pivot"] is not None:
            c.set_obstacle_pose(sd["pivot"], sd["quat"], sd["omega"], slot=k)


def _style(solids, light=so.DEFAULT_LIGHT, ambient=so.DEFAULT_AMBIENT):
    return capi.solid_defaults(looks={k: sd["look"] for k, sd in solids.items()}, light=light, ambient=ambient)


def _device_slots(c, solids):
    """The model's slots from what the device holds NOW: grid, field, offset, pose."""
    out = {}
    for k, sd in solids.items():
        ob, ps = c.obstacle(read=True, slot=k), c.obstacle_pose(slot=k)
        pose = None if ps is None else {"pivot": ps["pivot"], "q": ps["quat"], "omega": ps["omega"]}
        assert (pose is None) == (sd["pivot"] is None)
        out[k] = sc.model_slot(sd, {"dims": ob["dims"], "origin": ob["origin"], "spacing": ob["spacing"]}, ob["phi"], ob["offset"], pose)
    return out


def _particles(c):
    if c.n == 0:
        return np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros(0, np.uint32)
    return c.download_owned()


def _sprites(c, cam, sol):
    """(device planes, model planes, win) of one sph_render with solids"""
    pos, vel, idx = _particles(c)
    c.render(cam, background=BG)
    got = dict(zip(("rgba", "id", "depth"), c.read_image()))
    fluid = rm.render(pos, cam, vel=vel, index=idx, radius=c.params.particle_radius, background=BG)
    rgba, ident, depth, win = so.compose_render(fluid, sol)
    return got, dict(rgba=rgba, id=ident, depth=depth), win


def _surface(c, cam, sol, **surface):
    """(device planes, model planes, model namespace) of one sph_render_surface with solids"""
    pos, vel, idx = _particles(c)
    surface = dict(SURFACE, **surface)
    c.render_surface(cam, capi.surface_defaults(**surface), background=BG)
    got = dict(zip(("rgba", "id", "depth"), c.read_image()))
    got.update(zip(("raw", "thick", "normal"), c.read_surface()))
    sf = sm.surface_style(**surface)
    r = sm.render(pos, cam, sf, vel=vel, index=idx, radius=c.params.particle_radius, background=BG)
    out = so.compose_surface(r, cam, sf, sol, background=BG, radius=c.params.particle_radius)
    return got, {k: getattr(out, k) for k in got}, out


@pytest.fixture(scope="module")
def fluid_sol():
    """the model's march of the fluid scenes' solid through their camera, marched once; left unchanged"""
    return so.march(sc.FLUID_CAM(), {0: sc.fluid_slot()})


@pytest.mark.parametrize("name", [n for n in sc.SCENES if n != "two_slots"])
def test_solids_alone(name):
    """No particle: every scene through both renderers.  (The budget scene's exhausted rays miss on the device as in the model.)"""
    cam, solids, light, ambient = sc.SCENES[name]
    cam = cam()
    with _ctx(64) as c:
        _install(c, solids)
        c.set_render_solids(_style(solids, light, ambient))
        sol = so.march(cam, _device_slots(c, solids), light, ambient)
        print(name, "hit", int(sol.hit.sum()), "of", sol.hit.size, "exhausted", {k: int(s["exhausted"].sum()) for k, s in sol.stats.items()})
        assert sol.hit.any() and not sol.hit.all()
        got, want, win = _sprites(c, cam, sol)
        assert np.array_equal(win, sol.hit)
        _same(got, want, name + " sprites")
        assert (got["id"][win] == so.ID_SOLID + next(iter(solids))).all() and (got["id"][~win] == 0xFFFFFFFF).all()
        got, want, _ = _surface(c, cam, sol)
        _same(got, want, name + " surface")
        assert np.array_equal(_bits(got["normal"][win]), _bits(sol.ne[win]))


def test_two_slots_after_three_steps():
    """Slot 1 posed about a skew axis, slot 3 offset, overlapping; slot 0 in front of both with draw = 0.  Three steps first:
    offset and pose are the advanced ones."""
    cam, solids, light, ambient = sc.SCENES["two_slots"]
    cam = cam()
    with _ctx(64) as c:
        c.upload(np.array([[-0.9, -0.9, -0.9], [-0.85, -0.9, -0.9]], F))
        _install(c, solids)
        c.set_render_solids(_style(solids, light, ambient))
        c.step(sc.DT, 3)
        slots = _device_slots(c, solids)
        assert not np.array_equal(slots[3]["off"], np.array(solids[3]["off"], F))
        assert not np.array_equal(slots[1]["pose"]["q"], sc.pose_of(solids[1])["q"])
        sol = so.march(cam, slots, light, ambient)
        both = so.march(cam, {k: dict(s, draw=1) for k, s in slots.items()}, light, ambient)
        assert set(np.unique(sol.slot[sol.hit])) == {1, 3} and (both.slot[both.hit] == 0).sum() > 100   # slot 0 would have shown
        got, want, win = _sprites(c, cam, sol)
        _same(got, want, "two slots, sprites")
        assert not (got["id"] == so.ID_SOLID).any()
        got, want, _ = _surface(c, cam, sol)
        _same(got, want, "two slots, surface")


def test_fluid_in_front_of_behind_and_touching_a_solid(fluid_sol):
    """sph_render: the strict z_s < d decision pixel by pixel, and every pixel the solid does not win is the image with solids off."""
    cam, solids = sc.FLUID_CAM(), {0: sc.FLUID_SOLID}
    with _ctx() as c:
        c.upload(sc.fluid_particles())
        _install(c, solids)
        c.render(cam, background=BG)
        off = dict(zip(("rgba", "id", "depth"), c.read_image()))
        c.set_render_solids(_style(solids))
        sol = so.march(cam, _device_slots(c, solids))
        _same({"z": sol.z}, {"z": fluid_sol.z}, "the device's field is the model's")
        got, want, win = _sprites(c, cam, sol)
        covered = np.isfinite(off["depth"])
        print("solid in front", int((win & covered).sum()), "behind", int((sol.hit & covered & ~win).sum()), "alone", int((win & ~covered).sum()))
        assert (win & covered).sum() > 100 and (sol.hit & covered & ~win).sum() > 100 and (win & ~covered).sum() > 100
        _same(got, want, "fluid and solid, sprites")
        for k in off:
            assert np.array_equal(_bits(got[k][~win]), _bits(off[k][~win])), k
        assert (got["depth"][win] < off["depth"][win]).all()


@pytest.mark.parametrize("absorb", [(6.0, 2.0, 0.5), (0.0, 0.0, 0.0)])
def test_fluid_and_solid_through_the_surface(fluid_sol, absorb):
    """sph_render_surface: the blocks in front of, behind and on the solid, then a thin sheet the solid shows through by its
    thickness -- and not at all with absorb = 0, where tr = 0."""
    cam, solids = sc.FLUID_CAM(), {0: sc.FLUID_SOLID}
    with _ctx() as c:
        _install(c, solids)
        c.set_render_solids(_style(solids))
        for what, pos in (("blocks", sc.fluid_particles()), ("sheet", sc.thin_sheet())):
            c.upload(pos)
            got, want, out = _surface(c, cam, fluid_sol, absorb=absorb)
            print(what, "solid wins", int(out.win.sum()), "shows through", int(out.through.sum()))
            assert out.through.sum() > 100 and (out.win.sum() > 100 or what == "sheet")     # (the sheet hides most of the solid)
            _same(got, want, f"{what}, absorb {absorb}")
            c.set_render_solids(None)
            c.render_surface(cam, capi.surface_defaults(**dict(SURFACE, absorb=absorb)), background=BG)
            plain = c.read_image()[0]
            c.set_render_solids(_style(solids))
            changed = (plain != got["rgba"]).any(axis=2)
            assert not changed[~out.win & ~out.through].any()
            if any(absorb):
                assert changed[out.through].any()
            else:
                assert not changed[out.through].any()


def test_solids_off_is_the_library_without_them():
    """With obstacles installed: after set_render_solids(None) both images are those from before a style was ever set, and a
    context whose style was set and dropped allocates what one that never had it allocates."""
    cam, solids = sc.FLUID_CAM(), {0: sc.FLUID_SOLID}

    def images(c):
        c.render(cam, background=BG)
        a = c.read_image()
        c.render_surface(cam, capi.surface_defaults(**SURFACE), background=BG)
        return a + c.read_image() + c.read_surface()

    gc.collect()
    base = capi.memory_stats()
    with _ctx() as c:
        c.upload(sc.fluid_particles())
        _install(c, solids)
        assert c.render_solids() is None
        before = images(c)
        never = capi.memory_stats()
        c.set_render_solids(_style(solids))
        assert capi.memory_stats() == never                      # setting the style allocates nothing
        c.render(cam, background=BG)
        assert capi.memory_stats() == never                      # ... nor does sph_render with solids
        c.render_surface(cam, capi.surface_defaults(**SURFACE), background=BG)
        with_planes = capi.memory_stats()
        assert with_planes[0] - never[0] == 20 * cam.width * cam.height and with_planes[2] - never[2] == 3
        c.set_render_solids(None)
        assert c.render_solids() is None
        after = images(c)
        for a, b in zip(before, after):
            assert np.array_equal(_bits(a), _bits(b))
        c.render(capi.look_at(64, 48), background=BG)            # another image size: the planes leave with the image
        assert capi.memory_stats()[2] == never[2] - 4
    assert capi.memory_stats() == base
    with _ctx() as c:                                            # a style with no installed slot that is drawn: nothing either
        c.upload(sc.fluid_particles())
        c.set_render_solids(capi.solid_defaults())
        empty = images(c)
        _install(c, solids)
        c.set_render_solids(capi.solid_defaults(looks={0: dict(draw=0)}))
        hidden = images(c)
        for a, b in zip(empty, hidden):
            assert np.array_equal(_bits(a), _bits(b))
        for a, b in zip(before, hidden):
            assert np.array_equal(_bits(a), _bits(b))


def test_refusals_change_nothing():
    cam, solids = sc.FLUID_CAM(), {0: sc.FLUID_SOLID}
    with _ctx() as c:
        c.upload(sc.thin_sheet())
        _install(c, solids)
        good = _style(solids, light=(0.5, 1.0, -0.2), ambient=0.4)
        c.set_render_solids(good)
        c.render(cam, background=BG)
        image = c.read_image()
        bad = [capi.solid_defaults(ambient=float("nan")), capi.solid_defaults(ambient=1.5), capi.solid_defaults(ambient=-0.1),
               capi.solid_defaults(light=(0.0, 0.0, 0.0)), capi.solid_defaults(light=(1.0, float("inf"), 0.0)),
               capi.solid_defaults(looks={2: dict(color=(0.5, 1.25, 0.5))}), capi.solid_defaults(looks={3: dict(color=(0.5, 0.5, float("nan")))}),
               capi.solid_defaults(looks={0: dict(color=(-0.01, 0.5, 0.5))})]
        for s in bad:
            assert _code(c.set_render_solids, s) == E_INVALID
            assert bytes(c.render_solids()) == bytes(good)
        for a, b in zip(image, c.read_image()):
            assert np.array_equal(_bits(a), _bits(b))
        c.render(cam, background=BG)
        for a, b in zip(image, c.read_image()):
            assert np.array_equal(_bits(a), _bits(b))
    with capi.Context(64, box=sc.BOX, grid=sc.GRID, slab=(0, 16), ghost_capacity=64) as s:
        assert _code(s.set_render_solids, capi.solid_defaults()) == E_STATE
        assert _code(s.set_render_solids, None) == E_STATE
    d = capi.solid_defaults()
    assert [(l.draw, l.open, tuple(l.color)) for l in d.slot] == [(1, 0, (F(0.72), F(0.72), F(0.75)))] * capi.MAX_OBSTACLES
    assert tuple(d.light) == (1.0, 1.0, -1.0) and d.ambient == 0.25 and capi.RENDER_ID_SOLID == so.ID_SOLID


def test_rendering_with_solids_changes_no_step():
    """step, render, render_surface, step equals step, step: no particle bit, no offset, no pose, no load."""
    solids = {k: sd for k, sd in sc.SCENES["two_slots"][1].items() if k != 0}
    cam = sc.SCENES["two_slots"][0]()
    out = []
    for render in (True, False):
        with _ctx() as c:
            c.upload(sc.fluid_particles())
            _install(c, solids)
            c.set_render_solids(_style(solids))
            c.step(sc.DT, 1)
            if render:
                c.render(cam, background=BG)
                c.render_surface(cam, capi.surface_defaults(**SURFACE), background=BG)
            c.step(sc.DT, 1)
            out.append(c.download_owned() + (c.obstacle(slot=3)["offset"], c.obstacle_pose(slot=1)["quat"]))
    for a, b in zip(*out):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@contextlib.contextmanager
def _guard():
    gc.collect()
    capi.guard(BAND, True)
    try:
        yield
    finally:
        capi.guard(0)
        last = capi.guard_check()
    assert last[0] > 0 and last[1] == 0, last


def test_the_march_stores_nothing_outside_its_buffers():
    """Guard bands around every allocation, the pattern in every range: a ragged image (67 x 45: partial tiles on both edges)
    through both renderers, the same bits as without the bands, every band clean."""
    cam, solids, light, ambient = sc.SCENES["ragged_tiles"]
    cam = cam()
    planes = []
    for guarded in (False, True):
        with (_guard() if guarded else contextlib.nullcontext()):
            with _ctx() as c:
                c.upload(sc.thin_sheet())
                _install(c, solids)
                c.set_render_solids(_style(solids, light, ambient))
                c.render(cam, background=BG)
                a = c.read_image()
                c.render_surface(cam, capi.surface_defaults(**SURFACE), background=BG)
                planes.append(a + c.read_image() + c.read_surface())
                if guarded:
                    checked = capi.guard_check()
                    assert checked[0] > 0 and checked[1] == 0, checked
    assert (planes[0][1] >= so.ID_SOLID).any()
    for a, b in zip(*planes):
        assert np.array_equal(_bits(a), _bits(b))

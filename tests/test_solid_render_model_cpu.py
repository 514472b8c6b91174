"""CPU: the numpy model of the solids in the picture (tests/solid_render_model.py; include/sph_hip.h: sph_render_set_solids) held
to what it models -- a sphere's exact ray intersections from two cameras, the step budget of every scene the GPU tests render, the
zero direction components of an axis-aligned camera -- and to the models it stands on: its fluid shading over a constant colour
is surface_model's."""
import numpy as np
import pytest

import render_model as rm
import solid_render_cases as sc
import solid_render_model as so
import surface_model as sm

F = np.float32


@pytest.fixture(scope="module")
def marched():
    """every scene marched once, by name: (camera, slots, planes); shared and left unchanged"""
    out = {}
    for name, (cam, _, light, ambient) in sc.SCENES.items():
        slots = sc.model_slots(name)
        out[name] = (cam(), slots, so.march(cam(), slots, light, ambient))
    return out


def _exact_sphere(cam, centre, radius):
    """float64: (closest approach of every ray to the centre, the depth z of its first intersection with the sphere)"""
    ex, ey, le, O, D = so.rays(cam)
    O = np.array([float(o) for o in O])
    D = np.stack([d.astype(np.float64) for d in D], axis=1)
    oc = O - np.asarray(centre, np.float64)
    a, b = (D * D).sum(axis=1), (D * oc).sum(axis=1)
    c = float(oc @ oc) - radius * radius
    zc = -b / a
    dist = np.linalg.norm(oc + zc[:, None] * D, axis=1)
    disc = b * b - a * c
    z = np.where(disc >= 0, (-b - np.sqrt(np.maximum(disc, 0))) / a, np.inf)
    return dist, z, le.astype(np.float64)


@pytest.mark.parametrize("name", ["sphere", "sphere_other_side"])
def test_a_sphere_is_hit_where_its_rays_pass_it(marched, name):
    """Rays that pass the centre closer than r - s hit, within s of the exact intersection along the ray; rays that pass
    farther than r + s miss; the band between is not judged."""
    cam, slots, sol = marched[name]
    sh = sc.SCENES[name][1][0]["shapes"][0]
    r, s = float(sh["r"]), float(sc.S)
    dist, z, le = _exact_sphere(cam, sh["a"], r)
    hit, zs = sol.hit.reshape(-1), sol.z.reshape(-1).astype(np.float64)
    inside, outside = dist < r - s, dist > r + s
    err = np.abs(zs[inside] - z[inside]) * le[inside]
    print(name, int(inside.sum()), "rays inside,", int(outside.sum()), "outside; worst error in spacings", float(err.max() / s))
    assert inside.sum() > 300 and outside.sum() > 300
    assert hit[inside].all()
    assert (err <= s).all()
    assert not hit[outside].any()


def test_step_budget_of_every_scene(marched):
    """No ray that enters a grid uses up SPH_SOLID_MAX_STEPS, but in the one scene built for that."""
    for name, (_, slots, sol) in marched.items():
        for k, st in sol.stats.items():
            worst, spent = int(st["steps"].max()), int(st["exhausted"].sum())
            print(name, k, "entered", int(st["entered"].sum()), "most samples", worst, "exhausted", spent)
            assert st["entered"].any()
            assert not (st["exhausted"] & ~st["entered"]).any()
            if name in sc.EXHAUSTS:
                assert spent >= 1 and worst == so.MAX_STEPS
                assert not sol.hit.reshape(-1)[st["exhausted"]].any()           # a ray that uses up the steps misses
                assert sol.hit.any() and (~sol.hit).any()
            else:
                assert spent == 0 and worst < so.MAX_STEPS


def test_scenes_show_what_they_are_for(marched):
    hit = {name: m[2].hit for name, m in marched.items()}
    for name in sc.SCENES:
        assert 0.02 < hit[name].mean() < 1.0 or name == "bowl_closed", name
    two = marched["two_slots"][2]
    assert set(np.unique(two.slot[two.hit])) == {1, 3}                          # both drawn slots win pixels; slot 0 never
    closed, opened = marched["bowl_closed"][2], marched["bowl_open"][2]
    assert (opened.z[opened.hit & closed.hit] > closed.z[opened.hit & closed.hit] + 0.5).all()   # the far wall, not the box face
    fallback = marched["mesh_band3_inverted"][2]
    cam = marched["mesh_band3_inverted"][0]
    rot = np.array(list(cam.rot), F)
    up = np.array([rot[1], rot[4], rot[7]], F)                                  # the eye-space image of (0, 1, 0)
    flat = (fallback.ne == up).all(axis=2) & fallback.hit
    print("fallback normals:", int(flat.sum()), "of", int(fallback.hit.sum()))
    assert flat.sum() > 100 and np.array_equal(flat, fallback.hit)              # every ray meets the flat -W at the box face


def test_zero_direction_components_agree_with_a_nudged_camera(marched):
    """65 x 49 through the axis-aligned camera: ex = 0 on column 32 and ey = 0 on row 24 exactly, so D has zero components and
    the clip divides by zero.  The hits equal those of a camera nudged by one ulp, outside the band that is not judged."""
    cam, slots, sol = marched["axis_aligned"]
    ex, ey, _, _, D = so.rays(cam)
    ex, ey = ex.reshape(49, 65), ey.reshape(49, 65)
    assert (ex[:, 32] == 0).all() and (ey[24, :] == 0).all()
    assert (D[0].reshape(49, 65)[:, 32] == 0).all() and (D[1].reshape(49, 65)[24, :] == 0).all()
    nudged = rm.camera(cam.width, cam.height, list(cam.rot), [np.nextafter(F(cam.trans[0]), F(1)), np.nextafter(F(cam.trans[1]), F(1)),
                                                              cam.trans[2]], cam.focal_px, cam.near_z, cam.far_z)
    other = so.march(nudged, slots)
    sh = sc.SCENES["axis_aligned"][1][0]["shapes"][0]
    dist, _, _ = _exact_sphere(cam, sh["a"], float(sh["r"]))
    judged = (np.abs(dist - float(sh["r"])) > float(sc.S)).reshape(49, 65)
    centre = np.zeros((49, 65), bool)
    centre[:, 32] = centre[24, :] = True
    assert (judged & centre).sum() > 60 and (sol.hit & centre).sum() > 10 and (~sol.hit & centre & judged).sum() > 10
    assert np.array_equal(sol.hit[judged], other.hit[judged])
    both = judged & sol.hit
    assert (np.abs(sol.z[both] - other.z[both]) <= 1e-5).all()


def test_compositions():
    """The strict depth test of both compositions on hand-made planes, and the fluid shading over a constant colour is
    surface_model's own."""
    cam = sc.FLUID_CAM()
    slot = sc.fluid_slot()
    sol = so.march(cam, {0: slot})
    pos = sc.fluid_particles()
    fluid = rm.render(pos, cam, background=(10, 20, 30, 255))
    rgba, ident, depth, win = so.compose_render(fluid, sol)
    covered = np.isfinite(fluid[2])
    print("solid in front of fluid", int((win & covered).sum()), "behind it", int((sol.hit & covered & ~win).sum()), "alone", int((win & ~covered).sum()))
    assert (win & covered).sum() > 100 and (sol.hit & covered & ~win).sum() > 100 and (win & ~covered).sum() > 100
    assert (ident[win] == so.ID_SOLID).all() and np.array_equal(depth[win], sol.z[win])
    for got, was in zip((rgba, ident, depth), fluid):
        assert np.array_equal(got[~win], was[~win])
    tie = (fluid[0], fluid[1], np.where(sol.hit, sol.z, fluid[2]))                 # equal depths: the fluid keeps the pixel
    assert not so.compose_render(tie, sol)[3][covered].any()
    sf = sm.surface_style(smooth_radius_px=3, smooth_iterations=2)
    r = sm.render(sc.thin_sheet(), cam, sf, background=(10, 20, 30, 255))
    bg = np.empty(r.depth.shape + (3,), F)
    bg[:] = np.array([F(10) / F(255), F(20) / F(255), F(30) / F(255)], F)
    assert np.array_equal(so.fluid_rgba(r, cam, sf, bg), r.rgba)
    out = so.compose_surface(r, cam, sf, sol, background=(10, 20, 30, 255))
    assert out.through.sum() > 100 and (out.rgba[out.through] != r.rgba[out.through]).any()
    assert np.array_equal(out.rgba[~out.through & ~out.win], r.rgba[~out.through & ~out.win])
    none = sm.surface_style(smooth_radius_px=3, smooth_iterations=2, absorb=(0.0, 0.0, 0.0))
    r0 = sm.render(sc.thin_sheet(), cam, none, background=(10, 20, 30, 255))
    out0 = so.compose_surface(r0, cam, none, sol, background=(10, 20, 30, 255))
    assert out0.through.sum() > 100 and np.array_equal(out0.rgba[out0.through], r0.rgba[out0.through])   # tr = 0: nothing shows

"""numpy float32 model of the region membership of include/sph_hip.h (sph_remove, sph_count_in_regions): every operation
rounded to fp32, no multiply-add fusion, sums left to right -- the arithmetic of in_regions in csrc/sph_edit.hip, so that
model and device decide every particle identically.  Regions are tuples:
    ("sphere", centre, radius)   ("box", lo, hi)   ("halfspace", point, normal)"""
import numpy as np

KINDS = {"sphere": 0, "box": 1, "halfspace": 2}
MAX_REGIONS = 8
f32 = np.float32


def _in_one(pos, region):
    kind = region[0]
    if kind not in KINDS:
        raise ValueError(f"unknown region kind {kind!r}")
    x, y, z = (np.asarray(pos[:, k], dtype=f32) for k in range(3))
    a = np.asarray(region[1], dtype=f32)
    if not np.isfinite(a).all():
        raise ValueError("region field is not finite")
    if kind == "sphere":
        r = f32(region[2])
        if not np.isfinite(r):
            raise ValueError("region field is not finite")
        dx, dy, dz = x - a[0], y - a[1], z - a[2]
        d2 = (dx * dx + dy * dy).astype(f32) + dz * dz          # numpy rounds every float32 operation
        return d2.astype(f32) < f32(r * r)
    b = np.asarray(region[2], dtype=f32)
    if not np.isfinite(b).all():
        raise ValueError("region field is not finite")
    if kind == "box":
        return (a[0] <= x) & (x < b[0]) & (a[1] <= y) & (y < b[1]) & (a[2] <= z) & (z < b[2])
    s = ((x - a[0]) * b[0] + (y - a[1]) * b[1]).astype(f32) + (z - a[2]) * b[2]
    return s.astype(f32) < f32(0.0)


def selected(pos, regions):
    """Boolean mask over pos (n, 3): inside ANY of the 1..8 regions."""
    regions = list(regions)
    if not 1 <= len(regions) <= MAX_REGIONS:
        raise ValueError(f"{len(regions)} regions (1..{MAX_REGIONS})")
    pos = np.asarray(pos, dtype=f32).reshape(-1, 3)
    out = np.zeros(pos.shape[0], dtype=bool)
    for r in regions:
        out |= _in_one(pos, r)
    return out


def to_capi(regions):
    """The same regions as gpufluidsimulator_amd.capi.Region structs."""
    from gpufluidsimulator_amd import capi
    make = {"sphere": capi.Region.sphere, "box": capi.Region.box, "halfspace": capi.Region.halfspace}
    return [make[r[0]](r[1], r[2]) for r in regions]

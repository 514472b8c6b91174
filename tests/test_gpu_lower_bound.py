"""GPU: the library's binary search (first_not, csrc/sph_device.hpp) through the test hook sph_test_lower_bounds, which runs the
lower-bounds kernel of the slab messages (csrc/sph_halo.hip) on keys of the caller's, against numpy.searchsorted(keys, targets,
"left"): integers, so every answer must be equal exactly.  The layer bounds of a slab, the merges of arrivals and ghosts, the
sorts' ranks and the voxeliser's work list run the same function; the sorts' comparator searches over (key, slot) pairs cannot
be reached from here and stay with test_gpu_sort_merge.py and test_gpu_sort_reference.py."""
import numpy as np
import pytest

from gpufluidsimulator_amd import capi

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
# nothing, one key, the first sizes at which a midpoint can be off by one; either side of a wave and of 2^12 (a search of
# exactly 12 rounds, and one round more)
SIZES = [0, 1, 2, 3, 63, 64, 65, 4095, 4096, 4097]
SMALL = 65               # up to here EVERY distinct key (and that key + 1) is a target, beyond: a seeded sample of 32 of them
PER_CALL = 32            # targets the hook takes at a time


def _equal(value):
    return lambda n, rng: np.full(n, value, np.uint32)


def _dense_from_0(n, rng):           # 0, 1, 2, ...: key + 1 is the next key
    return np.arange(n, dtype=np.uint32)


def _dense_to_max(n, rng):           # ..., 2^32 - 2, 2^32 - 1
    return (MAX - (n - 1) + np.arange(n, dtype=np.uint64)).astype(np.uint32)


def _distinct(m, rng):
    """m distinct values in ascending order; with more than one of them the first is 0 and the last 2^32 - 1."""
    v = np.unique(rng.integers(1, MAX, 2 * m + 8, dtype=np.uint64))[:m]
    assert v.size == m
    if m >= 2:
        v[0], v[-1] = 0, MAX
    return v


def _spread(n, rng):                 # strictly increasing with random gaps
    return _distinct(n, rng).astype(np.uint32)


def _runs(n, rng):                   # runs of equal keys, 1 to 130 long: shorter and longer than a wave
    lengths = []
    while sum(lengths) < n:
        lengths.append(int(rng.integers(1, 131)))
    if lengths:
        lengths[-1] -= sum(lengths) - n
    return np.repeat(_distinct(len(lengths), rng), lengths).astype(np.uint32)


FAMILIES = {"equal_0": _equal(0), "equal_7": _equal(7), "equal_max": _equal(MAX), "dense_from_0": _dense_from_0,
            "dense_to_max": _dense_to_max, "spread": _spread, "runs": _runs}


def _targets(keys, rng):
    t = [0, MAX]
    if keys.size:
        distinct = np.unique(keys).astype(np.uint64)
        lo, hi = int(distinct[0]), int(distinct[-1])
        t += [lo, hi] + ([lo - 1] if lo > 0 else []) + ([hi + 1] if hi < MAX else [])
        chosen = distinct if keys.size <= SMALL else rng.choice(distinct, min(32, distinct.size), replace=False)
        for k in chosen.tolist():
            t += [k] + ([k + 1] if k < MAX else [])
    return rng.permutation(np.unique(np.array(t, np.uint64))).astype(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    with capi.Context(64, box=(2.0, 2.0, 2.0), grid=(32, 32, 32)) as c:
        yield c


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("n", SIZES)
def test_lower_bounds_are_numpys(ctx, n, family):
    rng = np.random.default_rng(3000 + 16 * n + sorted(FAMILIES).index(family))
    keys = FAMILIES[family](n, rng)
    assert keys.dtype == np.uint32 and keys.shape == (n,) and np.all(keys[1:] >= keys[:-1])
    if family in ("dense_from_0", "dense_to_max", "spread"):
        assert np.all(keys[1:] > keys[:-1])
    targets = _targets(keys, rng)
    assert 0 in targets and MAX in targets
    if n > SMALL and not family.startswith("equal"):
        assert targets.size > 32                      # the sample of 32 keys, most of them with their key + 1
    for first in range(0, targets.size, PER_CALL):
        tg = targets[first:first + PER_CALL]
        got = ctx.test_lower_bounds(keys, tg)
        want = np.searchsorted(keys, tg, "left")
        assert got.dtype == np.uint32 and np.array_equal(got, want), (family, n, tg, got, want)


def test_the_families_hold_both_ends_of_the_key_range():
    rng = np.random.default_rng(5)
    for name in ("spread", "runs"):
        keys = FAMILIES[name](4097, rng)
        assert keys[0] == 0 and keys[-1] == MAX
    assert _runs(4097, rng).size == 4097 and np.unique(_runs(4097, rng)).size < 4097
    assert _dense_to_max(3, rng).tolist() == [MAX - 2, MAX - 1, MAX]


def test_no_targets_and_too_many(ctx):
    keys = np.arange(10, dtype=np.uint32)
    assert ctx.test_lower_bounds(keys, np.zeros(0, np.uint32)).size == 0
    with pytest.raises(capi.SphError):
        ctx.test_lower_bounds(keys, np.zeros(PER_CALL + 1, np.uint32))

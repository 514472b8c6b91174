"""numpy statement of what the particle sort must produce -- TEST INFRASTRUCTURE, no GPU code.

The library sorts particles by cell key, stably: equal keys keep the order they had before the sort (csrc/sph_sort.hip).  The
first sort after an upload orders the upload positions; every later one re-sorts the slots of the previous order under the new
keys ("identical, element for element, to the full stable radix sort").  Both are one `argsort(kind="stable")`
here, and nothing in this module looks at anything the library returns.

Particles are put at cell CENTRES, so the key a position hashes to is `(z * gy + y) * gx + x` of the integer cell it was
made from -- no float rounding decides a cell.  The key distributions below are the shapes a radix sort can get wrong: every key
in one digit bucket, only the lowest or only the highest digit varying, sorted and reversed input, two buckets at the far ends.
"""
import numpy as np


def keys_of(cells_xyz, grid):
    """Cell key `(z * gy + y) * gx + x` (uint32) of integer cell coordinates (n, 3)."""
    c = np.asarray(cells_xyz, np.int64).reshape(-1, 3)
    gx, gy, gz = (int(g) for g in grid)
    assert c.min(initial=0) >= 0 and np.all(c < np.array([gx, gy, gz])), "cell outside the grid"
    return ((c[:, 2] * gy + c[:, 1]) * gx + c[:, 0]).astype(np.uint32)


def cells_of(keys, grid):
    """Inverse of keys_of."""
    k = np.asarray(keys, np.int64)
    gx, gy = int(grid[0]), int(grid[1])
    return np.stack([k % gx, (k // gx) % gy, k // (gx * gy)], axis=1)


def cell_centres(cells_xyz, box, grid):
    """float32 positions (n, 3) at the centres of the given integer cells of a box centred on the origin (sph_default_params).
    Computed in float64 and rounded once: the rounding error is ~1e-7 of the position, a cell's half edge away from any face."""
    c = np.asarray(cells_xyz, np.float64).reshape(-1, 3)
    box = np.asarray(box, np.float64).reshape(3)
    grid = np.asarray(grid, np.float64).reshape(3)
    return (-box / 2.0 + (c + 0.5) * (box / grid)).astype(np.float32)


# ---- key distributions over a grid: (n, grid, seed) -> integer cell coordinates (n, 3) -------------------------------------
def _interior(grid):
    return np.array([int(g) // 2 for g in grid], np.int64)


def uniform(n, grid, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, int(g), n) for g in grid], axis=1).astype(np.int64)


def one_cell(n, grid, seed):
    """All n in one interior cell: every tile of every pass holds a single digit."""
    return np.tile(_interior(grid), (n, 1))


def two_extremes(n, grid, seed):
    """Alternating between cell 0 and the last cell: keys 0 and ncells - 1, every digit at one of its two ends."""
    out = np.zeros((n, 3), np.int64)
    out[1::2] = np.array([int(g) - 1 for g in grid], np.int64)
    return out


def low_digit_only(n, grid, seed):
    """Only x varies, within 256 cells: the higher digits of all keys are equal."""
    rng = np.random.default_rng(seed)
    out = np.tile(_interior(grid), (n, 1))
    out[:, 0] = rng.integers(0, min(256, int(grid[0])), n)
    return out


def high_digit_only(n, grid, seed):
    """Only z varies: the lower digits of all keys are equal."""
    rng = np.random.default_rng(seed)
    out = np.tile(_interior(grid), (n, 1))
    out[:, 2] = rng.integers(0, int(grid[2]), n)
    return out


def ascending(n, grid, seed):
    """Uniform keys, already sorted."""
    return cells_of(np.sort(keys_of(uniform(n, grid, seed), grid), kind="stable"), grid)


def descending(n, grid, seed):
    """Uniform keys, sorted and reversed."""
    return ascending(n, grid, seed)[::-1].copy()


def skewed(n, grid, seed):
    """90 % in one interior cell (at random upload positions), the rest uniform."""
    rng = np.random.default_rng(seed)
    out = uniform(n, grid, seed + 1)
    heavy = rng.permutation(n)[: n - n // 10]
    out[heavy] = _interior(grid)
    return out


DISTRIBUTIONS = {f.__name__: f for f in (uniform, one_cell, two_extremes, low_digit_only, high_digit_only, ascending,
                                         descending, skewed)}


# ---- the expected results ---------------------------------------------------------------------------------------------------
def full_sort_expected(keys_by_upload_pos, index):
    """First sort after an upload: (sorted_keys, order), order[slot] = creation index of the particle in that slot.
    Equal keys stay in upload order."""
    keys = np.asarray(keys_by_upload_pos, np.uint32)
    index = np.asarray(index, np.uint32)
    perm = np.argsort(keys, kind="stable")
    return keys[perm], index[perm]


def resort_expected(prev_order, keys_by_index):
    """A later sort: the slots of the previous order (prev_order[slot] = creation index) re-sorted under the new keys
    (keys_by_index[creation index]); equal keys stay in the order of their previous slots.  Returns (sorted_keys, order)."""
    prev_order = np.asarray(prev_order, np.uint32)
    keys_in_slots = np.asarray(keys_by_index, np.uint32)[prev_order]
    perm = np.argsort(keys_in_slots, kind="stable")
    return keys_in_slots[perm], prev_order[perm]


def cells_expected(sorted_keys):
    """The cell table of a sorted key array: (key, start, count) of every occupied cell, ascending."""
    k, start, count = np.unique(np.asarray(sorted_keys, np.uint32), return_index=True, return_counts=True)
    return k.astype(np.uint32), start.astype(np.uint32), count.astype(np.uint32)

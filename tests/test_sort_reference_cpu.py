"""The numpy sort reference (tests/sort_reference.py) against pure Python, and its key distributions against what they promise.
No GPU: this is the check of the yardstick tests/test_gpu_sort_reference.py measures the library with."""
import numpy as np
import pytest

import sort_reference as sr

GRID = (64, 32, 16)
BOX = (4.0, 2.0, 1.0)


def _np_cell(p, bmin, bdim, g):
    """csrc/sph_device.hpp: cell_coord, in float32 (as tests/test_gpu_edge_cases.py states it)."""
    q = ((p.astype(np.float32) - np.float32(bmin)) / np.float32(bdim)) * np.float32(g)
    return np.clip(np.floor(q).astype(np.int64), 0, int(g) - 1)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_full_sort_expected_is_sorted_by_key_then_upload_position(seed):
    rng = np.random.default_rng(seed)
    n = 400
    keys = rng.integers(0, 7, n).astype(np.uint32)            # ~57 particles per key: ties everywhere
    index = rng.permutation(n).astype(np.uint32)
    got_keys, got_order = sr.full_sort_expected(keys, index)
    by_python = sorted(range(n), key=lambda i: (int(keys[i]), i))
    assert got_keys.tolist() == [int(keys[i]) for i in by_python]
    assert got_order.tolist() == [int(index[i]) for i in by_python]
    assert got_keys.dtype == np.uint32 and got_order.dtype == np.uint32


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_resort_expected_breaks_ties_by_previous_slot(seed):
    rng = np.random.default_rng(100 + seed)
    n = 300
    prev_order = rng.permutation(n).astype(np.uint32)         # slot -> creation index
    keys_by_index = rng.integers(0, 5, n).astype(np.uint32)
    got_keys, got_order = sr.resort_expected(prev_order, keys_by_index)
    by_python = sorted(range(n), key=lambda slot: (int(keys_by_index[prev_order[slot]]), slot))
    assert got_order.tolist() == [int(prev_order[s]) for s in by_python]
    assert got_keys.tolist() == [int(keys_by_index[prev_order[s]]) for s in by_python]
    # a chain of re-sorts never loses or duplicates a particle
    for _ in range(3):
        keys_by_index = rng.integers(0, 5, n).astype(np.uint32)
        got_keys, got_order = sr.resort_expected(got_order, keys_by_index)
        assert sorted(got_order.tolist()) == list(range(n))
        assert np.all(np.diff(got_keys.astype(np.int64)) >= 0)


def test_resort_of_unchanged_keys_is_the_identity():
    rng = np.random.default_rng(7)
    n = 256
    keys = rng.integers(0, 9, n).astype(np.uint32)
    index = rng.permutation(n).astype(np.uint32)
    k0, o0 = sr.full_sort_expected(keys, index)
    keys_by_index = np.empty(n, np.uint32)
    keys_by_index[index] = keys
    k1, o1 = sr.resort_expected(o0, keys_by_index)
    assert np.array_equal(k0, k1) and np.array_equal(o0, o1)


def test_cells_expected():
    k, s, c = sr.cells_expected(np.array([2, 2, 2, 5, 9, 9], np.uint32))
    assert k.tolist() == [2, 5, 9] and s.tolist() == [0, 3, 4] and c.tolist() == [3, 1, 2]
    k, s, c = sr.cells_expected(np.zeros(0, np.uint32))
    assert k.size == 0 and s.size == 0 and c.size == 0


def test_keys_and_cells_are_inverse_and_x_runs_fastest():
    assert sr.keys_of([[1, 0, 0], [0, 1, 0], [0, 0, 1], [63, 31, 15]], GRID).tolist() == [1, 64, 64 * 32, 64 * 32 * 16 - 1]
    cells = sr.uniform(500, GRID, 3)
    assert np.array_equal(sr.cells_of(sr.keys_of(cells, GRID), GRID), cells)
    with pytest.raises(AssertionError):
        sr.keys_of([[64, 0, 0]], GRID)


@pytest.mark.parametrize("box,grid", [(BOX, GRID), ((64.0, 64.0, 32.0), (1024, 1024, 512)), ((3.0, 5.0, 7.0), (48, 80, 112))])
def test_cell_centres_hash_back_to_their_cells(box, grid):
    """The library's float32 hash (floor(((p - min) / edge) * g)) of a centre is the cell it was made from, in every corner."""
    cells = np.concatenate([sr.uniform(2000, grid, 1), sr.two_extremes(4, grid, 0),
                            np.array([[0, grid[1] - 1, 0], [grid[0] - 1, 0, grid[2] - 1]], np.int64)])
    pos = sr.cell_centres(cells, box, grid)
    assert pos.dtype == np.float32 and pos.shape == (cells.shape[0], 3)
    back = np.stack([_np_cell(pos[:, a], -box[a] / 2, box[a], grid[a]) for a in range(3)], axis=1)
    assert np.array_equal(back, cells)


@pytest.mark.parametrize("name", sorted(sr.DISTRIBUTIONS))
def test_distributions_stay_in_the_grid_and_repeat(name):
    f = sr.DISTRIBUTIONS[name]
    for n in (1, 2, 1001):
        a = f(n, GRID, 5)
        assert a.shape == (n, 3) and a.dtype == np.int64
        assert a.min() >= 0 and np.all(a < np.array(GRID))
        assert np.array_equal(a, f(n, GRID, 5))                # the seed decides everything


def test_distributions_keep_their_promises():
    n, ncells = 5000, int(np.prod(GRID))
    interior = sr.keys_of([[g // 2 for g in GRID]], GRID)[0]
    key = lambda name, seed=11: sr.keys_of(sr.DISTRIBUTIONS[name](n, GRID, seed), GRID)

    k = key("uniform")
    assert np.unique(k).size > n // 2                          # 5000 draws from 32768 cells
    assert not np.array_equal(k, key("uniform", 12))

    assert np.unique(key("one_cell")).tolist() == [interior]
    assert 0 < interior < ncells - 1

    k = key("two_extremes")
    assert np.unique(k).tolist() == [0, ncells - 1]
    assert np.all(k[0::2] == 0) and np.all(k[1::2] == ncells - 1)

    c = sr.low_digit_only(n, (1024, 64, 16), 11)
    assert np.unique(c[:, 1]).size == 1 and np.unique(c[:, 2]).size == 1
    assert c[:, 0].max() < 256 and np.unique(c[:, 0]).size > 200
    c = sr.low_digit_only(n, GRID, 11)                          # a grid narrower than 256 cells: all of x
    assert np.unique(c[:, 0]).size == GRID[0]

    c = sr.high_digit_only(n, GRID, 11)
    assert np.unique(c[:, 0]).size == 1 and np.unique(c[:, 1]).size == 1 and np.unique(c[:, 2]).size == GRID[2]

    up, down = key("ascending").astype(np.int64), key("descending").astype(np.int64)
    assert np.all(np.diff(up) >= 0) and np.all(np.diff(down) <= 0)
    assert np.unique(up).size > n // 2 and np.array_equal(up, down[::-1])

    k = key("skewed")
    assert np.count_nonzero(k == interior) >= n - n // 10
    assert np.unique(k).size > n // 20                         # the other 10 % are spread out
    heavy_pos = np.flatnonzero(k == interior)
    assert heavy_pos[0] < 20 and heavy_pos[-1] > n - 20        # the heavy cell is all over the upload, not one run

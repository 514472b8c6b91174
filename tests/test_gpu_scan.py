"""GPU: the library's one-block prefix sum (scan_array_one_block, csrc/sph_device.hpp) through the test hook sph_test_scan,
against numpy.cumsum shifted by one in the same unsigned width.  Every count -> scan -> scatter pipeline of the library --
the movers' merge, sph_remove, the compat seam's B' list, the slab re-cut, the surface mesh, the mesh voxeliser -- runs this
one function; all sums are integers, so every prefix and the total must be equal exactly, wrap-around included."""
import numpy as np
import pytest

from gpufluidsimulator_amd import capi

pytestmark = pytest.mark.gpu

# a partial wave, exactly one wave, one over a wave; exactly one chunk of 1024 and one over it (the carry); two chunks, one
# over two chunks; a last chunk with a single live wave
SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 17]
WRAPS_FROM = 63          # random u32 values: from this size on (every size but 0 and 1) the sum exceeds 2^32, asserted first


@pytest.fixture(scope="module")
def ctx():
    with capi.Context(64, box=(2.0, 2.0, 2.0), grid=(32, 32, 32)) as c:
        yield c


def _check(ctx, values):
    dtype = values.dtype
    got, total = ctx.test_scan(values)
    inclusive = np.cumsum(values, dtype=dtype)                               # unsigned: wraps modulo 2^bits as the device does
    want = np.concatenate([np.zeros(1, dtype), inclusive[:-1]]) if values.size else np.zeros(0, dtype)
    assert got.dtype == dtype and got.shape == values.shape
    assert np.array_equal(got, want)
    assert total.dtype == dtype and total == (inclusive[-1] if values.size else 0)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", SIZES)
def test_all_ones(ctx, n, bits):
    _check(ctx, np.ones(n, np.uint32 if bits == 32 else np.uint64))


@pytest.mark.parametrize("n", SIZES)
def test_random_u32_wraps_as_numpy_does(ctx, n):
    v = np.random.default_rng(1000 + n).integers(0, 2 ** 32, n, dtype=np.uint64)      # up to 2^32 - 1
    if n >= WRAPS_FROM:
        assert int(v.sum()) > 2 ** 32                                                  # the 32-bit scan has to wrap
    _check(ctx, v.astype(np.uint32))


@pytest.mark.parametrize("n", SIZES)
def test_u64_of_values_below_2_to_32_whose_total_is_not(ctx, n):
    """What the voxeliser's 64-bit rows exist for: every item fits 32 bits, the sum does not."""
    v = np.random.default_rng(2000 + n).integers(0, 2 ** 32, n, dtype=np.uint64)
    if n >= WRAPS_FROM:
        assert int(v.max()) < 2 ** 32 < int(v.sum())
    _check(ctx, v)

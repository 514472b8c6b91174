"""pytest configuration: markers, paths, shared fixtures."""
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    # GPU runs use torch (streams, slab buffers) next to libsph_hip.so: torch's bundled HIP runtime must be
    # the one that gets loaded, i.e. torch first (gpufluidsimulator_amd.capi.load explains why)
    if "gpu" in (config.getoption("-m") or "") and "not gpu" not in (config.getoption("-m") or ""):
        import torch  # noqa: F401


def load_golden(name):
    """tests/golden/<name>.npz, or the parts a large fixture is stored in (<name>.partNN.npz, arrays cut into row
    blocks <key>@0, <key>@1, ...: oracle/make_golden.py keeps every file under 1 MiB)."""
    path = os.path.join(GOLDEN, name + ".npz")
    if os.path.exists(path):
        return np.load(path)
    parts = sorted(glob.glob(os.path.join(GOLDEN, glob.escape(name) + ".part*.npz")))
    assert parts, f"no fixture {name} in tests/golden"
    out, blocks = {}, {}
    for p in parts:
        with np.load(p) as z:
            for k in z.files:
                if "@" in k:
                    key, i = k.rsplit("@", 1)
                    blocks.setdefault(key, {})[int(i)] = z[k]
                else:
                    out[k] = z[k]
    for key, b in blocks.items():
        out[key] = np.concatenate([b[i] for i in range(len(b))])
    return out


@pytest.fixture(scope="session")
def golden():
    return load_golden


def bits(a):
    """View float32 data as uint32 for bit-exact comparisons."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)

"""GPU: the headless driver writes pictures (sph_headless -frames=DIR: ParticleSystem::setCamera / renderFrame / writeFrame on
top of sph_render) -- which files, their PPM header and size, that they show particles, and the refusal next to -gpus=N."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gpufluidsimulator_amd", "sph_headless")
ARGS = ["-benchmark", "-n=4096", "-i=4", "-framesize=96x64", "-frameevery=2"]


def _run(args):
    from gpufluidsimulator_amd import build
    build.build()            # (does nothing when the driver is newer than its sources)
    return subprocess.run([EXE] + args, capture_output=True, text=True, timeout=120)


def test_headless_writes_every_second_frame_as_ppm(tmp_path):
    frames = tmp_path / "frames"
    out = _run(ARGS + ["-frames=" + str(frames)])
    assert out.returncode == 0, out.stderr
    # numbered by the 0-based update the picture follows (stated in -help): updates 0 and 2 of 0..3
    assert sorted(os.listdir(frames)) == ["frame_000000.ppm", "frame_000002.ppm"]
    images = []
    for name in sorted(os.listdir(frames)):
        data = (frames / name).read_bytes()
        header = b"P6\n96 64\n255\n"
        assert data.startswith(header) and len(data) == len(header) + 96 * 64 * 3
        img = np.frombuffer(data[len(header):], np.uint8).reshape(64, 96, 3)
        lit = img.any(axis=2)                                  # the background is black
        assert 3 <= lit.sum() < 96 * 64 // 2                   # the dam in the box's corner, seen from three units back
        assert lit[32:, :48].sum() == lit.sum()                # ... the lower left of the reference's view
        assert len(np.unique(img[lit], axis=0)) >= 3           # shaded and ramp-coloured, not one flat colour
        images.append(img)


def test_headless_refuses_frames_with_slabs(tmp_path):
    frames = tmp_path / "frames"
    out = _run(ARGS + ["-frames=" + str(frames), "-gpus=2", "-onegpu"])
    assert out.returncode != 0 and "-frames" in out.stderr
    assert not frames.exists()

"""Command lines of the headless driver that end before any GPU call: an argument error, a plan_slabs error, or -help.

tests/test_headless_cli_cpu.py runs every one and compares exit status, stdout and stderr with tests/golden/headless_cli.json,
byte for byte.  Run as a script, this file records that golden file:

    python tests/headless_cli_cases.py [path/to/sph_headless]

The golden file was recorded with the driver as it was before its main() was split, on a machine without a GPU."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gpufluidsimulator_amd", "sph_headless")
GOLDEN = os.path.join(ROOT, "tests", "golden", "headless_cli.json")

B = "-benchmark"
COLLIDER = "-collider=0,0,0,0.1"
SHAPE = "-obstacle=sphere:0,0,0,0.2"
EMIT = "-emit=0,0.5,0,2,0,-1,0,2"
DRAIN = "-drain=-1,-1,-1,1,-0.5,1"
SLABS = ["-onegpu", "-n=4096", "-box=2"]          # with -gpus=N: plan_slabs decides, on the host

CASES = [
    # ---- help, the OpenGL note, dashes, first occurrence, unknown options
    ["-help"],
    [B, "-help"],
    ["--help"],
    ["-file=state.snap", "-help"],
    ["-help", "-collider=1"],
    ["-ic=foo", "-help"],
    [B, "-ic=foo"],
    ["-ic=foo"],
    [B, "-ic=grid", "-ic=foo", "-collider=1"],
    [B, "-ic=foo", "-ic=grid"],
    [B, "--ic=foo"],
    [B, "---collider=1"],
    [B, "collider=1"],
    [B, "-collider=1", "-collider=0,0,0,1"],
    [B, "-bogus", "-alsobogus=3", "-collider=1"],
    [B, "-n=8", "--n=4096", "-gpus=64", "--gpus=2"] + SLABS,
    # ---- -collider, -collidermass
    [B, "-collider=1,2,3"],
    [B, "-collider=0,0,0,0"],
    [B, "-collider=0,0,0,0.1,1"],
    [B, "-collider=0,0,0,-1,0,0,0"],
    [B, "-collider="],
    [B, "-collidermass=1"],
    [B, COLLIDER, "-collidermass=-1"],
    [B, COLLIDER, "-collidermass=1,2"],
    [B, COLLIDER, "-collidermass=nan"],
    [B, COLLIDER, "-collidermass=1,0,inf,0"],
    # ---- -obstacle and its options, -obstaclemesh and its options
    [B, "-obstacle=nocolon"],
    [B, "-obstacle=cube:0,0,0,1"],
    [B, "-obstacle=sphere:1,2,3"],
    [B, "-obstacle=box:0,0,0,1,1,1,0.1x"],
    [B, "-obstacle=box:1,2,3,4,5"],
    [B, "-obstacle=capsule:0,0,0,1,1,1"],
    [B, "-obstacle=plane:0,0,0,0,1,0,1"],
    [B, "-obstacle=!sphere:1"],
    [B, SHAPE, "-obstacle=box:0,0,0"],
    [B, SHAPE, "-obstaclevel=1,2"],
    [B, SHAPE, "-obstaclevel="],
    [B, "-obstacleband=0", "-obstaclemesh=solid.obj"],
    [B, "-obstacleband=17", "-obstaclemesh=solid.obj"],
    [B, "-obstacleband=3x", "-obstaclemesh=solid.obj"],
    [B, "-obstacleband=", "-obstaclemesh=solid.obj"],
    [B, "-obstaclemesh=solid.obj", SHAPE],
    [B, "-obstaclemesh="],
    [B, "-obstacleband=3"],
    [B, "-obstacleinvert"],
    [B, "-obstacleinvert=1"],
    [B, "-obstaclecell=0.05"],
    [B, "-obstaclevel=0,0,1"],
    # ---- -emit, -drain, -add
    [B, "-emit=1"],
    [B, "-emit=0,0,0,1.5,0,0,0,1"],
    [B, "-emit=0,0,0,-1,0,0,0,1"],
    [B, "-emit=0,0,0,1,0,0,0,0"],
    [B, "-drain=1,2,3"],
    [B, "-drain=0,0,0,1,1,1,0"],
    [B, "-add=1"],
    [B, "-add=-1,5"],
    [B, "-add=0,0"],
    # ---- -frames and its options
    [B, "-frames"],
    ["-frames"],
    [B, "-frames="],
    [B, "-frameevery=0"],
    [B, "-frameevery=2x"],
    [B, "-framesize=96"],
    [B, "-framesize=0x10"],
    [B, "-framesize=10x4097"],
    [B, "-framesize=10x10x"],
    [B, "-camera=1"],
    [B, "-camera=0,0,3,0,0,0,180"],
    [B, "-camera=0,0,3,0,0,0,60x"],
    [B, "-camera=0,1,0,0,0,0"],
    [B, "-camera=0,0,3,0,0,nan"],
    [B, "-color=rainbow"],
    [B, "-color=speed"],
    [B, "-color=speed:1:1"],
    [B, "-color=density:0:1x"],
    # ---- -surface, -tint, -absorb
    [B, "-surface"],
    [B, "-tint=1,1,1"],
    [B, "-frames=pictures", "-absorb=1,1,1"],
    [B, "-frames=pictures", "-surface=1"],
    [B, "-frames=pictures", "-surface=17,2"],
    [B, "-frames=pictures", "-surface=1,9"],
    [B, "-frames=pictures", "-surface=1,1,-1"],
    [B, "-frames=pictures", "-surface=1,1,1x"],
    [B, "-frames=pictures", "-surface", "-tint=1,2"],
    [B, "-frames=pictures", "-surface", "-absorb=1,2,-3"],
    # ---- -mesh and its options
    [B, "-mesh"],
    [B, "-mesh="],
    [B, "-meshevery=2"],
    [B, "-mesh=shapes", "-meshevery=0"],
    [B, "-mesh=shapes", "-meshcell=0"],
    [B, "-mesh=shapes", "-meshradius=nan"],
    [B, "-mesh=shapes", "-iso=1x"],
    [B, "-meshcell=0.1"],
    [B, "-meshradius=0.1"],
    [B, "-iso=0.4"],
    # ---- one device only, in the order of the rules
    [B, "-gpus=2", EMIT],
    [B, "-gpus=2", DRAIN],
    [B, "-gpus=2", "-add=1,8"],
    [B, "-gpus=1", "-slab", EMIT],
    [B, "-gpus=2", "-frames=pictures", "-surface"],
    [B, "-gpus=2", "-mesh=shapes"],
    [B, "-gpus=1", "-slab", "-mesh=shapes"],
    [B, "-gpus=2", "-frames=pictures"],
    [B, "-gpus=2", COLLIDER],
    [B, "-gpus=2", COLLIDER, "-collidermass=1"],
    [B, "-gpus=2", SHAPE],
    [B, "-gpus=2", "-obstaclemesh=solid.obj"],
    [B, "-gpus=1", "-slab", "-obstaclemesh=solid.obj"],
    [B, "-gpus=2", "-ic=random"],
    [B, "-gpus=2", "-load=state.snap"],
    [B, "-gpus=2", "-file=state.snap"],
    [B, "-gpus=2", "-sphere=1"],
    [B, "-gpus=2", "-save=state.snap"],
    [B, "-gpus=2", "-log=benchmark.txt"],
    [B, "-gpus=2", "-dump=2"],
    [B, "-gpus=1", "-slab", "-dump=2"],
    [B, "-gpus=2", "-lattice=16,16"],
    [B, "-gpus=2", "-protocol=2"],
    [B, "-gpus=2", "-protocol=x"],
    # ---- plan_slabs, and the -out file of the slab run
    ["-gpus=64"] + SLABS,
    [B, "-gpus=64"] + SLABS,
    [B, "-gpus=16", "-protocol=1"] + SLABS,
    [B, "-gpus=64", "-protocol=1", "-lattice=16,16,16", "-steps=2", "-i=3", "-nowarmup", "-out=positions.bin"] + SLABS,
    [B, "-gpus=17", "-grid=32", "-device=1"] + SLABS,
    [B, "-gpus=2", "-grid=128"] + SLABS,
    [B, "-gpus=1", "-slab", "-grid=128"] + SLABS,
    [B, "-gpus=2", "-out=/nonexistent-directory/positions.bin"] + SLABS,
    # ---- two mistakes: the first check in the driver's order reports
    [B, "-ic=foo", "-collider=1"],
    [B, "-collider=1", "-obstacle=foo"],
    [B, "-obstacle=foo", "-obstaclevel=1"],
    [B, "-obstaclevel=1", "-obstacleband=99"],
    [B, "-obstacleband=99", "-obstaclemesh="],
    [B, "-obstaclemesh=", SHAPE],
    [B, "-obstaclemesh=", "-collidermass=1"],
    [B, "-obstacleinvert", "-obstaclecell=0.05"],
    [B, "-obstaclecell=0.05", "-collidermass=1"],
    [B, "-collidermass=1", "-emit=1"],
    [B, "-emit=1", "-drain=1"],
    [B, "-drain=1", "-frames"],
    [B, "-frames", "-frameevery=0"],
    [B, "-frameevery=0", "-framesize=1"],
    [B, "-framesize=1", "-camera=1"],
    [B, "-camera=1", "-color=x"],
    [B, "-color=x", "-surface"],
    [B, "-surface", "-mesh"],
    [B, "-frames=pictures", "-surface=99,1", "-tint=-1,0,0"],
    [B, "-frames=pictures", "-surface", "-tint=x", "-absorb=y"],
    [B, "-frames=pictures", "-surface", "-absorb=y", "-mesh"],
    [B, "-mesh", "-meshevery=0"],
    [B, "-mesh=shapes", "-meshevery=0", "-meshcell=0"],
    [B, "-mesh=shapes", "-iso=0", "-meshradius=0", "-meshcell=0"],
    [B, "-meshcell=0"],
    [B, "-iso=0.4", "-add=1"],
    [B, "-add=1", "-gpus=2", EMIT],
    [B, "-gpus=2", EMIT, "-frames=pictures", "-surface"],
    [B, "-gpus=2", "-frames=pictures", "-surface", "-mesh=shapes"],
    [B, "-gpus=2", "-mesh=shapes", "-frames=pictures"],
    [B, "-gpus=2", "-frames=pictures", COLLIDER],
    [B, "-gpus=2", COLLIDER, SHAPE],
    [B, "-gpus=2", SHAPE, "-ic=random"],
    [B, "-gpus=2", "-obstaclemesh=solid.obj", "-dump=3"],
    [B, "-gpus=2", "-ic=random", "-lattice=1"],
    [B, "-gpus=2", "-lattice=1", "-protocol=2"],
    [B, "-gpus=2", "-protocol=2", "-grid=128"] + SLABS,
    [B, "-gpus=64", "-grid=128", "-out=/nonexistent-directory/positions.bin"] + SLABS,
]


def run_case(exe, args):
    out = subprocess.run([exe] + args, capture_output=True, stdin=subprocess.DEVNULL, timeout=60)
    return {"args": args, "status": out.returncode, "stdout": out.stdout.decode("utf-8"), "stderr": out.stderr.decode("utf-8")}


if __name__ == "__main__":
    exe = sys.argv[1] if len(sys.argv) > 1 else EXE
    with open(GOLDEN, "w") as f:
        json.dump([run_case(exe, args) for args in CASES], f, indent=1)
        f.write("\n")
    print(f"{len(CASES)} cases -> {GOLDEN}")

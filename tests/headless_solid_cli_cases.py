"""Command lines of the headless driver's -solid* options (the obstacle slots) that end before any GPU call, each with the exit
status and a piece of the one line it must write to stderr (status 0: to stdout) -- written down from the option forms, not
recorded from the driver.  tests/test_headless_solid_cli_cpu.py runs them."""
B = "-benchmark"
BALL = "sphere:0,0,0,0.2"
SLOT_FORM = "expected <k>:..., k = 0..3"
SHAPE_FORM = "expected <k>:<shape> with the shapes of -obstacle, or <k>:[!]mesh:FILE.obj"

CASES = [
    # ---- the slot in front of the colon
    ([B, "-solid=" + BALL], 1, "-solid=" + BALL + ": " + SLOT_FORM),
    ([B, "-solid=1"], 1, "-solid=1: " + SLOT_FORM),
    ([B, "-solid=4:" + BALL], 1, "-solid=4:" + BALL + ": " + SLOT_FORM),
    ([B, "-solid=-1:" + BALL], 1, SLOT_FORM),
    ([B, "-solid=12:" + BALL], 1, SLOT_FORM),
    ([B, "-solid="], 1, SLOT_FORM),
    # ---- the shape grammar of -obstacle behind it
    ([B, "-solid=1:nocolon"], 1, "-solid=1:nocolon: " + SHAPE_FORM),
    ([B, "-solid=1:cube:0,0,0,1"], 1, SHAPE_FORM),
    ([B, "-solid=2:sphere:1,2,3"], 1, SHAPE_FORM),
    ([B, "-solid=3:box:0,0,0,1,1,1,0.1x"], 1, SHAPE_FORM),
    ([B, "-solid=0:!sphere:1"], 1, SHAPE_FORM),
    ([B, "-solid=1:" + BALL, "-solid=1:box:0,0,0"], 1, "-solid=1:box:0,0,0: " + SHAPE_FORM),
    # ---- meshes
    ([B, "-solid=1:mesh:"], 1, "-solid=1:mesh:: expected <k>:[!]mesh:FILE.obj"),
    ([B, "-solid=1:!mesh:"], 1, "expected <k>:[!]mesh:FILE.obj"),
    ([B, "-solid=2:mesh:a.obj", "-solid=2:!mesh:b.obj"], 1, "slot 2 already has a mesh"),
    ([B, "-solid=1:mesh:a.obj", "-solid=1:" + BALL], 1, "-solid=1: a mesh and shapes exclude each other: a slot holds one grid"),
    ([B, "-solid=1:" + BALL, "-solid=1:mesh:a.obj"], 1, "-solid=1: a mesh and shapes exclude each other"),
    # ---- the options of a slot
    ([B, "-solid=1:" + BALL, "-solidcell=0.05"], 1, "-solidcell=0.05: expected <k>:<s>"),
    ([B, "-solid=1:" + BALL, "-solidcell=1:"], 1, "-solidcell=1:: expected <k>:<s>"),
    ([B, "-solid=1:" + BALL, "-solidcell=1:0.05x"], 1, "expected <k>:<s>"),
    ([B, "-solid=1:mesh:a.obj", "-solidband=1:0"], 1, "-solidband=1:0: expected <k>:<N>, k = 0..3, N = 1..16"),
    ([B, "-solid=1:mesh:a.obj", "-solidband=1:17"], 1, "N = 1..16"),
    ([B, "-solid=1:mesh:a.obj", "-solidband=1:3x"], 1, "N = 1..16"),
    ([B, "-solid=1:mesh:a.obj", "-solidband=4:3"], 1, "-solidband=4:3: expected <k>:<N>"),
    ([B, "-solid=1:" + BALL, "-solidband=1:3"], 1, "-solidband=1:... goes with a -solid=1:mesh:FILE.obj"),
    ([B, "-solid=1:" + BALL, "-solidvel=1:1,2"], 1, "-solidvel=1:1,2: expected <k>:ux,uy,uz"),
    ([B, "-solid=1:" + BALL, "-solidvel=1,2,3"], 1, "expected <k>:ux,uy,uz"),
    ([B, "-solid=1:" + BALL, "-solidvel=1:1,2,3,4"], 1, "expected <k>:ux,uy,uz"),
    ([B, "-solid=1:" + BALL, "-solidspin=1:0,0,0,1,2"], 1, "-solidspin=1:0,0,0,1,2: expected <k>:px,py,pz,wx,wy,wz"),
    ([B, "-solid=1:" + BALL, "-solidspin=1:0,0,0,1,2,3,4"], 1, "expected <k>:px,py,pz,wx,wy,wz"),
    # ---- an option of a slot without its solid
    ([B, "-solidcell=2:0.05"], 1, "-solidspin=2:... go with a -solid=2:..."),
    ([B, "-solid=1:" + BALL, "-solidvel=2:1,2,3"], 1, "go with a -solid=2:..."),
    ([B, "-solid=1:" + BALL, "-solidspin=3:0,0,0,0,0,1"], 1, "go with a -solid=3:..."),
    ([B, "-solidband=0:3"], 1, "go with a -solid=0:..."),
    # ---- slot 0 through both families
    ([B, "-solid=0:" + BALL, "-obstacle=" + BALL], 1, "-solid=0:... and -obstacle / -obstaclemesh both address slot 0"),
    ([B, "-obstaclemesh=solid.obj", "-solid=0:" + BALL], 1, "both address slot 0"),
    ([B, "-solid=0:mesh:a.obj", "-obstacle=" + BALL, "-solid=1:" + BALL], 1, "both address slot 0"),
    # ---- the -obstacle family answers first, as before
    ([B, "-obstacle=foo", "-solid=9"], 1, "-obstacle=foo: expected [!]sphere:"),
    ([B, "-obstaclemesh=solid.obj", "-obstacle=" + BALL, "-solid=1:" + BALL], 1, "-obstaclemesh and -obstacle exclude each other: a context holds one grid"),
    ([B, "-solid=9", "-collidermass=1"], 1, SLOT_FORM),
    # ---- slab runs
    ([B, "-gpus=2", "-solid=1:" + BALL], 1, "-solid is not supported with -gpus=2: sph_obstacle_select works on a whole-domain context"),
    ([B, "-gpus=1", "-slab", "-solid=3:mesh:a.obj"], 1, "-solid is not supported with -gpus=1 -slab"),
    ([B, "-gpus=2", "-obstacle=" + BALL, "-solid=1:" + BALL], 1, "-obstacle is not supported with -gpus=2"),
    # ---- help
    ([B, "-solidhelp"], 0, "[-solidspin=<k>:<px>,<py>,<pz>,<wx>,<wy>,<wz>]"),
    ([B, "-solid=1:" + BALL, "-solidvel=1:1,2,3", "-solidspin=1:0,0,0,0,0,1", "-solidcell=1:0.1", "-solid=2:!mesh:a.obj", "-solidband=2:4",
      "-solidhelp"], 0, "A context holds 4 obstacle slots, k = 0..3"),
    ([B, "-solidhelp", "-help"], 0, "usage: sph_headless [-benchmark]"),
]

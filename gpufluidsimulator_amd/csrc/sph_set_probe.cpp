// sph_set_probe.cpp -- a test program for the host class's obstacle slots (ParticleSystem::selectObstacle, selectedObstacle,
// clearAllObstacles of include/particleSystem.h; clearObstacles() clears the selected slot), in the manner of sph_pose_probe.cpp:
// tests/test_gpu_obstacle_set_host.py drives the class through this.
//
//   sph_set_probe <out> <updates> <slot of the box: 1..3> <24 numbers>
//       numbers: box centre (3), half extents (3), rounding, spacing ; offset (3) ; velocity (3) ; pivot (3) ; quat wxyz (4) ; omega (3)
//   4096 particles of the jittered lattice in a box of edge 4 on a 64^3 grid.  Slot 0 holds a static ramp (the half-space through
//   (-1.75, -1.85, 0) with normal (-0.5, 1, 0)), the given slot the posed, moving, sensed box.  After the updates <out> holds the
//   positions and the velocities (4096 x 4 floats each, by creation index) and then J[3], L[3] of the box's last update as
//   doubles.  Then the program clears the box's slot, makes one more update with the ramp alone, clears all, and prints the
//   selection and the installed mask at each stage: "sel <k> mask <m>" lines on stdout.
#include "../../include/particleSystem.h"

#include <cstdio>
#include <cstdlib>

static void report(ParticleSystem& ps, sph_ctx* c) {
    uint32_t mask = 0;
    sph_obstacle_installed(c, &mask);
    printf("sel %u mask %u\n", ps.selectedObstacle(), mask);
}

int main(int argc, char** argv) {
    if (argc != 4 + 24) {
        fprintf(stderr, "usage: sph_set_probe <out> <updates> <slot of the box: 1..3> <24 numbers>\n");
        return 2;
    }
    const int updates = atoi(argv[2]);
    const uint slot = (uint)atoi(argv[3]);
    float v[24];
    for (int k = 0; k < 24; k++) v[k] = strtof(argv[4 + k], nullptr);
    const uint n = 4096;
    ParticleSystem ps(n, make_float3(4.f, 4.f, 4.f), ParticleSystem::HIP_PARALLEL, uint3{64, 64, 64}, n);
    ps.reset(ParticleSystem::CONFIG_GRID);
    report(ps, ps.context());
    sph_shape ramp = {};
    ramp.kind = SPH_SHAPE_HALFSPACE;
    ramp.a[0] = -1.75f; ramp.a[1] = -1.85f; ramp.a[2] = 0.f;
    ramp.b[0] = -0.5f; ramp.b[1] = 1.f; ramp.b[2] = 0.f;
    sph_shape box = {};
    box.kind = SPH_SHAPE_BOX;
    for (int k = 0; k < 3; k++) { box.a[k] = v[k]; box.b[k] = v[3 + k]; }
    box.r = v[6];
    ps.selectObstacle(slot);                      // the later slot first: the order of installation is not the order of action
    ps.setObstacles(&box, 1, v[7]);
    ps.setObstacleMotion(v + 8, v + 11);
    ps.setObstaclePose(v + 14, v + 17, v + 21);
    ps.senseObstacleLoad(true);
    ps.selectObstacle(0);
    ps.setObstacles(&ramp, 1, v[7]);
    report(ps, ps.context());
    for (int i = 0; i < updates; i++) ps.update(0.0000005f, (float)i);
    double load[6];
    ps.selectObstacle(slot);
    ps.getObstacleLoad(load, load + 3);
    FILE* f = fopen(argv[1], "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[1]); return 1; }
    fwrite(ps.getArray(ParticleSystem::POSITION), sizeof(float) * 4, n, f);
    fwrite(ps.getArray(ParticleSystem::VELOCITY), sizeof(float) * 4, n, f);
    fwrite(load, sizeof(double), 6, f);
    fclose(f);
    ps.clearObstacles();                          // the selected slot: the box
    report(ps, ps.context());
    ps.update(0.0000005f, (float)updates);
    ps.clearAllObstacles();
    report(ps, ps.context());
    return 0;
}

// sph_pose_probe.cpp -- a test program for the host class's posed obstacle and load sensor (ParticleSystem::setObstaclePose,
// clearObstaclePose, senseObstacleLoad, getObstacleLoad of include/particleSystem.h): the headless driver has no option for them
// yet (its usage text is pinned), so tests/test_gpu_obstacle_pose_host.py drives the class through this instead.
//
//   sph_pose_probe <out> <updates> <drop pose: 0|1> <24 numbers>
//       numbers: box centre (3), half extents (3), rounding, spacing ; offset (3) ; velocity (3) ; pivot (3) ; quat wxyz (4) ; omega (3)
//   4096 particles of the jittered lattice in a box of edge 4 on a 64^3 grid; after the updates <out> holds the positions and
//   the velocities (4096 x 4 floats each, by creation index) and then J[3], L[3] of the last update as doubles.
#include "../../include/particleSystem.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
    if (argc != 4 + 24) {
        fprintf(stderr, "usage: sph_pose_probe <out> <updates> <drop pose: 0|1> <24 numbers>\n");
        return 2;
    }
    const int updates = atoi(argv[2]);
    const bool drop = atoi(argv[3]) != 0;
    float v[24];
    for (int k = 0; k < 24; k++) v[k] = strtof(argv[4 + k], nullptr);
    const uint n = 4096;
    ParticleSystem ps(n, make_float3(4.f, 4.f, 4.f), ParticleSystem::HIP_PARALLEL, uint3{64, 64, 64}, n);
    ps.reset(ParticleSystem::CONFIG_GRID);
    sph_shape box = {};
    box.kind = SPH_SHAPE_BOX;
    for (int k = 0; k < 3; k++) { box.a[k] = v[k]; box.b[k] = v[3 + k]; }
    box.r = v[6];
    ps.setObstacles(&box, 1, v[7]);
    ps.setObstacleMotion(v + 8, v + 11);
    ps.setObstaclePose(v + 14, v + 17, v + 21);
    if (drop) ps.clearObstaclePose();
    ps.senseObstacleLoad(true);
    for (int i = 0; i < updates; i++) ps.update(0.0000005f, (float)i);
    double load[6];
    ps.getObstacleLoad(load, load + 3);
    FILE* f = fopen(argv[1], "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[1]); return 1; }
    fwrite(ps.getArray(ParticleSystem::POSITION), sizeof(float) * 4, n, f);
    fwrite(ps.getArray(ParticleSystem::VELOCITY), sizeof(float) * 4, n, f);
    fwrite(load, sizeof(double), 6, f);
    fclose(f);
    return 0;
}

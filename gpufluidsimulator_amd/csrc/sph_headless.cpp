// sph_headless.cpp -- headless driver with the reference's command line (SPH/particles.cpp:676-706: -n= -box= -i= -benchmark
// -device= -file=) and its runBenchmark() output line (:176-192), on top of include/particleSystem.h; -gpus=N (no counterpart
// in the reference, a single-device program) steps z-slabs through the C ABI.  No GLUT / OpenGL.
// What each option means is stated once, by `sph_headless -help`; its form, by the parser's error message.
// Structure: parse_options() fills one Options struct -- the only code that sees argv, and none of it needs a device.  main()
// dispatches: -help, the slab run (slab_job, run_slabs) or the one-device run (run_one_device: set_up, before_update,
// after_update, report).
#include "../../include/particleSystem.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <cerrno>
#include <fcntl.h>
#include <poll.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

namespace {

const float kTimestep = 0.0000005f;        // particles.cpp:88

// ---- everything the command line can say ------------------------------------------------------------------------------
struct Options {
    struct {
        uint n = 262144;                   // NUM_PARTICLES, particleSystem.h:15
        float box = 2.0f;                  // BOX_SIZE
        int iterations = 100, substeps = 1, dump = 0, device = 0;      // (findCudaDevice: -device=N, else the first, helper_cuda.h:845)
        uint grid = 0;                     // 0: the reference's formula nextPow2(box / (0.66666 h))
        ParticleSystem::ParticleConfig ic = ParticleSystem::CONFIG_GRID;   // initParticleSystem resets to CONFIG_GRID
        const char* load = nullptr;        // -load=, or -file=
        bool help = false, warmup = true;
        uint capacity = 0;                 // -capacity=M; default -n, with -emit / -add twice -n: they need room to grow
        const char *out = nullptr, *save = nullptr, *log = nullptr;
        double logfreq = 2000.0;           // BENCHMARK_FREQ
        ParticleSystem::BenchmarkLogStyle logstyle = ParticleSystem::LOG_FRAMES;
    } run;
    struct {
        bool on = false, has_mass = false, has_accel = false;      // -collider; -collidermass; its ax,ay,az
        float center[3] = {0.f, 0.f, 0.f}, radius = 0.f, velocity[3] = {0.f, 0.f, 0.f}, mass = 0.f, accel[3] = {0.f, 0.f, 0.f};
    } collider;
    struct {                               // -obstacle= shapes or an -obstaclemesh=; the cell and the velocity serve either
        std::vector<sph_shape> shapes;
        const char* mesh = nullptr;
        bool invert = false, has_velocity = false;
        uint band = 0;                     // 0, as the cell: the library's default
        float cell = 0.f, velocity[3] = {0.f, 0.f, 0.f};
    } obstacle;
    struct Solid {                         // -solid=<k>:... and its options: slot k of the context (the -obstacle family is slot 0)
        bool given = false, invert = false, has_velocity = false, has_spin = false, has_cell = false;
        std::vector<sph_shape> shapes;
        std::string mesh;                  // the OBJ file of -solid=<k>:[!]mesh:FILE.obj, else empty
        uint band = 0;
        float cell = 0.f, velocity[3] = {0.f, 0.f, 0.f}, pivot[3] = {0.f, 0.f, 0.f}, omega[3] = {0.f, 0.f, 0.f};
        bool has_body = false;             // -solidbody=<k>:hinge,... | float,...: the fluid drives the slot (sph_obstacle_set_body)
        sph_obstacle_body body = {};
    } solid[SPH_MAX_OBSTACLES];
    bool solidhelp = false;
    bool solids() const { for (const Solid& s : solid) if (s.given) return true; return false; }
    struct { bool on = false; float center[3] = {0.f, 0.f, 0.f}, velocity[3] = {0.f, 0.f, 0.f}; int radius = 0, every = 0; } emit;
    struct { bool on = false; float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f}; int every = 1; } drain;
    struct { bool on = false; int at = -1, count = 0; } add;
    struct { bool given = false; int at = -1, radius = 10; } sphere;
    struct {
        const char* dir = nullptr;
        int every = 1, color_mode = SPH_COLOR_INDEX, width = 640, height = 480;
        float eye[3] = {0.f, 0.f, 3.f}, target[3] = {0.f, 0.f, 0.f}, fovy = 60.f, color_lo = 0.f, color_hi = 1.f;
    } frames;
    struct { bool on = false; sph_surface_style style; } surface;
    struct { bool on = false; sph_solid_style style; } drawsolids;      // -drawsolids and -solidlook=<k>:...
    struct { const char* dir = nullptr; int every = 1; sph_mesh_params params; } mesh;
    struct { int gpus = 1, protocol = 3; bool on = false, onegpu = false; uint32_t lattice[3] = {0, 0, 0}; uint64_t particles = 0; } slabs;
    bool grows() const { return emit.on || drain.on || add.on; }      // -out then has one row per creation index below the capacity
};

// ---- the parser: the only code that sees argv ---------------------------------------------------------------------------
struct Args {
    int argc; char** argv;
    static const char* match(const char* a, const char* name) {      // what follows `name` in a, any number of dashes skipped
        while (*a == '-') a++;
        const size_t l = strlen(name);
        return strncmp(a, name, l) ? nullptr : a + l;
    }
    bool flag(const char* name) const {                               // checkCmdLineFlag, helper_string.h:111
        for (int i = 1; i < argc; i++) if (const char* t = match(argv[i], name)) if (*t == 0 || *t == '=') return true;
        return false;
    }
    const char* value(const char* name) const {                       // of the first -name=...
        for (int i = 1; i < argc; i++) if (const char* t = match(argv[i], name)) if (*t == '=') return t + 1;
        return nullptr;
    }
};

__attribute__((format(printf, 1, 2))) bool fail(const char* fmt, ...) {      // the error line; false, for `return fail(...)`
    va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap);
    return false;
}

bool parse_every(const Args& a, const char* name, int& every) {      // -name=K, a whole number >= 1
    const char* v = a.value(name);
    if (char extra = 0; v && (sscanf(v, "%d%c", &every, &extra) != 1 || every < 1)) return fail("-%s=%s: expected a whole number >= 1\n", name, v);
    return true;
}

bool parse_run(const Args& a, Options& o) {
    auto& r = o.run;
    if (const char* v = a.value("n")) r.n = (uint)strtoul(v, nullptr, 10);
    if (const char* v = a.value("box")) r.box = (float)atof(v);
    if (const char* v = a.value("i")) r.iterations = atoi(v);
    if (const char* v = a.value("steps")) r.substeps = atoi(v);
    if (const char* v = a.value("dump")) r.dump = atoi(v);
    if (const char* v = a.value("device")) r.device = atoi(v);
    if (const char* v = a.value("grid")) r.grid = (uint)strtoul(v, nullptr, 10);
    if (const char* v = a.value("logfreq")) r.logfreq = atof(v);
    r.warmup = !a.flag("nowarmup");
    r.out = a.value("out"); r.save = a.value("save"); r.log = a.value("log");
    if (const char* v = a.value("ic")) {
        if (!strcmp(v, "random")) r.ic = ParticleSystem::CONFIG_RANDOM;
        else if (strcmp(v, "grid")) return fail("-ic=%s: expected grid or random\n", v);
    }
    // -file=<path>: the reference runs ONE update and would compare with a reference file (particles.cpp:690-692, 194-217;
    // the comparison itself is commented out upstream).  Here the file is a state snapshot (-save): it is loaded like -load.
    const char* file = a.value("file");
    r.load = a.value("load");
    if (file && !r.load) r.load = file;
    if (file && !a.value("i")) r.iterations = 1;                      // numIterations = 1, particles.cpp:692
    // -benchmark selects the headless path upstream (without it a GLUT window opens); this build has no other path
    if (!a.flag("benchmark") && !file) fprintf(stderr, "note: no OpenGL in this build -- running headless, as with -benchmark\n");
    r.help = a.flag("help");
    return true;
}

bool parse_collider(const Args& a, Options& o) {
    auto& c = o.collider;
    const char* v = a.value("collider"); if (!v) return true;
    const int k = sscanf(v, "%f,%f,%f,%f,%f,%f,%f", &c.center[0], &c.center[1], &c.center[2], &c.radius, &c.velocity[0], &c.velocity[1], &c.velocity[2]);
    if ((k != 4 && k != 7) || !(c.radius > 0.f)) return fail("-collider=%s: expected x,y,z,r or x,y,z,r,ux,uy,uz with r > 0\n", v);
    return c.on = true;
}

bool parse_collider_mass(const Args& a, Options& o) {      // (after the obstacles: the order of the checks is kept)
    auto& c = o.collider;
    const char* v = a.value("collidermass"); if (!v) return true;
    const int k = sscanf(v, "%f,%f,%f,%f", &c.mass, &c.accel[0], &c.accel[1], &c.accel[2]);
    const bool finite = std::isfinite(c.mass) && std::isfinite(c.accel[0]) && std::isfinite(c.accel[1]) && std::isfinite(c.accel[2]);
    if (!c.on || (k != 1 && k != 4) || !(c.mass >= 0.f) || !finite)
        return fail("-collidermass=%s: expected M or M,ax,ay,az with M >= 0, next to a -collider\n", v);
    c.has_accel = k == 4;
    return c.has_mass = true;
}

// one -obstacle= (a leading `!` inverts the shape).  The library checks the values; this only checks the form.
bool parse_shape(const char* arg, sph_shape* out) {
    sph_shape s{};
    if (*arg == '!') { s.invert = 1; arg++; }
    float v[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const char* colon = strchr(arg, ':');
    if (!colon) return false;
    const std::string kind(arg, colon);
    char tail = 0;
    const int k = sscanf(colon + 1, "%f,%f,%f,%f,%f,%f,%f%c", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &tail);
    for (int a = 0; a < 3; a++) s.a[a] = v[a];
    if (kind == "sphere" && k == 4) { s.kind = SPH_SHAPE_SPHERE; s.r = v[3]; }
    else if (kind == "box" && (k == 6 || k == 7)) { s.kind = SPH_SHAPE_BOX; for (int a = 0; a < 3; a++) s.b[a] = v[3 + a]; s.r = k == 7 ? v[6] : 0.f; }
    else if (kind == "capsule" && k == 7) { s.kind = SPH_SHAPE_CAPSULE; for (int a = 0; a < 3; a++) s.b[a] = v[3 + a]; s.r = v[6]; }
    else if (kind == "plane" && k == 6) { s.kind = SPH_SHAPE_HALFSPACE; for (int a = 0; a < 3; a++) s.b[a] = v[3 + a]; }
    else return false;
    *out = s;
    return true;
}

bool parse_obstacles(const Args& a, Options& o) {
    auto& ob = o.obstacle;
    for (int i = 1; i < a.argc; i++) {
        const char* t = Args::match(a.argv[i], "obstacle=");
        sph_shape sh;
        if (t && !parse_shape(t, &sh))
            return fail("-obstacle=%s: expected [!]sphere:cx,cy,cz,r | [!]box:cx,cy,cz,hx,hy,hz[,r] | [!]capsule:ax,ay,az,bx,by,bz,r | [!]plane:px,py,pz,nx,ny,nz\n", t);
        if (t) ob.shapes.push_back(sh);
    }
    const char* cell = a.value("obstaclecell"); if (cell) ob.cell = (float)atof(cell);
    if (const char* v = a.value("obstaclevel")) {
        if (sscanf(v, "%f,%f,%f", &ob.velocity[0], &ob.velocity[1], &ob.velocity[2]) != 3) return fail("-obstaclevel=%s: expected ux,uy,uz\n", v);
        ob.has_velocity = true;
    }
    ob.mesh = a.value("obstaclemesh");
    if (const char* v = a.value("obstacleband")) {
        char* end = nullptr;
        const long b = strtol(v, &end, 10);
        if (end == v || *end || b < 1 || b > SPH_OBSTACLE_MESH_MAX_BAND) return fail("-obstacleband=%s: expected 1..%d\n", v, SPH_OBSTACLE_MESH_MAX_BAND);
        ob.band = (uint)b;
    }
    ob.invert = a.flag("obstacleinvert");
    if (ob.mesh && !ob.shapes.empty()) return fail("-obstaclemesh and -obstacle exclude each other: a context holds one grid (no union of a mesh with shapes)\n");
    if (ob.mesh && !*ob.mesh) return fail("-obstaclemesh=: expected a Wavefront OBJ file\n");
    if (!ob.mesh && (ob.band || ob.invert)) return fail("-obstacleband / -obstacleinvert go with an -obstaclemesh\n");
    if (ob.shapes.empty() && !ob.mesh && (ob.has_velocity || cell)) return fail("-obstaclecell / -obstaclevel go with an -obstacle\n");
    return true;
}

// -solid=<k>:... and -solidcell / -solidband / -solidvel / -solidspin=<k>:..., all repeatable: the slots 0..3 of the context, each
// with the grammar of the -obstacle family behind the `<k>:`.  Only the form is checked here.
const char* solid_slot(const char* t, int* k) {                    // "<k>:rest" -> rest, or null
    if (t[0] < '0' || t[0] >= '0' + SPH_MAX_OBSTACLES || t[1] != ':') return nullptr;
    *k = t[0] - '0';
    return t + 2;
}

bool parse_solids(const Args& a, Options& o) {
    o.solidhelp = a.flag("solidhelp");
    const char* const slot_form = "expected <k>:..., k = 0..3\n";
    for (int i = 1; i < a.argc; i++) {
        int k = 0;
        if (const char* t = Args::match(a.argv[i], "solid=")) {
            const char* rest = solid_slot(t, &k);
            if (!rest) return fail("-solid=%s: %s", t, slot_form);
            auto& s = o.solid[k];
            const bool inv = *rest == '!';
            if (!strncmp(rest + (inv ? 1 : 0), "mesh:", 5)) {
                const char* file = rest + (inv ? 1 : 0) + 5;
                if (!*file) return fail("-solid=%s: expected <k>:[!]mesh:FILE.obj\n", t);
                if (!s.mesh.empty()) return fail("-solid=%s: slot %d already has a mesh\n", t, k);
                s.mesh = file; s.invert = inv;
            } else {
                sph_shape sh;
                if (!parse_shape(rest, &sh))
                    return fail("-solid=%s: expected <k>:<shape> with the shapes of -obstacle, or <k>:[!]mesh:FILE.obj\n", t);
                s.shapes.push_back(sh);
            }
            s.given = true;
        } else if (const char* t = Args::match(a.argv[i], "solidcell=")) {
            const char* rest = solid_slot(t, &k);
            char tail = 0;
            if (!rest || sscanf(rest, "%f%c", &o.solid[k].cell, &tail) != 1) return fail("-solidcell=%s: expected <k>:<s>, k = 0..3\n", t);
            o.solid[k].has_cell = true;
        } else if (const char* t = Args::match(a.argv[i], "solidband=")) {
            const char* rest = solid_slot(t, &k);
            char* end = nullptr;
            const long b = rest ? strtol(rest, &end, 10) : 0;
            if (!rest || end == rest || *end || b < 1 || b > SPH_OBSTACLE_MESH_MAX_BAND)
                return fail("-solidband=%s: expected <k>:<N>, k = 0..3, N = 1..%d\n", t, SPH_OBSTACLE_MESH_MAX_BAND);
            o.solid[k].band = (uint)b;
        } else if (const char* t = Args::match(a.argv[i], "solidvel=")) {
            const char* rest = solid_slot(t, &k);
            char tail = 0;
            float* u = rest ? o.solid[k].velocity : nullptr;
            if (!rest || sscanf(rest, "%f,%f,%f%c", &u[0], &u[1], &u[2], &tail) != 3) return fail("-solidvel=%s: expected <k>:ux,uy,uz, k = 0..3\n", t);
            o.solid[k].has_velocity = true;
        } else if (const char* t = Args::match(a.argv[i], "solidspin=")) {
            const char* rest = solid_slot(t, &k);
            char tail = 0;
            float* p = rest ? o.solid[k].pivot : nullptr; float* w = rest ? o.solid[k].omega : nullptr;
            if (!rest || sscanf(rest, "%f,%f,%f,%f,%f,%f%c", &p[0], &p[1], &p[2], &w[0], &w[1], &w[2], &tail) != 6)
                return fail("-solidspin=%s: expected <k>:px,py,pz,wx,wy,wz, k = 0..3\n", t);
            o.solid[k].has_spin = true;
        } else if (const char* t = Args::match(a.argv[i], "solidbody=")) {
            const char* rest = solid_slot(t, &k);
            const char* body_form = "-solidbody=%s: expected <k>:hinge,ax,ay,az,I[,tau] or <k>:float,mass,Ix,Iy,Iz[,gy], k = 0..3\n";
            if (!rest) return fail(body_form, t);
            if (o.solid[k].has_body) return fail("-solidbody=%s: slot %d already has a body\n", t, k);
            sph_obstacle_body b = {};
            float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            char tail = 0;
            if (const char* h = strncmp(rest, "hinge,", 6) ? nullptr : rest + 6) {
                if (sscanf(h, "%f,%f,%f,%f,%f%c", &v[0], &v[1], &v[2], &v[3], &v[4], &tail) != 5) {
                    v[4] = 0.f;
                    if (sscanf(h, "%f,%f,%f,%f%c", &v[0], &v[1], &v[2], &v[3], &tail) != 4) return fail(body_form, t);
                }
                const double len = std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]);
                if (!(len > 0.0) || !(v[3] > 0.f)) return fail("-solidbody=%s: the axis must not be zero and I must be positive\n", t);
                b.dof = SPH_BODY_HINGE;
                b.inertia[0] = v[3];
                for (int c = 0; c < 3; c++) { b.axis[c] = v[c]; b.torque[c] = (float)((double)v[4] * ((double)v[c] / len)); }
            } else if (const char* f = strncmp(rest, "float,", 6) ? nullptr : rest + 6) {
                if (sscanf(f, "%f,%f,%f,%f,%f%c", &v[0], &v[1], &v[2], &v[3], &v[4], &tail) != 5) {
                    v[4] = 0.f;
                    if (sscanf(f, "%f,%f,%f,%f%c", &v[0], &v[1], &v[2], &v[3], &tail) != 4) return fail(body_form, t);
                }
                if (!(v[0] > 0.f) || !(v[1] > 0.f) || !(v[2] > 0.f) || !(v[3] > 0.f))
                    return fail("-solidbody=%s: the mass and the three moments must be positive\n", t);
                b.dof = SPH_BODY_FREE_X | SPH_BODY_FREE_Y | SPH_BODY_FREE_Z | SPH_BODY_SPIN;
                b.mass = v[0];
                for (int c = 0; c < 3; c++) { b.inertia[c] = v[1 + c]; b.lo[c] = -1e30f; b.hi[c] = 1e30f; }
                b.accel[1] = v[4];
            } else {
                return fail(body_form, t);
            }
            o.solid[k].has_body = true;
            o.solid[k].body = b;
        }
    }
    for (int k = 0; k < SPH_MAX_OBSTACLES; k++) {
        const auto& s = o.solid[k];
        if (s.has_body && !(s.given && s.has_spin))
            return fail("-solidbody=%d:... goes with a -solid=%d:... and a -solidspin=%d:... (the pivot and the first angular velocity)\n", k, k, k);
        if (!s.given && (s.has_cell || s.band || s.has_velocity || s.has_spin))
            return fail("-solidcell / -solidband / -solidvel / -solidspin=%d:... go with a -solid=%d:...\n", k, k);
        if (!s.mesh.empty() && !s.shapes.empty())
            return fail("-solid=%d: a mesh and shapes exclude each other: a slot holds one grid (no union of a mesh with shapes)\n", k);
        if (s.mesh.empty() && s.band) return fail("-solidband=%d:... goes with a -solid=%d:mesh:FILE.obj\n", k, k);
    }
    if (o.solid[0].given && (!o.obstacle.shapes.empty() || o.obstacle.mesh))
        return fail("-solid=0:... and -obstacle / -obstaclemesh both address slot 0: give the solid through one of them\n");
    return true;
}

bool parse_emit_drain(const Args& a, Options& o) {
    if (const char* v = a.value("emit")) {
        auto& e = o.emit;
        float rr = 0.f;
        const int k = sscanf(v, "%f,%f,%f,%f,%f,%f,%f,%d", &e.center[0], &e.center[1], &e.center[2], &rr, &e.velocity[0], &e.velocity[1], &e.velocity[2], &e.every);
        e.radius = (int)rr;
        if (k != 8 || e.radius < 0 || (float)e.radius != rr || e.every < 1)
            return fail("-emit=%s: expected x,y,z,r,vx,vy,vz,every with r a whole number of lattice spacings >= 0 and every >= 1\n", v);
        e.on = true;
    }
    if (const char* v = a.value("drain")) {
        auto& d = o.drain;
        const int k = sscanf(v, "%f,%f,%f,%f,%f,%f,%d", &d.lo[0], &d.lo[1], &d.lo[2], &d.hi[0], &d.hi[1], &d.hi[2], &d.every);
        if ((k != 6 && k != 7) || d.every < 1) return fail("-drain=%s: expected x0,y0,z0,x1,y1,z1 or x0,y0,z0,x1,y1,z1,every with every >= 1\n", v);
        d.on = true;
    }
    return true;
}

bool parse_frames(const Args& a, Options& o) {
    auto& f = o.frames;
    char extra = 0;
    f.dir = a.value("frames");
    if (a.flag("frames") && (!f.dir || !*f.dir)) return fail("-frames: expected -frames=<directory>\n");
    if (!parse_every(a, "frameevery", f.every)) return false;
    if (const char* v = a.value("framesize")) {
        int fw = 0, fh = 0;
        if (sscanf(v, "%dx%d%c", &fw, &fh, &extra) != 2 || fw < 1 || fw > SPH_RENDER_MAX_SIZE || fh < 1 || fh > SPH_RENDER_MAX_SIZE)
            return fail("-framesize=%s: expected <W>x<H> with 1..%d each\n", v, SPH_RENDER_MAX_SIZE);
        f.width = fw; f.height = fh;
    }
    if (const char* v = a.value("camera")) {
        float c[7] = {f.eye[0], f.eye[1], f.eye[2], f.target[0], f.target[1], f.target[2], f.fovy};
        const int k = sscanf(v, "%f,%f,%f,%f,%f,%f,%f%c", &c[0], &c[1], &c[2], &c[3], &c[4], &c[5], &c[6], &extra);
        bool ok = (k == 6 || k == 7) && c[6] > 0.f && c[6] < 180.f;
        for (int q = 0; q < 7; q++) ok = ok && std::isfinite(c[q]);
        ok = ok && !(c[0] == c[3] && c[2] == c[5]);      // up is +y: the view direction must not be vertical (nor null)
        if (!ok) return fail("-camera=%s: expected ex,ey,ez,tx,ty,tz or ex,ey,ez,tx,ty,tz,fovy with 0 < fovy < 180 and a view direction that is not vertical\n", v);
        for (int q = 0; q < 3; q++) { f.eye[q] = c[q]; f.target[q] = c[3 + q]; }
        f.fovy = c[6];
    }
    if (const char* v = a.value("color")) {
        bool ok = true;
        if (!strcmp(v, "index")) f.color_mode = SPH_COLOR_INDEX;
        else if (!strncmp(v, "speed:", 6) || !strncmp(v, "density:", 8)) {
            f.color_mode = v[0] == 's' ? SPH_COLOR_SPEED : SPH_COLOR_DENSITY;
            ok = sscanf(strchr(v, ':') + 1, "%f:%f%c", &f.color_lo, &f.color_hi, &extra) == 2 && std::isfinite(f.color_lo) && std::isfinite(f.color_hi) &&
                 f.color_lo != f.color_hi;
        } else ok = false;
        if (!ok) return fail("-color=%s: expected index, speed:<lo>:<hi> or density:<lo>:<hi> with lo != hi\n", v);
    }
    auto& d = o.drawsolids;   // -drawsolids -solidlook (repeatable): options of -frames
    d.on = a.flag("drawsolids");
    sph_solid_defaults(&d.style);
    bool looks = false;
    for (int i = 1; i < a.argc; i++)
        if (const char* t = Args::match(a.argv[i], "solidlook=")) {
            int k = 0, open = 0;
            float c3[3] = {0.f, 0.f, 0.f};
            const char* rest = solid_slot(t, &k);
            const int got = rest ? sscanf(rest, "%f,%f,%f,%d%c", &c3[0], &c3[1], &c3[2], &open, &extra) : 0;
            bool ok = (got == 3 || got == 4) && (open == 0 || open == 1);
            for (int q = 0; q < 3; q++) ok = ok && c3[q] >= 0.f && c3[q] <= 1.f;      // (false for a NaN)
            if (!ok) return fail("-solidlook=%s: expected <k>:<r>,<g>,<b>[,<open>], k = 0..3, each colour in [0, 1], open 0 or 1\n", t);
            for (int q = 0; q < 3; q++) d.style.slot[k].color[q] = c3[q];
            d.style.slot[k].open = open;
            looks = true;
        }
    if ((d.on || looks) && (!o.frames.dir || !d.on))
        return fail("-drawsolids / -solidlook: expected -frames=<directory> -drawsolids [-solidlook=<k>:<r>,<g>,<b>[,<open>]]\n");
    auto& s = o.surface;      // -surface -tint -absorb: options of -frames
    s.on = a.flag("surface");
    sph_surface_defaults(&s.style);
    if (!s.on && !a.value("tint") && !a.value("absorb")) return true;
    if (!o.frames.dir || !s.on)
        return fail("-surface / -tint / -absorb: expected -frames=<directory> -surface[=<r>,<K>[,<tau>]] [-tint=<r>,<g>,<b>] [-absorb=<r>,<g>,<b>]\n");
    if (const char* v = a.value("surface")) {
        int sr = 0, sk = 0;
        float tau = 0.f;
        const int k = sscanf(v, "%d,%d,%f%c", &sr, &sk, &tau, &extra);
        if ((k != 2 && k != 3) || sr < 0 || sr > SPH_SURFACE_MAX_RADIUS_PX || sk < 0 || sk > SPH_SURFACE_MAX_ITERATIONS || !std::isfinite(tau) || tau < 0.f)
            return fail("-surface=%s: expected <r>,<K> or <r>,<K>,<tau> with r 0..%d, K 0..%d and tau >= 0\n", v, SPH_SURFACE_MAX_RADIUS_PX, SPH_SURFACE_MAX_ITERATIONS);
        s.style.smooth_radius_px = (uint32_t)sr;
        s.style.smooth_iterations = (uint32_t)sk;
        s.style.depth_falloff = tau;
    }
    const char* names[2] = {"tint", "absorb"};
    float* fields[2] = {s.style.tint, s.style.absorb};
    for (int n = 0; n < 2; n++)
        if (const char* v = a.value(names[n])) {
            float c3[3] = {0.f, 0.f, 0.f};
            bool ok = sscanf(v, "%f,%f,%f%c", &c3[0], &c3[1], &c3[2], &extra) == 3;
            for (int q = 0; q < 3; q++) ok = ok && std::isfinite(c3[q]) && c3[q] >= 0.f;
            if (!ok) return fail("-%s=%s: expected <r>,<g>,<b>, each finite and >= 0\n", names[n], v);
            for (int q = 0; q < 3; q++) fields[n][q] = c3[q];
        }
    return true;
}

bool parse_mesh(const Args& a, Options& o) {
    auto& m = o.mesh;
    char extra = 0;
    m.dir = a.value("mesh");
    sph_mesh_defaults(&m.params);
    if (a.flag("mesh") && (!m.dir || !*m.dir)) return fail("-mesh: expected -mesh=<directory>\n");
    if (!parse_every(a, "meshevery", m.every)) return false;
    const char* names[3] = {"meshcell", "meshradius", "iso"};
    float* fields[3] = {&m.params.spacing, &m.params.radius, &m.params.iso};
    bool any = a.value("meshevery") != nullptr;
    for (int n = 0; n < 3; n++)
        if (const char* v = a.value(names[n])) {
            float x = 0.f;
            if (sscanf(v, "%f%c", &x, &extra) != 1 || !std::isfinite(x) || !(x > 0.f))
                return fail("-%s=%s: expected a number > 0 (an option of -mesh=<directory>)\n", names[n], v);
            *fields[n] = x;
            any = true;
        }
    if (!m.dir && any) return fail("-meshevery / -meshcell / -meshradius / -iso: expected -mesh=<directory> next to them\n");
    return true;
}

// what joins the fluid at one update, -add and -sphere, and the room for all who join (after -emit: the default depends on it)
bool parse_add_sphere(const Args& a, Options& o) {
    auto& r = o.run;
    if (const char* v = a.value("add")) {
        if (sscanf(v, "%d,%d", &o.add.at, &o.add.count) != 2 || o.add.at < 0 || o.add.count < 1) return fail("-add=%s: expected <update>,<count>\n", v);
        o.add.on = true;
    }
    if (const char* v = a.value("sphere")) {
        o.sphere.given = true; o.sphere.at = atoi(v);
        if (const char* c = strchr(v, ',')) o.sphere.radius = atoi(c + 1);
    }
    r.capacity = r.n;
    if (o.emit.on || o.add.on) r.capacity = r.n < 0x7FFFFFFFu / 2u ? 2u * r.n : r.n;
    if (const char* v = a.value("capacity")) r.capacity = (uint)strtoul(v, nullptr, 10);
    return true;
}

// -gpus and its options, and what a slab run cannot take
bool parse_slabs(const Args& a, Options& o) {
    auto& s = o.slabs;
    if (const char* v = a.value("gpus")) s.gpus = atoi(v);
    s.on = s.gpus > 1 || (s.gpus == 1 && a.flag("slab"));     // (-gpus=1 -slab: the same machinery with one rank -- fork, RCCL communicator of one)
    if (!s.on) return true;
    const struct { bool given; const char* what; const char* reason; } one_device_only[] = {      // the first row that was given reports
        {o.grows(), "-emit / -drain / -add are", "sph_emit and sph_remove work on a whole-domain context (the slab step sizes its messages from "
                                                 "the previous step's counts); run them on one device"},
        {o.surface.on, "-surface is", "sph_render_surface works on a whole-domain context (the ranks would have to composite their images); run it on one device"},
        {o.drawsolids.on, "-drawsolids is", "sph_render_set_solids works on a whole-domain context (a slab context does not render); run it on one device"},
        {o.mesh.dir != nullptr, "-mesh is", "sph_mesh_extract works on a whole-domain context (the ranks would have to share a lattice seam); run it on one device"},
        {o.frames.dir != nullptr, "-frames is", "sph_render works on a whole-domain context (the ranks would have to composite their images); run it on one device"},
        {o.collider.on, "-collider is", "run it on one device, or set the sphere on every rank through the library "
                                        "(gpufluidsimulator_amd.slab.NativeSlabSimulation(colliders=...))"},
        {!o.obstacle.shapes.empty(), "-obstacle is", "sph_obstacle_build works on a whole-domain context (the slab step makes several force launches per step); "
                                                     "run it on one device"},
        {o.obstacle.mesh != nullptr, "-obstaclemesh is", "sph_obstacle_build_obj works on a whole-domain context; run it on one device"},
        {o.solids(), "-solid is", "sph_obstacle_select works on a whole-domain context (the slab step makes several force launches per step); "
                                  "run it on one device"},
    };
    for (const auto& rule : one_device_only)
        if (rule.given) return fail("%s not supported with -gpus=%d%s: %s\n", rule.what, s.gpus, s.gpus == 1 ? " -slab" : "", rule.reason);
    if (o.run.ic != ParticleSystem::CONFIG_GRID || o.run.load || o.sphere.given || o.run.save || o.run.log || o.run.dump)
        return fail("-gpus=%d runs the dam-break lattice (-ic=grid) and takes -n -box -grid -i -steps -lattice -out -device -onegpu -nowarmup\n", s.gpus);
    uint32_t cube = (uint32_t)std::floor(std::cbrt((double)o.run.n));
    while ((uint64_t)cube * cube * cube < o.run.n) cube++;                      // the lattice of reset(CONFIG_GRID), the first -n points of it
    s.lattice[0] = s.lattice[1] = s.lattice[2] = cube; s.particles = o.run.n;
    if (const char* v = a.value("lattice")) {
        if (sscanf(v, "%u,%u,%u", &s.lattice[0], &s.lattice[1], &s.lattice[2]) != 3) return fail("-lattice=nx,ny,nz\n");
        s.particles = (uint64_t)s.lattice[0] * s.lattice[1] * s.lattice[2];
    }
    if (const char* v = a.value("protocol")) s.protocol = atoi(v);
    if (s.protocol != 1 && s.protocol != 3) return fail("-protocol=%d: 3 (three message groups per step) or 1 (one)\n", s.protocol);
    s.onegpu = a.flag("onegpu");
    return true;
}

// The groups in the order of their checks: a command line with two mistakes reports the first of them.  -help is looked at
// right after -ic (parse_run) and ends the parsing.
bool parse_options(int argc, char** argv, Options& o) {
    const Args a{argc, argv};
    if (!parse_run(a, o)) return false;
    if (o.run.help) return true;
    if (!(parse_collider(a, o) && parse_obstacles(a, o) && parse_solids(a, o) && parse_collider_mass(a, o) && parse_emit_drain(a, o) && parse_frames(a, o) &&
          parse_mesh(a, o) && parse_add_sphere(a, o) && parse_slabs(a, o)))
        return false;
    // -logstyle=oscar: the line form of the reference's committed logs (benchmarks/oscar/); default: what its source writes (particleSystem.cpp:703-714)
    const char* st = o.run.log ? a.value("logstyle") : nullptr;
    if (st && strcmp(st, "oscar") && strcmp(st, "frames")) return fail("-logstyle=%s: expected oscar or frames\n", st);
    if (st && !strcmp(st, "oscar")) o.run.logstyle = ParticleSystem::LOG_OSCAR;
    return true;
}

void print_help() {
    printf("usage: sph_headless [-benchmark] [-n=<particles>] [-box=<edge>] [-i=<iterations>] [-device=<id>] [-grid=<cells per axis>] [-ic=grid|random] [-steps=<per "
           "update>] [-gpus=<N> [-onegpu] [-slab] [-lattice=nx,ny,nz] [-protocol=1|3]] [-dump=<count>] [-log=<file> [-logfreq=<ms>] [-logstyle=oscar|frames]] "
           "[-sphere=<update>[,<radius>]] [-collider=<x>,<y>,<z>,<radius>[,<ux>,<uy>,<uz>]] [-collidermass=<M>[,<ax>,<ay>,<az>]] [-obstacle=<shape> ... "
           "[-obstaclecell=<s>] [-obstaclevel=<ux>,<uy>,<uz>]] [-obstaclemesh=<file.obj> [-obstacleband=<N>] [-obstacleinvert] [-obstaclecell=<s>] "
           "[-obstaclevel=<ux>,<uy>,<uz>]] [-emit=<x>,<y>,<z>,<r>,<vx>,<vy>,<vz>,<every>] [-drain=<x0>,<y0>,<z0>,<x1>,<y1>,<z1>[,<every>]] [-add=<update>,<count>] "
           "[-capacity=<particles>] [-out=<file>] [-save=<file>] [-load=<file>] [-file=<file>] [-frames=<dir> [-frameevery=<K>] [-framesize=<W>x<H>] "
           "[-camera=<ex>,<ey>,<ez>,<tx>,<ty>,<tz>[,<fovy>]] [-color=index|speed:<lo>:<hi>|density:<lo>:<hi>] [-surface[=<r>,<K>[,<tau>]] [-tint=<r>,<g>,<b>] "
           "[-absorb=<r>,<g>,<b>]]] [-mesh=<dir> [-meshevery=<K>] [-meshcell=<s>] [-meshradius=<r>] [-iso=<v>]]\n"
           "  -collider: a solid sphere the fluid flows around, moving at (ux, uy, uz) (default: at rest); one device only\n"
           "  -collidermass: the -collider sphere is a free body of mass M > 0 that the fluid pushes, under the acceleration (ax, ay, az) (default: (0, gravity_y, 0) of "
           "the run), or with M = 0 a kinematic obstacle whose load is wanted; prints its centre, velocity and last impulse at the end; one device only\n"
           "  -obstacle: a solid the fluid collides with, [!]sphere:cx,cy,cz,r | [!]box:cx,cy,cz,hx,hy,hz[,r] | [!]capsule:ax,ay,az,bx,by,bz,r | "
           "[!]plane:px,py,pz,nx,ny,nz (solid behind the normal); repeatable, the union is rasterised on the device as one grid of signed distances over the box, `!` "
           "inverts a shape; -obstaclecell the grid spacing (default: the particle diameter), -obstaclevel a uniform velocity of the whole grid; one device only\n"
           "  -obstaclemesh: a closed triangle mesh (Wavefront OBJ: v and f lines) as the solid, voxelised on the device into signed distances -obstacleband nodes wide "
           "(1..16, default 3); -obstacleinvert: the fluid is inside the mesh; honours -obstaclecell and -obstaclevel; prints triangles used and skipped, lost crossings "
           "and odd columns (a closed mesh: 0 and 0); not together with -obstacle; one device only\n"
           "  -emit: every <every> updates append a lattice ball of radius <r> spacings at (x, y, z) moving at (vx, vy, vz), if its place is clear\n"
           "  -drain: every <every> updates (default 1) remove the particles inside the box [x0,x1) x [y0,y1) x [z0,z1); one device only\n"
           "  -frames: render the particles on the device after the updates 0, K, 2K, ... (-frameevery=K, default 1) and write <dir>/frame_NNNNNN.ppm (binary PPM), "
           "NNNNNN = the 0-based number of the update the picture follows; -framesize default 640x480 (1..4096 each), -camera default 0,0,3,0,0,0,60 (eye, target, "
           "vertical field of view in degrees: the reference's view), -color default index (the reference's colouring), or speed / density mapped from [lo, hi]; one "
           "device only\n"
           "  -surface: with -frames, draw the fluid as a surface instead of sphere sprites: the spheres' depth smoothed <K> times (0..8, default 2) over a radius of <r> "
           "pixels (0..16, default 5) with the depth falloff <tau> (world units, default 0 = four particle radii), normals from the smoothed depth and a water-like "
           "shading; -tint the base colour (default 0.25,0.55,0.95), -absorb the absorption per unit of thickness and channel (default 6,2,0.5; 0,0,0 = no thickness "
           "pass); one device only\n"
           "  -mesh: extract the fluid's surface on the device as a closed triangle mesh after the updates 0, K, 2K, ... (-meshevery=K, default 1) and write "
           "<dir>/mesh_NNNNN.obj (Wavefront OBJ), NNNNN = the 0-based number of the update the mesh follows; -meshcell the lattice spacing (default: the particle "
           "radius), -meshradius each particle's reach (default three spacings, at most eight), -iso the level of the surface (default 0.5); independent of -frames; one "
           "device only\n");
}

// -solidhelp: the options of the obstacle slots (the text of -help is that of the releases before them)
void print_solid_help() {
    printf("usage: sph_headless ... [-solid=<k>:<shape> ...] [-solid=<k>:[!]mesh:<file.obj>] [-solidcell=<k>:<s>] [-solidband=<k>:<N>] "
           "[-solidvel=<k>:<ux>,<uy>,<uz>] [-solidspin=<k>:<px>,<py>,<pz>,<wx>,<wy>,<wz>] "
           "[-solidbody=<k>:hinge,<ax>,<ay>,<az>,<I>[,<tau>] | <k>:float,<mass>,<Ix>,<Iy>,<Iz>[,<gy>]] [-frames=<dir> -drawsolids "
           "[-solidlook=<k>:<r>,<g>,<b>[,<open>]]]\n"
           "  A context holds %d obstacle slots, k = 0..%d; after every update the installed slots push the fluid in ascending order of k, in one pass.\n"
           "  -solid: a solid in slot k, with the shapes of -obstacle (several with one k form a union) or a closed triangle mesh ([!]mesh:, `!`: the fluid is inside "
           "it); repeatable\n"
           "  -solidcell / -solidband / -solidvel: the grid spacing, the mesh's band and the uniform velocity of slot k, as -obstaclecell / -obstacleband / -obstaclevel\n"
           "  -solidspin: slot k turns about the pivot (px, py, pz) with the angular velocity (wx, wy, wz), from the identity pose, and its load sensor is on\n"
           "  -solidbody: the FLUID drives slot k from then on, on the device (goes with -solidspin, which gives the pivot and the first angular velocity): "
           "hinge, a wheel or a flap about the fixed axis (ax, ay, az) through the pivot with the moment I and a constant torque tau about it (default 0); "
           "float, a free body of that mass with the principal moments (Ix, Iy, Iz) about the pivot, its centre of mass, under the acceleration gy (default 0), "
           "its offset unbounded.  At the end a body slot also prints its offset, velocity and angular velocity\n"
           "  -drawsolids: with -frames, the installed slots are drawn into the pictures, sprites or -surface: their distance grids ray-marched on the device, "
           "in front of or behind the fluid by depth; -solidlook the colour of slot k (default 0.72,0.72,0.75) and, with open = 1, the stretch of solid a ray "
           "starts in left out, so that one looks into a vessel; repeatable\n"
           "  The -obstacle family addresses slot 0: a slot 0 given through both is refused.  At the end every installed slot prints its offset, its quaternion and the "
           "momentum J and angular momentum L it took in the last update.  One device only.\n", SPH_MAX_OBSTACLES, SPH_MAX_OBSTACLES - 1);
}

// the reference's line (particles.cpp:191-192), then the same as JSON; `more` goes on inside the JSON object
void print_result(unsigned long long particles, int iterations, int substeps, double secs, unsigned devices, const char* more) {
    const double avg = secs / (iterations > 0 ? iterations : 1);
    printf("particles, Throughput = %.4f KParticles/s, Time = %.5f s, Size = %llu particles, NumDevsUsed = %u, Workgroup = %u\n",
           (1.0e-3 * (double)particles) / avg, avg, particles, devices, 0);
    printf("{\"particle_steps_per_s\": %.1f, \"particles\": %llu, \"iterations\": %d, \"steps_per_update\": %d, \"seconds\": %.6f%s}\n",
           (double)particles * iterations * substeps / secs, particles, iterations, substeps, secs, more);
}

// ---- -gpus=N: z-slabs through the C ABI ---------------------------------------------------------------------------
struct SlabJob {
    uint32_t lattice[3];
    uint64_t particles;              // the first `particles` lattice points (creation index = x + nx (y + ny z))
    float box;
    uint32_t grid;
    int iterations, substeps;
    bool warmup;
    float dt;
    const char* out;                 // xyzw per creation index, then vxyz0 (as the one-device -out)
    int protocol;                    // message groups per step: 3, or 1 (-protocol=1: sph_slab_set_protocol, two ghost layers)
};

struct Plan { std::vector<uint32_t> cuts; std::vector<uint64_t> hist; uint64_t per_layer = 0; };

// the cell layer of lattice plane iz of reset(CONFIG_GRID) -- a particle radius from the wall, a diameter apart -- moved by dz
uint32_t plane_layer(const SlabJob& j, uint32_t iz, double dz = 0.0) {
    const double radius = 1.0 / 64.0, z = -j.box / 2.0 + radius + 2.0 * radius * iz + dz;
    const long c = (long)std::floor((z + j.box / 2.0) / j.box * j.grid);
    return (uint32_t)std::min<long>(std::max<long>(c, 0), (long)j.grid - 1);
}

// Count-balanced cuts of whole cell layers, every slab at least two layers (gpufluidsimulator_amd/slab.py: choose_cuts).
// The lattice planes must not straddle a cell face (every BASELINE config: planes sit a quarter of a cell from the faces,
// the jitter is 0.08 of a cell), so that a slab is one run of creation indices generated on its own device.
bool plan_slabs(const SlabJob& j, int world, Plan& pl, std::string& err) {
    const uint32_t nx = j.lattice[0], ny = j.lattice[1], nz = j.lattice[2], gz = j.grid;
    const double amp = 0.5 * j.box * 0.01 * (1.0 / 64.0) + 1e-4;      // the jitter of a plane's particles
    pl.hist.assign(gz, 0);
    for (uint32_t iz = 0; iz < nz; iz++) {
        const uint64_t first = (uint64_t)iz * nx * ny;
        if (first >= j.particles) break;
        const uint64_t cnt = std::min<uint64_t>((uint64_t)nx * ny, j.particles - first);
        if (plane_layer(j, iz, -amp) != plane_layer(j, iz, amp)) { err = "a lattice plane straddles a cell face: use `python bench.py --gpus N`"; return false; }
        pl.hist[plane_layer(j, iz)] += cnt;
    }
    const uint32_t min_layers = j.protocol == 1 ? 4u : 2u;      // (the one-message step: four layers per slab, slab.py choose_cuts)
    if ((uint64_t)world * min_layers > gz) { err = "more slabs than groups of " + std::to_string(min_layers) + " cell layers"; return false; }
    std::vector<uint64_t> prefix(gz + 1, 0);
    for (uint32_t z = 0; z < gz; z++) { prefix[z + 1] = prefix[z] + pl.hist[z]; pl.per_layer = std::max(pl.per_layer, pl.hist[z]); }
    pl.cuts.assign(1, 0u);
    for (int r = 1; r < world; r++) {
        const double target = (double)j.particles * r / world;
        uint32_t z = (uint32_t)(std::lower_bound(prefix.begin(), prefix.end(), (uint64_t)std::ceil(target)) - prefix.begin());
        if (z > 0 && std::fabs((double)prefix[z - 1] - target) <= std::fabs((double)prefix[std::min(z, gz)] - target)) z--;
        z = std::max(z, pl.cuts.back() + min_layers);
        z = std::min(z, gz - min_layers * (uint32_t)(world - r));
        pl.cuts.push_back(z);
    }
    pl.cuts.push_back(gz);
    return true;
}

struct RankResult { double seconds = 0.0; uint32_t owned = 0; double ping_us[3] = {0, 0, 0}; int rc = 0; char err[256] = {0}; };

// a barrier between the ranks: threads share a counter, processes talk to the parent through pipes.  vote(ok) is the same
// barrier carrying one bit each way: every rank says whether it is fine, everybody learns whether ALL are (the parent --
// or the last thread to arrive -- forms the AND).  The "ready" round in front of the transport uses it: a rank whose
// context, lattice or device set-up failed must stop the others BEFORE they enter ncclCommInitRank, where they would wait
// for it for ever (no time-out of the library covers that call).
struct Gate {
    std::mutex mu; std::condition_variable cv; int world = 1, waiting = 0; uint64_t round = 0;
    bool all_ok = true, result = true;
    int to_parent = -1, from_parent = -1;        // process mode
    bool vote(bool ok) {
        if (to_parent >= 0) {
            char b = ok ? 1 : 0;
            if (write(to_parent, &b, 1) != 1 || read(from_parent, &b, 1) != 1) _exit(3);      // the parent is gone
            return b == 1;
        }
        std::unique_lock<std::mutex> g(mu);
        const uint64_t my = round;
        all_ok = all_ok && ok;
        if (++waiting == world) { waiting = 0; result = all_ok; all_ok = true; round++; cv.notify_all(); }
        else cv.wait(g, [&] { return round != my; });
        return result;
    }
    void wait() { (void)vote(true); }
};

void rank_main(const SlabJob& j, const Plan& pl, int rank, int world, int device, sph_local_hub* hub, const uint8_t* rccl_id, Gate& gate,
               RankResult& res) {
    auto fail = [&](const char* what) { res.rc = -1; snprintf(res.err, sizeof res.err, "rank %d: %s: %s", rank, what, sph_last_error()); };
    const uint32_t z_lo = pl.cuts[rank], z_hi = pl.cuts[rank + 1];
    uint64_t n_own = 0, first = 0;
    {   // my lattice planes: one run of creation indices
        const uint32_t nx = j.lattice[0], ny = j.lattice[1];
        bool any = false;
        for (uint32_t iz = 0; iz < j.lattice[2]; iz++) {
            const uint64_t f = (uint64_t)iz * nx * ny;
            if (f >= j.particles) break;
            const uint32_t c = plane_layer(j, iz);
            if (c < z_lo || c >= z_hi) continue;
            if (!any) { first = f; any = true; }
            n_own += std::min<uint64_t>((uint64_t)nx * ny, j.particles - f);
        }
    }
    const float dims[3] = {j.box, j.box, j.box};
    const uint32_t grid[3] = {j.grid, j.grid, j.grid};
    sph_params prm;
    sph_default_params(&prm, dims, grid);
    const uint32_t ghost_layers = j.protocol == 1 ? 2u : 1u;
    const uint32_t gcap = (uint32_t)((j.protocol == 1 ? 5 : 3) * pl.per_layer + 1024);
    const uint32_t cap = (uint32_t)(1.5 * (double)std::max<uint64_t>(n_own, j.particles / world)) + 4096u;
    sph_ctx* ctx = nullptr; sph_transport* tr = nullptr; sph_slab* slab = nullptr;
    bool ok = sph_create_slab_layers(&ctx, device, cap, &prm, z_lo, z_hi, gcap, ghost_layers) == 0;
    if (!ok) fail("sph_create_slab_layers");
    if (ok && n_own && sph_reset_lattice(ctx, j.lattice, 1, nullptr, first, (uint32_t)n_own) < 0) { ok = false; fail("sph_reset_lattice"); }
    if (ok && sph_sync(ctx) < 0) { ok = false; fail("set-up"); }
    // test hooks (tests/test_gpu_host_class.py): this rank fails its set-up / never reaches the READY round
    if (const char* e = getenv("SPH_HEADLESS_TEST_FAIL_SETUP")) if (ok && atoi(e) == rank) { ok = false; res.rc = -1; snprintf(res.err, sizeof res.err, "rank %d: set-up failed (test hook)", rank); }
    if (const char* e = getenv("SPH_HEADLESS_TEST_HANG_RANK")) if (atoi(e) == rank) for (;;) pause();
    // READY round: nobody creates its transport unless every rank has its context and particles (see Gate::vote)
    if (!gate.vote(ok)) {
        if (ok) { res.rc = -1; snprintf(res.err, sizeof res.err, "rank %d: stopped before the transport was created: another rank failed its set-up", rank); }
        if (ctx) sph_destroy(ctx);
        return;
    }
    if (ok && (hub ? sph_local_transport_create(&tr, hub, rank) : sph_rccl_transport_create(&tr, rccl_id, rank, world, device)) < 0) {
        ok = false; fail("transport");
    }
    if (ok && sph_slab_create(&slab, ctx, rank, world, tr, 0) < 0) { ok = false; fail("sph_slab_create"); }
    if (ok && j.protocol == 1 && sph_slab_set_protocol(slab, 1) < 0) { ok = false; fail("sph_slab_set_protocol"); }
    if (ok) {       // preflight: one exchange-shaped group at the step's three message sizes, contents checked
        const size_t sizes[3] = {8192, (size_t)std::min<uint64_t>(pl.per_layer * 32, (uint64_t)(gcap + 1) * 32),
                                 (size_t)std::min<uint64_t>(pl.per_layer * 8, (uint64_t)(gcap + 1) * 32)};
        for (int k = 0; k < 3 && ok; k++) {
            double o[3];
            if (sph_slab_ping(slab, std::max<size_t>(sizes[k] & ~(size_t)3, 4), 3, o) < 0) { ok = false; fail("sph_slab_ping"); }
            else res.ping_us[k] = o[0];
        }
        // the innermost layers' force pass goes in front of the step's wait (sph_slab_set_early_force)
        // unless the links are so fast that it cannot pay (a migrant message under ~12 us and a halo-A message under ~45)
        // -- nor when the slab is so big that the deep density launch, queued in front of the wait anyway, outlasts the two
        // messages on the path (~half the particles at ~18,800 per us) -- and never when the ranks share a device (-onegpu):
        // their big kernels would evict each other's L2 working sets.  (gpufluidsimulator_amd/slab.py: early_force_rule)
        if (ok) {
            const bool slow = res.ping_us[0] >= 12.0 || res.ping_us[1] >= 45.0;
            const bool exposed = res.ping_us[0] + res.ping_us[1] + 20.0 > 0.5 * (double)n_own / 18.8e3;
            sph_slab_set_early_force(slab, (!hub && slow && exposed) ? 1 : 0);
        }
    }
    if (ok && j.warmup && (sph_slab_step(slab, j.dt, (uint32_t)j.substeps) < 0 || sph_slab_sync(slab) < 0)) { ok = false; fail("warm-up step"); }
    gate.wait();
    const auto t0 = std::chrono::steady_clock::now();
    if (ok && (sph_slab_step(slab, j.dt, (uint32_t)(j.iterations * j.substeps)) < 0 || sph_slab_sync(slab) < 0)) { ok = false; fail("sph_slab_step"); }
    gate.wait();
    res.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (ok) res.owned = sph_num_particles(ctx);
    if (ok && j.out) {          // every rank writes the rows of the particles it owns into the shared file
        const uint32_t n = res.owned;
        std::vector<float> p((size_t)n * 3), v((size_t)n * 3);
        std::vector<uint32_t> idx(n);
        if (sph_download_owned(ctx, p.data(), v.data(), idx.data()) < 0) { ok = false; fail("sph_download_owned"); }
        const int fd = ok ? open(j.out, O_RDWR) : -1;
        const size_t bytes = (size_t)j.particles * 4 * sizeof(float) * 2;
        float* m = fd >= 0 ? (float*)mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0) : (float*)MAP_FAILED;
        if (ok && m == (float*)MAP_FAILED) { ok = false; res.rc = -1; snprintf(res.err, sizeof res.err, "rank %d: cannot map %s", rank, j.out); }
        if (ok) {
            float* vel = m + (size_t)j.particles * 4;
            for (uint32_t s = 0; s < n; s++) {
                const size_t i = idx[s];
                if (i >= j.particles) continue;
                for (int a = 0; a < 3; a++) { m[4 * i + a] = p[3 * (size_t)s + a]; vel[4 * i + a] = v[3 * (size_t)s + a]; }
                m[4 * i + 3] = 1.0f; vel[4 * i + 3] = 0.0f;
            }
            munmap(m, bytes);
        }
        if (fd >= 0) close(fd);
    }
    if (slab) sph_slab_destroy(slab);
    if (tr) { if (hub) sph_local_transport_destroy(tr); else sph_rccl_transport_destroy(tr); }
    if (ctx) sph_destroy(ctx);
}

// a per-round deadline of the -gpus=N parent, in seconds (environment override for tests)
double deadline_for(const char* env, double dflt) { const char* e = getenv(env); const double v = e ? atof(e) : 0.0; return v > 0.0 ? v : dflt; }
bool read_all(int fd, void* p, size_t n) { char* c = (char*)p; while (n) { ssize_t k = read(fd, c, n); if (k <= 0) return false; c += k; n -= (size_t)k; } return true; }
bool write_all(int fd, const void* p, size_t n) { const char* c = (const char*)p; while (n) { ssize_t k = write(fd, c, n); if (k <= 0) return false; c += k; n -= (size_t)k; } return true; }

int run_slabs(const SlabJob& j, int world, bool onegpu, int device0) {
    setenv("SPH_SLAB_TIMEOUT_S", "30", 0);      // a rank that failed must not leave the others in the library's 120 s waits
    Plan pl; std::string err;
    if (!plan_slabs(j, world, pl, err)) { fprintf(stderr, "-gpus=%d: %s\n", world, err.c_str()); return EXIT_FAILURE; }
    if (j.out) {
        const int fd = open(j.out, O_RDWR | O_CREAT | O_TRUNC, 0644);
        if (fd < 0 || ftruncate(fd, (off_t)(j.particles * 4 * sizeof(float) * 2)) != 0) { fprintf(stderr, "cannot create %s\n", j.out); return EXIT_FAILURE; }
        close(fd);
    }
    printf("Run %llu particles simulation for %d iterations... (grid %u^3, box %g, %d z-slabs, cuts", (unsigned long long)j.particles,
           j.iterations, j.grid, j.box, world);
    for (uint32_t c : pl.cuts) printf(" %u", c);
    printf(")\n\n");
    fflush(stdout);
    std::vector<RankResult> res(world);
    if (onegpu) {       // N threads, one device, device-to-device transport
        int is950 = 0;
        if (sph_device_count(&is950) <= 0 || !is950 || sph_select_device(device0) < 0) { fprintf(stderr, "No gfx950 (MI355X) device found, exiting\n"); return EXIT_FAILURE; }
        sph_local_hub* hub = nullptr;
        if (sph_local_hub_create(&hub, world, device0) < 0) { fprintf(stderr, "%s\n", sph_last_error()); return EXIT_FAILURE; }
        Gate gate; gate.world = world;
        std::vector<std::thread> th;
        for (int r = 0; r < world; r++) th.emplace_back([&, r] { rank_main(j, pl, r, world, device0, hub, nullptr, gate, res[r]); });
        for (auto& t : th) t.join();
        sph_local_hub_destroy(hub);
    } else {            // N processes, forked BEFORE anything touches a GPU; rank r on device device0 + r, RCCL
        std::vector<int> id_pipe(2 * world, -1), up(2 * world, -1), down(2 * world, -1), out_pipe(2 * world, -1);
        for (int r = 0; r < world; r++)
            if (pipe(&id_pipe[2 * r]) || pipe(&up[2 * r]) || pipe(&down[2 * r]) || pipe(&out_pipe[2 * r])) { perror("pipe"); return EXIT_FAILURE; }
        std::vector<pid_t> kids(world);
        for (int r = 0; r < world; r++) {
            kids[r] = fork();
            if (kids[r] < 0) { perror("fork"); return EXIT_FAILURE; }
            if (kids[r] == 0) {
                // keep only this rank's ends of the pipes: a pipe whose other end is still open somewhere never reports that
                // its owner died (the parent's read would block for ever on a rank that crashed)
                for (int q = 0; q < world; q++) {
                    close(up[2 * q]); close(down[2 * q + 1]); close(out_pipe[2 * q]);
                    if (q != r) { close(up[2 * q + 1]); close(down[2 * q]); close(out_pipe[2 * q + 1]); close(id_pipe[2 * q]); }
                    if (r != 0 || q == 0) close(id_pipe[2 * q + 1]);
                }
                RankResult rr;
                uint8_t msg[129] = {0};                    // [0]: 1 = an RCCL id follows, 0 = rank 0 has none (abort)
                int ndev = sph_device_count(nullptr);
                if (ndev < device0 + world) { rr.rc = -1; snprintf(rr.err, sizeof rr.err, "rank %d: %d GPUs asked for, %d visible (one GPU: -onegpu)", r, device0 + world, ndev); }
                if (!rr.rc && sph_select_device(device0 + r) < 0) { rr.rc = -1; snprintf(rr.err, sizeof rr.err, "rank %d: %s", r, sph_last_error()); }
                if (r == 0) {
                    if (!rr.rc && sph_rccl_unique_id(msg + 1) < 0) { rr.rc = -1; snprintf(rr.err, sizeof rr.err, "rank 0: %s", sph_last_error()); }
                    msg[0] = rr.rc ? 0 : 1;                // an explicit "no id" instead of 128 zeros the others would try to connect with
                    for (int q = 1; q < world; q++) write_all(id_pipe[2 * q + 1], msg, sizeof msg);
                } else if (!read_all(id_pipe[2 * r], msg, sizeof msg)) { if (!rr.rc) { rr.rc = -1; snprintf(rr.err, sizeof rr.err, "rank %d: no RCCL id from rank 0", r); } }
                else if (msg[0] != 1 && !rr.rc) { rr.rc = -1; snprintf(rr.err, sizeof rr.err, "rank %d: rank 0 could not make an RCCL id", r); }
                Gate gate; gate.to_parent = up[2 * r + 1]; gate.from_parent = down[2 * r];
                if (!rr.rc) rank_main(j, pl, r, world, device0 + r, nullptr, msg + 1, gate, rr);
                else (void)gate.vote(false);               // the READY round: the parent tells everybody to stop
                write_all(out_pipe[2 * r + 1], &rr, sizeof rr);
                _exit(rr.rc ? 1 : 0);
            }
        }
        signal(SIGPIPE, SIG_IGN);                      // (a write to a rank that died must be an error code, not this process's end)
        for (int r = 0; r < world; r++) { close(up[2 * r + 1]); close(down[2 * r]); close(out_pipe[2 * r + 1]); close(id_pipe[2 * r]); close(id_pipe[2 * r + 1]); }
        // The parent never blocks on one rank: it polls every live rank's pipe with a DEADLINE per round.  A rank that hangs
        // where no time-out of the library reaches (ncclCommInitRank waiting for a rank that never comes, a wedged device)
        // would otherwise hold the whole job for ever: on expiry the children are killed, reaped, and the run fails.
        std::vector<bool> dead(world, false);
        auto kill_all = [&](const char* why) {
            fprintf(stderr, "-gpus=%d: %s: killing the ranks\n", world, why);
            for (int r = 0; r < world; r++) kill(kids[r], SIGKILL);
            for (int r = 0; r < world; r++) { int st = 0; waitpid(kids[r], &st, 0); }
        };
        // one byte from every live rank (0/1), then the AND of them back to every live rank; false: deadline expired
        auto round_trip = [&](const char* name, double deadline_s, bool& all_ok) -> bool {
            std::vector<int> got(world, -1);
            const auto t0 = std::chrono::steady_clock::now();
            for (;;) {
                std::vector<pollfd> fds; std::vector<int> who;
                for (int r = 0; r < world; r++) if (!dead[r] && got[r] < 0) { fds.push_back(pollfd{up[2 * r], POLLIN, 0}); who.push_back(r); }
                if (fds.empty()) break;
                const double left = deadline_s - std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                if (left <= 0.0) {
                    std::string late;
                    for (int r : who) late += " " + std::to_string(r);
                    fprintf(stderr, "-gpus=%d: no answer at the '%s' barrier from rank(s)%s after %.0f s\n", world, name, late.c_str(), deadline_s);
                    return false;
                }
                const int k = poll(fds.data(), (nfds_t)fds.size(), (int)std::min(left * 1e3 + 1.0, 1000.0));
                if (k < 0 && errno != EINTR) { perror("poll"); return false; }
                for (size_t i = 0; k > 0 && i < fds.size(); i++) {
                    if (!(fds[i].revents & (POLLIN | POLLHUP | POLLERR))) continue;
                    char b = 0;
                    if (read(fds[i].fd, &b, 1) == 1) got[who[i]] = b ? 1 : 0;
                    else { dead[who[i]] = true; fprintf(stderr, "rank %d died\n", who[i]); }      // (end of file: it closed its end)
                }
            }
            all_ok = true;
            for (int r = 0; r < world; r++) all_ok = all_ok && !dead[r] && got[r] == 1;
            const char b = all_ok ? 1 : 0;
            for (int r = 0; r < world; r++) if (!dead[r] && write(down[2 * r + 1], &b, 1) != 1) dead[r] = true;
            return true;
        };
        const double d_setup = deadline_for("SPH_HEADLESS_SETUP_S", 300.0), d_run = deadline_for("SPH_HEADLESS_RUN_S", 3600.0);
        bool go = false, dummy = false;
        if (!round_trip("ready", d_setup, go)) { kill_all("set-up did not finish"); return EXIT_FAILURE; }
        if (go) {                                      // the two barriers of rank_main: in front of and behind the timed steps
            if (!round_trip("start", d_setup, dummy)) { kill_all("transport set-up / warm-up did not finish"); return EXIT_FAILURE; }
            if (!round_trip("end", d_run, dummy)) { kill_all("the timed steps did not finish"); return EXIT_FAILURE; }
        }
        for (int r = 0; r < world; r++) { if (dead[r] || !read_all(out_pipe[2 * r], &res[r], sizeof(RankResult))) { res[r].rc = -1; snprintf(res[r].err, sizeof res[r].err, "rank %d: no result", r); } }
        for (int r = 0; r < world; r++) { int st = 0; waitpid(kids[r], &st, 0); }
    }
    double secs = 0.0; uint64_t owned = 0; bool bad = false;
    for (int r = 0; r < world; r++) {
        if (res[r].rc) { fprintf(stderr, "%s\n", res[r].err); bad = true; }
        secs = std::max(secs, res[r].seconds); owned += res[r].owned;
    }
    if (bad) return EXIT_FAILURE;
    if (owned != j.particles) { fprintf(stderr, "the slabs hold %llu of %llu particles\n", (unsigned long long)owned, (unsigned long long)j.particles); return EXIT_FAILURE; }
    char more[256];
    snprintf(more, sizeof more, ", \"gpus\": %d, \"ranks_as\": \"%s\", \"ping_us\": [%.1f, %.1f, %.1f]", world, onegpu ? "threads" : "processes",
             res[0].ping_us[0], res[0].ping_us[1], res[0].ping_us[2]);
    print_result(j.particles, j.iterations, j.substeps, secs, (unsigned)world, more);
    return 0;
}

SlabJob slab_job(const Options& o) {
    SlabJob j{};
    for (int a = 0; a < 3; a++) j.lattice[a] = o.slabs.lattice[a];
    j.box = o.run.box;
    j.grid = o.run.grid ? o.run.grid : sph_grid_dim_for_edge(o.run.box, 0.1f);
    j.iterations = o.run.iterations; j.substeps = o.run.substeps; j.warmup = o.run.warmup; j.dt = kTimestep;
    j.particles = o.slabs.particles; j.out = o.run.out; j.protocol = o.slabs.protocol;
    return j;
}

// ---- one device: the reference's run on a ParticleSystem ---------------------------------------------------------------
struct Run {
    ParticleSystem* ps = nullptr;
    uint particles = 0;                    // -n, or what the snapshot holds
    uint ball_points = 0, start = 0, emitted = 0;      // of the faucet's ball; particles at the first update; appended since
    bool full_noted = false;
};

// the ParticleSystem as the options ask for it: collider, obstacles, log, frames, mesh
bool set_up(const Options& o, Run& run) {
    const auto& r = o.run;
    int is950 = 0;      // cudaInit (particleSystem.cu:432-435) -> findCudaDevice -> cudaSetDevice, then initParticleSystem
    if (sph_device_count(&is950) <= 0 || !is950) return fail("No gfx950 (MI355X) device found, exiting\n");
    if (sph_select_device(r.device) < 0) return fail("-device=%d: %s\n", r.device, sph_last_error());
    ParticleSystem* ps = run.ps = new ParticleSystem(r.n, make_float3(r.box, r.box, r.box), ParticleSystem::HIP_PARALLEL, uint3{r.grid, r.grid, r.grid}, r.capacity);
    ps->reset(r.ic);                                      // initParticleSystem, particles.cpp:119-132
    run.particles = r.n;
    if (r.load) {
        ps->loadState(r.load);
        run.particles = (uint)ps->getNumParticles();      // the snapshot decides how many particles there are
    }
    ps->setIterations(r.substeps);
    if (const auto& c = o.collider; c.on) {
        ps->setColliderPos(make_float3(c.center[0], c.center[1], c.center[2]));
        ps->setColliderRadius(c.radius);
        ps->setColliderVelocity(make_float3(c.velocity[0], c.velocity[1], c.velocity[2]));
        ps->enableCollider(true);
        if (c.has_mass) {
            sph_params rp; sph_get_params(ps->context(), &rp);
            const float grav[3] = {0.f, rp.gravity_y, 0.f};
            ps->setColliderMass(c.mass, c.has_accel ? c.accel : grav);
            if (c.mass == 0.f) ps->senseColliderImpulse(true);       // a kinematic obstacle: the impulse is all that is asked for
        }
    }
    const auto& ob = o.obstacle;
    if (!ob.shapes.empty()) ps->setObstacles(ob.shapes.data(), (uint)ob.shapes.size(), ob.cell);
    if (ob.mesh) ps->setObstacleMeshOBJ(ob.mesh, ob.cell, ob.band, ob.invert);
    if (ob.has_velocity) ps->setObstacleMotion(nullptr, ob.velocity);
    if (ob.mesh) {
        uint64_t ms[4];
        ps->getObstacleMeshStats(ms);
        printf("obstacle mesh: %llu triangles used, %llu skipped, %llu lost crossings, %llu odd columns\n", (unsigned long long)ms[0],
               (unsigned long long)ms[1], (unsigned long long)ms[2], (unsigned long long)ms[3]);
    }
    for (uint k = 0; k < (uint)SPH_MAX_OBSTACLES; k++) {       // the slots of -solid=<k>:..., each as the -obstacle family sets slot 0
        const auto& s = o.solid[k];
        if (!s.given) continue;
        ps->selectObstacle(k);
        if (!s.shapes.empty()) ps->setObstacles(s.shapes.data(), (uint)s.shapes.size(), s.cell);
        else ps->setObstacleMeshOBJ(s.mesh.c_str(), s.cell, s.band, s.invert);
        if (s.has_velocity) ps->setObstacleMotion(nullptr, s.velocity);
        if (s.has_spin) {
            const float identity[4] = {1.f, 0.f, 0.f, 0.f};
            ps->setObstaclePose(s.pivot, identity, s.omega);
            ps->senseObstacleLoad(true);
        }
        if (s.has_body) ps->setObstacleBody(s.body);
        if (!s.mesh.empty()) {
            uint64_t ms[4];
            ps->getObstacleMeshStats(ms);
            printf("solid %u mesh: %llu triangles used, %llu skipped, %llu lost crossings, %llu odd columns\n", k, (unsigned long long)ms[0],
                   (unsigned long long)ms[1], (unsigned long long)ms[2], (unsigned long long)ms[3]);
        }
    }
    ps->selectObstacle(0);
    if (r.log) ps->setBenchmarkLog(r.log, r.logfreq, r.logstyle);
    if (const auto& f = o.frames; f.dir) {
        if (mkdir(f.dir, 0755) != 0 && errno != EEXIST) return fail("-frames=%s: cannot create the directory\n", f.dir);
        ps->setCamera(f.width, f.height, f.eye, f.target, f.fovy);
        ps->setRenderColor(f.color_mode, f.color_lo, f.color_hi);
        ps->setRenderSurface(o.surface.on, &o.surface.style);
        ps->setRenderSolids(o.drawsolids.on, &o.drawsolids.style);
    }
    if (const auto& m = o.mesh; m.dir) {
        uint32_t md[3]; float mo[3];
        if (sph_mesh_lattice(ps->context(), &m.params, md, mo) < 0) return fail("-mesh: %s\n", sph_last_error());
        if (mkdir(m.dir, 0755) != 0 && errno != EEXIST) return fail("-mesh=%s: cannot create the directory\n", m.dir);
        ps->setMeshParams(&m.params);
    }
    const float sp = ps->getParticleRadius() * 2.0f;      // the faucet's ball: as many lattice points as addSphere's loops accept
    if (const int er = o.emit.radius; o.emit.on)
        for (int z = -er; z <= er; z++)
            for (int y = -er; y <= er; y++)
                for (int x = -er; x <= er; x++) {
                    const float dx = x * sp, dy = y * sp, dz = z * sp;
                    if (sqrtf(dx * dx + dy * dy + dz * dz) <= ps->getParticleRadius() * 2.0f * er) run.ball_points++;
                }
    return true;
}

// before update i: the faucet, the kill volume, -add's particles, -sphere's ball
void before_update(const Options& o, Run& run, int i) {
    ParticleSystem* ps = run.ps;
    const float pr = ps->getParticleRadius();
    if (const auto& e = o.emit; e.on && i % e.every == 0) {       // unless a particle is still in the ball's place, or the capacity is used up
        sph_region nozzle = {SPH_REGION_SPHERE, {e.center[0], e.center[1], e.center[2]}, {0.f, 0.f, 0.f}, pr + (pr * 2.0f) * e.radius};
        const bool room = (uint64_t)ps->getNumParticles() + run.ball_points <= (uint64_t)ps->getCapacity() &&
                          (uint64_t)run.start + run.emitted + run.ball_points <= (uint64_t)ps->getCapacity();
        if (!room && !run.full_noted) { fprintf(stderr, "note: -emit stops at update %d: the capacity %d is used up (-capacity=)\n", i, ps->getCapacity()); run.full_noted = true; }
        if (room && ps->countParticles(&nozzle, 1) == 0) run.emitted += (uint)ps->emitSphere(e.center, e.velocity, e.radius, pr * 2.0f);
    }
    if (const auto& d = o.drain; d.on && i % d.every == 0) {
        sph_region kill = {SPH_REGION_BOX, {d.lo[0], d.lo[1], d.lo[2]}, {d.hi[0], d.hi[1], d.hi[2]}, 0.f};
        ps->removeParticles(&kill, 1);
    }
    if (i == o.add.at) {                 // at rest, at the points of sph_ic_random_box(seed 2024)
        const int count = o.add.count;
        std::vector<float> xyz((size_t)count * 3), xyzw((size_t)count * 4, 1.0f);
        const float dims[3] = {o.run.box, o.run.box, o.run.box};
        sph_ic_random_box((uint64_t)count, dims, 0.f, 2024u, 1.0f, xyz.data(), nullptr);
        for (int k = 0; k < count; k++) for (int a = 0; a < 3; a++) xyzw[4 * (size_t)k + a] = xyz[3 * (size_t)k + a];
        run.emitted += (uint)count;
        ps->addParticles(xyzw.data(), nullptr, count);
    }
    if (i == o.sphere.at) {              // the ball the GUI's key '4' drops (addSphere, particles.cpp:306-318), centred at the top instead of frand()
        const float tr = pr + (pr * 2.0f) * o.sphere.radius;
        float pos[4] = {0.0f, ps->getBoxMax().y - tr, 0.0f, 0.0f}, vel[4] = {0.f, 0.f, 0.f, 0.f};
        ps->addSphere(0, pos, vel, o.sphere.radius, pr * 2.0f);
    }
}

// after update i: its picture and its mesh, named by the 0-based number of the update
void after_update(const Options& o, Run& run, int i) {
    if (o.frames.dir && i % o.frames.every == 0) {
        const std::string path = std::string(o.frames.dir) + "/frame_" + std::to_string(1000000 + i % 1000000).substr(1) + ".ppm";
        run.ps->renderFrame();
        run.ps->writeFrame(path.c_str());
    }
    if (o.mesh.dir && i % o.mesh.every == 0) {
        const std::string path = std::string(o.mesh.dir) + "/mesh_" + std::to_string(100000 + i % 100000).substr(1) + ".obj";
        run.ps->writeMeshOBJ(path.c_str());
    }
}

bool report(const Options& o, Run& run, double secs) {
    ParticleSystem* ps = run.ps;
    if (o.grows()) printf("emitted %u particles, %d left of %u + %u\n", run.emitted, ps->getNumParticles(), run.start, run.emitted);
    print_result(run.particles, o.run.iterations, o.run.substeps, secs, 1, "");
    if (o.collider.has_mass) {       // floats with 9, doubles with 17 digits: they read back exactly
        double J[3]; ps->getColliderImpulse(J);
        const float3 cc = ps->getColliderPos(), cu = ps->getColliderVelocity();
        printf("collider: centre %.9g %.9g %.9g velocity %.9g %.9g %.9g impulse %.17g %.17g %.17g\n", cc.x, cc.y, cc.z, cu.x, cu.y, cu.z,
               J[0], J[1], J[2]);
    }
    if (o.solids()) {       // every installed slot: floats with 9, doubles with 17 digits
        uint32_t mask = 0;
        sph_obstacle_installed(ps->context(), &mask);
        for (uint k = 0; k < (uint)SPH_MAX_OBSTACLES; k++) {
            if (!(mask >> k & 1u)) continue;
            ps->selectObstacle(k);
            float off[3]; double q[4], J[3], L[3];
            sph_obstacle_get(ps->context(), nullptr, off, nullptr);
            sph_obstacle_get_pose(ps->context(), nullptr, nullptr, q, nullptr, nullptr);
            ps->getObstacleLoad(J, L);
            printf("solid %u: offset %.9g %.9g %.9g quaternion %.17g %.17g %.17g %.17g J %.17g %.17g %.17g L %.17g %.17g %.17g\n", k, off[0], off[1],
                   off[2], q[0], q[1], q[2], q[3], J[0], J[1], J[2], L[0], L[1], L[2]);
            if (o.solid[k].has_body) {      // where the fluid took it: the block, fetched
                float bo[3], bu[3], bw[3]; double bq[4];
                ps->getObstacleState(bo, bu, bq, bw);
                printf("solid %u body: offset %.9g %.9g %.9g velocity %.9g %.9g %.9g omega %.9g %.9g %.9g\n", k, bo[0], bo[1], bo[2], bu[0],
                       bu[1], bu[2], bw[0], bw[1], bw[2]);
            }
        }
        ps->selectObstacle(0);
    }
    if (o.mesh.dir) {       // the mesh of the final state through ParticleSystem::extractMesh: its size and an FNV-1a hash of its bytes
        std::vector<float> mp, mn; std::vector<uint32_t> mt;
        ps->extractMesh(mp, mn, mt);
        unsigned long long hsh = 1469598103934665603ull;
        auto mix = [&hsh](const void* data, size_t bytes) {
            const unsigned char* b = (const unsigned char*)data;
            for (size_t q = 0; q < bytes; q++) { hsh ^= b[q]; hsh *= 1099511628211ull; }
        };
        mix(mp.data(), mp.size() * 4); mix(mn.data(), mn.size() * 4); mix(mt.data(), mt.size() * 4);
        printf("mesh: %zu vertices, %zu triangles, fnv1a64 %016llx\n", mp.size() / 3, mt.size() / 3, hsh);
    }
    if (o.run.dump > 0) ps->dumpParticles(0, (uint)o.run.dump);
    if (o.run.out) {      // xyzw per creation index, then vxyz0, raw fp32
        FILE* f = fopen(o.run.out, "wb");
        if (!f) return fail("cannot open %s\n", o.run.out);
        const size_t rows = o.grows() ? (size_t)ps->getCapacity() : (size_t)run.particles;
        fwrite(ps->getArray(ParticleSystem::POSITION), sizeof(float) * 4, rows, f);
        fwrite(ps->getArray(ParticleSystem::VELOCITY), sizeof(float) * 4, rows, f);
        fclose(f);
    }
    if (o.run.save) ps->saveState(o.run.save);
    return true;
}

int run_one_device(const Options& o) {
    Run run;
    if (!set_up(o, run)) return EXIT_FAILURE;
    ParticleSystem* ps = run.ps;
    const uint3 g = ps->getGridSize();
    printf("Run %u particles simulation for %d iterations... (grid %ux%ux%u, box %g)\n\n", run.particles, o.run.iterations, g.x, g.y, g.z, o.run.box);
    if (o.run.warmup) ps->update(kTimestep, 0);           // warm-up step, not timed
    sph_sync(ps->context());
    const auto t0 = std::chrono::steady_clock::now();
    run.start = (uint)ps->getNumParticles();
    for (int i = 0; i < o.run.iterations; ++i) {
        before_update(o, run, i);
        ps->update(kTimestep, (float)i);
        after_update(o, run, i);
    }
    sph_sync(ps->context());
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!report(o, run, secs)) return EXIT_FAILURE;
    delete ps;
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    Options o;
    if (!parse_options(argc, argv, o)) return EXIT_FAILURE;
    if (o.run.help) { print_help(); return 0; }
    if (o.solidhelp) { print_solid_help(); return 0; }
    if (o.slabs.on) return run_slabs(slab_job(o), o.slabs.gpus, o.slabs.onegpu, o.run.device);
    return run_one_device(o);
}

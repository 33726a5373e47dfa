// observe_host_check.hip — the device-free helpers of gamd_amd/csrc/observe.hip (the sample clock, the five buffer tables, the
// k-vector lists and the argument blocks of the observers with a potential) exercised as a stand-alone host program, meant to
// be built with the host sanitizers.  No HIP call is made.
//
//   cd gamd_amd/csrc && S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all" &&
//   for f in report traj structure classical water_classical drive water_drive minimize water_minimize; do
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c $f.hip -o /tmp/ohc_$f.o || break; done &&
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c ../../tools/observe_host_check.hip -o /tmp/ohc_main.o &&
//   hipcc -fsanitize=address,undefined /tmp/ohc_main.o /tmp/ohc_report.o /tmp/ohc_traj.o /tmp/ohc_structure.o /tmp/ohc_classical.o \
//     /tmp/ohc_water_classical.o /tmp/ohc_drive.o /tmp/ohc_water_drive.o /tmp/ohc_minimize.o /tmp/ohc_water_minimize.o -o /tmp/ohc && /tmp/ohc
// (the parameter block of gamd_minimize has a program of its own: tools/minimize_host_check.cpp)
#include "../gamd_amd/csrc/observe.hip"

#include <cstdio>
#include <cstdlib>
#include <set>

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// one observer's clock against a plain count of completed steps
struct Model {
    SampleClock c;
    long long done = 0, since = 0, samples = 0;      // steps since create, steps since clear while armed, samples since clear
    void configure(long long interval) {             // what observer_configure does to the clock
        if (interval == 0) { c.interval = 0; return; }
        c.interval = 0; c.clear(); c.interval = c.sample_interval = interval;
        since = samples = 0;
    }
    void run(long long n_steps) {
        const long long before = c.taken(true);
        c.begin_run(n_steps);
        long long expect_ordinal = before;
        for (long long s = 0; s < n_steps; ++s) {
            const bool want = c.interval > 0 && (since + s + 1) % c.interval == 0;
            REQUIRE(c.sampled(s) == want);
            if (!want) continue;
            REQUIRE(c.completed(s) == since + s + 1);
            REQUIRE(c.ordinal(s) == expect_ordinal++);
            ++samples;
        }
        if (c.interval > 0) since += n_steps;
        done += n_steps;
        REQUIRE(c.taken(true) == samples && c.taken(false) == 0);
    }
};

static void check_clock() {
    Model m;
    m.run(7);                                                    // never configured: nothing sampled, nothing taken
    REQUIRE(m.c.g == 0 && m.c.taken(true) == 0);
    const long long intervals[] = {2, 3, 5, 1, 4096};
    const long long runs[] = {30, 1, 0, 7, 30, 2, 13};
    for (long long iv : intervals) {
        m.configure(iv);
        for (long long n : runs) m.run(n);
        REQUIRE(m.c.g == 83 && m.c.taken(true) == 83 / iv);
        m.configure(0);                                          // off: the count stays readable and stops growing
        m.run(11);
        REQUIRE(m.c.g == 83 && m.c.taken(true) == 83 / iv && !m.c.sampled(0));
    }
    m.configure(3);
    m.c.begin_run(0x3fffffff);                                   // the longest run gamd_md_run accepts, twice
    m.c.begin_run(0x3fffffff);
    REQUIRE(m.c.taken(true) == 2ll * 0x3fffffff / 3 && m.c.ordinal(0x3fffffff - 1) == m.c.taken(true) - 1);
    m.c.clear();
    REQUIRE(m.c.taken(true) == 0 && m.c.interval == 3);
}

static void check_kvectors() {
    for (int n2max : {0, 1, 9, 156, 256}) {
        const std::vector<int> kv = struct_kvectors(n2max);
        REQUIRE(kv.size() % 3 == 0);
        long long ball = 0;                                      // integer points with 0 < |n|^2 <= n2max
        for (int x = -16; x <= 16; ++x)
            for (int y = -16; y <= 16; ++y)
                for (int z = -16; z <= 16; ++z) ball += (x * x + y * y + z * z > 0 && x * x + y * y + z * z <= n2max) ? 1 : 0;
        REQUIRE((long long)kv.size() / 3 * 2 == ball);
        std::set<std::array<int, 3>> seen;
        std::array<int, 4> prev{0, 0, 0, 0};
        for (size_t k = 0; k < kv.size(); k += 3) {
            const int x = kv[k], y = kv[k + 1], z = kv[k + 2], n2 = x * x + y * y + z * z;
            REQUIRE(n2 >= 1 && n2 <= n2max && (x != 0 ? x : (y != 0 ? y : z)) > 0);
            REQUIRE(!seen.count({-x, -y, -z}) && seen.insert({x, y, z}).second);
            const std::array<int, 4> key{n2, x, y, z};
            REQUIRE(prev < key);
            prev = key;
        }
        std::printf("n2max %3d: %zu k-vectors\n", n2max, kv.size() / 3);
    }
    REQUIRE(struct_kvectors(9).size() == 3 * 61 && struct_kvectors(1) == (std::vector<int>{0, 0, 1, 0, 1, 0, 1, 0, 0}));
}

static void check_tables() {
    gamd_handle h;
    h.n_boxes = 2; h.n_per_box = 258; h.n = 516; h.cfg.kind = GAMD_KIND_WATER;
    h.obs = observers_new();
    Recorder& rc = h.obs->rec;
    rc.max_frames = 8; rc.fields = GAMD_TRAJ_X | GAMD_TRAJ_IMAGE; rc.n_lags = 4; rc.subtract_com = 0;
    const ObsBufs t = traj_bufs(&h);
    std::set<DevBuf*> distinct;
    size_t scratch = 0;
    for (const ObsBuf& b : t) { distinct.insert(b.buf); scratch += b.cleared ? 0 : 1; }
    REQUIRE(distinct.size() == t.size() && scratch == 2);
    REQUIRE(t[1].buf == &rc.fx && t[1].want == sizeof(float) * 8 * 3 * 516 && t[2].want == 0 && t[3].want == 0);
    REQUIRE(t[4].buf == &rc.fimg && t[4].want == sizeof(int) * 8 * 3 * 516 && t[11].buf == &rc.ring_com && t[11].want == 0);
    REQUIRE(t[14].buf == &rc.msd && t[14].want == sizeof(double) * 2 * 2 * 4);
    StructSampler& sp = h.obs->ss;
    sp.bins = 64; sp.pairs = 3; sp.n_k = 61;
    const ObsBufs s = struct_bufs(&h);
    REQUIRE(s.size() == 4 && s[0].want == 8u * 2 * 3 * 64 && s[1].buf == &sp.kvec && !s[1].cleared && s[1].want == 4u * 3 * 61);
    REQUIRE(s[2].want == 8u * 2 * 2 * 2 * 2 * 61 && !s[2].cleared && s[3].want == 8u * 2 * 3 * 61 && s[3].cleared);
    Reporter& rp = h.obs->rep;
    rp.max_samples = 4096; rp.bins = 0; rp.pairs = 3;
    const ObsBufs r = report_bufs(&h);
    REQUIRE(r.size() == 4 && r[0].want == 8u * 4096 && r[1].want == 8u * 4096 * 2 && r[2].want == 0 && r[3].want == 8u * 2 && !r[3].cleared);
    // the observers with a potential: the common rows in the common order, water's own between them, sizes by the kernels' enums
    Classical& cl = h.obs->cl;
    cl.max_samples = 5;
    const size_t S = 32, blocks = 2;                             // two row tiles of 256: 32 slices of 17 atoms; two blocks per box
    REQUIRE(classical_tiles(&h) == 2 && classical_slices(&h) == (int)S && classical_chunk(&h) == 9 && classical_blocks(&h) == (int)blocks);
    const ObsBufs c = classical_bufs(&h);
    REQUIRE(c.size() == 7 && c[0].buf == &cl.steps && c[0].want == 8u * 5 && c[1].buf == &cl.rows && c[1].want == 8u * CLASSICAL_ROW * 2 * 5);
    REQUIRE(c[2].buf == &cl.part && c[2].want == 8u * CLASSICAL_PART * 516 * S && c[3].buf == &cl.f_cl && c[3].want == 8u * 3 * 516);
    REQUIRE(c[4].buf == &cl.blk && c[4].want == 8u * CLASSICAL_ROW * 2 * blocks && c[5].buf == &cl.eval_rows && c[5].want == 8u * CLASSICAL_ROW * 2);
    REQUIRE(c[6].buf == &cl.eval_box && c[6].want == 4u * 3 * 2);
    for (size_t k = 0; k < c.size(); ++k) REQUIRE(c[k].cleared == (k < 2));
    WaterClassical& wc = h.obs->wc;
    wc.max_samples = 3; wc.n_k = 61;
    const ObsBufs w = water_bufs(&h);
    DevBuf* const order[] = {&wc.steps, &wc.rows, &wc.part, &wc.rpart, &wc.f_cl, &wc.blk, &wc.kvec, &wc.rho_partial, &wc.sk, &wc.ublk,
                             &wc.eval_rows, &wc.eval_box};
    const size_t want[] = {8u * 3, 8u * WATER_ROW * 2 * 3, 8u * WATER_PART * 516 * S, 8u * 3 * 516 * S, 8u * 3 * 516, 8u * WATER_ACC * 2 * blocks,
                           4u * 3 * 61, 8u * 2 * 2 * 2 * 61, 8u * 3 * 2 * 61, 8u * 2 * 1, 8u * WATER_ROW * 2, 4u * 3 * 2};
    REQUIRE(w.size() == 12 && struct_rho_blocks(&h) == 2 && water_kchunk(&h, 61) == 2);
    for (size_t k = 0; k < w.size(); ++k) REQUIRE(w[k].buf == order[k] && w[k].want == want[k] && w[k].cleared == (k < 2));
    // no buffer sits in two tables or twice in one
    distinct.clear();
    for (const ObsBufs* tab : {&t, &s, &r, &c, &w})
        for (const ObsBuf& b : *tab) distinct.insert(b.buf);
    REQUIRE(distinct.size() == t.size() + s.size() + r.size() + c.size() + w.size());
    // the five clocks are five objects, and the list hands them out in the order of the samples on the stream
    const auto list = observer_list(&h);
    REQUIRE(list[OBS_REPORT].clock == &rp.clock && list[OBS_TRAJ].clock == &rc.clock && list[OBS_STRUCT].clock == &sp.clock);
    REQUIRE(list[OBS_CLASSICAL].clock == &cl.clock && list[OBS_WATER].clock == &wc.clock && list.size() == 5);
    REQUIRE(list[OBS_REPORT].bufs == report_bufs && list[OBS_TRAJ].bufs == traj_bufs && list[OBS_STRUCT].bufs == struct_bufs &&
            list[OBS_CLASSICAL].bufs == classical_bufs && list[OBS_WATER].bufs == water_bufs);
    REQUIRE(list[OBS_CLASSICAL].check_run == LjPotential::check_box && list[OBS_WATER].check_run == water_check_run);
    rp.clock.interval = rp.clock.sample_interval = 2; rc.clock.interval = rc.clock.sample_interval = 3;
    const float box[6] = {20.f, 20.f, 20.f, 21.f, 21.f, 21.f};
    observers_begin_run(&h, box, nullptr, 6);
    REQUIRE(observers_sampled(&h, 1) && observers_sampled(&h, 2) && !observers_sampled(&h, 0) && !observers_sampled(&h, 4));
    REQUIRE(rp.clock.g == 6 && rc.clock.g == 6 && sp.clock.g == 0 && rc.classes == 1 && rc.box0.size() == 6);
    REQUIRE(cl.clock.g == 0 && wc.clock.g == 0);
    observers_free(&h);                                          // nothing was allocated: no HIP call
    REQUIRE(h.obs == nullptr);
}

// integer points with 0 < |n|^2 <= n2max
static long long ball(int n2max) {
    long long c = 0;
    for (int x = -42; x <= 42; ++x)
        for (int y = -42; y <= 42; ++y)
            for (int z = -42; z <= 42; ++z) c += (x * x + y * y + z * z > 0 && x * x + y * y + z * z <= n2max) ? 1 : 0;
    return c;
}

// water_klist: the bound follows the longest edge, the list is rebuilt only when the bound moves, and the refusals take nothing
static void check_klist() {
    const float box[6] = {20.f, 20.f, 20.f, 21.f, 20.f, 19.f};
    int n2max = -1;
    std::vector<int> kv;
    REQUIRE(water_klist(1.0, box, 2, &n2max, &kv) == 0);         // (21 / 2 pi)^2 = 11.17
    REQUIRE(n2max == 11 && (long long)kv.size() / 3 * 2 == ball(11) && kv == struct_kvectors(11));
    const std::vector<int> mark{7};
    kv = mark;                                                   // an unchanged bound returns without touching the list
    REQUIRE(water_klist(1.0, box, 2, &n2max, &kv) == 0 && n2max == 11 && kv == mark);
    const float wider[6] = {20.f, 21.5f, 20.f, 21.f, 20.f, 19.f}; // (21.5 / 2 pi)^2 = 11.71: the same bound
    REQUIRE(water_klist(1.0, wider, 2, &n2max, &kv) == 0 && n2max == 11 && kv == mark);
    const float longer[6] = {20.f, 20.f, 20.f, 21.f, 25.f, 19.f}; // (25 / 2 pi)^2 = 15.83: rebuilt
    REQUIRE(water_klist(1.0, longer, 2, &n2max, &kv) == 0 && n2max == 15 && (long long)kv.size() / 3 * 2 == ball(15));
    REQUIRE(water_klist(1.0, box, 1, &n2max, &kv) == 0 && n2max == 10 && (long long)kv.size() / 3 * 2 == ball(10));   // box 0 alone: 10.13
    // refusals: the bound past 1700, a list longer than WATER_MAX_K below it, and no vector at all; bound and list stay
    kv = mark; n2max = 11;
    REQUIRE(water_klist(13.0, box, 2, &n2max, &kv) == -22 && std::strstr(g_err, "gives more than 131072 k-vectors"));
    REQUIRE(ball(1650) / 2 > WATER_MAX_K);
    REQUIRE(water_klist(12.155, box, 2, &n2max, &kv) == -22 && std::strstr(g_err, ", more than 131072"));               // bound 1650
    REQUIRE(water_klist(0.1, box, 2, &n2max, &kv) == -22 && std::strstr(g_err, "admits no k-vector"));
    REQUIRE(n2max == 11 && kv == mark);
    std::printf("water_klist: %lld / %lld / %lld vectors for the bounds 10 / 11 / 15\n", ball(10) / 2, ball(11) / 2, ball(15) / 2);
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// potential_args: the two argument blocks get the same Lennard-Jones constants and geometry from the same parameters, for
// shift {on, off} x switch {on, off}; u0 is the pair term's own u at r_cut
static void check_args() {
    gamd_handle h;
    h.n_boxes = 2; h.n_per_box = 258; h.n = 516; h.cfg.kind = GAMD_KIND_WATER;
    h.obs = observers_new();
    Classical& cl = h.obs->cl;
    WaterClassical& wc = h.obs->wc;
    wc.q_h = 0.417; wc.alpha = 0.35; wc.k_cut = 3.0; wc.coulomb = 138.935456; wc.n_k = 61;
    for (int shift = 0; shift < 2; ++shift)
        for (double r_switch : {0.0, 8.5, 9.5, 11.0}) {          // off, on, and twice not below r_cut: off
            for (PotentialLog* pl : {static_cast<PotentialLog*>(&cl), static_cast<PotentialLog*>(&wc)}) {
                pl->sigma = 3.15075; pl->epsilon = 0.635968; pl->r_cut = 9.5; pl->r_switch = r_switch; pl->shift = shift;
            }
            const ClassicalArgs a = LjPotential::args(&h, 10.0);
            const WaterArgs b = WaterPotential::args(&h, 10.0);
            REQUIRE(same_bits(a.sig2, b.sig2) && same_bits(a.eps4, b.eps4) && same_bits(a.rc2, b.rc2) && same_bits(a.u0, b.u0));
            REQUIRE(same_bits(a.rs, b.rs) && same_bits(a.inv_w, b.inv_w) && same_bits(a.len, b.len) && a.len == 10.0);
            REQUIRE(a.tiles == b.tiles && a.slices == b.slices && a.chunk == b.chunk && a.blocks == b.blocks && a.n == 516 && b.n == 516);
            REQUIRE(a.tiles == 2 && a.slices == 32 && a.chunk == 9 && a.blocks == 2 && a.slices * a.chunk >= 258);
            REQUIRE(same_bits(a.eps24, 6.0 * b.eps4));           // what k_water_pairs passes for 24 epsilon
            const bool sw = r_switch == 8.5;
            REQUIRE(a.rs == (sw ? 8.5 : -1.0) && a.inv_w == (sw ? 1.0 : 0.0));
            const double s2 = a.sig2 * (1.0 / a.rc2), s6 = (s2 * s2) * s2;
            REQUIRE(same_bits(a.u0, shift ? a.eps4 * (s6 * s6 - s6) : 0.0) && (a.u0 < 0.0) == (shift != 0));
            REQUIRE(b.n_k == 61 && b.kslices == 32 && b.kchunk == 2 && b.kblocks == 1 && b.rho_blocks == 2 && same_bits(b.q_o, -2.0 * 0.417));
            REQUIRE(same_bits(b.coul, 138.935456 * 10.0) && a.bx.n_boxes == 2 && b.bx.n_per_box == 258 && !a.part && !b.rpart);
        }
    observers_free(&h);
}

// the classical force sources: which handles may take which, and the run check's refusals in front of any device work
static void check_drive() {
    gamd_handle h;
    h.n_boxes = 2; h.n_per_box = 258; h.n = 516; h.cfg.kind = GAMD_KIND_WATER;
    h.obs = observers_new();
    REQUIRE(h.force_source == GAMD_FORCE_NETWORK);
    REQUIRE(GAMD_FORCE_NETWORK == 0 && GAMD_FORCE_CLASSICAL == 1 && GAMD_FORCE_WATER_CLASSICAL == 2);
    REQUIRE(drive_check_source(&h, GAMD_FORCE_CLASSICAL) == -22 && std::strstr(g_err, "GAMD_KIND_WATER") && std::strstr(g_err, "GAMD_FORCE_WATER_CLASSICAL"));
    REQUIRE(drive_check_source(&h, GAMD_FORCE_WATER_CLASSICAL) == -22 && std::strstr(g_err, "gamd_water_configure"));
    h.cfg.kind = GAMD_KIND_LJ;
    REQUIRE(drive_check_source(&h, GAMD_FORCE_WATER_CLASSICAL) == -22 && std::strstr(g_err, "GAMD_KIND_LJ"));
    REQUIRE(drive_check_source(&h, GAMD_FORCE_CLASSICAL) == -22 && std::strstr(g_err, "gamd_classical_configure"));
    Classical& cl = h.obs->cl;
    cl.sigma = 3.4; cl.epsilon = 0.995792; cl.r_cut = 10.2; cl.r_switch = 6.8; cl.shift = 1; cl.params_set = true;
    REQUIRE(drive_check_source(&h, GAMD_FORCE_CLASSICAL) == 0);
    h.force_source = GAMD_FORCE_CLASSICAL;
    const float box[6] = {27.27f, 27.27f, 27.27f, 27.27f, 20.39f, 27.27f};     // box 1, edge 1 is below 2 r_cut = 20.4
    REQUIRE(drive_check_run(&h, box, nullptr) == -22 && std::strstr(g_err, "r_cut") && std::strstr(g_err, "box[1][1]"));
    cl.params_set = false;
    REQUIRE(drive_check_run(&h, box, nullptr) == -22 && std::strstr(g_err, "gamd_classical_configure"));
    REQUIRE(!cl.part.p && !cl.f_cl.p);                                          // a refused run allocated nothing
    // water: parameters, a pending run, species, the box rule — each in front of the k-vector list and of any allocation
    h.cfg.kind = GAMD_KIND_WATER;
    h.force_source = GAMD_FORCE_WATER_CLASSICAL;
    WaterClassical& wc = h.obs->wc;
    REQUIRE(drive_check_run(&h, box, nullptr) == -22 && std::strstr(g_err, "gamd_water_configure"));
    wc.q_h = 0.417; wc.sigma = 3.15075; wc.epsilon = 0.635968; wc.r_cut = 10.2; wc.r_switch = 0.0; wc.shift = 0;
    wc.alpha = 0.35; wc.k_cut = 3.0; wc.coulomb = 138.935456; wc.params_set = true;
    REQUIRE(drive_check_source(&h, GAMD_FORCE_WATER_CLASSICAL) == 0);
    h.pending.active = true;
    REQUIRE(drive_check_run(&h, box, nullptr) == -22 && std::strstr(g_err, "still enqueued"));
    h.pending.active = false;
    REQUIRE(drive_check_run(&h, box, nullptr) == -22 && std::strstr(g_err, "species"));
    const uint8_t* some_species = reinterpret_cast<const uint8_t*>(&h);        // only tested against null
    REQUIRE(drive_check_run(&h, box, some_species) == -22 && std::strstr(g_err, "r_cut") && std::strstr(g_err, "box[1][1]"));
    REQUIRE(wc.n2max == -1 && !wc.kvec.p && !wc.part.p && !wc.rpart.p && !wc.f_cl.p);   // a refused run built and allocated nothing
    observers_free(&h);
}

int main() {
    check_drive();
    check_clock();
    check_kvectors();
    check_tables();
    check_klist();
    check_args();
    std::printf("observe_host_check: ok\n");
    return 0;
}

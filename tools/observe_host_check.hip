// observe_host_check.hip — the device-free helpers of gamd_amd/csrc/observe.hip (the sample clock, the buffer tables and the
// k-vector list) exercised as a stand-alone host program, meant to be built with the host sanitizers.  No HIP call is made.
//
//   cd gamd_amd/csrc && S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all" &&
//   for f in report traj structure; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c $f.hip -o /tmp/ohc_$f.o; done &&
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c ../../tools/observe_host_check.hip -o /tmp/ohc_main.o &&
//   hipcc -fsanitize=address,undefined /tmp/ohc_main.o /tmp/ohc_report.o /tmp/ohc_traj.o /tmp/ohc_structure.o -o /tmp/ohc && /tmp/ohc
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
    // the three clocks are three objects, and the list hands them out in the order of the samples on the stream
    const auto list = observer_list(&h);
    REQUIRE(list[OBS_REPORT].clock == &rp.clock && list[OBS_TRAJ].clock == &rc.clock && list[OBS_STRUCT].clock == &sp.clock);
    rp.clock.interval = rp.clock.sample_interval = 2; rc.clock.interval = rc.clock.sample_interval = 3;
    const float box[6] = {20.f, 20.f, 20.f, 21.f, 21.f, 21.f};
    observers_begin_run(&h, box, nullptr, 6);
    REQUIRE(observers_sampled(&h, 1) && observers_sampled(&h, 2) && !observers_sampled(&h, 0) && !observers_sampled(&h, 4));
    REQUIRE(rp.clock.g == 6 && rc.clock.g == 6 && sp.clock.g == 0 && rc.classes == 1 && rc.box0.size() == 6);
    observers_free(&h);                                          // nothing was allocated: no HIP call
    REQUIRE(h.obs == nullptr);
}

int main() {
    check_clock();
    check_kvectors();
    check_tables();
    std::printf("observe_host_check: ok\n");
    return 0;
}

// observe.hip — host side of the run observers, the consumers at the sample point of an enqueued gamd_md_run / gamd_md_run_nhc
// (behind the second half of every interval-th step): the run reporter (gamd_report_*, report.hip), the run recorder
// (gamd_traj_*, traj.hip), the structure sampler (gamd_struct_*, structure.hip), the classical observer (gamd_classical_*,
// classical.hip; gamd_classical_eval runs its kernels outside a run) and the water classical observer (gamd_water_*,
// water_classical.hip; gamd_water_eval).  Each is its configuration plus a SampleClock,
// a buffer table and an entry in observer_list(), through which the MD driver of gamd_api.hip sees it (observers_*, gamd_host.h).
// The last two are observers with a potential: a PotentialLog and a traits struct (LjPotential, WaterPotential) behind one
// sample, one read call and one eval call (potential_*).
#include "gamd_host.h"
#include "gamd_minimize_host.h"
#include "gamd_lbfgs_host.h"
#include "gamd_pme_dev.h"
#include "gamd_cells_dev.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>

namespace {

// Every observer counts the completed MD steps of the runs it was armed for by itself and samples the multiples of its interval.
struct SampleClock {
    long long interval = 0;            // 0: off — nothing is enqueued
    long long sample_interval = 0;     // the interval g was counted with (stays when the observer is switched off: what it took stays readable)
    long long g = 0;                   // completed MD steps since configure / reset, runs still in the stream included
    long long g0 = 0;                  // the same in front of the pending run's first step
    long long completed(long long s) const { return g0 + s + 1; }          // step s of the pending run completes as ...
    bool sampled(long long s) const { return interval > 0 && completed(s) % interval == 0; }
    // the sample's ordinal, chosen on the host: a sample enqueued again after a freeze writes the same row
    long long ordinal(long long s) const { return completed(s) / interval - 1; }
    void begin_run(long long n_steps) { g0 = g; if (interval > 0) g += n_steps; }
    // samples since configure / reset; readable: the observer still holds what it took (each has its own test)
    long long taken(bool readable) const { return (sample_interval > 0 && readable) ? g / sample_interval : 0; }
    void clear() { g = 0; }
};

// buffer table entry: want = bytes under the current configuration (0: not needed); cleared: zeroed by configure / reset
// (the partial-sum scratch and uploaded tables are not)
struct ObsBuf { DevBuf* buf; size_t want; bool cleared; };
using ObsBufs = std::vector<ObsBuf>;

// exact sizes (a smaller configuration after a larger one re-allocates: observer_clear and the read calls go by bytes)
int bufs_resize(const ObsBufs& bufs) {
    for (const ObsBuf& b : bufs) {
        if (b.buf->bytes != b.want) b.buf->release();
        if (b.want && b.buf->ensure(b.want, true)) return -12;
    }
    return 0;
}

// run reporter: configuration and the device-resident log / histogram
struct Reporter {
    SampleClock clock;
    long long max_samples = 0;
    double ndf = 0.0;
    int bins = 0, pairs = 1, exclude = 0;
    float rmax = 0.f;
    DevBuf steps, ke, counts, partial;
};

// run recorder: configuration, frames, image counters, ring and running sums
struct Recorder {
    SampleClock clock;
    long long max_frames = 0;
    int fields = 0, n_lags = 0, subtract_com = 0;
    int classes = 0;                   // 0: no run since configure / reset; else the classes of the first run
    std::vector<float> box0;           // [n_boxes][3] of the first run since configure / reset (empty: none yet)
    DevBuf steps, fx, fv, ff, fimg;    // frames
    DevBuf x_prev, image, ambiguous;
    DevBuf ring_x, ring_img, ring_v, ring_com, com_partial, corr_partial, msd, vacf, class_atoms;
};

// structure sampler: configuration, k-vector list, histogram and S(k) sums
struct StructSampler {
    SampleClock clock;
    int bins = 0, pairs = 1, exclude = 0, n_k = 0;
    float rmax = 0.f;
    std::vector<int> kvec_host;        // [n_k][3]
    DevBuf counts, kvec, rho_partial, sk_sum;
};

// What the observers with a potential share: the Lennard-Jones parameters (taken by every gamd_*_configure of theirs, armed or
// not), the log rows and the work buffers of one evaluation
struct PotentialLog {
    SampleClock clock;
    long long max_samples = 0;
    bool params_set = false;           // the eval call needs parameters, not an armed observer
    bool evaluated = false;            // f_cl holds the forces of a sample or an eval call
    double sigma = 0.0, epsilon = 0.0, r_cut = 0.0, r_switch = 0.0;
    int shift = 0;
    DevBuf steps, rows;                // log
    DevBuf part, f_cl, blk;            // one evaluation
    DevBuf eval_rows, eval_box;        // the eval call: its row and its box edges
};

// the cell table of a potential's pair pass (gamd_water_cells, gamd_classical_cells): the switch, and per box the tables
struct CellTables {
    bool cells = false;                // the pairs walk cell_table.hip's per-box table (water_cells.hip, classical_cells.hip)
    bool cells_sampled = false;        // ... and the table holds the atoms of a sample, an eval call, a driven step or a minimiser's pass
    int cell_cap = 0;                  // cells per box the tables have room for (grows with the boxes the handle is given)
    std::vector<float> cell_box;       // [n_boxes][3] the edges the last enqueued table is built for (what the read call goes by)
    double cell_rcut = 0.0;            // ... and its cutoff
    std::vector<float> cell_box_next;  // [n_boxes][3] the edges the tables are sized for: those of the next evaluation (cells_apply)
    // an evaluation is being enqueued under the cutoff r_cut: its table is the one a read call finds behind the stream
    void enqueued(double r_cut) { cell_box = cell_box_next; cell_rcut = r_cut; cells_sampled = true; }
    DevBuf cell_start, cell_fill;      // cells on: per box and cell
    DevBuf cell_of, cell_members, cell_order, cell_table;   // ... per atom
    // the switch off: no table, no room
    void drop() {
        cells = cells_sampled = false;
        cell_cap = 0; cell_box.clear(); cell_box_next.clear();
        for (DevBuf* b : {&cell_start, &cell_fill, &cell_of, &cell_members, &cell_order, &cell_table}) b->release();
    }
    // the table in force for an evaluation that is being enqueued under r_cut: its buffers, or null while the switch is off (b is
    // the caller's room for them)
    const CellTabBufs* bufs(double r_cut, int* sticky, CellTabBufs& b) {
        if (!cells) return nullptr;
        b = CellTabBufs{r_cut, cell_cap, sticky, cell_start.as<int>(), cell_fill.as<int>(), cell_of.as<int>(), cell_members.as<int>(),
                        cell_order.as<int>(), cell_table.as<CellTabAtom>()};
        enqueued(r_cut);
        return &b;
    }
    // ... whose pair rows are ONE slice
    template <typename Args>
    void one_slice(Args& a, int n_per_box) const { if (cells) { a.slices = 1; a.chunk = n_per_box; } }
};

// classical observer: Lennard-Jones and nothing else
struct Classical : PotentialLog, CellTables {};

// water classical observer: O-O Lennard-Jones plus the Ewald parameters, the k-vector list in force (built for the longest edge
// of the boxes of the last configure, run or gamd_water_eval) and the work buffers that go by it
struct WaterClassical : PotentialLog, CellTables {
    double q_h = 0.0, alpha = 0.0, k_cut = 0.0, coulomb = 0.0;
    int n2max = -1, n_k = 0;           // the list in force: every n with 0 < |n|^2 <= n2max (-1: none yet)
    DevBuf rpart;                      // one evaluation: per atom and k slice
    DevBuf kvec, rho_partial, sk, ublk;// ... per k-vector
    double w_h = 0.0;                  // gamd_water_msite: the hydrogens' weight of the TIP4P M-site, 0 = 3-site
    DevBuf sites, ljpart;              // w_h != 0: per atom, and per atom and pair slice (water_msite.hip)
    bool virial = false;               // gamd_water_virial: every sample also writes its row of vrows (water_virial.hip)
    bool vwork = false;                // the virial's work buffers are wanted: the log has been on, or gamd_water_virial_eval called
    DevBuf vrows;                      // the virial log, slot for slot with rows
    DevBuf vpart, vljpart, vublk, vblk, veval_rows;     // one evaluation, and the eval call's row
    int pme_order = 0, pme_n[3] = {0, 0, 0};            // gamd_water_pme: the spline order (0 = the plain sum) and the grid per box
    DevBuf pme_gq, pme_gc;             // order != 0: per box and grid point, the integer spread and the complex transform (water_pme.hip)
    DevBuf pme_tw, pme_mod;            // ... the twiddles and the three axes' moduli, uploaded by gamd_water_pme
    // (CellTables: gamd_water_cells)
    bool min_configured = false;       // gamd_water_minimize_potential: the minimisers follow the three switches above (water_relax.hip)
};

// energy minimiser (gamd_minimize, minimize.hip): no observer — no clock, no entry in observer_list() — but a user of the
// classical potential's parameters and work buffers with state of its own
struct Minimizer {
    DevBuf x64, v64, f64;              // [n][3] doubles
    DevBuf f32;                        // [n][3] floats: the force source's output in front of the per-box store
    DevBuf state, stopped, rows;
};

// L-BFGS energy minimisers (gamd_minimize_lbfgs, lbfgs.hip; gamd_water_minimize_lbfgs, water_lbfgs.hip): as Minimizer, with buffers
// of their own — gamd_minimize's and gamd_water_minimize's stay as they are
struct Lbfgs {
    DevBuf x, xt, f, ft, d;            // [n][3] doubles
    DevBuf ring;                       // [2 m][n][3] doubles, for the largest m a call has asked for
    DevBuf f32;                        // [n][3] floats: the force source's output in front of the per-box store
    DevBuf blk, state, gates, rows;
};

}  // namespace

struct Observers { Reporter rep; Recorder rec; StructSampler ss; Classical cl; WaterClassical wc; Minimizer mn; Lbfgs lb; };

namespace {

// blocks per box of k_report_ke, of k_traj_corr / k_traj_com and of k_struct_rho (fixed per handle: the summation trees never change)
int report_ke_blocks(const gamd_handle* h) { return std::max(1, std::min(64, (h->n_per_box + 1023) / 1024)); }
int traj_corr_blocks(const gamd_handle* h) { return std::max(1, std::min(16, (h->n_per_box + 1023) / 1024)); }
int struct_rho_blocks(const gamd_handle* h) { return std::max(1, std::min(64, (h->n_per_box + 255) / 256)); }

ObsBufs report_bufs(gamd_handle* h) {
    Reporter& rp = h->obs->rep;
    const size_t nb = (size_t)h->n_boxes, rows = (size_t)rp.max_samples;
    return {{&rp.steps, sizeof(long long) * rows, true}, {&rp.ke, sizeof(double) * rows * nb, true},
            {&rp.counts, sizeof(unsigned long long) * nb * (size_t)rp.pairs * (size_t)rp.bins, true},
            {&rp.partial, sizeof(double) * nb * (size_t)report_ke_blocks(h), false}};
}

ObsBufs traj_bufs(gamd_handle* h) {
    Recorder& rc = h->obs->rec;
    const size_t nb = (size_t)h->n_boxes, n3 = 3 * (size_t)h->n, fr = (size_t)rc.max_frames, lags = (size_t)rc.n_lags;
    const size_t cls = h->cfg.kind == GAMD_KIND_WATER ? 2 : 1, blocks = (size_t)traj_corr_blocks(h);
    auto frames = [&](int field, size_t elem) { return (rc.fields & field) ? elem * fr * n3 : 0; };
    return {{&rc.steps, sizeof(long long) * fr, true},
            {&rc.fx, frames(GAMD_TRAJ_X, sizeof(float)), true}, {&rc.fv, frames(GAMD_TRAJ_V, sizeof(float)), true},
            {&rc.ff, frames(GAMD_TRAJ_F, sizeof(float)), true}, {&rc.fimg, frames(GAMD_TRAJ_IMAGE, sizeof(int)), true},
            {&rc.x_prev, sizeof(float) * n3, true}, {&rc.image, sizeof(int) * n3, true}, {&rc.ambiguous, sizeof(unsigned long long), true},
            {&rc.ring_x, sizeof(float) * lags * n3, true}, {&rc.ring_img, sizeof(int) * lags * n3, true}, {&rc.ring_v, sizeof(float) * lags * n3, true},
            {&rc.ring_com, rc.subtract_com ? sizeof(double) * lags * nb * 3 : 0, true},
            {&rc.com_partial, rc.subtract_com ? sizeof(double) * nb * blocks * 4 : 0, false},
            {&rc.corr_partial, sizeof(double) * nb * lags * blocks * cls * 2, false},
            {&rc.msd, sizeof(double) * nb * cls * lags, true}, {&rc.vacf, sizeof(double) * nb * cls * lags, true},
            {&rc.class_atoms, lags ? sizeof(long long) * nb * cls : 0, true}};
}

ObsBufs struct_bufs(gamd_handle* h) {
    StructSampler& sp = h->obs->ss;
    const size_t nb = (size_t)h->n_boxes, K = (size_t)sp.n_k, cls = sp.pairs == 3 ? 2 : 1;
    return {{&sp.counts, sizeof(unsigned long long) * nb * (size_t)sp.pairs * (size_t)sp.bins, true},
            {&sp.kvec, sizeof(int) * 3 * K, false},                 // uploaded by gamd_struct_configure
            {&sp.rho_partial, sizeof(double) * 2 * nb * (size_t)struct_rho_blocks(h) * cls * K, false},
            {&sp.sk_sum, sizeof(double) * nb * (size_t)sp.pairs * K, true}};
}

// observers with a potential: J slices per row (258 atoms still fill more than two workgroups), atoms per slice, blocks of the
// per-atom pass — fixed per handle: the summation order never changes
int classical_tiles(const gamd_handle* h) { return (h->n_per_box + 255) / 256; }
int classical_slices(const gamd_handle* h) { const int T = classical_tiles(h); return std::max(1, std::min(32, (1024 + T - 1) / T)); }
int classical_chunk(const gamd_handle* h) { const int S = classical_slices(h); return (h->n_per_box + S - 1) / S; }
int classical_blocks(const gamd_handle* h) { return std::max(1, std::min(64, (h->n_per_box + 255) / 256)); }

// ... and the rows of their buffer tables: doubles per log row, per atom and slice, per box and block
ObsBufs potential_bufs(gamd_handle* h, PotentialLog& pl, size_t row, size_t part, size_t acc) {
    const size_t nb = (size_t)h->n_boxes, rows = (size_t)pl.max_samples, n = (size_t)h->n;
    return {{&pl.steps, sizeof(long long) * rows, true}, {&pl.rows, sizeof(double) * row * nb * rows, true},
            {&pl.part, sizeof(double) * part * n * (size_t)classical_slices(h), false},
            {&pl.f_cl, sizeof(double) * 3 * n, false},
            {&pl.blk, sizeof(double) * acc * nb * (size_t)classical_blocks(h), false},
            {&pl.eval_rows, sizeof(double) * row * nb, false}, {&pl.eval_box, sizeof(float) * 3 * nb, false}};
}

// the cell table's own: nothing while the pairs are walked all against all
void cell_bufs_append(gamd_handle* h, CellTables& ct, ObsBufs& t) {
    const size_t nb = (size_t)h->n_boxes, n = (size_t)h->n, c = ct.cells ? 1 : 0, cap = (size_t)ct.cell_cap;
    t.push_back({&ct.cell_start, c * sizeof(int) * nb * (cap + 1), false});
    t.push_back({&ct.cell_fill, c * sizeof(int) * nb * cap, false});
    for (DevBuf* b : {&ct.cell_of, &ct.cell_members, &ct.cell_order}) t.push_back({b, c * sizeof(int) * n, false});
    t.push_back({&ct.cell_table, c * sizeof(CellTabAtom) * n, false});
}

ObsBufs classical_bufs(gamd_handle* h) {
    ObsBufs t = potential_bufs(h, h->obs->cl, CLASSICAL_ROW, CLASSICAL_PART, CLASSICAL_ROW);
    cell_bufs_append(h, h->obs->cl, t);
    return t;
}

// energy minimiser: all of it work buffers (k_min_init writes every one in front of its first reader)
ObsBufs minimize_bufs(gamd_handle* h) {
    Minimizer& mn = h->obs->mn;
    const size_t nb = (size_t)h->n_boxes, n3 = 3 * (size_t)h->n;
    return {{&mn.x64, sizeof(double) * n3, false}, {&mn.v64, sizeof(double) * n3, false}, {&mn.f64, sizeof(double) * n3, false},
            {&mn.f32, sizeof(float) * n3, false}, {&mn.state, sizeof(double) * 2 * MIN_STATE * nb, false},
            {&mn.stopped, sizeof(int) * nb, false}, {&mn.rows, sizeof(double) * MIN_ROW * nb, false}};
}

// L-BFGS energy minimisers: all of it work buffers (k_lbfgs_init / k_wlb_init write what a pass reads in front of its first write);
// acc: the columns of the minimiser's block row (a handle is of one kind, so only one of the two ever sizes the buffers)
ObsBufs lbfgs_bufs(gamd_handle* h, int m, int acc) {
    Lbfgs& lb = h->obs->lb;
    const size_t nb = (size_t)h->n_boxes, n3 = 3 * (size_t)h->n;
    return {{&lb.x, sizeof(double) * n3, false}, {&lb.xt, sizeof(double) * n3, false}, {&lb.f, sizeof(double) * n3, false},
            {&lb.ft, sizeof(double) * n3, false}, {&lb.d, sizeof(double) * n3, false}, {&lb.ring, sizeof(double) * n3 * 2 * (size_t)m, false},
            {&lb.f32, sizeof(float) * n3, false}, {&lb.blk, sizeof(double) * (size_t)acc * nb * (size_t)classical_blocks(h), false},
            {&lb.state, sizeof(double) * 2 * LBFGS_SLOT * nb, false}, {&lb.gates, sizeof(int) * 2 * nb, false},
            {&lb.rows, sizeof(double) * LBFGS_ROW * nb, false}};
}

// water classical observer: the pair pass has the classical observer's tiles, slices and blocks; the k slices of the reciprocal
// force pass are as many as the pair slices, the blocks of the rho(k) pass the structure sampler's
int water_kchunk(const gamd_handle* h, int n_k) { const int S = classical_slices(h); return std::max(1, (n_k + S - 1) / S); }

size_t water_pme_blocks(const WaterClassical& wc) { return wc.pme_order ? (size_t)pme_blocks(wc.pme_n[0], wc.pme_n[1], wc.pme_n[2]) : 0; }

ObsBufs water_bufs(gamd_handle* h) {
    WaterClassical& wc = h->obs->wc;
    const size_t nb = (size_t)h->n_boxes, n = (size_t)h->n, K = (size_t)wc.n_k;
    ObsBufs t = potential_bufs(h, wc, WATER_ROW, WATER_PART, WATER_ACC);
    t.insert(t.begin() + 3, {&wc.rpart, sizeof(double) * 3 * n * (size_t)classical_slices(h), false});      // behind part
    t.insert(t.begin() + 6, {{&wc.kvec, sizeof(int) * 3 * K, false},                                         // behind blk; uploaded by water_klist_apply
                             {&wc.rho_partial, sizeof(double) * 2 * nb * (size_t)struct_rho_blocks(h) * K, false},
                             {&wc.sk, sizeof(double) * 3 * nb * K, false},
                             {&wc.ublk, sizeof(double) * nb * std::max((K + 255) / 256, water_pme_blocks(wc)), false}});
    // particle-mesh Ewald's own: nothing while the plain sum is in force
    const size_t G = wc.pme_order ? (size_t)wc.pme_n[0] * (size_t)wc.pme_n[1] * (size_t)wc.pme_n[2] : 0;
    t.push_back({&wc.pme_gq, sizeof(unsigned long long) * nb * G, false});
    t.push_back({&wc.pme_gc, sizeof(double) * 2 * nb * G, false});
    cell_bufs_append(h, wc, t);
    // the M-site's own: nothing while the potential is 3-site
    const size_t m = wc.w_h != 0.0 ? 1 : 0;
    t.push_back({&wc.sites, m * sizeof(double) * 3 * n, false});
    t.push_back({&wc.ljpart, m * sizeof(double) * W4_LJ * (n / 3) * (size_t)classical_slices(h), false});
    // the virial log's own: nothing until gamd_water_virial / gamd_water_virial_eval asks
    const size_t v = wc.vwork ? 1 : 0;
    t.push_back({&wc.vrows, (wc.virial ? 1 : 0) * sizeof(double) * WATER_VIR_ROW * nb * (size_t)wc.max_samples, true});
    t.push_back({&wc.vpart, v * sizeof(double) * WATER_VIR_PART * n * (size_t)classical_slices(h), false});
    t.push_back({&wc.vljpart, v * m * sizeof(double) * (n / 3) * (size_t)classical_slices(h), false});
    t.push_back({&wc.vublk, v * sizeof(double) * nb * ((K + 255) / 256), false});
    t.push_back({&wc.vblk, v * sizeof(double) * WATER_VIR_ACC * nb * (size_t)classical_blocks(h), false});
    t.push_back({&wc.veval_rows, v * sizeof(double) * WATER_VIR_ROW * nb, false});
    return t;
}

// the work buffers of a table only (the log is gamd_*_configure's)
int bufs_ensure_work(const ObsBufs& bufs) {
    for (const ObsBuf& b : bufs)
        if (!b.cleared && b.buf->ensure(b.want, true)) return -12;
    return 0;
}

// what every observer's argument block starts with
template <typename Args>
void sample_args(const gamd_handle* h, Args& a) { a.n = h->n; a.bx = box_ref(h); a.devflags = h->devflags.as<int>(); }

// v, species, masses (amu) and length unit of the pending run, whichever integrator carries it
struct Particles { const float* v; const uint8_t* species; double mass, mass_h, len; };
Particles pending_particles(const MdPending& p) {
    if (p.kind == 0) return {p.m.v, p.m.species, (double)p.mass, (double)p.mass_h, (double)p.m.len};
    return {p.a.v, p.a.species, (double)p.a.mass, (double)p.a.mass_h, (double)p.a.len};
}

// the reporter's sample of step s of the pending run, behind its second half: the kinetic-energy row and the frame's pair histogram
int enqueue_report_sample(gamd_handle* h, long long s) {
    const MdPending& p = h->pending;
    const Reporter& rp = h->obs->rep;
    const Particles pt = pending_particles(p);
    ReportArgs a{};
    sample_args(h, a);
    a.sticky = h->sticky_dev;
    a.v = pt.v; a.species = pt.species; a.len = pt.len; a.mass = pt.mass; a.mass_h = pt.mass_h;
    a.partial = rp.partial.as<double>();
    a.blocks = report_ke_blocks(h);
    a.steps = rp.steps.as<long long>();
    a.ke = rp.ke.as<double>();
    a.g = rp.clock.completed(s);
    a.slot = rp.clock.ordinal(s);
    int r;
    if (a.slot < rp.max_samples && (r = launch_report_ke(a, p.st))) return fail(-1, "reporter launch failed (%d)", r);
    if (rp.bins > 0) {
        a.counters = h->cur_counters;
        a.pos_s = h->pos_s.as<float4>();
        a.col = h->col.as<int>(); a.erow = h->erow.as<int>(); a.row_ptr = h->row_ptr.as<int>(); a.perm = h->perm.as<int>();
        a.e_cap = h->e_cap;
        for (int d = 0; d < 3; ++d) { a.box[d] = h->box[d]; a.half[d] = 0.5f * h->box[d]; }
        a.n_bins = rp.bins; a.n_pairs = rp.pairs;
        a.r_max = rp.rmax; a.bin_scale = (float)rp.bins;
        a.all_edges = rp.rmax >= h->cfg.cutoff ? 1 : 0;
        a.exclude_same_molecule = rp.exclude;
        a.counts = rp.counts.as<unsigned long long>();
        // ~16 edge slots per thread; every workgroup flushes its non-zero bins with one atomic each
        a.rdf_blocks = (int)std::max<long long>(1, std::min<long long>(h->n_cu, h->e_cap / h->n_boxes / 4096));
        if ((r = launch_report_rdf(a, p.st))) return fail(-1, "reporter launch failed (%d)", r);
    }
    return 0;
}

// the recorder's classes in a run: 2 = water with species (O, H), else 1
int traj_run_classes(const gamd_handle* h, const uint8_t* species_dev) { return (h->cfg.kind == GAMD_KIND_WATER && species_dev) ? 2 : 1; }

// the recorder's sample of step s of the pending run, behind its second half
int enqueue_traj_sample(gamd_handle* h, long long s) {
    const MdPending& p = h->pending;
    const Recorder& rc = h->obs->rec;
    const Particles pt = pending_particles(p);
    TrajArgs a{};
    sample_args(h, a);
    for (int d = 0; d < 3; ++d) a.box[d] = h->box[d];
    a.x = p.x; a.f = p.f;
    a.v = pt.v; a.species = pt.species; a.mass = pt.mass; a.mass_h = pt.mass_h;
    a.g = rc.clock.completed(s);
    a.q = rc.clock.ordinal(s);
    a.frame = a.q < rc.max_frames ? a.q : -1;
    a.steps = rc.steps.as<long long>();
    a.fx = rc.fx.as<float>(); a.fv = rc.fv.as<float>(); a.ff = rc.ff.as<float>(); a.fimg = rc.fimg.as<int>();
    a.x_prev = rc.x_prev.as<float>();
    a.image = rc.image.as<int>();
    a.ambiguous = rc.ambiguous.as<unsigned long long>();
    a.n_lags = rc.n_lags;
    a.classes = traj_run_classes(h, p.species);
    if (rc.n_lags > 0) {
        a.slot = (int)(a.q % rc.n_lags);
        a.active = (int)std::min<long long>(a.q, rc.n_lags - 1) + 1;
        a.subtract_com = rc.subtract_com;
        a.ring_x = rc.ring_x.as<float>(); a.ring_img = rc.ring_img.as<int>(); a.ring_v = rc.ring_v.as<float>();
        a.ring_com = rc.ring_com.as<double>();
        a.com_partial = rc.com_partial.as<double>();
        a.com_blocks = a.corr_blocks = traj_corr_blocks(h);
        a.corr_partial = rc.corr_partial.as<double>();
        a.msd = rc.msd.as<double>(); a.vacf = rc.vacf.as<double>();
        a.class_atoms = rc.class_atoms.as<long long>();
    }
    if (int r = launch_traj_sample(a, p.st)) return fail(-1, "recorder launch failed (%d)", r);
    return 0;
}

// the structure sampler's sample of the pending run, behind a second half (no row of its own: the host counts the frames)
int enqueue_struct_sample(gamd_handle* h, long long) {
    const MdPending& p = h->pending;
    const StructSampler& sp = h->obs->ss;
    StructArgs a{};
    sample_args(h, a);
    a.sticky = h->sticky_dev;
    for (int d = 0; d < 3; ++d) { a.box[d] = h->box[d]; a.half[d] = 0.5f * h->box[d]; }
    a.n_pairs = sp.pairs;
    int r;
    if (sp.bins > 0) {
        a.pos_s = h->pos_s.as<float4>();
        a.perm = h->perm.as<int>();
        a.n_bins = sp.bins;
        a.r_max = sp.rmax; a.bin_scale = (float)sp.bins;
        a.exclude_same_molecule = sp.exclude;
        a.tiles = (h->n_per_box + 255) / 256;
        a.counts = sp.counts.as<unsigned long long>();
        if ((r = launch_struct_pairs(a, p.st))) return fail(-1, "structure sampler launch failed (%d)", r);
    }
    if (sp.n_k > 0) {
        a.x = p.x;
        a.species = p.species;
        a.classes = sp.pairs == 3 ? 2 : 1;
        a.n_k = sp.n_k;
        a.kvec = sp.kvec.as<int>();
        a.rho_blocks = struct_rho_blocks(h);
        a.rho_partial = sp.rho_partial.as<double>();
        a.sk_sum = sp.sk_sum.as<double>();
        if ((r = launch_struct_sk(a, p.st))) return fail(-1, "structure sampler launch failed (%d)", r);
    }
    return 0;
}

// The fields the argument blocks of the observers with a potential share by name: the Lennard-Jones constants, the length
// unit, the geometry of the pair and per-atom passes and their work buffers.  Positions, forces, species, box and output row
// are the caller's.
template <typename Args>
void potential_args(const gamd_handle* h, const PotentialLog& pl, double len, Args& a) {
    sample_args(h, a);
    a.sig2 = pl.sigma * pl.sigma;
    a.eps4 = 4.0 * pl.epsilon;
    a.rc2 = pl.r_cut * pl.r_cut;
    a.u0 = 0.0;
    if (pl.shift) {                                         // u_LJ(r_cut) by gamd_lj_term's own operations (gamd_potential_dev.h)
        const double s2 = a.sig2 * (1.0 / a.rc2), s6 = (s2 * s2) * s2;
        a.u0 = a.eps4 * (s6 * s6 - s6);
    }
    const bool sw = pl.r_switch > 0.0 && pl.r_switch < pl.r_cut;
    a.rs = sw ? pl.r_switch : -1.0;
    a.inv_w = sw ? 1.0 / (pl.r_cut - pl.r_switch) : 0.0;
    a.len = len;
    a.tiles = classical_tiles(h); a.slices = classical_slices(h); a.chunk = classical_chunk(h); a.blocks = classical_blocks(h);
    a.part = pl.part.as<double>(); a.f_cl = pl.f_cl.as<double>(); a.blk = pl.blk.as<double>();
}

// one of each +-n with 0 < |n|^2 <= n2max, sorted by (|n|^2, nx, ny, nz) (defined below)
std::vector<int> struct_kvectors(int n2max);

enum { WATER_MAX_K = 131072 };

// water classical observer: the integer triples the boxes `box` ([n_boxes][3]) need under k_cut — every n with 0 < |n|^2 <=
// (k_cut Lmax / 2 pi)^2, Lmax the longest edge (a box gives the vectors beyond its own k_cut the weight zero on the device;
// the bound is taken a few ulp up so that no vector a box's own test admits is missing).  Host only.
int water_klist(double k_cut, const float* box, int n_boxes, int* n2max, std::vector<int>* kv) {
    double lmax = 0.0;
    for (int k = 0; k < 3 * n_boxes; ++k) lmax = std::max(lmax, (double)box[k]);
    const double m = k_cut * lmax / 6.283185307179586;
    const double m2 = m * m * (1.0 + 1e-12);
    // K grows as (2 pi / 3) n2max^1.5: 131 072 is passed near n2max = 1576
    if (!(m2 < 1700.0))
        return fail(-22, "water classical potential: k_cut = %g gives more than %d k-vectors in a box with an edge of %g", k_cut, (int)WATER_MAX_K, lmax);
    const int n2 = (int)std::floor(m2);
    if (n2 == *n2max) return 0;                             // the list in force
    std::vector<int> v = n2 > 0 ? struct_kvectors(n2) : std::vector<int>();
    if (v.empty()) return fail(-22, "water classical potential: k_cut = %g admits no k-vector in a box with an edge of %g", k_cut, lmax);
    if (v.size() / 3 > (size_t)WATER_MAX_K)
        return fail(-22, "water classical potential: k_cut = %g gives %zu k-vectors in a box with an edge of %g, more than %d", k_cut,
                    v.size() / 3, lmax, (int)WATER_MAX_K);
    *n2max = n2; kv->swap(v);
    return 0;
}

// ... and the list put in force: the k-dependent work buffers sized for it, the triples uploaded (on the handle's own stream,
// landed on return).  No run is pending.
int water_klist_apply(gamd_handle* h, int n2max, const std::vector<int>& kv) {
    WaterClassical& wc = h->obs->wc;
    if (n2max == wc.n2max) return 0;
    DeviceGuard guard(h->dev);
    InitStream init(h->init_stream);
    wc.n2max = -1;                                          // none, should anything below fail
    wc.n_k = (int)(kv.size() / 3);
    for (DevBuf* b : {&wc.kvec, &wc.rho_partial, &wc.sk, &wc.ublk}) b->release();
    if (bufs_ensure_work(water_bufs(h))) return fail(-12, "water classical potential allocation failed");
    HIP_TRY(init_upload(wc.kvec.p, kv.data(), sizeof(int) * kv.size()));
    wc.n2max = n2max;
    return 0;
}

// the cell tables (gamd_water_cells, gamd_classical_cells) of the potential `wc` (buffer table `bufs`) for the boxes `box`
// ([n_boxes][3], every edge at least 2 r_cut): room for the box with the most cells, the edges kept for the evaluations to come
// (the read call goes by those of the last evaluation that was enqueued, CellTables::enqueued).  The
// water potential's callers have no run pending; the Lennard-Jones potential's may (a run behind a run), and a table that
// would have to grow under an enqueued run is refused.
template <typename State>
int cells_apply(gamd_handle* h, State& wc, ObsBufs (*bufs)(gamd_handle*), const char* who, const float* box) {
    int cap = 1;
    for (int b = 0; b < h->n_boxes; ++b) {
        int nc[3];
        cap = std::max(cap, gamd_cells_count((double)box[3 * b], (double)box[3 * b + 1], (double)box[3 * b + 2], wc.r_cut, nc));
    }
    const bool grow = cap > wc.cell_cap || !wc.cell_start.p || !wc.cell_table.p;
    if (grow && h->pending.active)
        return fail(-22, "an MD run is still enqueued: call gamd_sync_status before a run whose boxes need larger cell tables (%d cells per box)", cap);
    wc.cell_box_next.assign(box, box + 3 * (size_t)h->n_boxes);
    if (!h->pending.active) wc.cells_sampled = false;       // (behind an enqueued run its table stays the one to read)
    if (grow) {
        DeviceGuard guard(h->dev);
        InitStream init(h->init_stream);
        const int before = wc.cell_cap;
        wc.cell_cap = std::max(cap, before);
        for (DevBuf* b : {&wc.cell_start, &wc.cell_fill}) b->release();
        if (bufs_ensure_work(bufs(h))) {
            wc.cell_cap = before;
            return fail(-12, "%s potential: allocation of the cell tables (%d cells per box, %d boxes) failed", who, cap, h->n_boxes);
        }
    }
    return 0;
}
// the two switches of the cell table, gamd_classical_cells and gamd_water_cells (`entry`; `conf`: the configure call the
// parameters come from): off drops the tables, on allocates what goes by the atoms — 44 bytes per atom; the per-cell tables are
// sized by the boxes of the next run, eval or minimise call (cells_apply)
template <typename State>
int cells_switch(gamd_handle* h, State& pl, ObsBufs (*bufs)(gamd_handle*), const char* entry, const char* conf, int32_t on) {
    if (!pl.params_set) return fail(-22, "%s needs the parameters of a %s call (interval 0 will do)", entry, conf);
    if (h->pending.active) return fail(-22, "an MD run is still enqueued: call gamd_sync_status before %s", entry);
    if (on != 0 && on != 1) return fail(-22, "%s: on = %d is not 0 (all pairs) or 1 (the cell table)", entry, (int)on);
    if (!on) { pl.drop(); return 0; }
    if (pl.cells) return 0;                                 // on already: the table of the last evaluation stays readable
    pl.cells = true;
    DeviceGuard guard(h->dev);
    InitStream init(h->init_stream);
    if (bufs_ensure_work(bufs(h))) {
        pl.drop();
        return fail(-12, "%s: allocation of the cell tables of %d atoms failed", entry, h->n);
    }
    return 0;
}

int water_cells_apply(gamd_handle* h, const float* box) { return cells_apply(h, h->obs->wc, water_bufs, "water classical", box); }

// every edge of every box the caller hands in
int check_box_positive(const gamd_handle* h, const float* box) {
    for (int k = 0; k < 3 * h->n_boxes; ++k)
        if (!(box[k] > 0.f)) return fail(-22, "box[%d][%d] = %g is not positive", k / 3, k % 3, (double)box[k]);
    return 0;
}

// the minimum image is the nearest image only inside the sphere of half the shortest edge
int potential_check_box(const gamd_handle* h, const PotentialLog& pl, const char* who, const float* box) {
    for (int k = 0; k < 3 * h->n_boxes; ++k)
        if (!(2.0 * pl.r_cut <= (double)box[k]))
            return fail(-22, "%s potential: r_cut = %g exceeds half of box[%d][%d] = %g (the minimum image is the nearest "
                             "image only below that)", who, pl.r_cut, k / 3, k % 3, (double)box[k]);
    return 0;
}

// What an observer with a potential supplies besides its entry in observer_list(): its name in the error texts and in the C
// ABI, the width of its log row and the column of it that only a frozen handle leaves NaN, its state, its argument block but
// for positions, forces, species, box and output row (potential_args plus what is its own), its launcher, and check_box():
// what a run or its eval call must bring, which may prepare the handle for these boxes (no run is pending).
struct LjPotential {
    using Args = ClassicalArgs;
    static constexpr const char* who = "classical";
    static constexpr const char* api = "gamd_classical";
    enum { ROW = CLASSICAL_ROW, FROZEN_COL = 2 };
    static Classical& state(const gamd_handle* h) { return h->obs->cl; }
    static ObsBufs bufs(gamd_handle* h) { return classical_bufs(h); }
    static Args args(gamd_handle* h, double len) {
        Args a{};
        potential_args(h, state(h), len, a);
        a.eps24 = 24.0 * state(h).epsilon;
        state(h).one_slice(a, h->n_per_box);                // gamd_classical_cells
        return a;
    }
    static void species(Args&, const uint8_t*) {}
    // the cell table in force (gamd_classical_cells), or null
    static const CellTabBufs* cell_bufs(const gamd_handle* h, CellTabBufs& b) { return state(h).bufs(state(h).r_cut, h->sticky_dev, b); }
    static int launch(const gamd_handle* h, const Args& a, hipStream_t st) {
        CellTabBufs b;
        return launch_classical(a, st, cell_bufs(h, b));
    }
    static int sample_extra(const gamd_handle*, const Args&, const Particles&, hipStream_t) { return 0; }
    static int check_box(gamd_handle* h, const float* box, const uint8_t*) {
        if (int r = potential_check_box(h, state(h), who, box)) return r;
        // the cell tables sized for these boxes (grown here when they need more)
        return state(h).cells ? cells_apply(h, state(h), classical_bufs, who, box) : 0;
    }
    // a force source as well (potential_drive): the forces alone, rounded to fp32, into the run's f
    static int drive(const gamd_handle* h, const Args& a, float* f_out, hipStream_t st) {
        CellTabBufs b;
        return launch_classical_drive(a, f_out, st, cell_bufs(h, b));
    }
};

struct WaterPotential {
    using Args = WaterArgs;
    static constexpr const char* who = "water classical";
    static constexpr const char* api = "gamd_water";
    enum { ROW = WATER_ROW, FROZEN_COL = 4 };
    static WaterClassical& state(const gamd_handle* h) { return h->obs->wc; }
    static ObsBufs bufs(gamd_handle* h) { return water_bufs(h); }
    static Args args(gamd_handle* h, double len) {
        const WaterClassical& wc = state(h);
        Args a{};
        potential_args(h, wc, len, a);
        const double pi = 3.141592653589793;
        a.q_h = wc.q_h; a.q_o = -2.0 * wc.q_h;
        a.coul = wc.coulomb * len;
        a.alpha = wc.alpha; a.two_a_rpi = (2.0 * wc.alpha) / std::sqrt(pi);
        a.kc2 = wc.k_cut * wc.k_cut; a.inv_4a2 = 1.0 / (4.0 * (wc.alpha * wc.alpha));
        a.two_pi = 2.0 * pi;
        a.coul4pi = (4.0 * pi) * a.coul; a.coul8pi = (8.0 * pi) * a.coul;
        a.self_c = (a.coul * wc.alpha) / std::sqrt(pi);
        a.n_k = wc.n_k; a.kslices = classical_slices(h); a.kchunk = water_kchunk(h, wc.n_k); a.kblocks = (wc.n_k + 255) / 256;
        a.rho_blocks = struct_rho_blocks(h);
        a.kvec = wc.kvec.as<int>();
        a.rho_partial = wc.rho_partial.as<double>(); a.sk = wc.sk.as<double>(); a.ublk = wc.ublk.as<double>();
        a.rpart = wc.rpart.as<double>();
        return a;
    }
    static void species(Args& a, const uint8_t* species_dev) { a.species = species_dev; }
    // the site model in force (gamd_water_msite): w_h = 0 is the 3-site launcher as it was
    static W4Args msite(const gamd_handle* h, const Args& a) {
        const WaterClassical& wc = state(h);
        return W4Args{a, wc.w_h, 1.0 - 2.0 * wc.w_h, (a.chunk + 2) / 3, wc.sites.as<double>(), wc.ljpart.as<double>()};
    }
    // particle-mesh Ewald in force (gamd_water_pme): `a` with one k slice and the convolution's blocks, the sites of the site model
    static PmeArgs pme(const gamd_handle* h, const Args& a) {
        const WaterClassical& wc = state(h);
        PmeArgs p{a, wc.w_h != 0.0 ? wc.sites.as<double>() : nullptr, wc.pme_order, wc.pme_n[0], wc.pme_n[1], wc.pme_n[2],
                  wc.pme_gq.as<unsigned long long>(), wc.pme_gc.as<double>(), wc.pme_tw.as<double>(), wc.pme_mod.as<double>()};
        p.w.kslices = 1; p.w.kblocks = (int)water_pme_blocks(wc);
        return p;
    }
    // (the cell table in force, gamd_water_cells: the pair rows are one slice, k_w4_lj's too)
    static int launch(const gamd_handle* h, Args a, hipStream_t st) {
        WaterClassical& wc = state(h);
        wc.one_slice(a, h->n_per_box);
        CellTabBufs cb;
        const CellTabBufs* c = wc.bufs(wc.r_cut, h->sticky_dev, cb);
        if (wc.pme_order) {
            const PmeArgs p = pme(h, a);
            return wc.w_h != 0.0 ? launch_w4_classical(msite(h, p.w), st, &p, c) : launch_water_classical(p.w, st, &p, c);
        }
        return wc.w_h != 0.0 ? launch_w4_classical(msite(h, a), st, nullptr, c) : launch_water_classical(a, st, nullptr, c);
    }
    // the virial's kernels behind launch() on the same argument block (water_virial.hip): the row of a.slot into `vrows`
    static int virial(const gamd_handle* h, const Args& a, const float* v, double mass_o, double mass_h, double* vrows, hipStream_t st) {
        const WaterClassical& wc = state(h);
        const bool m = wc.w_h != 0.0;
        return launch_water_virial(WVirArgs{a, wc.w_h, (classical_chunk(h) + 2) / 3, m ? wc.sites.as<double>() : nullptr, v, mass_o, mass_h,
                                            wc.vpart.as<double>(), m ? wc.vljpart.as<double>() : nullptr, wc.vublk.as<double>(),
                                            wc.vblk.as<double>(), vrows}, st);
    }
    // what a sample of a run adds while the virial log is on: v behind the step's second half, the reporter's masses
    static int sample_extra(const gamd_handle* h, const Args& a, const Particles& pt, hipStream_t st) {
        const WaterClassical& wc = state(h);
        if (!wc.virial) return 0;
        return virial(h, a, pt.v, pt.mass, pt.mass_h > 0.0 ? pt.mass_h : pt.mass, wc.vrows.as<double>(), st);
    }
    // species, 2 r_cut <= every edge, a k-vector list of at most 131 072 triples for these boxes (built and uploaded here when
    // the boxes need another one than the list in force)
    static int check_box(gamd_handle* h, const float* box, const uint8_t* species_dev) {
        WaterClassical& wc = state(h);
        if (!species_dev) return fail(-22, "water classical potential: the charges need species (O = 1, H = 0, atoms ordered O,H,H)");
        if (int r = potential_check_box(h, wc, who, box)) return r;
        if (wc.cells)                                       // the cell tables sized for these boxes (grown here when they need more)
            if (int r = water_cells_apply(h, box)) return r;
        if (wc.pme_order) return 0;                         // particle-mesh Ewald: no k-vector list, k_cut is not read
        int n2max = wc.n2max;
        std::vector<int> kv;
        if (int r = water_klist(wc.k_cut, box, h->n_boxes, &n2max, &kv)) return r;
        return water_klist_apply(h, n2max, kv);
    }
    // a force source as well (potential_drive): the forces alone, rounded to fp32, into the run's f
    static int drive(const gamd_handle* h, Args a, float* f_out, hipStream_t st) {
        WaterClassical& wc = state(h);
        wc.one_slice(a, h->n_per_box);
        CellTabBufs cb;
        const CellTabBufs* c = wc.bufs(wc.r_cut, h->sticky_dev, cb);
        if (wc.pme_order) {
            const PmeArgs p = pme(h, a);
            return wc.w_h != 0.0 ? launch_w4_drive(msite(h, p.w), f_out, st, &p, c) : launch_water_drive(p.w, f_out, st, &p, c);
        }
        return wc.w_h != 0.0 ? launch_w4_drive(msite(h, a), f_out, st, nullptr, c) : launch_water_drive(a, f_out, st, nullptr, c);
    }
};

// the sample of step s of the pending run, behind its second half: f holds the network forces at x
template <typename P>
int potential_sample(gamd_handle* h, long long s) {
    const MdPending& p = h->pending;
    PotentialLog& pl = P::state(h);
    if (pl.clock.ordinal(s) >= pl.max_samples) return 0;    // the log is full: counted as dropped by the read call
    typename P::Args a = P::args(h, pending_particles(p).len);
    for (int d = 0; d < 3; ++d) a.box[d] = h->box[d];
    a.x = p.x; a.f = p.f; P::species(a, p.species);
    a.rows = pl.rows.as<double>(); a.steps = pl.steps.as<long long>();
    a.g = pl.clock.completed(s);
    a.slot = pl.clock.ordinal(s);
    if (int r = P::launch(h, a, p.st)) return fail(-1, "%s observer launch failed (%d)", P::who, r);
    if (int r = P::sample_extra(h, a, pending_particles(p), p.st)) return fail(-1, "%s observer launch failed (%d)", P::who, r);
    pl.evaluated = true;
    return 0;
}

// the force evaluation of a classical-source step of the pending run (gamd_md_force_source), behind the step's neighbour
// stage: the potential's forces at the run's x, rounded to fp32, into the run's f.  No row, no clock: every step is driven.
template <typename P>
int potential_drive(gamd_handle* h, hipStream_t st) {
    const MdPending& p = h->pending;
    typename P::Args a = P::args(h, pending_particles(p).len);
    for (int d = 0; d < 3; ++d) a.box[d] = h->box[d];
    a.x = p.x; P::species(a, p.species);
    if (int r = P::drive(h, a, p.f, st)) return fail(-1, "%s force source launch failed (%d)", P::who, r);
    P::state(h).evaluated = true;
    return 0;
}

int water_check_run(gamd_handle* h, const float* box, const uint8_t* species_dev) {
    if (h->pending.active) return fail(-22, "an MD run is still enqueued: call gamd_sync_status before the next run of a handle whose water classical observer is on");
    return WaterPotential::check_box(h, box, species_dev);
}

// run recorder: image counters and ring are only meaningful in one box and with one set of classes
int traj_check_run(gamd_handle* h, const float* box, const uint8_t* species_dev) {
    const Recorder& rc = h->obs->rec;
    if (rc.n_lags > 0 && rc.classes && rc.classes != traj_run_classes(h, species_dev))
        return fail(-22, "run recorder: species given in one run and not in another since gamd_traj_configure / gamd_traj_reset");
    if ((rc.n_lags > 0 || (rc.fields & GAMD_TRAJ_IMAGE)) && !rc.box0.empty())
        for (size_t k = 0; k < rc.box0.size(); ++k)
            if (rc.box0[k] != box[k])
                return fail(-22, "run recorder: the box differs from the box of the first run since gamd_traj_configure / "
                                 "gamd_traj_reset (image counters and correlation functions need one box; call gamd_traj_reset)");
    return 0;
}
void traj_begin_run(gamd_handle* h, const float* box, const uint8_t* species_dev) {
    Recorder& rc = h->obs->rec;
    if (rc.clock.interval <= 0) return;
    if (rc.box0.empty()) rc.box0.assign(box, box + 3 * (size_t)h->n_boxes);
    if (!rc.classes) rc.classes = traj_run_classes(h, species_dev);
}
void traj_forget(gamd_handle* h) { h->obs->rec.classes = 0; h->obs->rec.box0.clear(); }

// structure sampler: the minimum image is the nearest image only inside the sphere of half the shortest edge, and the S(k)
// classes need the species in the caller's order
int struct_check_run(gamd_handle* h, const float* box, const uint8_t* species_dev) {
    const StructSampler& sp = h->obs->ss;
    if (sp.bins > 0)
        for (int k = 0; k < 3 * h->n_boxes; ++k)
            if (!(2.0f * sp.rmax <= box[k]))
                return fail(-22, "structure sampler: rdf_rmax = %g exceeds half of box[%d][%d] = %g (the minimum image is the nearest "
                                 "image only below that)", (double)sp.rmax, k / 3, k % 3, (double)box[k]);
    if (sp.n_k > 0 && sp.pairs == 3 && !species_dev)
        return fail(-22, "structure sampler: the partial structure factors of a water handle need species");
    return 0;
}

// What an observer supplies.  The order of the list is the order of the samples on the stream and of the run checks.
struct Observer {
    SampleClock* clock;
    ObsBufs (*bufs)(gamd_handle*);
    int (*sample)(gamd_handle*, long long s);                                        // armed and clock->sampled(s)
    int (*check_run)(gamd_handle*, const float* box, const uint8_t* species_dev);    // armed; may be null
    void (*begin_run)(gamd_handle*, const float* box, const uint8_t* species_dev);   // what it keeps of a run besides the clock; may be null
    void (*forget)(gamd_handle*);                                                    // ... and how configure / reset drop it; may be null
};
enum { OBS_REPORT = 0, OBS_TRAJ = 1, OBS_STRUCT = 2, OBS_CLASSICAL = 3, OBS_WATER = 4, OBS_COUNT = 5 };
std::array<Observer, OBS_COUNT> observer_list(const gamd_handle* h) {
    Observers& o = *h->obs;
    return {{{&o.rep.clock, report_bufs, enqueue_report_sample, nullptr, nullptr, nullptr},
             {&o.rec.clock, traj_bufs, enqueue_traj_sample, traj_check_run, traj_begin_run, traj_forget},
             {&o.ss.clock, struct_bufs, enqueue_struct_sample, struct_check_run, nullptr, nullptr},
             {&o.cl.clock, classical_bufs, potential_sample<LjPotential>, LjPotential::check_box, nullptr, nullptr},
             {&o.wc.clock, water_bufs, potential_sample<WaterPotential>, water_check_run, nullptr, nullptr}}};
}

// clear an observer's step count and what it took (configuration and scratch stay): on the init stream, landed on return
int observer_clear(gamd_handle* h, const Observer& ob) {
    ob.clock->clear();
    if (ob.forget) ob.forget(h);
    for (const ObsBuf& b : ob.bufs(h))
        if (b.cleared && b.buf->p) HIP_TRY(hipMemsetAsync(b.buf->p, 0, b.buf->bytes, tl_init_stream));
    HIP_TRY(hipStreamSynchronize(tl_init_stream));
    return 0;
}

// The common part of gamd_*_configure behind the checks of the parameter block.  apply() writes the new configuration into the
// observer's state, sizes its buffers (bufs_resize) and uploads what it needs on the device.
template <typename Apply>
int observer_configure(gamd_handle* h, int which, long long interval, const char* entry, Apply apply) {
    const Observer ob = observer_list(h)[which];
    if (h->pending.active) return fail(-22, "an MD run is still enqueued: call gamd_sync_status before %s", entry);
    if (interval == 0) { ob.clock->interval = 0; return 0; }        // off: what was recorded stays readable
    DeviceGuard guard(h->dev);
    InitStream init(h->init_stream);
    ob.clock->interval = 0;                                          // off, should anything below fail
    if (int r = apply()) return r;
    if (int r = observer_clear(h, ob)) return r;
    ob.clock->interval = ob.clock->sample_interval = interval;
    return 0;
}

int observer_reset(gamd_handle* h, int which, const char* entry) {
    if (!h) return fail(-22, "null handle");
    if (h->pending.active) return fail(-22, "an MD run is still enqueued: call gamd_sync_status before %s", entry);
    DeviceGuard guard(h->dev);
    InitStream init(h->init_stream);
    return observer_clear(h, observer_list(h)[which]);
}

// the grids of the all-pairs kernels: boxes in grid.y, and (tiles_who given) the upper triangle of 256-atom tiles in 24 bits
int check_boxes_tiles(const gamd_handle* h, const char* who, const char* tiles_who) {
    if (h->n_boxes > 65535) return fail(-22, "the %s needs n_boxes <= 65535", who);
    const long long T = (h->n_per_box + 255) / 256;
    if (tiles_who && T * (T + 1) / 2 > 0xffffffll) return fail(-22, "the %s needs at most 5791 tiles of 256 atoms per box", tiles_who);
    return 0;
}

// the tail of the gamd_*_configure of an observer with a potential, behind its parameters
template <typename P>
int potential_configure(gamd_handle* h, int which, long long interval, long long max_samples, const char* entry) {
    return observer_configure(h, which, interval, entry, [&]() {
        P::state(h).max_samples = max_samples > 0 ? max_samples : 4096;
        return bufs_resize(P::bufs(h)) ? fail(-12, "%s observer allocation failed", P::who) : 0;
    });
}

template <typename P>
int potential_read(gamd_handle* h, void* stream, int64_t* steps, double* rows, int64_t max_rows, int64_t* n_rows, int64_t* dropped,
                   double* f_cl, int64_t f_cl_elems) {
    if (!h) return fail(-22, "null handle");
    if (max_rows < 0) return fail(-22, "max_rows is negative");
    const PotentialLog& pl = P::state(h);
    DeviceGuard guard(h->dev);
    hipStream_t st = (hipStream_t)stream;
    const long long nb = h->n_boxes;
    const long long taken = pl.clock.taken(pl.steps.p != nullptr);
    const long long kept = std::min<long long>(taken, pl.max_samples);
    const long long n_copy = std::min<long long>(kept, max_rows);
    if (f_cl && f_cl_elems < 3ll * h->n) return fail(-22, "f_cl has room for %lld elements, the forces have %lld", (long long)f_cl_elems, 3ll * h->n);
    if (n_copy > 0 && steps) HIP_TRY(hipMemcpyAsync(steps, pl.steps.p, sizeof(int64_t) * (size_t)n_copy, hipMemcpyDeviceToHost, st));
    if (n_copy > 0 && rows) HIP_TRY(hipMemcpyAsync(rows, pl.rows.p, sizeof(double) * (size_t)(n_copy * nb * P::ROW), hipMemcpyDeviceToHost, st));
    if (f_cl && pl.evaluated && pl.f_cl.p) HIP_TRY(hipMemcpyAsync(f_cl, pl.f_cl.p, sizeof(double) * 3 * (size_t)h->n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (int t = check_traps(h)) return t;
    if (n_rows) *n_rows = kept;
    if (dropped) *dropped = taken - kept;
    return 0;
}

// the kernels of a sample on given positions, outside a run: the forces to f_out_dev (may be null), the row of every box to `row`;
// extra(a, st) enqueues what the caller adds behind them on the same argument block
template <typename P, typename Extra>
int potential_eval(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev, const float* box, float length_per_nm,
                   double* f_out_dev, std::vector<double>& row, void* stream, Extra extra) {
    if (!h) return fail(-22, "null handle");
    if (!pos_dev || !box) return fail(-22, "null argument");
    PotentialLog& pl = P::state(h);
    if (!pl.params_set) return fail(-22, "%s_eval needs the parameters of a %s_configure call (interval 0 will do)", P::api, P::api);
    if (h->pending.active) return fail(-22, "an MD run is still enqueued: call gamd_sync_status before %s_eval", P::api);
    if (int r = check_box_positive(h, box)) return r;
    if (int r = P::check_box(h, box, species_dev)) return r;
    DeviceGuard guard(h->dev);
    hipStream_t st = (hipStream_t)stream;
    InitStream init(st);
    if (bufs_ensure_work(P::bufs(h))) return fail(-12, "%s potential allocation failed", P::who);
    const size_t nb = (size_t)h->n_boxes;
    HIP_TRY(init_upload(pl.eval_box.p, box, sizeof(float) * 3 * nb));
    // a frozen handle's kernels return at once: the row would be what the last call left
    HIP_TRY(hipMemsetAsync(pl.eval_rows.p, 0xff, sizeof(double) * P::ROW * nb, st));
    typename P::Args a = P::args(h, length_per_nm > 0.f ? (double)length_per_nm : 10.0);
    a.box_edges = pl.eval_box.as<float>();
    a.x = pos_dev; a.f = nullptr; P::species(a, species_dev);
    a.rows = pl.eval_rows.as<double>(); a.steps = nullptr; a.slot = 0; a.g = 0;
    if (int r = P::launch(h, a, st)) return fail(-1, "%s potential launch failed (%d)", P::who, r);
    if (int r = extra(a, st)) return fail(-1, "%s potential launch failed (%d)", P::who, r);
    pl.evaluated = true;
    if (f_out_dev) HIP_TRY(hipMemcpyAsync(f_out_dev, pl.f_cl.p, sizeof(double) * 3 * (size_t)h->n, hipMemcpyDeviceToDevice, st));
    row = std::vector<double>(P::ROW * nb);
    HIP_TRY(hipMemcpyAsync(row.data(), pl.eval_rows.p, sizeof(double) * row.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (int t = check_traps(h)) return t;
    for (size_t b = 0; b < nb; ++b)
        if (std::isnan(row[P::ROW * b + P::FROZEN_COL]))
            return fail(-1, "%s_eval: the handle is frozen by a neighbour-buffer overflow (call gamd_sync_status)", P::api);
    return 0;
}

template <typename P>
int potential_eval(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev, const float* box, float length_per_nm,
                   double* f_out_dev, std::vector<double>& row, void* stream) {
    return potential_eval<P>(h, pos_dev, species_dev, box, length_per_nm, f_out_dev, row, stream,
                             [](const typename P::Args&, hipStream_t) { return 0; });
}

// What a minimiser supplies besides the potential it builds on: its name in the error texts, its argument block (the
// potential's, FIRE's and what is its own, which its entry point fills), its launchers, the code a frozen handle is refused with,
// and whether the caller's x64 is a copy behind the run (LJ) or written by its store-x kernel (water).
struct LjMinimizer {
    using P = LjPotential;
    using Args = MinArgs;
    static constexpr const char* api = "gamd_minimize";
    enum { FROZEN_CODE = -1, COPY_X64 = 1 };
    static P::Args& potential(Args& m) { return m.c; }
    static void route_args(const gamd_handle*, P::Args&) {}
    static int init(const gamd_handle*, const Args& m, const float* x, hipStream_t st) { return launch_minimize_init(m, x, st); }
    static int iter(const gamd_handle* h, const Args& m, hipStream_t st) {
        CellTabBufs b;
        return launch_minimize_iter(m, st, P::cell_bufs(h, b));
    }
    static int store_x(const gamd_handle*, const Args& m, float* x, double*, hipStream_t st) { return launch_minimize_store_x(m, x, st); }
};

// gamd_water_minimize_potential: what the two water minimisers share while the switch is on — the potential's block as the
// route leaves it (WaterPotential::launch's one pair slice under the cell table, WaterPotential::pme's one k slice and the
// convolution's blocks under particle-mesh Ewald), and the route of a pass (p, cb: the caller's room)
struct WaterRelax {
    static bool on(const gamd_handle* h) { return WaterPotential::state(h).min_configured; }
    static void route_args(const gamd_handle* h, WaterArgs& a) {
        const WaterClassical& wc = WaterPotential::state(h);
        if (!wc.min_configured) return;
        wc.one_slice(a, h->n_per_box);
        if (wc.pme_order) { a.kslices = 1; a.kblocks = (int)water_pme_blocks(wc); }
    }
    static WRxRoute route(const gamd_handle* h, const WaterArgs& a, PmeArgs& p, CellTabBufs& cb) {
        WaterClassical& wc = WaterPotential::state(h);
        const bool m = wc.w_h != 0.0;
        WRxRoute r{wc.w_h, m ? (a.chunk + 2) / 3 : 0, m ? wc.sites.as<double>() : nullptr, m ? wc.ljpart.as<double>() : nullptr, nullptr,
                   wc.bufs(wc.r_cut, h->sticky_dev, cb)};
        if (wc.pme_order) { p = WaterPotential::pme(h, a); r.pme = &p; }
        return r;
    }
};

struct WaterMinimizer {
    using P = WaterPotential;
    using Args = WMinArgs;
    static constexpr const char* api = "gamd_water_minimize";
    enum { FROZEN_CODE = -22, COPY_X64 = 0 };
    static P::Args& potential(Args& m) { return m.w; }
    static void route_args(const gamd_handle* h, P::Args& a) { WaterRelax::route_args(h, a); }
    static int init(const gamd_handle* h, const Args& m, const float* x, hipStream_t st) {
        return WaterRelax::on(h) ? launch_wmin_init_routed(m, x, st) : launch_wmin_init(m, x, st);
    }
    // the switch on: the route of the configured potential (water_relax.hip); off: the six launches as they were
    static int iter(const gamd_handle* h, const Args& m, hipStream_t st) {
        if (!WaterRelax::on(h)) return launch_wmin_iter(m, st);
        PmeArgs p; CellTabBufs cb;
        return launch_wrx_iter(m, WaterRelax::route(h, m.w, p, cb), st);
    }
    static int store_x(const gamd_handle* h, const Args& m, float* x, double* x64_out, hipStream_t st) {
        return WaterRelax::on(h) ? launch_wmin_store_x_routed(m, x, x64_out, st) : launch_wmin_store_x(m, x, x64_out, st);
    }
};

// The minimiser's run behind the checks that are its entry point's own: the boxes, every allocation, the look at the frozen
// flag, init, the iterations in chunks of check_every with a look at the gates behind each, the pass behind the last iteration,
// x, the force source's own kernels on exactly that x, f, the rows.  `m` arrives with what is the minimiser's own filled in.
template <typename M>
int minimize_run(gamd_handle* h, typename M::Args m, float* x_dev, const uint8_t* species_dev, const float* box, double len,
                 float* f_dev, double* x64_dev, const gamd_minimize_params& q, double* rows_host, void* stream) {
    using P = typename M::P;
    if (!x_dev || !f_dev || !box) return fail(-22, "null argument");
    if (int r = check_box_positive(h, box)) return r;
    if (int r = P::check_box(h, box, species_dev)) return r;
    PotentialLog& pl = P::state(h);
    DeviceGuard guard(h->dev);
    hipStream_t st = (hipStream_t)stream;
    InitStream init(st);
    // every allocation in front of the first enqueue
    if (bufs_ensure_work(P::bufs(h)) || bufs_ensure_work(minimize_bufs(h))) return fail(-12, "%s: allocation failed", M::api);
    const size_t nb = (size_t)h->n_boxes, n3 = 3 * (size_t)h->n;
    std::vector<int> stopped(nb, 0);
    std::vector<double> rows(MIN_ROW * nb, 0.0);
    HIP_TRY(init_upload(pl.eval_box.p, box, sizeof(float) * 3 * nb));
    // the force source's kernels return at once on a frozen handle: f would be what the last call left
    int frozen = 0;
    HIP_TRY(hipMemcpyAsync(&frozen, h->devflags.as<int>() + DEVFLAG_FROZEN, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (frozen) return fail(M::FROZEN_CODE, "%s: the handle is frozen by a neighbour-buffer overflow (call gamd_sync_status)", M::api);
    Minimizer& mn = h->obs->mn;
    typename P::Args& a = M::potential(m);
    a = P::args(h, len);
    a.box_edges = pl.eval_box.template as<float>();
    P::species(a, species_dev);
    const typename P::Args plain = a;                       // the force source's block behind the run
    M::route_args(h, a);
    FireArgs& fi = m.fire;
    fi.x64 = mn.x64.as<double>(); fi.v64 = mn.v64.as<double>(); fi.f64 = mn.f64.as<double>();
    fi.state = mn.state.as<double>(); fi.stopped = mn.stopped.as<int>(); fi.rows = mn.rows.as<double>();
    fi.tol = q.tolerance; fi.dt_start = q.dt_start; fi.dt_max = q.dt_max; fi.f_inc = q.f_inc; fi.f_dec = q.f_dec;
    fi.alpha_start = q.alpha_start; fi.f_alpha = q.f_alpha; fi.max_step = q.max_step; fi.n_min = q.n_min;
    int r;
    if ((r = M::init(h, m, x_dev, st))) return fail(-1, "%s launch failed (%d)", M::api, r);
    bool all_stopped = false;
    while (fi.it < q.max_iter && !all_stopped) {
        const long long chunk = std::min<long long>(q.check_every, q.max_iter - fi.it);
        for (long long k = 0; k < chunk; ++k, ++fi.it)
            if ((r = M::iter(h, m, st))) return fail(-1, "%s launch failed (%d)", M::api, r);
        HIP_TRY(hipMemcpyAsync(stopped.data(), mn.stopped.p, sizeof(int) * nb, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        all_stopped = std::all_of(stopped.begin(), stopped.end(), [](int s) { return s != 0; });
    }
    if (!all_stopped) {                                     // U and rms where max_iter left the boxes that still run
        fi.last = 1;
        if ((r = M::iter(h, m, st))) return fail(-1, "%s launch failed (%d)", M::api, r);
    }
    // x (and the water minimiser's x64), then the force source's own kernels on exactly that x
    if ((r = M::store_x(h, m, x_dev, x64_dev, st))) return fail(-1, "%s launch failed (%d)", M::api, r);
    typename P::Args drive = plain;
    drive.x = x_dev;
    if ((r = P::drive(h, drive, mn.f32.as<float>(), st))) return fail(-1, "%s launch failed (%d)", M::api, r);
    pl.evaluated = true;
    if ((r = launch_minimize_store_f(fi, a.n, a.bx, mn.f32.as<float>(), f_dev, st))) return fail(-1, "%s launch failed (%d)", M::api, r);
    if (M::COPY_X64 && x64_dev) HIP_TRY(hipMemcpyAsync(x64_dev, mn.x64.p, sizeof(double) * n3, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(rows.data(), mn.rows.p, sizeof(double) * rows.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (int t = check_traps(h)) return t;
    if (rows_host) std::memcpy(rows_host, rows.data(), sizeof(double) * rows.size());
    int worst = 0;
    for (size_t b = 0; b < nb; ++b) worst = std::max(worst, (int)rows[MIN_ROW * b]);
    return worst;
}

// What an L-BFGS minimiser supplies besides the potential it builds on, as LjMinimizer and WaterMinimizer do for FIRE: its name,
// its argument block (the potential's, the L-BFGS members — the same names in both — and what is its own, which its entry point
// fills), the columns of its block row, its launchers, the code a frozen handle is refused with, and whether the caller's x64 is
// a copy behind the run (LJ) or written by its store-x kernel (water).
struct LjLbfgs {
    using P = LjPotential;
    using Args = LbfgsArgs;
    static constexpr const char* api = "gamd_minimize_lbfgs";
    enum { FROZEN_CODE = -1, COPY_X64 = 1, ACC = LBFGS_ACC };
    static P::Args& potential(Args& l) { return l.c; }
    static void route_args(const gamd_handle*, P::Args&) {}
    static int init(const gamd_handle*, const Args& l, const float* x, hipStream_t st) { return launch_lbfgs_init(l, x, st); }
    static int eval(const gamd_handle* h, const Args& l, hipStream_t st) {
        CellTabBufs b;
        return launch_lbfgs_eval(l, st, P::cell_bufs(h, b));
    }
    static int store_x(const gamd_handle*, const Args& l, const int* gates, float* x, double*, hipStream_t st) {
        return launch_lbfgs_store_x(l, gates, x, st);
    }
};

struct WaterLbfgs {
    using P = WaterPotential;
    using Args = WLbfgsArgs;
    static constexpr const char* api = "gamd_water_minimize_lbfgs";
    enum { FROZEN_CODE = -22, COPY_X64 = 0, ACC = WLB_ACC };
    static P::Args& potential(Args& l) { return l.w; }
    static void route_args(const gamd_handle* h, P::Args& a) { WaterRelax::route_args(h, a); }
    static int init(const gamd_handle* h, const Args& l, const float* x, hipStream_t st) {
        return WaterRelax::on(h) ? launch_wlbfgs_init_routed(l, x, st) : launch_wlbfgs_init(l, x, st);
    }
    // the switch on: the route of the configured potential on the trial positions (water_relax.hip); off: the six launches as they were
    static int eval(const gamd_handle* h, const Args& l, hipStream_t st) {
        if (!WaterRelax::on(h)) return launch_wlbfgs_eval(l, st);
        PmeArgs p; CellTabBufs cb;
        return launch_wrx_eval(l, WaterRelax::route(h, l.w, p, cb), st);
    }
    static int store_x(const gamd_handle* h, const Args& l, const int* gates, float* x, double* x64_out, hipStream_t st) {
        return WaterRelax::on(h) ? launch_wlbfgs_store_x_routed(l, gates, x, x64_out, st) : launch_wlbfgs_store_x(l, gates, x, x64_out, st);
    }
};

// An L-BFGS entry behind the checks that need no device: minimize_run's order of things — the boxes, every allocation, the look
// at the frozen flag, init, the evaluations in chunks of check_every with a look at the gates behind each (pass max_iter stops
// every box that still runs), x (and the water minimiser's x64), the force source's own kernels on exactly that x, f, the rows.
// `l` arrives with what is the minimiser's own filled in.
template <typename M>
int lbfgs_run(gamd_handle* h, typename M::Args l, float* x_dev, const uint8_t* species_dev, const float* box, double len, float* f_dev,
              double* x64_dev, const gamd_lbfgs_params& q, double* rows_host, void* stream) {
    using P = typename M::P;
    static constexpr const char* api = M::api;
    if (!x_dev || !f_dev || !box) return fail(-22, "null argument");
    if (int r = check_box_positive(h, box)) return r;
    if (int r = P::check_box(h, box, species_dev)) return r;
    PotentialLog& pl = P::state(h);
    DeviceGuard guard(h->dev);
    hipStream_t st = (hipStream_t)stream;
    InitStream init(st);
    // every allocation in front of the first enqueue
    if (bufs_ensure_work(P::bufs(h)) || bufs_ensure_work(lbfgs_bufs(h, q.m, M::ACC))) return fail(-12, "%s: allocation failed", api);
    const size_t nb = (size_t)h->n_boxes, n3 = 3 * (size_t)h->n;
    std::vector<int> gates(nb, 0);
    std::vector<double> rows(LBFGS_ROW * nb, 0.0);
    HIP_TRY(init_upload(pl.eval_box.p, box, sizeof(float) * 3 * nb));
    // the force source's kernels return at once on a frozen handle: f would be what the last call left
    int frozen = 0;
    HIP_TRY(hipMemcpyAsync(&frozen, h->devflags.as<int>() + DEVFLAG_FROZEN, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (frozen) return fail(M::FROZEN_CODE, "%s: the handle is frozen by a neighbour-buffer overflow (call gamd_sync_status)", api);
    Lbfgs& lb = h->obs->lb;
    typename P::Args& a = M::potential(l);
    a = P::args(h, len);
    a.box_edges = pl.eval_box.template as<float>();
    P::species(a, species_dev);
    const typename P::Args plain = a;                       // the force source's block behind the run
    M::route_args(h, a);
    l.x = lb.x.as<double>(); l.xt = lb.xt.as<double>(); l.f = lb.f.as<double>(); l.ft = lb.ft.as<double>(); l.d = lb.d.as<double>();
    l.ring = lb.ring.as<double>(); l.blk = lb.blk.as<double>(); l.state = lb.state.as<double>(); l.gates = lb.gates.as<int>();
    l.rows = lb.rows.as<double>(); l.sticky = h->sticky_dev;
    l.tol = q.tolerance; l.max_step = q.max_step; l.c1 = q.c1; l.curv = q.curv; l.m = q.m; l.max_ls = q.max_ls; l.max_iter = q.max_iter;
    int r;
    if ((r = M::init(h, l, x_dev, st))) return fail(-1, "%s launch failed (%d)", api, r);
    bool all_stopped = false;
    while (l.it <= q.max_iter && !all_stopped) {            // pass 0 is the start's, pass k evaluation k
        const long long chunk = std::min<long long>(q.check_every, q.max_iter + 1 - l.it);
        for (long long k = 0; k < chunk; ++k, ++l.it)
            if ((r = M::eval(h, l, st))) return fail(-1, "%s launch failed (%d)", api, r);
        HIP_TRY(hipMemcpyAsync(gates.data(), lb.gates.as<int>() + (size_t)(l.it & 1) * nb, sizeof(int) * nb, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        all_stopped = std::all_of(gates.begin(), gates.end(), [](int s) { return s != 0; });
    }
    const int* gates_dev = lb.gates.as<int>() + (size_t)(l.it & 1) * nb;    // the set the last pass wrote
    // x (and the water minimiser's x64), then the force source's own kernels on exactly that x
    if ((r = M::store_x(h, l, gates_dev, x_dev, x64_dev, st))) return fail(-1, "%s launch failed (%d)", api, r);
    typename P::Args drive = plain;
    drive.x = x_dev;
    if ((r = P::drive(h, drive, lb.f32.as<float>(), st))) return fail(-1, "%s launch failed (%d)", api, r);
    pl.evaluated = true;
    FireArgs gate{};                                        // launch_minimize_store_f reads the gates alone: 1 + GAMD_MIN_FAILED is 1 + GAMD_LBFGS_FAILED
    gate.stopped = const_cast<int*>(gates_dev);
    if ((r = launch_minimize_store_f(gate, a.n, a.bx, lb.f32.as<float>(), f_dev, st))) return fail(-1, "%s launch failed (%d)", api, r);
    if (M::COPY_X64 && x64_dev) HIP_TRY(hipMemcpyAsync(x64_dev, lb.x.p, sizeof(double) * n3, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(rows.data(), lb.rows.p, sizeof(double) * rows.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (int t = check_traps(h)) return t;
    if (rows_host) std::memcpy(rows_host, rows.data(), sizeof(double) * rows.size());
    int worst = 0;
    for (size_t b = 0; b < nb; ++b) worst = std::max(worst, (int)rows[LBFGS_ROW * b]);
    return worst;
}

// What the two water minimisers refuse behind their parameter blocks and in front of the device, under the name of the entry:
// the geometry (0 = TIP3P, scaled by the unit), the handle's kind, the molecules, the potential's parameters, a pending run and
// the three forms of the potential the minimisers follow only while gamd_water_minimize_potential is on.  On 0 the unit-weight
// canonical triangle of SETTLE is in ra, rb, rc.
int water_minimize_checks(const char* api, gamd_handle* h, double len, double r_oh, double r_hh, double* ra, double* rb, double* rc) {
    if (!(r_oh >= 0.0) || !(r_hh >= 0.0) || !std::isfinite(r_oh) || !std::isfinite(r_hh))
        return fail(-22, "%s: r_oh = %g, r_hh = %g: a length is not positive", api, r_oh, r_hh);
    if (r_oh == 0.0) r_oh = 0.9572 * (len / 10.0);          // TIP3P, as the md parameter blocks document it
    if (r_hh == 0.0) r_hh = (2.0 * 0.9572 * std::sin(0.5 * 104.52 * (3.141592653589793 / 180.0))) * (len / 10.0);    // 1.5139 A
    if (!(r_hh < 2.0 * r_oh)) return fail(-22, "%s: r_hh = %g is not below 2 r_oh = %g: no such triangle", api, r_hh, 2.0 * r_oh);
    if (!h) return fail(-22, "null handle");
    if (h->cfg.kind != GAMD_KIND_WATER)
        return fail(-22, "%s: a GAMD_KIND_LJ handle has no molecules and no charges (GAMD_KIND_WATER handles only; "
                         "gamd_minimize relaxes Lennard-Jones boxes)", api);
    if (h->n_per_box % 3) return fail(-22, "%s: n_atoms = %d per box is not a multiple of 3 (atoms ordered O,H,H)", api, h->n_per_box);
    WaterClassical& wc = WaterPotential::state(h);
    if (!wc.params_set) return fail(-22, "%s needs the parameters of a gamd_water_configure call (interval 0 will do)", api);
    if (h->pending.active) return fail(-22, "an MD run is still enqueued: call gamd_sync_status before %s", api);
    if (!wc.min_configured) {                               // gamd_water_minimize_potential is off: the oldest form alone
        if (wc.w_h != 0.0)
            return fail(-22, "%s: the TIP4P M-site is set (gamd_water_msite, w_h = %.9g) and there is no 4-site rigid minimiser "
                             "while gamd_water_minimize_potential is off: switch it on, or minimise with w_h = 0, set the weight, "
                             "then take f from gamd_water_eval", api, wc.w_h);
        if (wc.pme_order)
            return fail(-22, "%s: particle-mesh Ewald is on (gamd_water_pme, order %d) and there is no PME minimiser while "
                             "gamd_water_minimize_potential is off: switch it on, or minimise under the plain sum, switch PME on, "
                             "then take f from gamd_water_eval", api, wc.pme_order);
        if (wc.cells)
            return fail(-22, "%s: the cell table is on (gamd_water_cells) and the minimiser's f is the all-pairs force bit for "
                             "bit while gamd_water_minimize_potential is off: switch it on, or minimise with the cells off, "
                             "switch them on, then take f from gamd_water_eval", api);
    }
    *rc = 0.5 * r_hh;
    const double t = std::sqrt(r_oh * r_oh - *rc * *rc);
    *ra = (2.0 * t) / 3.0; *rb = t / 3.0;
    return 0;
}

// one of each +-n with 0 < |n|^2 <= n2max (the one whose first non-zero component is positive), sorted by (|n|^2, nx, ny, nz)
std::vector<int> struct_kvectors(int n2max) {
    int m = 0;
    while ((m + 1) * (m + 1) <= n2max) ++m;
    std::vector<std::array<int, 4>> v;
    for (int x = 0; x <= m; ++x)
        for (int y = -m; y <= m; ++y)
            for (int z = -m; z <= m; ++z) {
                const int n2 = x * x + y * y + z * z;
                if (n2 == 0 || n2 > n2max) continue;
                const int lead = x != 0 ? x : (y != 0 ? y : z);
                if (lead > 0) v.push_back({n2, x, y, z});
            }
    std::sort(v.begin(), v.end());
    std::vector<int> out;
    for (const auto& e : v) { out.push_back(e[1]); out.push_back(e[2]); out.push_back(e[3]); }
    return out;
}

}  // namespace

// ---- towards the MD driver (gamd_host.h) ------------------------------------------------------------------------------------
Observers* observers_new() { return new Observers(); }

void observers_free(gamd_handle* h) {
    for (const Observer& ob : observer_list(h))
        for (const ObsBuf& b : ob.bufs(h)) b.buf->release();
    for (const ObsBuf& b : minimize_bufs(h)) b.buf->release();
    for (const ObsBuf& b : lbfgs_bufs(h, 0, 0)) b.buf->release();
    delete h->obs; h->obs = nullptr;
}

int observers_check_run(gamd_handle* h, const float* box, const uint8_t* species_dev) {
    for (const Observer& ob : observer_list(h))
        if (ob.check_run && ob.clock->interval > 0)
            if (int r = ob.check_run(h, box, species_dev)) return r;
    return 0;
}

void observers_begin_run(gamd_handle* h, const float* box, const uint8_t* species_dev, long long n_steps) {
    for (const Observer& ob : observer_list(h)) {
        if (ob.begin_run) ob.begin_run(h, box, species_dev);
        ob.clock->begin_run(n_steps);
    }
}

bool observers_sampled(const gamd_handle* h, long long s) {
    for (const Observer& ob : observer_list(h))
        if (ob.clock->sampled(s)) return true;
    return false;
}

int observers_enqueue(gamd_handle* h, long long s) {
    for (const Observer& ob : observer_list(h))
        if (ob.clock->sampled(s))
            if (int r = ob.sample(h, s)) return r;
    return 0;
}

// ---- the classical force sources (gamd_host.h): one traits entry per source, GAMD_FORCE_CLASSICAL (Lennard-Jones, GAMD_KIND_LJ
// handles) and GAMD_FORCE_WATER_CLASSICAL (3-site water, GAMD_KIND_WATER handles) -----------------------------------------------
int drive_check_source(gamd_handle* h, int source) {
    if (source == GAMD_FORCE_CLASSICAL) {
        if (h->cfg.kind != GAMD_KIND_LJ)
            return fail(-22, "gamd_md_force_source: a GAMD_KIND_WATER handle has no Lennard-Jones force source (that potential has no "
                             "electrostatics; GAMD_KIND_LJ handles only — GAMD_FORCE_WATER_CLASSICAL = 2 drives 3-site water)");
        if (!LjPotential::state(h).params_set)
            return fail(-22, "gamd_md_force_source: the classical source needs the parameters of a gamd_classical_configure call (interval 0 will do)");
        return 0;
    }
    if (source == GAMD_FORCE_WATER_CLASSICAL) {
        if (h->cfg.kind != GAMD_KIND_WATER)
            return fail(-22, "gamd_md_force_source: a GAMD_KIND_LJ handle has no molecules and no charges for the water classical "
                             "source (GAMD_KIND_WATER handles only — GAMD_FORCE_CLASSICAL = 1 drives Lennard-Jones)");
        if (!WaterPotential::state(h).params_set)
            return fail(-22, "gamd_md_force_source: the water classical source needs the parameters of a gamd_water_configure call (interval 0 will do)");
        return 0;
    }
    return fail(-22, "internal: force source %d has no potential", source);
}

namespace {
template <typename P>
int potential_drive_check_run(gamd_handle* h, const float* box, const uint8_t* species_dev) {
    if (int r = P::check_box(h, box, species_dev)) return r;
    DeviceGuard guard(h->dev);
    InitStream init(h->init_stream);
    if (bufs_ensure_work(P::bufs(h))) return fail(-12, "%s potential allocation failed", P::who);
    return 0;
}
}  // namespace

int drive_check_run(gamd_handle* h, const float* box, const uint8_t* species_dev) {
    if (int r = drive_check_source(h, h->force_source)) return r;
    if (h->force_source == GAMD_FORCE_CLASSICAL) return potential_drive_check_run<LjPotential>(h, box, species_dev);
    // the k-vector list may be swapped for these boxes: nothing of an earlier run may still read it
    if (h->pending.active) return fail(-22, "an MD run is still enqueued: call gamd_sync_status before the next run of a handle whose force source is the water classical potential");
    return potential_drive_check_run<WaterPotential>(h, box, species_dev);
}

int drive_enqueue(gamd_handle* h) {
    return h->force_source == GAMD_FORCE_WATER_CLASSICAL ? potential_drive<WaterPotential>(h, h->pending.st)
                                                         : potential_drive<LjPotential>(h, h->pending.st);
}

static_assert(sizeof(gamd_report_params) == 40 && offsetof(gamd_report_params, ndf) == 16 && offsetof(gamd_report_params, rdf_rmax) == 28,
              "gamd_report_params layout is part of the C ABI (gamd_amd/_lib.py mirrors it)");
static_assert(sizeof(gamd_traj_params) == 32 && offsetof(gamd_traj_params, fields) == 16 && offsetof(gamd_traj_params, n_lags) == 20 &&
              offsetof(gamd_traj_params, subtract_com) == 24,
              "gamd_traj_params layout is part of the C ABI (gamd_amd/_lib.py mirrors it)");
static_assert(sizeof(gamd_struct_params) == 32 && offsetof(gamd_struct_params, rdf_bins) == 8 && offsetof(gamd_struct_params, rdf_rmax) == 12 &&
              offsetof(gamd_struct_params, sk_n2max) == 20,
              "gamd_struct_params layout is part of the C ABI (gamd_amd/_lib.py mirrors it)");
static_assert(sizeof(gamd_classical_params) == 56 && offsetof(gamd_classical_params, sigma) == 16 && offsetof(gamd_classical_params, r_switch) == 40 &&
              offsetof(gamd_classical_params, shift) == 48,
              "gamd_classical_params layout is part of the C ABI (gamd_amd/_lib.py mirrors it)");
static_assert(GAMD_CLASSICAL_ROW == CLASSICAL_ROW, "the row of gamd_classical_read is the kernels' row");
static_assert(sizeof(gamd_water_params) == 88 && offsetof(gamd_water_params, q_h) == 16 && offsetof(gamd_water_params, r_switch) == 48 &&
              offsetof(gamd_water_params, shift) == 56 && offsetof(gamd_water_params, alpha) == 64 && offsetof(gamd_water_params, coulomb_const) == 80,
              "gamd_water_params layout is part of the C ABI (gamd_amd/_lib.py mirrors it)");
static_assert(GAMD_WATER_ROW == WATER_ROW, "the row of gamd_water_read is the kernels' row");
static_assert(GAMD_WATER_VIRIAL_ROW == WATER_VIR_ROW, "the row of gamd_water_virial_read is the kernels' row");
static_assert(sizeof(gamd_minimize_params) == 88 && offsetof(gamd_minimize_params, max_iter) == 8 && offsetof(gamd_minimize_params, dt_start) == 24 &&
              offsetof(gamd_minimize_params, max_step) == 72 && offsetof(gamd_minimize_params, n_min) == 80,
              "gamd_minimize_params layout is part of the C ABI (gamd_amd/_lib.py mirrors it)");
static_assert(GAMD_MINIMIZE_ROW == MIN_ROW && GAMD_MIN_CONVERGED == MIN_CONVERGED && GAMD_MIN_MAX_ITER == MIN_MAX_ITER && GAMD_MIN_FAILED == MIN_FAILED,
              "the row and the states of gamd_minimize are the kernels'");
static_assert(sizeof(gamd_lbfgs_params) == 64 && offsetof(gamd_lbfgs_params, max_iter) == 8 && offsetof(gamd_lbfgs_params, max_step) == 24 &&
              offsetof(gamd_lbfgs_params, m) == 48 && offsetof(gamd_lbfgs_params, max_ls) == 52 && offsetof(gamd_lbfgs_params, reserved) == 56,
              "gamd_lbfgs_params layout is part of the C ABI (gamd_amd/_lib.py mirrors it)");
static_assert(GAMD_LBFGS_ROW == LBFGS_ROW && GAMD_LBFGS_CONVERGED == LBFGS_CONVERGED && GAMD_LBFGS_MAX_ITER == LBFGS_MAX_ITER &&
              GAMD_LBFGS_FAILED == LBFGS_FAILED && GAMD_LBFGS_LINE_SEARCH == LBFGS_LINE_SEARCH && LBFGS_FAILED == MIN_FAILED,
              "the row and the states of gamd_minimize_lbfgs are the kernels'; a failed box's gate is gamd_minimize's");

extern "C" {

int32_t gamd_report_configure(gamd_handle* h, const gamd_report_params* p) {
    // the parameter block is checked first: these answers need no device
    if (!p) return fail(-22, "null argument");
    if (p->interval < 0) return fail(-22, "interval = %lld is negative", (long long)p->interval);
    if (p->max_samples < 0 || p->max_samples > (1ll << 24)) return fail(-22, "max_samples = %lld outside [0, 2^24]", (long long)p->max_samples);
    if (p->rdf_bins < 0 || p->rdf_bins > GAMD_HIST_MAX_BINS) return fail(-22, "rdf_bins = %d outside [0, %d]", (int)p->rdf_bins, GAMD_HIST_MAX_BINS);
    if (!(p->rdf_rmax >= 0.f)) return fail(-22, "rdf_rmax = %g is negative", (double)p->rdf_rmax);
    if (!(p->ndf >= 0.0)) return fail(-22, "ndf = %g is negative", p->ndf);
    if (!h) return fail(-22, "null handle");
    if (p->rdf_rmax > h->cfg.cutoff)
        return fail(-22, "rdf_rmax = %g exceeds the cutoff %g: pairs beyond it are not in the edge list", (double)p->rdf_rmax, (double)h->cfg.cutoff);
    return observer_configure(h, OBS_REPORT, p->interval, "gamd_report_configure", [&]() {
        Reporter& rp = h->obs->rep;
        rp.max_samples = p->max_samples > 0 ? p->max_samples : 4096;
        rp.ndf = p->ndf > 0.0 ? p->ndf : 3.0 * (double)h->n_per_box;
        rp.bins = p->rdf_bins;
        rp.pairs = h->cfg.kind == GAMD_KIND_WATER ? 3 : 1;
        rp.rmax = p->rdf_rmax > 0.f ? p->rdf_rmax : h->cfg.cutoff;
        rp.exclude = p->exclude_same_molecule ? 1 : 0;
        return bufs_resize(report_bufs(h)) ? fail(-12, "reporter allocation failed") : 0;
    });
}

int32_t gamd_report_reset(gamd_handle* h) { return observer_reset(h, OBS_REPORT, "gamd_report_reset"); }

int32_t gamd_report_read(gamd_handle* h, void* stream, int64_t* steps, double* ke, double* temperature, int64_t max_rows,
                         int64_t* n_rows, uint64_t* counts, int64_t count_elems, int64_t* frames, int64_t* dropped,
                         int32_t dims[3]) {
    if (!h) return fail(-22, "null handle");
    if (max_rows < 0) return fail(-22, "max_rows is negative");
    const Reporter& rp = h->obs->rep;
    DeviceGuard guard(h->dev);
    hipStream_t st = (hipStream_t)stream;
    const long long nb = h->n_boxes;
    const long long taken = rp.clock.taken(rp.steps.p != nullptr);
    const long long rows = std::min<long long>(taken, rp.max_samples);
    const long long n_copy = std::min<long long>(rows, max_rows);
    const long long elems = nb * (long long)rp.pairs * (long long)rp.bins;
    if (counts && rp.counts.p && count_elems < elems) return fail(-22, "counts has room for %lld elements, the histogram has %lld", (long long)count_elems, elems);
    if (n_copy > 0 && steps) HIP_TRY(hipMemcpyAsync(steps, rp.steps.p, sizeof(int64_t) * (size_t)n_copy, hipMemcpyDeviceToHost, st));
    if (n_copy > 0 && ke) HIP_TRY(hipMemcpyAsync(ke, rp.ke.p, sizeof(double) * (size_t)(n_copy * nb), hipMemcpyDeviceToHost, st));
    if (n_copy > 0 && temperature && !ke) return fail(-22, "temperature needs ke");
    if (counts && rp.counts.p && elems > 0) HIP_TRY(hipMemcpyAsync(counts, rp.counts.p, sizeof(uint64_t) * (size_t)elems, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (int t = check_traps(h)) return t;
    if (temperature)
        for (long long k = 0; k < n_copy * nb; ++k) temperature[k] = 2.0 * ke[k] / (rp.ndf * 0.00831446261815324);
    if (n_rows) *n_rows = rows;
    if (frames) *frames = (rp.bins > 0 && rp.counts.p) ? taken : 0;
    if (dropped) *dropped = taken - rows;
    if (dims) { dims[0] = (int32_t)nb; dims[1] = rp.pairs; dims[2] = rp.counts.p ? rp.bins : 0; }
    return 0;
}

int32_t gamd_traj_configure(gamd_handle* h, const gamd_traj_params* p) {
    if (!p) return fail(-22, "null argument");
    if (p->interval < 0) return fail(-22, "interval = %lld is negative", (long long)p->interval);
    if (p->max_frames < 0 || p->max_frames > (1ll << 24)) return fail(-22, "max_frames = %lld outside [0, 2^24]", (long long)p->max_frames);
    if (p->fields & ~(GAMD_TRAJ_X | GAMD_TRAJ_V | GAMD_TRAJ_F | GAMD_TRAJ_IMAGE)) return fail(-22, "fields = %d has unknown bits", (int)p->fields);
    if (p->n_lags < 0 || p->n_lags > 4096) return fail(-22, "n_lags = %d outside [0, 4096]", (int)p->n_lags);
    if (!h) return fail(-22, "null handle");
    if (p->n_lags > 0 && h->n_boxes > 65535) return fail(-22, "correlation functions need n_boxes <= 65535");
    return observer_configure(h, OBS_TRAJ, p->interval, "gamd_traj_configure", [&]() {
        Recorder& rc = h->obs->rec;
        rc.max_frames = p->max_frames;
        rc.fields = p->fields;
        rc.n_lags = p->n_lags;
        rc.subtract_com = (p->subtract_com && p->n_lags > 0) ? 1 : 0;
        return bufs_resize(traj_bufs(h)) ? fail(-12, "recorder allocation failed") : 0;
    });
}

int32_t gamd_traj_reset(gamd_handle* h) { return observer_reset(h, OBS_TRAJ, "gamd_traj_reset"); }

int32_t gamd_traj_read_frames(gamd_handle* h, void* stream, int64_t first, int64_t count, int64_t* steps, float* x, float* v,
                              float* f, int32_t* image, int64_t* n_frames, int64_t* dropped) {
    if (!h) return fail(-22, "null handle");
    if (first < 0 || count < 0) return fail(-22, "first / count is negative");
    const Recorder& rc = h->obs->rec;
    DeviceGuard guard(h->dev);
    hipStream_t st = (hipStream_t)stream;
    const long long taken = rc.clock.taken(rc.x_prev.p != nullptr);
    const long long kept = std::min<long long>(taken, rc.max_frames);
    const long long n_copy = std::max<long long>(0, std::min<long long>(kept - first, count));
    const size_t n3 = 3 * (size_t)h->n;
    if (n_copy > 0) {
        const size_t off = (size_t)first * n3, elems = (size_t)n_copy * n3;
        if (steps) HIP_TRY(hipMemcpyAsync(steps, rc.steps.as<long long>() + first, sizeof(int64_t) * (size_t)n_copy, hipMemcpyDeviceToHost, st));
        if (x && rc.fx.p) HIP_TRY(hipMemcpyAsync(x, rc.fx.as<float>() + off, sizeof(float) * elems, hipMemcpyDeviceToHost, st));
        if (v && rc.fv.p) HIP_TRY(hipMemcpyAsync(v, rc.fv.as<float>() + off, sizeof(float) * elems, hipMemcpyDeviceToHost, st));
        if (f && rc.ff.p) HIP_TRY(hipMemcpyAsync(f, rc.ff.as<float>() + off, sizeof(float) * elems, hipMemcpyDeviceToHost, st));
        if (image && rc.fimg.p) HIP_TRY(hipMemcpyAsync(image, rc.fimg.as<int>() + off, sizeof(int32_t) * elems, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (int t = check_traps(h)) return t;
    if (n_frames) *n_frames = kept;
    if (dropped) *dropped = taken - kept;
    return 0;
}

int32_t gamd_traj_read_dynamics(gamd_handle* h, void* stream, double* msd_sum, double* vacf_sum, int64_t elems, int64_t* n_samples,
                                uint64_t* ambiguous, int64_t* class_atoms, int32_t dims[3]) {
    if (!h) return fail(-22, "null handle");
    const Recorder& rc = h->obs->rec;
    DeviceGuard guard(h->dev);
    hipStream_t st = (hipStream_t)stream;
    const long long nb = h->n_boxes, cls = rc.msd.p ? rc.classes : 0, lags = rc.msd.p ? rc.n_lags : 0;
    const long long need = nb * cls * lags;
    if ((msd_sum || vacf_sum) && elems < need) return fail(-22, "msd_sum / vacf_sum have room for %lld elements, the sums have %lld", (long long)elems, need);
    if (need > 0 && msd_sum) HIP_TRY(hipMemcpyAsync(msd_sum, rc.msd.p, sizeof(double) * (size_t)need, hipMemcpyDeviceToHost, st));
    if (need > 0 && vacf_sum) HIP_TRY(hipMemcpyAsync(vacf_sum, rc.vacf.p, sizeof(double) * (size_t)need, hipMemcpyDeviceToHost, st));
    if (ambiguous) {
        *ambiguous = 0;
        if (rc.ambiguous.p) HIP_TRY(hipMemcpyAsync(ambiguous, rc.ambiguous.p, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    }
    if (class_atoms && nb * cls > 0) HIP_TRY(hipMemcpyAsync(class_atoms, rc.class_atoms.p, sizeof(int64_t) * (size_t)(nb * cls), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (int t = check_traps(h)) return t;
    if (n_samples) *n_samples = rc.clock.taken(rc.x_prev.p != nullptr);
    if (dims) { dims[0] = (int32_t)nb; dims[1] = (int32_t)cls; dims[2] = (int32_t)lags; }
    return 0;
}

int32_t gamd_struct_configure(gamd_handle* h, const gamd_struct_params* p) {
    if (!p) return fail(-22, "null argument");
    if (p->interval < 0) return fail(-22, "interval = %lld is negative", (long long)p->interval);
    if (p->rdf_bins < 0 || p->rdf_bins > GAMD_HIST_MAX_BINS) return fail(-22, "rdf_bins = %d outside [0, %d]", (int)p->rdf_bins, GAMD_HIST_MAX_BINS);
    if (p->rdf_bins > 0 && !(p->rdf_rmax > 0.f)) return fail(-22, "rdf_rmax = %g is not positive", (double)p->rdf_rmax);
    // K grows as (2 pi / 3) n2max^1.5: 4096 is passed near n2max = 156
    if (p->sk_n2max < 0 || p->sk_n2max > 256) return fail(-22, "sk_n2max = %d gives more than 4096 k-vectors (or is negative)", (int)p->sk_n2max);
    std::vector<int> kv = p->sk_n2max > 0 ? struct_kvectors(p->sk_n2max) : std::vector<int>();
    if (kv.size() / 3 > 4096) return fail(-22, "sk_n2max = %d gives %zu k-vectors, more than 4096", (int)p->sk_n2max, kv.size() / 3);
    if (!h) return fail(-22, "null handle");
    if (int r = check_boxes_tiles(h, "structure sampler", p->rdf_bins > 0 ? "pair histogram" : nullptr)) return r;
    return observer_configure(h, OBS_STRUCT, p->interval, "gamd_struct_configure", [&]() {
        StructSampler& sp = h->obs->ss;
        sp.bins = p->rdf_bins;
        sp.pairs = h->cfg.kind == GAMD_KIND_WATER ? 3 : 1;
        sp.rmax = p->rdf_rmax;
        sp.exclude = p->exclude_same_molecule ? 1 : 0;
        sp.n_k = (int)(kv.size() / 3);
        sp.kvec_host = kv;
        if (bufs_resize(struct_bufs(h))) return fail(-12, "structure sampler allocation failed");
        if (sp.n_k) HIP_TRY(init_upload(sp.kvec.p, kv.data(), sizeof(int) * kv.size()));
        return 0;
    });
}

int32_t gamd_struct_reset(gamd_handle* h) { return observer_reset(h, OBS_STRUCT, "gamd_struct_reset"); }

int32_t gamd_struct_read(gamd_handle* h, void* stream, uint64_t* counts, int64_t count_elems, double* sk_sum, int64_t sk_elems,
                         int32_t* kvec, int64_t kvec_elems, int64_t* frames, int32_t dims[4]) {
    if (!h) return fail(-22, "null handle");
    const StructSampler& sp = h->obs->ss;
    DeviceGuard guard(h->dev);
    hipStream_t st = (hipStream_t)stream;
    const long long nb = h->n_boxes, bins = sp.counts.p ? sp.bins : 0, K = sp.sk_sum.p ? sp.n_k : 0;
    const long long c_elems = nb * (long long)sp.pairs * bins, s_elems = nb * (long long)sp.pairs * K;
    if (counts && count_elems < c_elems) return fail(-22, "counts has room for %lld elements, the histogram has %lld", (long long)count_elems, c_elems);
    if (sk_sum && sk_elems < s_elems) return fail(-22, "sk_sum has room for %lld elements, the sums have %lld", (long long)sk_elems, s_elems);
    if (kvec && kvec_elems < 3 * K) return fail(-22, "kvec has room for %lld elements, the list has %lld", (long long)kvec_elems, 3 * K);
    if (counts && c_elems > 0) HIP_TRY(hipMemcpyAsync(counts, sp.counts.p, sizeof(uint64_t) * (size_t)c_elems, hipMemcpyDeviceToHost, st));
    if (sk_sum && s_elems > 0) HIP_TRY(hipMemcpyAsync(sk_sum, sp.sk_sum.p, sizeof(double) * (size_t)s_elems, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (int t = check_traps(h)) return t;
    if (kvec && K > 0) std::memcpy(kvec, sp.kvec_host.data(), sizeof(int32_t) * 3 * (size_t)K);
    if (frames) *frames = sp.clock.taken(bins > 0 || K > 0);
    if (dims) { dims[0] = (int32_t)nb; dims[1] = sp.pairs; dims[2] = (int32_t)bins; dims[3] = (int32_t)K; }
    return 0;
}

int32_t gamd_classical_configure(gamd_handle* h, const gamd_classical_params* p) {
    if (!p) return fail(-22, "null argument");
    if (p->interval < 0) return fail(-22, "interval = %lld is negative", (long long)p->interval);
    if (p->max_samples < 0 || p->max_samples > (1ll << 24)) return fail(-22, "max_samples = %lld outside [0, 2^24]", (long long)p->max_samples);
    if (!(p->sigma > 0.0) || !std::isfinite(p->sigma)) return fail(-22, "sigma = %g is not positive", p->sigma);
    if (!std::isfinite(p->epsilon)) return fail(-22, "epsilon = %g is not finite", p->epsilon);
    if (!(p->r_cut > 0.0) || !std::isfinite(p->r_cut)) return fail(-22, "r_cut = %g is not positive", p->r_cut);
    if (!(p->r_switch >= 0.0)) return fail(-22, "r_switch = %g is negative", p->r_switch);
    if (!h) return fail(-22, "null handle");
    if (h->cfg.kind != GAMD_KIND_LJ)
        return fail(-22, "classical potential: a GAMD_KIND_WATER handle needs electrostatics, which this Lennard-Jones potential does "
                         "not have (GAMD_KIND_LJ handles only; gamd_water_configure evaluates 3-site water)");
    if (int r = check_boxes_tiles(h, "classical observer", "classical observer")) return r;
    if (h->pending.active) return fail(-22, "an MD run is still enqueued: call gamd_sync_status before gamd_classical_configure");
    Classical& cl = h->obs->cl;
    cl.sigma = p->sigma; cl.epsilon = p->epsilon; cl.r_cut = p->r_cut; cl.r_switch = p->r_switch; cl.shift = p->shift ? 1 : 0;
    cl.params_set = true;
    return potential_configure<LjPotential>(h, OBS_CLASSICAL, p->interval, p->max_samples, "gamd_classical_configure");
}

int32_t gamd_classical_reset(gamd_handle* h) { return observer_reset(h, OBS_CLASSICAL, "gamd_classical_reset"); }

int32_t gamd_classical_read(gamd_handle* h, void* stream, int64_t* steps, double* rows, int64_t max_rows, int64_t* n_rows,
                            int64_t* dropped, double* f_cl, int64_t f_cl_elems) {
    return potential_read<LjPotential>(h, stream, steps, rows, max_rows, n_rows, dropped, f_cl, f_cl_elems);
}

int32_t gamd_classical_eval(gamd_handle* h, const float* pos_dev, const float* box, float length_per_nm, double* f_out_dev,
                            double* energy, double* virial, double* pairs, void* stream) {
    std::vector<double> row;
    if (int r = potential_eval<LjPotential>(h, pos_dev, nullptr, box, length_per_nm, f_out_dev, row, stream)) return r;
    for (int b = 0; b < h->n_boxes; ++b) {
        if (energy) energy[b] = row[CLASSICAL_ROW * b];
        if (virial) virial[b] = row[CLASSICAL_ROW * b + 1];
        if (pairs) pairs[b] = row[CLASSICAL_ROW * b + 2];
    }
    return 0;
}

namespace {
// what the two read calls of a cell table share: the table of box `box` of the potential `ct` (cutoff r_cut) to the host
int cells_read(gamd_handle* h, const CellTables& ct, const char* entry, const char* sw, void* stream, int32_t box, int32_t* nc,
               int32_t* start, int64_t max_start, int32_t* order, int64_t max_order) {
    if (!ct.cells) return fail(-22, "%s: the cell table is off (%s)", entry, sw);
    if (!ct.cells_sampled || ct.cell_box.size() != 3 * (size_t)h->n_boxes)
        return fail(-22, "%s: nothing has been sampled since the cell table was switched on or the boxes were given", entry);
    if (box < 0 || box >= h->n_boxes) return fail(-22, "%s: box = %d outside [0, %d)", entry, (int)box, h->n_boxes);
    if (!nc) return fail(-22, "null argument");
    const float* L = ct.cell_box.data() + 3 * (size_t)box;
    const long long cells = gamd_cells_count((double)L[0], (double)L[1], (double)L[2], ct.cell_rcut, nc);
    if (cells > ct.cell_cap) return fail(-1, "%s: %lld cells, the tables hold %d", entry, cells, ct.cell_cap);
    if (start && max_start < cells + 1) return fail(-22, "start has room for %lld elements, the box has %lld cells + 1", (long long)max_start, cells);
    if (order && max_order < h->n_per_box) return fail(-22, "order has room for %lld elements, a box has %d atoms", (long long)max_order, h->n_per_box);
    DeviceGuard guard(h->dev);
    hipStream_t st = (hipStream_t)stream;
    if (start)
        HIP_TRY(hipMemcpyAsync(start, ct.cell_start.as<int>() + (size_t)box * ((size_t)ct.cell_cap + 1), sizeof(int) * (size_t)(cells + 1),
                               hipMemcpyDeviceToHost, st));
    if (order)
        HIP_TRY(hipMemcpyAsync(order, ct.cell_order.as<int>() + (size_t)box * (size_t)h->n_per_box, sizeof(int) * (size_t)h->n_per_box,
                               hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (int t = check_traps(h)) return t;
    return 0;
}
}  // namespace

int32_t gamd_classical_cells(gamd_handle* h, int32_t on) {
    if (!h) return fail(-22, "null handle");
    if (h->cfg.kind != GAMD_KIND_LJ)
        return fail(-22, "gamd_classical_cells: a GAMD_KIND_WATER handle has no Lennard-Jones classical potential (GAMD_KIND_LJ handles "
                         "only; gamd_water_cells switches the cell table of the water classical potential)");
    return cells_switch(h, h->obs->cl, classical_bufs, "gamd_classical_cells", "gamd_classical_configure", on);
}

int32_t gamd_classical_cells_read(gamd_handle* h, void* stream, int32_t box, int32_t* nc, int32_t* start, int64_t max_start,
                                  int32_t* order, int64_t max_order) {
    if (!h) return fail(-22, "null handle");
    if (h->cfg.kind != GAMD_KIND_LJ) return fail(-22, "gamd_classical_cells_read: GAMD_KIND_LJ handles only");
    const Classical& cl = h->obs->cl;
    return cells_read(h, cl, "gamd_classical_cells_read", "gamd_classical_cells", stream, box, nc, start, max_start, order, max_order);
}

int32_t gamd_minimize(gamd_handle* h, float* x_dev, const float* box, float length_per_nm, float* f_dev, double* x64_dev,
                      const gamd_minimize_params* params, double* rows_host, void* stream) {
    // the parameter block is checked first: these answers need no device
    gamd_minimize_params q;
    if (int r = minimize_fill_params(params, &q, g_err, sizeof(g_err))) return r;
    if (!h) return fail(-22, "null handle");
    if (h->cfg.kind != GAMD_KIND_LJ)
        return fail(-22, "gamd_minimize: a GAMD_KIND_WATER handle has no classical potential to minimise (the Lennard-Jones "
                         "potential has no electrostatics; GAMD_KIND_LJ handles only)");
    Classical& cl = LjPotential::state(h);
    if (!cl.params_set) return fail(-22, "gamd_minimize needs the parameters of a gamd_classical_configure call (interval 0 will do)");
    if (h->pending.active) return fail(-22, "an MD run is still enqueued: call gamd_sync_status before gamd_minimize");
    return minimize_run<LjMinimizer>(h, MinArgs{}, x_dev, nullptr, box, length_per_nm > 0.f ? (double)length_per_nm : 10.0, f_dev, x64_dev, q,
                                     rows_host, stream);
}

int32_t gamd_minimize_lbfgs(gamd_handle* h, float* x_dev, const float* box, float length_per_nm, float* f_dev, double* x64_dev,
                            const gamd_lbfgs_params* params, double* rows_host, void* stream) {
    // the parameter block is checked first: these answers need no device
    gamd_lbfgs_params q;
    if (int r = lbfgs_fill_params(params, &q, g_err, sizeof(g_err))) return r;
    if (!h) return fail(-22, "null handle");
    if (h->cfg.kind != GAMD_KIND_LJ)
        return fail(-22, "gamd_minimize_lbfgs: a GAMD_KIND_WATER handle has no classical potential to minimise (the Lennard-Jones "
                         "potential has no electrostatics; GAMD_KIND_LJ handles only)");
    Classical& cl = LjPotential::state(h);
    if (!cl.params_set) return fail(-22, "gamd_minimize_lbfgs needs the parameters of a gamd_classical_configure call (interval 0 will do)");
    if (h->pending.active) return fail(-22, "an MD run is still enqueued: call gamd_sync_status before gamd_minimize_lbfgs");
    return lbfgs_run<LjLbfgs>(h, LbfgsArgs{}, x_dev, nullptr, box, length_per_nm > 0.f ? (double)length_per_nm : 10.0, f_dev, x64_dev, q, rows_host, stream);
}

int32_t gamd_water_configure(gamd_handle* h, const gamd_water_params* p) {
    if (!p) return fail(-22, "null argument");
    if (p->interval < 0) return fail(-22, "interval = %lld is negative", (long long)p->interval);
    if (p->max_samples < 0 || p->max_samples > (1ll << 24)) return fail(-22, "max_samples = %lld outside [0, 2^24]", (long long)p->max_samples);
    if (!std::isfinite(p->q_h)) return fail(-22, "q_h = %g is not finite", p->q_h);
    if (!(p->sigma_o > 0.0) || !std::isfinite(p->sigma_o)) return fail(-22, "sigma_o = %g is not positive", p->sigma_o);
    if (!std::isfinite(p->epsilon_o)) return fail(-22, "epsilon_o = %g is not finite", p->epsilon_o);
    if (!(p->r_cut > 0.0) || !std::isfinite(p->r_cut)) return fail(-22, "r_cut = %g is not positive", p->r_cut);
    if (!(p->r_switch >= 0.0)) return fail(-22, "r_switch = %g is negative", p->r_switch);
    if (!(p->alpha > 0.0) || !std::isfinite(p->alpha)) return fail(-22, "alpha = %g is not positive", p->alpha);
    if (!(p->k_cut > 0.0) || !std::isfinite(p->k_cut)) return fail(-22, "k_cut = %g is not positive", p->k_cut);
    if (!std::isfinite(p->coulomb_const)) return fail(-22, "coulomb_const = %g is not finite", p->coulomb_const);
    if (!h) return fail(-22, "null handle");
    if (h->cfg.kind != GAMD_KIND_WATER)
        return fail(-22, "water classical potential: a GAMD_KIND_LJ handle has no molecules and no charges (GAMD_KIND_WATER handles only; "
                         "gamd_classical_configure evaluates Lennard-Jones)");
    if (h->n_per_box % 3) return fail(-22, "water classical potential: n_atoms = %d per box is not a multiple of 3 (atoms ordered O,H,H)", h->n_per_box);
    if (int r = check_boxes_tiles(h, "water classical observer", "water classical observer")) return r;
    if (h->pending.active) return fail(-22, "an MD run is still enqueued: call gamd_sync_status before gamd_water_configure");
    WaterClassical& wc = h->obs->wc;
    // the k-vector list of the handle's current boxes, in front of anything that is taken: a refused block changes nothing
    int n2max = wc.n2max;
    std::vector<int> kv;
    const bool have_box = h->boxes_host.size() == 3 * (size_t)h->n_boxes;
    if (have_box && !wc.pme_order)                          // (particle-mesh Ewald is sticky and reads no list: k_cut is kept for order 0)
        if (int r = water_klist(p->k_cut, h->boxes_host.data(), h->n_boxes, &n2max, &kv)) return r;
    wc.q_h = p->q_h; wc.sigma = p->sigma_o; wc.epsilon = p->epsilon_o; wc.r_cut = p->r_cut; wc.r_switch = p->r_switch;
    wc.shift = p->shift ? 1 : 0; wc.alpha = p->alpha; wc.k_cut = p->k_cut; wc.coulomb = p->coulomb_const;
    wc.params_set = true;
    if (have_box && !wc.pme_order)
        if (int r = water_klist_apply(h, n2max, kv)) return r;
    return potential_configure<WaterPotential>(h, OBS_WATER, p->interval, p->max_samples, "gamd_water_configure");
}

int32_t gamd_water_msite(gamd_handle* h, double w_h) {
    if (!h) return fail(-22, "null handle");
    if (h->cfg.kind != GAMD_KIND_WATER)
        return fail(-22, "gamd_water_msite: a GAMD_KIND_LJ handle has no molecules and no charges (GAMD_KIND_WATER handles only)");
    WaterClassical& wc = h->obs->wc;
    if (!wc.params_set) return fail(-22, "gamd_water_msite needs the parameters of a gamd_water_configure call (interval 0 will do)");
    if (h->pending.active) return fail(-22, "an MD run is still enqueued: call gamd_sync_status before gamd_water_msite");
    if (!std::isfinite(w_h) || !(w_h >= 0.0) || !(w_h < 0.5))
        return fail(-22, "gamd_water_msite: w_h = %g is not in [0, 0.5) (the oxygen's weight 1 - 2 w_h must stay positive)", w_h);
    const double before = wc.w_h;
    wc.w_h = w_h;
    DeviceGuard guard(h->dev);
    InitStream init(h->init_stream);
    if (bufs_ensure_work(water_bufs(h))) {
        wc.w_h = before;
        return fail(-12, "gamd_water_msite: allocation failed");
    }
    return 0;
}

int32_t gamd_water_pme(gamd_handle* h, const gamd_water_pme_params* p) {
    if (!h) return fail(-22, "null handle");
    if (!p) return fail(-22, "null argument");
    if (h->cfg.kind != GAMD_KIND_WATER)
        return fail(-22, "gamd_water_pme: a GAMD_KIND_LJ handle has no charges and no reciprocal sum (GAMD_KIND_WATER handles only)");
    WaterClassical& wc = h->obs->wc;
    if (!wc.params_set) return fail(-22, "gamd_water_pme needs the parameters of a gamd_water_configure call (interval 0 will do)");
    if (h->pending.active) return fail(-22, "an MD run is still enqueued: call gamd_sync_status before gamd_water_pme");
    if (p->order == 0) {                                    // the plain sum: the list of k_cut is built by the next run or eval
        wc.pme_order = 0;
        for (DevBuf* b : {&wc.pme_gq, &wc.pme_gc, &wc.pme_tw, &wc.pme_mod}) b->release();
        return 0;
    }
    if (!gamd_pme_order_ok(p->order))
        return fail(-22, "gamd_water_pme: order = %d is not 0 (off), 4 or 6 (odd orders are not offered: their interpolation modulus "
                         "vanishes at m = n / 2)", (int)p->order);
    const int n[3] = {p->nx, p->ny, p->nz};
    for (int d = 0; d < 3; ++d)
        if (!gamd_pme_length_ok(n[d]))
            return fail(-22, "gamd_water_pme: grid length n%c = %d is not one of 8, 16, 32, 64, 128", "xyz"[d], n[d]);
    if (wc.virial)
        return fail(-22, "gamd_water_pme: the virial log is armed (gamd_water_virial) and there is no PME virial: switch the log off first");
    wc.pme_order = p->order;
    for (int d = 0; d < 3; ++d) wc.pme_n[d] = n[d];
    DeviceGuard guard(h->dev);
    InitStream init(h->init_stream);
    std::vector<double> tw = gamd_pme_twiddles(), mod;
    for (int d = 0; d < 3; ++d) {
        const std::vector<double> m = gamd_pme_moduli(p->order, n[d]);
        mod.insert(mod.end(), m.begin(), m.end());
    }
    // 24 bytes per box and grid point, and the tables
    if (bufs_ensure_work(water_bufs(h)) || wc.pme_tw.ensure(sizeof(double) * tw.size(), true) ||
        wc.pme_mod.ensure(sizeof(double) * mod.size(), true)) {
        wc.pme_order = 0;                                   // the plain sum: the grids of a setting before may be gone
        for (DevBuf* b : {&wc.pme_gq, &wc.pme_gc, &wc.pme_tw, &wc.pme_mod}) b->release();
        return fail(-12, "gamd_water_pme: allocation of the %d x %d x %d grids of %d boxes failed", n[0], n[1], n[2], h->n_boxes);
    }
    HIP_TRY(init_upload(wc.pme_tw.p, tw.data(), sizeof(double) * tw.size()));
    HIP_TRY(init_upload(wc.pme_mod.p, mod.data(), sizeof(double) * mod.size()));
    return 0;
}

int32_t gamd_water_cells(gamd_handle* h, int32_t on) {
    if (!h) return fail(-22, "null handle");
    if (h->cfg.kind != GAMD_KIND_WATER)
        return fail(-22, "gamd_water_cells: a GAMD_KIND_LJ handle has no water potential (GAMD_KIND_WATER handles only; "
                         "gamd_classical_cells switches the cell table of the Lennard-Jones classical potential)");
    return cells_switch(h, h->obs->wc, water_bufs, "gamd_water_cells", "gamd_water_configure", on);
}

int32_t gamd_water_minimize_potential(gamd_handle* h, int32_t on) {
    if (!h) return fail(-22, "null handle");
    if (h->cfg.kind != GAMD_KIND_WATER)
        return fail(-22, "gamd_water_minimize_potential: a GAMD_KIND_LJ handle has no water potential (GAMD_KIND_WATER handles "
                         "only; gamd_minimize follows gamd_classical_cells by itself)");
    WaterClassical& wc = h->obs->wc;
    if (!wc.params_set)
        return fail(-22, "gamd_water_minimize_potential needs the parameters of a gamd_water_configure call (interval 0 will do)");
    if (h->pending.active) return fail(-22, "an MD run is still enqueued: call gamd_sync_status before gamd_water_minimize_potential");
    if (on != 0 && on != 1)
        return fail(-22, "gamd_water_minimize_potential: on = %d is not 0 (3-site, plain sum, all pairs only) or 1 (the potential as "
                         "configured)", (int)on);
    wc.min_configured = on == 1;
    return 0;
}

int32_t gamd_water_cells_read(gamd_handle* h, void* stream, int32_t box, int32_t* nc, int32_t* start, int64_t max_start, int32_t* order,
                              int64_t max_order) {
    if (!h) return fail(-22, "null handle");
    if (h->cfg.kind != GAMD_KIND_WATER) return fail(-22, "gamd_water_cells_read: GAMD_KIND_WATER handles only");
    const WaterClassical& wc = h->obs->wc;
    return cells_read(h, wc, "gamd_water_cells_read", "gamd_water_cells", stream, box, nc, start, max_start, order, max_order);
}

int32_t gamd_water_reset(gamd_handle* h) { return observer_reset(h, OBS_WATER, "gamd_water_reset"); }

int32_t gamd_water_read(gamd_handle* h, void* stream, int64_t* steps, double* rows, int64_t max_rows, int64_t* n_rows,
                        int64_t* dropped, double* f_cl, int64_t f_cl_elems) {
    return potential_read<WaterPotential>(h, stream, steps, rows, max_rows, n_rows, dropped, f_cl, f_cl_elems);
}

int32_t gamd_water_eval(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev, const float* box, float length_per_nm,
                        double* f_out_dev, double* rows, void* stream) {
    std::vector<double> row;
    if (int r = potential_eval<WaterPotential>(h, pos_dev, species_dev, box, length_per_nm, f_out_dev, row, stream)) return r;
    if (rows) std::memcpy(rows, row.data(), sizeof(double) * row.size());
    return 0;
}

int32_t gamd_water_virial(gamd_handle* h, int32_t on) {
    if (!h) return fail(-22, "null handle");
    if (h->cfg.kind != GAMD_KIND_WATER)
        return fail(-22, "gamd_water_virial: a GAMD_KIND_LJ handle has no molecules (GAMD_KIND_WATER handles only; the row of "
                         "gamd_classical_read carries the Lennard-Jones virial)");
    WaterClassical& wc = h->obs->wc;
    if (!wc.params_set) return fail(-22, "gamd_water_virial needs the parameters of a gamd_water_configure call (interval 0 will do)");
    if (h->pending.active) return fail(-22, "an MD run is still enqueued: call gamd_sync_status before gamd_water_virial");
    if (!on) { wc.virial = false; return 0; }               // off: what was logged stays readable
    if (wc.pme_order)
        return fail(-22, "gamd_water_virial: particle-mesh Ewald is on (gamd_water_pme, order %d) and there is no PME virial: the log "
                         "needs the plain sum (gamd_water_pme with order 0)", wc.pme_order);
    const bool before = wc.virial, work_before = wc.vwork;
    wc.virial = wc.vwork = true;
    DeviceGuard guard(h->dev);
    InitStream init(h->init_stream);
    const size_t want = sizeof(double) * WATER_VIR_ROW * (size_t)h->n_boxes * (size_t)wc.max_samples;
    if (wc.vrows.bytes != want) wc.vrows.release();
    if (bufs_ensure_work(water_bufs(h)) || (want && wc.vrows.ensure(want, true))) {
        wc.virial = before; wc.vwork = work_before;
        return fail(-12, "gamd_water_virial: allocation failed");
    }
    if (wc.vrows.p) {
        HIP_TRY(hipMemsetAsync(wc.vrows.p, 0, wc.vrows.bytes, tl_init_stream));
        HIP_TRY(hipStreamSynchronize(tl_init_stream));
    }
    return 0;
}

int32_t gamd_water_virial_read(gamd_handle* h, void* stream, double* rows, int64_t max_rows, int64_t* n_rows) {
    if (!h) return fail(-22, "null handle");
    if (max_rows < 0) return fail(-22, "max_rows is negative");
    if (h->cfg.kind != GAMD_KIND_WATER) return fail(-22, "gamd_water_virial_read: GAMD_KIND_WATER handles only");
    const WaterClassical& wc = h->obs->wc;
    if (!wc.vrows.p) return fail(-22, "gamd_water_virial_read: the virial log has not been on (gamd_water_virial) since the rows were allocated");
    DeviceGuard guard(h->dev);
    hipStream_t st = (hipStream_t)stream;
    const long long nb = h->n_boxes;
    const long long kept = std::min<long long>(wc.clock.taken(wc.steps.p != nullptr), wc.max_samples);
    const long long n_copy = std::min<long long>(kept, max_rows);
    if (n_copy > 0 && rows)
        HIP_TRY(hipMemcpyAsync(rows, wc.vrows.p, sizeof(double) * (size_t)(n_copy * nb * WATER_VIR_ROW), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (int t = check_traps(h)) return t;
    if (n_rows) *n_rows = kept;
    return 0;
}

int32_t gamd_water_virial_eval(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev, const float* vel_dev,
                               const float* box, float length_per_nm, double mass_o_amu, double mass_h_amu, double* rows,
                               double* water_rows, void* stream) {
    if (!h) return fail(-22, "null handle");
    if (!(mass_o_amu > 0.0) || !(mass_h_amu > 0.0) || !std::isfinite(mass_o_amu) || !std::isfinite(mass_h_amu))
        return fail(-22, "gamd_water_virial_eval: mass_o_amu = %g, mass_h_amu = %g: a mass is not positive", mass_o_amu, mass_h_amu);
    if (h->cfg.kind != GAMD_KIND_WATER) return fail(-22, "gamd_water_virial_eval: a GAMD_KIND_LJ handle has no molecules (GAMD_KIND_WATER handles only)");
    WaterClassical& wc = h->obs->wc;
    if (h->pending.active) return fail(-22, "an MD run is still enqueued: call gamd_sync_status before gamd_water_virial_eval");
    if (wc.pme_order)
        return fail(-22, "gamd_water_virial_eval: particle-mesh Ewald is on (gamd_water_pme, order %d) and there is no PME virial: "
                         "evaluate under the plain sum (gamd_water_pme with order 0)", wc.pme_order);
    wc.vwork = true;                                        // the work buffers are ensured with the potential's (potential_eval)
    std::vector<double> row;
    const size_t nv = WATER_VIR_ROW * (size_t)h->n_boxes;
    int r = potential_eval<WaterPotential>(h, pos_dev, species_dev, box, length_per_nm, nullptr, row, stream,
                                           [&](const WaterArgs& a, hipStream_t st) {
        // a frozen handle's kernels return at once (potential_eval answers for that)
        if (hipMemsetAsync(wc.veval_rows.p, 0xff, sizeof(double) * nv, st) != hipSuccess) return -2;
        return WaterPotential::virial(h, a, vel_dev, mass_o_amu, mass_h_amu, wc.veval_rows.as<double>(), st);
    });
    if (r) return r;
    if (water_rows) std::memcpy(water_rows, row.data(), sizeof(double) * row.size());
    if (rows) {
        DeviceGuard guard(h->dev);
        hipStream_t st = (hipStream_t)stream;
        HIP_TRY(hipMemcpyAsync(rows, wc.veval_rows.p, sizeof(double) * nv, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

int32_t gamd_water_minimize(gamd_handle* h, float* x_dev, const uint8_t* species_dev, const float* box, float length_per_nm,
                            double r_oh, double r_hh, float* f_dev, double* x64_dev, const gamd_minimize_params* params,
                            double* rows_host, void* stream) {
    // the parameter block is checked first: these answers need no device
    gamd_minimize_params q;
    if (int r = minimize_fill_params(params, &q, g_err, sizeof(g_err))) return r;
    const double len = length_per_nm > 0.f ? (double)length_per_nm : 10.0;
    WMinArgs m{};
    if (int r = water_minimize_checks("gamd_water_minimize", h, len, r_oh, r_hh, &m.ra, &m.rb, &m.rc)) return r;
    return minimize_run<WaterMinimizer>(h, m, x_dev, species_dev, box, len, f_dev, x64_dev, q, rows_host, stream);
}

int32_t gamd_water_minimize_lbfgs(gamd_handle* h, float* x_dev, const uint8_t* species_dev, const float* box, float length_per_nm,
                                  double r_oh, double r_hh, float* f_dev, double* x64_dev, const gamd_lbfgs_params* params,
                                  double* rows_host, void* stream) {
    // the parameter block is checked first: these answers need no device
    gamd_lbfgs_params q;
    if (int r = lbfgs_fill_params(params, &q, g_err, sizeof(g_err), "gamd_water_minimize_lbfgs")) return r;
    const double len = length_per_nm > 0.f ? (double)length_per_nm : 10.0;
    WLbfgsArgs l{};
    if (int r = water_minimize_checks("gamd_water_minimize_lbfgs", h, len, r_oh, r_hh, &l.ra, &l.rb, &l.rc)) return r;
    return lbfgs_run<WaterLbfgs>(h, l, x_dev, species_dev, box, len, f_dev, x64_dev, q, rows_host, stream);
}

}  // extern "C"

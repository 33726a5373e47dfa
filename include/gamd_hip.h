/* gamd_hip.h — C ABI of libgamd_hip.so, the MI355X (gfx950) implementation of GAMD's
 * force-inference hot path.
 *
 * The reference has no FFI layer: its hot path sits behind Python objects
 * (SURVEY.md §8b).  This header is the boundary a maintainer binds with ctypes
 * (INTEGRATION.md shows the stub); every entry point names the reference
 * interface it replaces (paths relative to /root/reference/code).
 *
 * Conventions
 *   - plain C types only; all `*_dev` pointers are caller-owned DEVICE pointers,
 *     all other pointers are HOST pointers; `stream` is a hipStream_t passed as void*
 *     (NULL = default stream).  Work is ordered on that stream only (it may be a non-blocking stream: nothing relies
 *     on the NULL stream's implicit ordering; what a call allocates and initialises has landed before it returns).
 *   - every function returns an int32 status: 0 = ok, 1 = ok after the neighbour
 *     buffers overflowed and were regrown (the analogue of jax-md's
 *     did_buffer_overflow -> re-allocate, graph_utils.py:41-42), < 0 = error
 *     (text via gamd_last_error).  No exceptions cross the ABI.
 *   - one handle per box (or per gamd_config.n_boxes independent boxes), any number of handles per GPU and per
 *     process.  A HANDLE is not thread-safe (one caller at a time; the reference is single-threaded too); DIFFERENT
 *     handles may be driven from different threads at the same time — the library keeps no mutable state outside the
 *     handle, and gamd_last_error is per thread.
 *   - atoms keep the CALLER's order at the boundary; internally they are renumbered
 *     in cell order every call.
 */
#ifndef GAMD_HIP_H
#define GAMD_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gamd_handle gamd_handle;

enum { GAMD_EDGE_F32 = 0, GAMD_EDGE_BF16 = 1, GAMD_EDGE_F16X3 = 2 };

enum { GAMD_KIND_LJ = 0, GAMD_KIND_WATER = 1 };        /* SimpleMDNetNew | WaterMDNetNew / WaterMDDynamicBoxNet */
enum { GAMD_NBR_JAXMD = 0, GAMD_NBR_TORCH = 1 };        /* dr^2 < rc^2 + self pair | |dr| <= rc, no self */

/* Constructor arguments.  Replaces build_model() + NeighborSearcher(BOX_SIZE, cutoff):
 * LJ/train_network_lj.py:68-88,108-112; water/train_network_tip3p.py:75-97;
 * graph_utils.py:12-27.  Widths: whatever build_model passes (nn_module.py:561-601, --encoding_size / --hidden_dim /
 * --edge_embedding_dim, LJ/train_network_lj.py:394-396): encoding_size, edge_embedding_dim and hidden_dim in [1, 256]
 * (hidden_dim above 128: edge_dtype f32 only).  The kernels work in 128-wide blocks; other widths are zero-padded when the weights are packed (padded features
 * are exact zeros through every layer, the two LayerNorms divide by the true width).  128 / 128 / 128 (every shipped LJ / TIP
 * config, LJ/test_script/test_langevin.py:63-73) runs the specialised kernels, anything wider than 128 the generic-width
 * ones (the DFT-water config 256 / 128 / 256, water/test_script/test_nosehoover_hb.py:69-81; the trainers' defaults).
 * Normalisation between the conv layers (nn_module.py:171-196): LayerNorm (use_layer_norm=True, every rollout driver) or
 * eval-mode BatchNorm1d (use_layer_norm=False, the constructors' default) -- chosen by the weights: a state_dict that carries
 * graph_conv.norm_layers.<l>.running_mean / running_var is a BatchNorm checkpoint (num_batches_tracked is not needed).
 * update_edge=True models (SmoothConvLayerNew.update_edge_emb, nn_module.py:91-92, :140-146) are recognised the same way, by
 * their graph_conv.conv.<l>.edge_layer_norm.weight / .bias keys: fp32 edge MLP, encoding_size == edge_embedding_dim. */
typedef struct gamd_config {
    int32_t n_atoms;
    int32_t kind;            /* GAMD_KIND_*  */
    int32_t n_layers;        /* conv_layer (4 in build_model) */
    int32_t use_bond;        /* water: 45th edge feature from the bond graph (nn_module.py:450-454) */
    int32_t nbr_flavour;     /* GAMD_NBR_*  */
    int32_t device;          /* HIP device ordinal */
    float cutoff;            /* CUTOFF_RADIUS */
    float box[3];            /* initial box (may change per call) */
    int64_t edge_capacity;   /* 0 = estimate from density */
    int32_t keep_stages;     /* 1 = keep per-stage tensors for the debug getters */
    int32_t edge_dtype;      /* GAMD_EDGE_F32 (bit-exact fp32 MFMA, default) | GAMD_EDGE_BF16 (BASELINE config 5: edge-MLP
                                operands rounded to bf16, fp32 accumulate; S/D adds, SiLU, sums in fp32; the node side's GEMMs fp32-grade: split-fp16
                                as in F16X3)
                                | GAMD_EDGE_F16X3 (fp32-grade edge-MLP on the fp16 matrix pipe: every operand split into
                                hi + lo fp16, W x = Wh xh + (Wh xl + Wl xh), fp32 accumulate; meets F32's 1e-5 parity bar on every
                                shipped architecture and golden; 3-4 x the fp32 kernels' rounding error, so a deep model with
                                heavy cancellation can land just above it: opt-in, labelled with its own dtype).
                                Both exist for every width and feature set (at most 2^22 - 2 atoms per handle when
                                encoding_size > 128); fp32 only: self_loop_mode 1 and update_edge models */
    int32_t encoding_size;   /* node width H: 0 (= 128) or 1 .. 256 (build_model 'encoding_size') */
    int32_t edge_embedding_dim; /* edge-embedding width Eh: 0 (= 128) or 1 .. 256 ('edge_embedding_dim') */
    int32_t hidden_dim;      /* 0 (= 128) or 1 .. 256 ('hidden_dim'); above 128: GAMD_EDGE_F32 only (wide_d.hip) */
    int32_t no_expand_edge;  /* 1 = expand_edge=False: edge features are (unit vector, standardised length[, bond])
                                without the 40 RBFs (nn_module.py:329-336; --disable_expand_edge,
                                water/train_network_real_large.py:363) */
    float neighbor_skin;     /* 0 = exact cell-list rebuild every call (default).  > 0: Verlet-skin reuse like the reference's
                                jax-md list (graph_utils.py:21-25 dr_threshold = cutoff/6, :36-44 update): candidates
                                within cutoff + skin are rebuilt only when an atom has moved more than skin/2, the exact
                                cutoff is re-applied every call, so the edge SET is the same either way */
    int32_t self_loop_mode;  /* what `fluid_graph.add_self_loop()` with its result DISCARDED does (nn_module.py:650-652, :364,
                                :518).  0 = GAMD_SELF_LOOP_DGL07_NOOP (default): nothing — under the pinned DGL 0.7.0 (DGL >= 0.5)
                                add_self_loop is functional and returns a new graph, so the graph that is used has no extra
                                edges.  1 = GAMD_SELF_LOOP_APPEND_ZERO_FEATURE: what an in-place add_self_loop (DGL < 0.5) would
                                have done: one extra edge i -> i per atom whose embedding e is DGL's zero fill (it is appended
                                after edata['e'] was set).  The one reference semantic that cannot be executed in the build
                                container (DGL absent), hence the switch.  fp32 edge dtype only. */
    int32_t kernel_select;   /* 0 = automatic.  Bit flags for tests (never change results beyond fp32 rounding):
                                GAMD_KSEL_FORCE_GENERIC_WIDTH (1): run a 128/128 configuration on the generic-width kernels
                                of wide.hip; GAMD_KSEL_FORCE_HALF_QUANTUM (2): run the generic-width fp32 conv layer on 16-edge
                                work units (wide16.hip, v_mfma_f32_16x16x4_f32; bit-identical results, measured slower at every
                                size tried: never chosen automatically); GAMD_KSEL_NO_LAYER0_HOIST (4): LJ models in fp32 on the
                                128-wide kernels run layer 0 in its general form (four GEMMs per edge) instead of the layer-0
                                form (three GEMMs per edge, the last Linear applied per atom; equal up to fp32 rounding);
                                GAMD_KSEL_NO_LN_FOLD (8): the fp32 128-wide kernels form the edge embedding e = LayerNorm(...)
                                in the encoder, as they do under keep_stages, instead of folding the LayerNorm's affine part
                                into every conv layer's first matrix (equal up to fp32 rounding) */
    int32_t small_tile_limit;/* fp32 path: edge counts of at most this many 32-edge tiles run the latency-oriented conv kernel
                                (one tile per 4-wave workgroup, bit-identical results).  0 = default (512), -1 = never */
    int32_t n_boxes;         /* 0 or 1: one box (default).  B > 1: B INDEPENDENT boxes of n_atoms atoms each, evaluated and
                                integrated in one set of launches — the reference's several-graphs-per-forward
                                (build_graph_batches + dgl.batch, nn_module.py:655-661, :520-527, :676-679) and the "more
                                replicas than GPUs" half of the ensemble.  Every `[n][3]` / `[n]` device array of the entry
                                points below is then `[B][n][3]` / `[B][n]` (box-major, contiguous), every `box` argument is
                                HOST float [B][3] (a box per graph, as WaterMDDynamicBoxNet.forward's box_size_lst), bonds name
                                atoms of one box and apply to each, gamd_md_run's seed means seed + b for box b, and
                                gamd_md_run_nhc's chain_state_dev is [B][3*chain_length + 2] with ndf per box.  Atoms of
                                different boxes are never neighbours (the box index is folded into the cell index); results are
                                bit-identical to the boxes evaluated one by one (each box's CSR rows start on a 16-edge
                                boundary; gamd_get_counts / GAMD_DBG_COL include those <= 15 padding slots per box, source
                                index B*n).  A neighbour-buffer overflow in any box regrows the shared buffers. */
} gamd_config;
enum { GAMD_SELF_LOOP_DGL07_NOOP = 0, GAMD_SELF_LOOP_APPEND_ZERO_FEATURE = 1 };
enum { GAMD_KSEL_FORCE_GENERIC_WIDTH = 1, GAMD_KSEL_FORCE_HALF_QUANTUM = 2, GAMD_KSEL_NO_LAYER0_HOIST = 4, GAMD_KSEL_NO_LN_FOLD = 8 };

const char* gamd_version(void);
const char* gamd_last_error(void);

int32_t gamd_create(const gamd_config* cfg, gamd_handle** out);
int32_t gamd_destroy(gamd_handle* h);

/* Weights contract = the reference state_dict: call once per key with the
 * reference's key name (e.g. "graph_conv.conv.0.src_affine.weight"), fp32 host data, row-major
 * torch shape; then gamd_finalize_weights packs them into MFMA fragment order on the device.
 * Replaces model.load_state_dict / load_from_checkpoint (LJ/train_network_lj.py:85-87,
 * LJ/test_script/test_langevin.py:74). */
int32_t gamd_load_weight(gamd_handle* h, const char* name, const float* data, const int64_t* shape, int32_t ndim);
int32_t gamd_finalize_weights(gamd_handle* h);

/* scaler.npz mean/var.  Replaces load_training_stats (LJ/train_network_lj.py:119-123). */
int32_t gamd_set_scaler(gamd_handle* h, double mean, double var);

/* Bond list [n_bonds][2] (both directions are implied).  Replaces build_bond_graph
 * (nn_module.py:529-534) fed by create_water_bond (water/train_network_tip3p.py:38-42). */
int32_t gamd_set_bonds(gamd_handle* h, const int32_t* bonds, int64_t n_bonds);

/* Enqueue neighbour build + full network forward for positions `pos_dev` [n][3] fp32 (any periodic
 * image), optional species [n] (u8: O=1/H=0 -> node feature, water/test_script/test_nosehoover.py:82-89),
 * box[3].  Writes the NORMALISED network output [n][3] fp32 to out_norm_dev (what
 * pnet_model([pos],[edge_idx]) returns, nn_module.py:672-685 / :545-558) and, if out_denorm_dev is not NULL,
 * out*sqrt(var)+mean in fp32 (device-side copy of denormalize(), train_network_lj.py:128-131).
 * Replaces search_for_neighbor + get_edge_idx + model.forward (LJ/train_network_lj.py:135-147,166-199).
 * Does not synchronise; call gamd_sync_status afterwards. */
int32_t gamd_forces_async(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev, const float* box,
                          float* out_norm_dev, float* out_denorm_dev, void* stream);

/* Float node features for the water models: feat_dev [n] fp32 (device, caller-owned, must stay valid for the calls
 * that follow) is what the reference feeds to node_encoder = Linear(1 -> H) as `x` (nn_module.py:554, :403); NULL
 * (default) = use (float)species, i.e. the O = 1 / H = 0 flag the drivers build (water/test_script/test_nosehoover.py:82-89).
 * species_dev stays the integer type the integrators pick masses by. */
int32_t gamd_set_node_features(gamd_handle* h, const float* feat_dev);

/* Wait for the stream and report what the enqueued work ran into:
 *   0    nothing.
 *   1    a neighbour buffer overflowed inside an enqueued gamd_md_run / gamd_md_run_nhc: the device froze positions,
 *        velocities and thermostat chain at the last consistent point (integrator and node kernels return while the
 *        overflow flag is set), this call regrew the buffers, re-evaluated the forces there and finished the remaining
 *        steps: the trajectory is the one an ample buffer would have produced.
 *   -34  a neighbour buffer overflowed in gamd_forces_async: regrown, the caller must re-issue that call (gamd_forces
 *        does it for you).
 *   -33  non-finite forces in a reduced-precision edge dtype (bf16 / f16x3): an MFMA operand left the fp16 range
 *        (|x| > 65504) or the input was not finite.  (The fp32 path returns non-finite forces silently, like the
 *        reference; gamd_get_device_flags tells.) */
int32_t gamd_sync_status(gamd_handle* h, void* stream);

/* flags[0]: 1 if any force evaluation since the last call of this function produced a non-finite force component
 * (then cleared); flags[1..3] reserved (0). */
int32_t gamd_get_device_flags(gamd_handle* h, int32_t flags[4]);

/* gamd_forces_async + gamd_sync_status + automatic regrow-and-retry; returns 0 or 1. */
int32_t gamd_forces(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev, const float* box,
                    float* out_norm_dev, float* out_denorm_dev, void* stream);

/* The reference's host-array boundary in one call: predict_forces(pos) takes and returns HOST arrays
 * (LJ/train_network_lj.py:133-157, water/train_network_tip3p.py:142-159).  pos_host: float32 [n][3], wrapped and rounded as
 * :141-142 do (np.mod in float64, then float32), any host memory; out_host: float32 [n][3] — the normalised network output
 * (denormalize = 0: what pnet_model returns at :152; the caller denormalises in float64 as :155) or out * sqrt(var) + mean in
 * fp32 (denormalize = 1).  The positions go through a pinned staging buffer of the handle; the copy in, the kernels and the
 * copy out are enqueued on `stream`, the call synchronises ONCE and replays itself after a regrow.  species_dev / box as in
 * gamd_forces.  Returns 0, or 1 if a neighbour buffer was regrown.  PCIe-inclusive: never what bench.py reports as `value`. */
int32_t gamd_forces_host(gamd_handle* h, const float* pos_host, const uint8_t* species_dev, const float* box, float* out_host,
                         int32_t denormalize, void* stream);

/* Same network forward on a CALLER-SUPPLIED directed edge list instead of the built-in radius search:
 * centre_dev[e] / neigh_dev[e] (int32, device) = rows 0 / 1 of the reference's edge_idx tensor; messages flow
 * neigh -> centre.  Replaces the model-level call pnet_model([pos], [edge_idx]) / ([pos], feat, [edge_idx])
 * (nn_module.py:672-685, :545-558, build_graph :636-653).  Atoms are NOT renumbered on this path; every row
 * keeps the caller's edge order.  Synchronises; returns 0, or 1 if the edge buffers had to grow. */
int32_t gamd_forces_edges(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev, const float* box,
                          const int32_t* centre_dev, const int32_t* neigh_dev, int64_t n_edges,
                          float* out_norm_dev, float* out_denorm_dev, void* stream);

/* Neighbour build only (stage entry point for parity tests / profiling). */
int32_t gamd_build_neighbors(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev, const float* box,
                             void* stream);

/* n_edges = directed edge count of the last build (incl. self edges in the jax-md flavour). */
int32_t gamd_get_counts(gamd_handle* h, int64_t* n_edges, int64_t* n_pieces, int64_t* edge_capacity);

/* Verlet-skin bookkeeping: candidate-list rebuilds so far, size of the candidate list in use, its capacity.  The analogue of watching nbrs.did_buffer_overflow / re-allocation in graph_utils.py:36-44. */
int32_t gamd_get_skin_stats(gamd_handle* h, int64_t* n_rebuilds, int64_t* n_candidates, int64_t* candidate_capacity);

/* Debug / parity getters: copy a stage tensor of the last call to HOST memory (synchronises).
 * Need keep_stages = 1 for H / FEAT. */
enum {
    GAMD_DBG_PERM = 0,      /* int32 [n]      sorted -> original atom id */
    GAMD_DBG_ROWPTR = 1,    /* int32 [n+1]    CSR by destination, sorted ids */
    GAMD_DBG_COL = 2,       /* int32 [E]      source atom (sorted id) per CSR edge */
    GAMD_DBG_EFRAG = 3,     /* fp32  [ceil(E/32)][Eh/128][4][4][64][4]  e in fragment order */
    GAMD_DBG_FEAT = 4,      /* fp32  [E][48]  raw edge features (first 44|45, or 4|5 unexpanded, columns valid) */
    GAMD_DBG_CYCLES = 5,    /* int64 [n_cu][8][16]  per-wave cycle sums of the instrumented conv-edge kernel (profiling build) */
    GAMD_DBG_PARTIAL = 6,   /* fp32  [pieces][H]  the LAST conv layer's partial-sum pieces (one row per run of edges with the same
                               destination inside a 16-edge chunk), in CSR order */
    GAMD_DBG_H0 = 16        /* fp32  [n][H] residual stream h_l, sorted order: GAMD_DBG_H0 + l */
};
int32_t gamd_debug_get(gamd_handle* h, int32_t what, void* host_out, size_t bytes);

/* Split BAOAB Langevin step of the reference drivers, on device:
 *   first half  B A O A   HackLangevinIntegrator     hack_integrator.py:141-165
 *   force eval            predict_forces             LJ/test_script/test_langevin.py:108
 *   second half B         HackHalfVelocityIntegrator hack_integrator.py:175-178
 * x [n][3] Angstrom, v [n][3] Angstrom/ps, f [n][3] kJ/mol/nm (denormalised; in: forces at x, out: forces
 * at the new x).  Enqueues n_steps steps without synchronising; gamd_sync_status afterwards reports 0, or 1 when a
 * neighbour buffer overflowed on the way (state frozen on the device, buffers regrown, run resumed and finished). */
typedef struct gamd_md_params {
    float dt_ps;             /* 0.002 in the drivers */
    float mass_amu;          /* 39.9 for argon */
    float temperature_k;     /* 100 */
    float gamma_per_ps;      /* 25 */
    uint64_t seed;
    uint64_t first_step;     /* RNG counter of the first step */
    /* zero-initialised = the LJ behaviour (one mass, Angstrom, no constraints) */
    float mass_h_amu;        /* > 0 and species given: mass of the species-0 atoms (H, 1.008); mass_amu is then the O mass */
    float length_per_nm;     /* length unit of x, v, box per nm: 0 or 10 = Angstrom; 18.8972613 = bohr (DFT model:
                                positions in bohr, water/test_script/test_nosehoover_hb.py:106-109) */
    int32_t rigid_water;     /* 1 = atoms are O,H,H triples held rigid, as OpenMM does for the constrained water systems
                                of the water drivers at every addConstrainPositions / addConstrainVelocities of
                                hack_integrator.py:145-164,178,277-280,427-428 (SETTLE + analytic velocity constraint) */
    float r_oh, r_hh;        /* constraint lengths in the length unit (TIP3P: 0.9572, 1.5139 A) */
    int32_t remove_cm_motion;/* 1 = subtract the centre-of-mass velocity (sum m v / sum m, per box) at the top of every step, as
                                OpenMM's CMMotionRemover does through addUpdateContextState() (hack_integrator.py:142) when the
                                System carries one: the water drivers' openmmtools WaterBox does, the LJ fluid does not.  GNN
                                forces do not sum to zero, so without it the centre of mass random-walks in long rollouts */
} gamd_md_params;
int32_t gamd_md_run(gamd_handle* h, float* x_dev, float* v_dev, float* f_dev, const uint8_t* species_dev,
                    const float* box, const gamd_md_params* p, int64_t n_steps, void* stream);

/* Split Nose-Hoover-chain step of the reference drivers, on device:
 *   first half   propagateNHC; v += dt/2 f_last/m; x += dt v     HackNoseHooverIntegrator      hack_integrator.py:182-330
 *   force eval                                                    predict_forces                LJ/test_script/test_nosehoover.py:113
 *   second half  v += dt/2 f_gnn/m; propagateNHC                  HackHalfNoseHooverIntegrator  hack_integrator.py:334-493
 * One chain state (xi, vxi, G) is shared by both halves (the drivers copy it across every step,
 * test_nosehoover.py:104-118).  chain_state_dev: double [3*chain_length + 2] device buffer owned by the caller
 * (xi[M], vxi[M], G[M], last scale, last 2*KE); pass reset != 0 to initialise it (xi = vxi = 0, G = -freq^2). */
typedef struct gamd_nhc_params {
    float dt_ps;              /* 0.002 */
    float mass_amu;           /* 39.9 */
    float temperature_k;      /* 100 */
    float frequency_per_ps;   /* collision_frequency: 25 */
    int32_t chain_length;     /* 10 in the drivers (<= 16) */
    int32_t num_mts;          /* 5 */
    int32_t num_yoshidasuzuki;/* 1, 3 or 5 */
    int32_t reset;
    double ndf;               /* degrees of freedom (3N for the unconstrained LJ system; 6 per rigid water) */
    /* zero-initialised = the LJ behaviour (one mass, Angstrom, no constraints) */
    float mass_h_amu;        /* > 0 and species given: mass of the species-0 atoms (H, 1.008); mass_amu is then the O mass */
    float length_per_nm;     /* length unit of x, v, box per nm: 0 or 10 = Angstrom; 18.8972613 = bohr (DFT model:
                                positions in bohr, water/test_script/test_nosehoover_hb.py:106-109) */
    int32_t rigid_water;     /* 1 = atoms are O,H,H triples held rigid, as OpenMM does for the constrained water systems
                                of the water drivers at every addConstrainPositions / addConstrainVelocities of
                                hack_integrator.py:145-164,178,277-280,427-428 (SETTLE + analytic velocity constraint) */
    float r_oh, r_hh;        /* constraint lengths in the length unit (TIP3P: 0.9572, 1.5139 A) */
    int32_t remove_cm_motion;/* as in gamd_md_params, at the place hack_integrator.py:271-272 has it: propagateNHC() takes KE2 from
                                the velocities as they are and scales them, THEN addUpdateContextState() removes the centre-of-mass
                                velocity, then the kick (ndf is 3 smaller with a remover, :226-235) */
} gamd_nhc_params;
int32_t gamd_md_run_nhc(gamd_handle* h, float* x_dev, float* v_dev, float* f_dev, const uint8_t* species_dev,
                        const float* box, const gamd_nhc_params* p, double* chain_state_dev, int64_t n_steps, void* stream);

/* Run reporter: the log the reference's rollout drivers keep with OpenMM's
 *   StateDataReporter(file, 100 | 250, step=True, time=True, kineticEnergy=True, temperature=True, separator='\t')
 * (LJ/test_script/test_langevin.py:79-83, LJ/test_script/test_nosehoover.py:82-87, water/test_script/test_langevin.py:89-94,
 * water/test_script/test_nosehoover.py:91-96, the _hb drivers alike), kept ON THE DEVICE while gamd_md_run / gamd_md_run_nhc
 * are enqueued, plus the pair-distance histogram of a radial distribution function over the sampled frames.
 * The reporter counts the completed MD steps g of the handle since it was configured or reset (across calls).  Step g is
 * sampled when g % interval == 0, behind its second half (HackHalfVelocityIntegrator / HackHalfNoseHooverIntegrator and, for
 * rigid water, the velocity constraint behind the kick): where the drivers' reporter fires, since they call
 * simulation.step(1) twice per iteration and the report interval is even.  A sample is
 *   - one log row {g, KE per box}: KE = sum_i 1/2 m_i |v_i|^2 in kJ/mol (OpenMM's m*v*v/2 of a CustomIntegrator), v converted
 *     to nm/ps with the run's length_per_nm, m_i the run's mass_amu / mass_h_amu (the fp32 values of the parameter block),
 *     summed in double in a fixed order: the same bits run after run.  Row number = g / interval - 1; rows beyond
 *     max_samples are dropped and counted;
 *   - rdf_bins > 0: every directed edge src -> dst of that step's force evaluation with src != dst (the frame's exact pair
 *     list, in skin mode too) adds 1 to the 64-bit counter [box][pair class][bin], bin = min((int)(r * rdf_bins / rdf_rmax),
 *     rdf_bins - 1) of the fp32 min-image distance r < rdf_rmax (rdf_rmax == cutoff: every edge).  Pair classes: one for
 *     GAMD_KIND_LJ handles; three for GAMD_KIND_WATER: O-O, O-H (both directions), H-H, O = node feature != 0 (the
 *     species flag).  exclude_same_molecule: pairs whose caller-order atom ids share id / 3 (O,H,H triples) are skipped.
 * Nothing synchronises or returns to the host inside a run; a run that froze on a neighbour-buffer overflow and was resumed
 * by gamd_sync_status gives the log and the counts of an ample buffer.  A handle whose reporter is off enqueues exactly what
 * it enqueues without one; with it on, skin-mode runs launch the second half of a SAMPLED step on its own. */
typedef struct gamd_report_params {
    int64_t interval;        /* 0 = reporter off (buffers are kept); > 0: sample every interval-th completed step */
    int64_t max_samples;     /* log rows allocated by gamd_report_configure; 0 = 4096 */
    double ndf;              /* degrees of freedom per box for the temperature; 0 = 3 * n_atoms */
    int32_t rdf_bins;        /* 0 = no histogram; at most 1024 */
    float rdf_rmax;          /* upper edge of the last bin, 0 < rdf_rmax <= cutoff (0 with rdf_bins > 0: the cutoff) */
    int32_t exclude_same_molecule;
    int32_t reserved;        /* 0 */
} gamd_report_params;
/* p: HOST.  Allocates and clears the log and the histogram (drains nothing: call it between runs, after gamd_sync_status);
 * -22 for a negative interval or max_samples, rdf_bins outside [0, 1024], rdf_rmax < 0 or above the cutoff. */
int32_t gamd_report_configure(gamd_handle* h, const gamd_report_params* p);
/* Step count g = 0, log and histogram cleared; the configuration stays. */
int32_t gamd_report_reset(gamd_handle* h);
/* Synchronises `stream` once (it does NOT resume a frozen run: call gamd_sync_status first) and copies to HOST arrays, any
 * of which may be NULL: steps int64 [max_rows], ke and temperature double [max_rows][n_boxes] (T = 2 KE / (ndf kB), kB =
 * 0.00831446261815324 kJ/mol/K), counts uint64 [n_boxes][pair classes][rdf_bins] (count_elems = room in elements; fewer
 * than that product is -22).  *n_rows = rows in the log (at most max_rows are written), *frames = frames in the histogram,
 * *dropped = samples that found the log full, dims[0..2] = n_boxes, pair classes, rdf_bins. */
int32_t gamd_report_read(gamd_handle* h, void* stream, int64_t* steps, double* ke, double* temperature, int64_t max_rows,
                         int64_t* n_rows, uint64_t* counts, int64_t count_elems, int64_t* frames, int64_t* dropped,
                         int32_t dims[3]);

/* Run recorder: the trajectory the reference's data generators dump every 50 steps (pos / vel / forces,
 * dataset/generate_lj_data.py:93-106, read back by train_utils.LJDataNew / WaterDataNew) and the dynamical observables that
 * need the UNWRAPPED displacement, kept ON THE DEVICE while gamd_md_run / gamd_md_run_nhc are enqueued.
 * The recorder counts the completed MD steps g of the handle since it was configured or reset (across calls, with a counter
 * of its own: its interval is independent of the reporter's).  Step g is sampled when g % interval == 0, behind its second
 * half (for rigid water: behind the velocity constraint), where the reporter samples.  Sample ordinal q = g / interval - 1.
 *   - Frame: a sample with q < max_frames stores the selected fields in the caller's atom order: x, v, f fp32
 *     [n_boxes][n][3], the bits of the caller's buffers at that point; image int32 [n_boxes][n][3]; and the step number g.
 *     Later samples are counted as dropped (the sums below still cover them).
 *   - Image counters: the integrators wrap positions into the box every step, so the recorder keeps the positions of the
 *     previous sample and an int32 count per atom and component: image = 0 at q = 0; afterwards d = x - x_prev,
 *     k = rint(d / L) in double, image -= k, so that u = (double)x + (double)image * (double)L is the unwrapped coordinate
 *     (L: the fp32 edge of the atom's box).  Exact as long as no atom moves L / 2 or more between two samples; every
 *     (atom, sample) with a component where |d - k L| > L / 4 is counted in a 64-bit `ambiguous` counter.  Rigid water needs
 *     nothing special (a molecule is re-wrapped by a lattice vector).  The counters belong to ONE box geometry: while n_lags > 0
 *     or GAMD_TRAJ_IMAGE is set, a run whose box differs from the box of the first run since configure / reset returns -22.
 *   - Correlation functions (n_lags > 0): every sample is a time origin; a device ring of n_lags slots holds each origin's
 *     x, image, v.  At sample q, for every lag j = 0 .. min(q, n_lags - 1) with origin o = q - j, per box b and class c:
 *       msd_sum[b][c][j]  += sum_i |du_i|^2,   du_i = (x_q - x_o) + (image_q - image_o) L   (every operand widened to double)
 *       vacf_sum[b][c][j] += sum_i v_i(q) . v_i(o)
 *     in (length unit of the run)^2 and (length unit / ps)^2.  subtract_com: du_i is taken relative to the displacement of
 *     the box's mass-weighted mean of u (masses: the run's mass_amu / mass_h_amu).  Classes: one for GAMD_KIND_LJ handles
 *     or a NULL species_dev; two for water: species flag != 0 (O) is class 0, H is class 1 (the same in every run since
 *     configure / reset, or -22).  The host normalises with (Q - j) * class_atoms[b][c], Q = number of samples.  Double sums
 *     in a fixed order, no floating-point atomics: the same bits run after run.
 * Nothing synchronises or returns to the host inside a run; a run that froze on a neighbour-buffer overflow and was resumed
 * by gamd_sync_status gives the frames and sums of an ample buffer.  A handle whose recorder is off (the default) enqueues
 * exactly what it enqueues without one; with it on, skin-mode runs launch the second half of a SAMPLED step on its own. */
enum { GAMD_TRAJ_X = 1, GAMD_TRAJ_V = 2, GAMD_TRAJ_F = 4, GAMD_TRAJ_IMAGE = 8 };
typedef struct gamd_traj_params {
    int64_t interval;      /* 0 = recorder off (buffers kept); > 0: sample every interval-th completed step */
    int64_t max_frames;    /* frames kept (first max_frames samples; later ones are counted as dropped); 0 = keep no frames */
    int32_t fields;        /* GAMD_TRAJ_* bit mask of what a kept frame holds */
    int32_t n_lags;        /* 0 = no correlation functions; else lags 0 .. n_lags-1 in units of interval, at most 4096 */
    int32_t subtract_com;  /* 1 = MSD of displacements relative to the box's mass-weighted centre-of-mass displacement */
    int32_t reserved;      /* 0 */
} gamd_traj_params;
/* p: HOST.  Allocates and clears frames, image counters, ring and sums (drains nothing: call it between runs, after
 * gamd_sync_status).  Device memory: 24 B per atom, 12 B per atom, field and frame, 36 B per atom and lag.  -22 for a negative
 * interval or max_frames, unknown field bits, n_lags outside [0, 4096], or while a run is pending; -12 when an allocation fails. */
int32_t gamd_traj_configure(gamd_handle* h, const gamd_traj_params* p);
/* Step count g = 0; frames, image counters, ring and sums cleared (the next run may use another box); the configuration stays. */
int32_t gamd_traj_reset(gamd_handle* h);
/* Synchronises `stream` once (it does NOT resume a frozen run: call gamd_sync_status first) and copies frames
 * [first, first + count) that exist to HOST arrays, any of which may be NULL (a field that was not recorded is left
 * untouched): steps int64 [count], x / v / f float and image int32 [count][n_boxes][n][3].  *n_frames = frames kept in all,
 * *dropped = samples that found the frame buffer full. */
int32_t gamd_traj_read_frames(gamd_handle* h, void* stream, int64_t first, int64_t count, int64_t* steps,
                              float* x, float* v, float* f, int32_t* image, int64_t* n_frames, int64_t* dropped);
/* Synchronises `stream` once and copies to HOST arrays, any of which may be NULL: msd_sum and vacf_sum double
 * [n_boxes][classes][n_lags] (elems = room in elements of each; fewer than that product is -22), *n_samples = samples taken
 * (time origins Q), *ambiguous = the counter above, class_atoms int64 [n_boxes][classes], dims[0..2] = n_boxes, classes,
 * n_lags (classes is 0 until the first run since configure / reset). */
int32_t gamd_traj_read_dynamics(gamd_handle* h, void* stream, double* msd_sum, double* vacf_sum, int64_t elems,
                                int64_t* n_samples, uint64_t* ambiguous, int64_t* class_atoms, int32_t dims[3]);

/* Structure sampler: the pair-distance histogram of a radial distribution function out to ANY rdf_rmax up to half the
 * shortest box edge (the reporter's g(r) above walks the edge list and ends at the cutoff) and the partial static structure
 * factors S_ab(k), kept ON THE DEVICE while gamd_md_run / gamd_md_run_nhc are enqueued.
 * The sampler counts the completed MD steps g of the handle since it was configured or reset (across calls, with a counter of
 * its own: its interval is independent of the reporter's and the recorder's).  Step g is sampled when g % interval == 0,
 * behind its second half (for rigid water: behind the velocity constraint), where the other two sample.  A sample is
 *   - rdf_bins > 0: for every box, every unordered pair {i, j}, i != j, of that box's atoms is evaluated ONCE: the fp32
 *     min-image distance r of the wrapped positions of that step's force evaluation (per component d = x_i - x_j or
 *     x_j - x_i, t = d + L/2, t += L if t < 0, t -= L if t >= L, d' = t - L/2; r = sqrtf((dx*dx + dy*dy) + dz*dz), no
 *     contraction).  A pair with r < rdf_rmax adds 2 to the 64-bit counter [box][pair class][bin], bin = min((int)(r *
 *     rdf_bins / rdf_rmax), rdf_bins - 1): the reporter's directed-count convention, so the same normalisation applies
 *     (m_aa = N_a^2, m_ab = 2 N_a N_b).  Pair classes as the reporter's: one for GAMD_KIND_LJ handles; O-O, O-H, H-H for
 *     GAMD_KIND_WATER, O = node feature != 0.  exclude_same_molecule: pairs whose caller-order atom ids share id / 3 are
 *     skipped.  (d + L/2) - L/2 does not round symmetrically in d: against the reporter's histogram only pairs that sit on a
 *     bin edge to fp32 rounding may differ.
 *     Cost: N (N - 1) / 2 distances per box and sample — O(N^2), meant for up to about 10^5 atoms per box.
 *     Precondition: 2 * rdf_rmax <= the shortest edge of every box of the run; otherwise gamd_md_run / gamd_md_run_nhc return
 *     -22 (the message names rdf_rmax) before anything is enqueued.
 *   - sk_n2max > 0: wave vectors k = 2 pi (n_x / L_x, n_y / L_y, n_z / L_z) for the integer triples with 0 < |n|^2 <= sk_n2max,
 *     one of each +-n (the one whose first non-zero component is positive), sorted by (|n|^2, n_x, n_y, n_z): K = 61 / 128 /
 *     462 for sk_n2max = 9 / 16 / 36; at most 4096.  Per box and class c, rho_c(n) = sum_i exp(-2 pi i n.s_i), s_i = (double)x_i
 *     / (double)L per component from the caller's position buffer, the phase n_x s_x + n_y s_y + n_z s_z and sincospi(2 phase)
 *     in double, the atoms summed in a fixed assignment and order.  Then sk_sum[box][pair][k] += Re(rho_a conj(rho_b)) for the
 *     pair classes above (LJ: |rho|^2; classes O, H by species_dev != 0, which a water handle must then be given).  The same
 *     bits run after run.  The host normalises S_ab(k) = sk_sum / (frames * sqrt(N_a N_b)) (Ashcroft-Langreth).
 * Device memory: 8 B per box, pair class and bin; 8 B per box, pair class and k-vector; 16 B per box, class, k-vector and
 * block of 256 atoms (at most 64 blocks).
 * Nothing synchronises or returns to the host inside a run; a run that froze on a neighbour-buffer overflow and was resumed
 * by gamd_sync_status gives the counts and sums of an ample buffer.  A handle whose sampler is off (the default) enqueues
 * exactly what it enqueues without one; with it on, skin-mode runs launch the second half of a SAMPLED step on its own. */
typedef struct gamd_struct_params {
    int64_t interval;        /* 0 = sampler off (buffers are kept); > 0: sample every interval-th completed step */
    int32_t rdf_bins;        /* 0 = no histogram; at most 1024 */
    float rdf_rmax;          /* upper edge of the last bin, > 0 when rdf_bins > 0 (no default: half the shortest box edge at most) */
    int32_t exclude_same_molecule;
    int32_t sk_n2max;        /* 0 = no structure factors; else every n with 0 < |n|^2 <= sk_n2max (K <= 4096) */
    int32_t reserved[2];     /* 0 */
} gamd_struct_params;
/* p: HOST.  Builds the k-vector list, allocates and clears histogram and sums (drains nothing: call it between runs, after
 * gamd_sync_status).  -22 for a negative interval, rdf_bins outside [0, 1024], rdf_bins > 0 without rdf_rmax > 0, an sk_n2max
 * with more than 4096 k-vectors, or while a run is pending; -12 when an allocation fails. */
int32_t gamd_struct_configure(gamd_handle* h, const gamd_struct_params* p);
/* Step count g = 0, histogram and sums cleared; the configuration and the k-vector list stay. */
int32_t gamd_struct_reset(gamd_handle* h);
/* Synchronises `stream` once (it does NOT resume a frozen run: call gamd_sync_status first) and copies to HOST arrays, any
 * of which may be NULL: counts uint64 [n_boxes][pair classes][rdf_bins], sk_sum double [n_boxes][pair classes][K], kvec int32
 * [K][3] (count_elems / sk_elems / kvec_elems = room in elements; fewer than needed is -22).  *frames = samples taken,
 * dims[0..3] = n_boxes, pair classes, rdf_bins, K. */
int32_t gamd_struct_read(gamd_handle* h, void* stream, uint64_t* counts, int64_t count_elems, double* sk_sum, int64_t sk_elems,
                         int32_t* kvec, int64_t kvec_elems, int64_t* frames, int32_t dims[4]);

/* Classical observer: where a classical potential exists the reference judges a rollout by it — the potential energy of the
 * GNN-driven run against the classical run (LJ/test_script/lj.ipynb cells 5-6; potentialEnergy / totalEnergy of
 * dataset/generate_lj_data.py:87-90) and the network force against the classical force on every frame (gt_force,
 * LJ/test_script/test_langevin.py:102-106; cosine, MAE, RMSE, relative MAE of lj.ipynb cell 3).  This observer evaluates the
 * switched, shifted Lennard-Jones potential ON THE DEVICE while gamd_md_run / gamd_md_run_nhc are enqueued, and
 * gamd_classical_eval evaluates it on given positions outside a run.  GAMD_KIND_LJ handles only, one pair class; no long-range
 * dispersion correction, no electrostatics (a GAMD_KIND_WATER handle is refused with -22; gamd_water_configure below evaluates
 * 3-site water).
 * The potential, for the minimum-image distance r of a pair (d = x_i - x_j, per component d - L rint(d / L) in double, L the
 * fp32 box edge widened; r^2 = (dx^2 + dy^2) + dz^2):
 *     u_LJ(r) = 4 epsilon [(sigma / r)^12 - (sigma / r)^6],   u0 = u_LJ(r_cut) with `shift`, else 0
 *     S(r) = 1 for r <= r_switch;  1 - 6 t^5 + 15 t^4 - 10 t^3, t = (r - r_switch) / (r_cut - r_switch), beyond it (OpenMM's
 *     switching function); r_switch = 0 or r_switch >= r_cut: no switching
 *     u(r) = (u_LJ - u0) S for r^2 < r_cut^2, else 0;   F_ij = -u'(r) d / r
 * Per box: E = sum_{i<j} u, the virial W = sum_{i<j} d . F_ij = -sum r u'(r), and the number of pairs inside r_cut.  sigma,
 * r_cut, r_switch are in the handle's length unit (like gamd_config.cutoff), epsilon in kJ/mol, forces in kJ/mol/nm through the
 * run's (or the call's) length_per_nm, like f; E and W in kJ/mol.  Everything is computed in double from the caller's fp32
 * position buffer in the caller's atom order, every atom walks its full row (N (N - 1) pair terms per box and sample — O(N^2):
 * meant for sampling intervals, not for every step), powers by multiplication, no contraction, no floating-point atomics, fixed
 * summation order: the same bits run after run.
 * The observer counts the completed MD steps g of the handle since it was configured or reset (across calls, with a counter of
 * its own).  Step g is sampled when g % interval == 0, behind its second half, where the other observers sample: f then holds
 * the network forces at the sampled positions.  A sample writes row g / interval - 1 (rows beyond max_samples are dropped and
 * counted): {g; per box E, W, pairs, and the force-error sums of f (widened to double) against the classical force f_cl:
 * sum_i sum_c |D_ic|, sum_i |D_i|^2, sum_i cos(f_i, f_cl,i), sum_i |f_cl,i|, sum_i |f_i| with D = f - f_cl, and the number of
 * atoms left out of the cosine sum because f_i or f_cl,i is zero}.  The last sample's f_cl stays readable.
 * Precondition: 2 * r_cut <= the shortest edge of every box (the minimum image is the nearest image only below that);
 * otherwise gamd_md_run / gamd_md_run_nhc / gamd_classical_eval return -22 (the message names r_cut) before anything is enqueued.
 * Device memory: 48 B per atom and slice (at most 32 slices per row), 24 B per atom, 72 B per box and row.
 * Nothing synchronises or returns to the host inside a run; a run that froze on a neighbour-buffer overflow and was resumed by
 * gamd_sync_status gives the rows of an ample buffer (a sample that runs twice writes the same bits twice).  A handle whose
 * classical observer is off (the default) enqueues exactly what it enqueues without one; with it on, skin-mode runs launch the
 * second half of a SAMPLED step on its own. */
typedef struct gamd_classical_params {
    int64_t interval;        /* 0 = observer off: the parameters below are still taken (gamd_classical_eval uses them), rows kept */
    int64_t max_samples;     /* rows allocated by gamd_classical_configure with interval > 0; 0 = 4096 */
    double sigma;            /* length unit of the handle, > 0 */
    double epsilon;          /* kJ/mol, finite */
    double r_cut;            /* length unit of the handle, > 0 */
    double r_switch;         /* 0 or >= r_cut: no switching; else 0 < r_switch < r_cut */
    int32_t shift;           /* 1: u0 = u_LJ(r_cut) */
    int32_t reserved;        /* 0 */
} gamd_classical_params;
enum { GAMD_CLASSICAL_ROW = 9 };   /* doubles per box and row: E, W, pairs, the five sums in the order above, atoms left out */
/* p: HOST.  Takes the parameters; with interval > 0 allocates and clears the rows (drains nothing: call it between runs, after
 * gamd_sync_status).  -22 for a negative interval or max_samples, sigma or r_cut not positive, a non-finite epsilon, a negative
 * r_switch, a GAMD_KIND_WATER handle, more than 65535 boxes, or while a run is pending; -12 when an allocation fails. */
int32_t gamd_classical_configure(gamd_handle* h, const gamd_classical_params* p);
/* Step count g = 0, rows cleared; parameters and configuration stay. */
int32_t gamd_classical_reset(gamd_handle* h);
/* Synchronises `stream` once (it does NOT resume a frozen run: call gamd_sync_status first) and copies to HOST arrays, any of
 * which may be NULL: steps int64 [max_rows], rows double [max_rows][n_boxes][GAMD_CLASSICAL_ROW], f_cl double [n_boxes * n_atoms][3]
 * (the classical forces of the last sample or gamd_classical_eval call; f_cl_elems = room in elements, fewer than 3 n is -22;
 * left untouched when nothing was evaluated yet).  *n_rows = rows in the log (at most max_rows are written), *dropped = samples
 * that found the log full. */
int32_t gamd_classical_read(gamd_handle* h, void* stream, int64_t* steps, double* rows, int64_t max_rows, int64_t* n_rows,
                            int64_t* dropped, double* f_cl, int64_t f_cl_elems);
/* The same kernels on given positions, outside any run, with the parameters of the last gamd_classical_configure (interval 0
 * will do): pos_dev float [n_boxes * n_atoms][3] DEVICE (any periodic image), box HOST [n_boxes][3], length_per_nm (0 = 10,
 * Angstrom), f_out_dev double [n_boxes * n_atoms][3] DEVICE (kJ/mol/nm; may be NULL), energy / virial / pairs HOST double
 * [n_boxes] (any may be NULL).  Enqueued on `stream`, which is synchronised once.  -22 before gamd_classical_configure, while a
 * run is pending, or when 2 * r_cut exceeds a box edge. */
int32_t gamd_classical_eval(gamd_handle* h, const float* pos_dev, const float* box, float length_per_nm, double* f_out_dev,
                            double* energy, double* virial, double* pairs, void* stream);

/* The pairs of the Lennard-Jones classical potential over a cell table instead of all against all: an optional, sticky property
 * of the handle, switched as gamd_water_cells is.  on = 0 (the default): every entry point launches what it launched before
 * this switch existed and gives the same bits.  on = 1: the observer's sample, gamd_classical_eval, the GAMD_FORCE_CLASSICAL
 * source and gamd_minimize (every iteration, from its double positions, and its final force) replace their pair launch by six
 * (clear, count, scan, fill, rank, pairs) on the caller's stream.  Per evaluation and box the atoms are ordered by
 * (cell, atom index) — cells of edge >= r_cut / 2, nc_d = min(floor(2 L_d / (r_cut (1 + 2^-20))), 64) per axis from the box's
 * own edges — and every atom walks the table's runs under the 5 x 5 (x, y) columns around its cell (every cell of an axis with
 * fewer than five), on the positions as they are given, with the all-pairs walk's operations: the set of pairs and the pair
 * count are exactly the all-pairs path's; E, W and the forces differ from it in the ORDER of the sums only and lie within the
 * same 1e-12 of their sums of absolute terms of the float64 reference.  The same bits come back run after run, from fresh
 * handles, per box of a several-box handle, in chunked runs, across a neighbour-buffer overflow; a driven frame still carries
 * fp32(f_cl of gamd_classical_eval on its positions) and gamd_minimize's f is that at its x.  NOT promised in bits: the same
 * atoms given in other periodic images may fall into a neighbouring cell at a face, which changes the order of the sums (within
 * the bound above).  Whether the table pays at a size: profiles/run_classical_cells.md.  Not built: a table kept across steps
 * with a skin, non-orthorhombic boxes.
 * -22, with a message naming the reason: a null handle, a GAMD_KIND_WATER handle (gamd_water_cells is that potential's), no
 * accepted gamd_classical_configure, a pending run, on not 0 or 1; from a run that follows a pending run when its boxes need
 * larger tables.  -12 when the tables cannot be allocated (44 B per atom, 8 B per box and cell); the switch is then off. */
int32_t gamd_classical_cells(gamd_handle* h, int32_t on);

/* Diagnostic: the cell table of box `box` as the last sample, gamd_classical_eval call, driven step or gamd_minimize call left
 * it, to the host; arguments, meaning and refusals are gamd_water_cells_read's (below). */
int32_t gamd_classical_cells_read(gamd_handle* h, void* stream, int32_t box, int32_t* nc, int32_t* start, int64_t max_start,
                                  int32_t* order, int64_t max_order);

/* Force source of an enqueued run: the classical run next to the GNN run — the reference's LJ data generator is a
 * Nose-Hoover-chain run under the classical force (dataset/generate_lj_data.py:74-107), and lj.ipynb cells 5-6 plot the
 * GNN-driven logs against its log.  Sticky per handle, GAMD_FORCE_NETWORK by default.  It decides where the forces of
 * gamd_md_run and gamd_md_run_nhc come from, the resume inside gamd_sync_status included; gamd_forces*, gamd_forces_host,
 * gamd_forces_edges and gamd_profile evaluate the network whatever the source.
 * GAMD_FORCE_CLASSICAL: every step runs the neighbour stage as before (skin check, exact re-filter, fused integrator halves,
 * counters, overflow detection — the observers and the freeze / resume machinery hang on it) and then, in place of encoder,
 * conv layers and decoder, two launches: the pair pass of the classical observer on the run's x and box (same tiles, slices
 * and arithmetic) and a per-atom pass that adds an atom's slice partials in order from 0, forms f_cl = F * length_per_nm in
 * double and stores (float)f_cl, rounded to nearest, into the run's f in the caller's atom order.  f is bit for bit the fp32
 * rounding of what gamd_classical_eval gives on the same positions, run after run (no floating-point atomics, no contraction,
 * plain stores: a step enqueued again after a freeze writes the same bits).  On entry f must hold the classical forces at x
 * (gamd_classical_eval's, rounded to fp32).  The parameters are those of the last gamd_classical_configure, which may change
 * them between runs while the source stays; the classical observer may be armed or not (a step that is driven and sampled is
 * evaluated twice, to the same bits).  O(N^2) per step and box.
 * Precondition of a classical-source run: 2 * r_cut <= the shortest edge of every box; otherwise gamd_md_run /
 * gamd_md_run_nhc return -22 (the message names r_cut) before anything is enqueued.  The potential's work buffers are ensured
 * there as well (-12 when that fails): nothing is allocated inside a run.  The handle must be finalized like for every run.
 * -22, with a message naming the reason: a null handle, an unknown source, while a run is pending, GAMD_FORCE_CLASSICAL on a
 * GAMD_KIND_WATER handle, GAMD_FORCE_CLASSICAL before an accepted gamd_classical_configure (interval 0 will do).
 * GAMD_FORCE_WATER_CLASSICAL: the same for a GAMD_KIND_WATER handle under the 3-site water potential of gamd_water_configure
 * (O-O Lennard-Jones plus a plain Ewald sum, in double) — the reference's water data generator is a rigid-water
 * Nose-Hoover-chain run under that potential (dataset/generate_tip3p_data.py:76-103).  Behind the neighbour stage five
 * launches: the pair pass of the water observer with the force accumulators only, the observer's own three reciprocal-space
 * kernels (charge density, S(k), per-atom k sums), and a per-atom pass that adds the pair slices and the k slices in order
 * from 0 and stores f_cl and (float)f_cl.  f is bit for bit the fp32 rounding of what gamd_water_eval gives on the same
 * positions and species, and must hold that on entry.  O(N^2 + N K) per step and box, K the k-vectors of the list.
 * A water-source run needs, or gamd_md_run / gamd_md_run_nhc return -22 before anything is enqueued (x, v, f untouched):
 * rigid_water in its parameters (the potential has no bond or angle term and excludes same-molecule pairs, so only the
 * constraints hold a molecule together), species, 2 * r_cut <= every box edge, and no run pending on the handle (the k-vector
 * list is built or swapped for the run's boxes at that point).
 * -22 from gamd_md_force_source besides the above: GAMD_FORCE_WATER_CLASSICAL on a GAMD_KIND_LJ handle, or before an accepted
 * gamd_water_configure (interval 0 will do).
 * gamd_water_minimize (below) relaxes a start and leaves x and f as this source expects them.  With gamd_water_msite the
 * source drives the 4-site (TIP4P) form of the potential by seven launches; a start is then minimised under that form with
 * gamd_water_minimize_potential on (below), or with w_h = 0 (see there).
 * Particle-mesh Ewald is gamd_water_pme (below).  Not built: the PME virial, odd orders, grids that are no power of two, real-to-complex transforms,
 * a barostat.  The default parameters of gamd_water_configure remain UNVERIFIED
 * against OpenMM. */
enum { GAMD_FORCE_NETWORK = 0, GAMD_FORCE_CLASSICAL = 1, GAMD_FORCE_WATER_CLASSICAL = 2 };
int32_t gamd_md_force_source(gamd_handle* h, int32_t source);

/* Water classical observer: the classical potential of 3-site water — the reference logs OpenMM's potential energy for its
 * TIP3P data and trains on getForces (dataset/generate_tip3p_data.py:91-103), and its rollout driver fetches classical forces
 * beside the network's (water/test_script/test_nosehoover_hb.py:107).  GAMD_KIND_WATER handles, atoms in the caller's order
 * O,H,H: molecule = caller-order index / 3 (n_atoms must be a multiple of 3), O = species flag != 0, charges q_H and
 * q_O = -2 q_H (every molecule neutral: no background term).  Electrostatics are a plain Ewald sum in double, exact to the
 * stated truncation (no PME grid).  Per box, with d the minimum-image vector of a pair (per component d - L rint(d / L), L the
 * fp32 edge widened), r = |d|, C = coulomb_const * length_per_nm, V = L_x L_y L_z:
 *     U_LJ    = the switched, shifted 12-6 form of gamd_classical_params (sigma_o, epsilon_o, r_cut, r_switch, shift), O-O pairs
 *               of different molecules with r^2 < r_cut^2
 *     U_real  = C sum_{i<j, different molecules, r^2 < r_cut^2} q_i q_j erfc(alpha r) / r
 *     U_excl  = -C sum_{i<j, same molecule} q_i q_j erf(alpha r) / r                 (minimum image, no cutoff)
 *     U_recip = (4 pi C / V) sum_k A(k) |S(k)|^2,  A(k) = exp(-k^2 / 4 alpha^2) / k^2,  S(k) = sum_j q_j exp(-i k.r_j),
 *               k = 2 pi (n_x / L_x, n_y / L_y, n_z / L_z) over one of each +-n with 0 < |k| <= k_cut
 *     U_self  = -C alpha / sqrt(pi) sum_i q_i^2
 * and the forces are the exact negative gradients of these terms times length_per_nm (kJ/mol/nm).  The integer triples are one
 * list per handle, built for the longest edge of the boxes of the run or call and sorted by (|n|^2, n_x, n_y, n_z); a box gives
 * the vectors beyond its own k_cut the weight A = 0.  At most 131 072 triples: a longer list is refused with -22 (the message
 * names k_cut).  The TIP4P M-site is set by gamd_water_msite (below): until then a handle evaluates the 3-site form of the
 * parameters it is given.  The row holds no virial: with rigid molecules the atomic virial is not the pressure, and the
 * molecular virial is a log of its own (gamd_water_virial, below).
 * Sample point, step counter, rows, resume rule and the off state are those of the classical observer above.  A row holds, per
 * box: U_LJ, U_real + U_excl, U_recip, U_self, the different-molecule pairs inside r_cut, the five force-error sums of f against
 * the classical force in the order of gamd_classical_params, the atoms left out of the cosine, and sum_i q_i, which is exactly
 * 0.0 for a species vector with one O and two H per molecule (the charges are summed as integers -2, +1 and scaled once).
 * Precondition: 2 * r_cut <= the shortest edge of every box, and a species vector; otherwise gamd_md_run / gamd_md_run_nhc /
 * gamd_water_eval return -22 before anything is enqueued.  Cost per sample and box: N (N - 1) pair terms and 2 N K reciprocal
 * terms (K k-vectors), all in double.
 * Device memory: 48 B per atom and pair slice, 24 B per atom and k slice (at most 32 slices each), 24 B per atom, 12 B + 24 B per
 * k-vector (and box), 16 B per box, k-vector and block of 256 atoms (at most 64 blocks), 96 B per box and row. */
typedef struct gamd_water_params {
    int64_t interval;        /* 0 = observer off: the parameters below are still taken (gamd_water_eval uses them), rows kept */
    int64_t max_samples;     /* rows allocated by gamd_water_configure with interval > 0; 0 = 4096 */
    double q_h;              /* hydrogen charge in e, finite; q_O = -2 q_h */
    double sigma_o;          /* length unit of the handle, > 0 */
    double epsilon_o;        /* kJ/mol, finite */
    double r_cut;            /* length unit of the handle, > 0: real-space Coulomb and Lennard-Jones cutoff */
    double r_switch;         /* Lennard-Jones only; 0 or >= r_cut: no switching */
    int32_t shift;           /* 1: u0 = u_LJ(r_cut) */
    int32_t reserved;        /* 0 */
    double alpha;            /* Ewald splitting parameter, 1 / length unit, > 0 */
    double k_cut;            /* reciprocal cutoff, 1 / length unit, > 0 */
    double coulomb_const;    /* 1 / (4 pi eps0) in kJ nm / (mol e^2), finite (138.935456) */
} gamd_water_params;
enum { GAMD_WATER_ROW = 12 };      /* doubles per box and row, in the order above */
/* p: HOST.  Takes the parameters and builds the k-vector list for the handle's current boxes; with interval > 0 allocates and
 * clears the rows (drains nothing: call it between runs, after gamd_sync_status).  -22 for a negative interval or max_samples,
 * sigma_o, r_cut, alpha or k_cut not positive, a non-finite q_h, epsilon_o or coulomb_const, a negative r_switch, a k_cut with no
 * or more than 131 072 k-vectors, a GAMD_KIND_LJ handle, n_atoms not a multiple of 3, more than 65535 boxes, or while a run is
 * pending; -12 when an allocation fails. */
int32_t gamd_water_configure(gamd_handle* h, const gamd_water_params* p);
/* Step count g = 0, rows cleared; parameters and configuration stay. */
int32_t gamd_water_reset(gamd_handle* h);
/* As gamd_classical_read, with rows double [max_rows][n_boxes][GAMD_WATER_ROW]. */
int32_t gamd_water_read(gamd_handle* h, void* stream, int64_t* steps, double* rows, int64_t max_rows, int64_t* n_rows,
                        int64_t* dropped, double* f_cl, int64_t f_cl_elems);
/* The same kernels on given positions, outside any run, with the parameters of the last gamd_water_configure (interval 0 will
 * do): pos_dev float [n_boxes * n_atoms][3] DEVICE (any periodic image), species_dev uint8 [n_boxes * n_atoms] DEVICE, box HOST
 * [n_boxes][3], length_per_nm (0 = 10, Angstrom), f_out_dev double [n_boxes * n_atoms][3] DEVICE (kJ/mol/nm; may be NULL), rows
 * HOST double [n_boxes][GAMD_WATER_ROW] (may be NULL; the force-error sums are 0).  Enqueued on `stream`, which is synchronised
 * once.  -22 before gamd_water_configure, without species, while a run is pending, when 2 * r_cut exceeds a box edge or the
 * boxes need more than 131 072 k-vectors. */
int32_t gamd_water_eval(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev, const float* box, float length_per_nm,
                        double* f_out_dev, double* rows, void* stream);
/* The TIP4P M-site: the reference's third ground-truth generator is WaterBox(model='tip4pew')
 * (dataset/generate_tip4p_data.py), and it drops the M-site before the network (train_utils.py:58-59) — so do handles,
 * integrators and SETTLE here, which see O,H,H.  The site lives inside the potential: w_h > 0 moves the negative charge of every
 * molecule from the oxygen onto a virtual site M (OpenMM's ThreeParticleAverageSite with weights 1 - 2 w_h, w_h, w_h;
 * TIP4P-Ew: w_h = 0.106676721).  Per molecule, atoms in the caller's order O,H,H (molecule = index / 3, the oxygen first):
 *     d_k  = H_k - O per component as d - L rint(d / L)      (the atoms may be in any periodic image)
 *     M    = O' + w_h (d_1 + d_2), in double from the fp32 positions widened, O' = O - L floor(O / L)
 * The CHARGE SITES of a molecule are M (q = -2 q_H), H1 and H2 (q_H, wrapped into [0, L) like O'); the LENNARD-JONES SITE is O.
 * Every Coulomb term of the formulas above is taken on charge-site positions: U_real over different-molecule site pairs with
 * site distance r^2 < r_cut^2, U_excl over the three same-molecule site pairs M-H1, M-H2, H1-H2, S(k) and U_recip over the
 * sites; U_self is unchanged (sum q^2 is).  U_LJ is taken on O-O distances with a cutoff test of its own on the O-O distance:
 * a pair of molecules can be inside for one term and outside for the other.  With F_s the complete force on a charge site
 * (pair slices added in order from 0, plus the k term) and F_LJ the Lennard-Jones force, per component and in this order
 *     F_O  = F_LJ(O) + (1 - 2 w_h) F_M
 *     F_Hk = F_s(Hk) + w_h F_M
 * and then times length_per_nm: the exact negative gradient with respect to the three real atoms.  The GAMD_WATER_ROW layout is
 * unchanged; its pair entry counts the different-molecule CHARGE-SITE pairs inside r_cut, and sum q is still exactly 0.0.
 * The M-site is a property of the potential, not a force source: gamd_water_eval, the observer inside gamd_md_run /
 * gamd_md_run_nhc and a GAMD_FORCE_WATER_CLASSICAL run all follow the weight in force.  w_h = 0 restores the 3-site potential,
 * served by the 3-site kernels bit for bit; the weight holds across later gamd_water_configure calls until it is changed.
 * With w_h != 0 the observer is eight launches (a site prepass, the Coulomb pair pass, the O-O Lennard-Jones pass, charge
 * density, S(k), per-atom k sums, the per-atom pass, the final row) and the force source seven behind the neighbour stage (its
 * pair passes are the observer's: energies are computed and not read); f is bit for bit the fp32 rounding of gamd_water_eval's forces, and must hold that on entry.
 * gamd_water_minimize with w_h != 0 minimises under the 4-site form while gamd_water_minimize_potential is on (below); while it
 * is off (the default) it returns -22 (the message names the M-site and the switch) before anything is enqueued.  Start recipe
 * without the switch: gamd_water_minimize with w_h = 0, gamd_water_msite(h, w_h), gamd_water_eval on the minimised x, its forces
 * rounded to fp32 as f on entry of the run.
 * -22, with a message naming the reason: a null handle, a GAMD_KIND_LJ handle, no accepted gamd_water_configure, a pending
 * run, w_h not finite, negative or >= 0.5.  -12 when the extra work buffers cannot be allocated: they are ensured here or at
 * run entry, never inside a run.  Device memory added while w_h != 0: 24 B per atom (the sites) and 32 B per molecule and pair
 * slice (the oxygen's Lennard-Jones force and energy, apart from the site force).
 * Particle-mesh Ewald (gamd_water_pme, below) serves the M-site form as well.  Not built: the PME virial, odd orders, grids that are no power of two, real-to-complex transforms
 * (the molecular virial is gamd_water_virial below; the long-range dispersion correction
 * is a host function of the Python package).  The TIP4P-Ew parameters the Python
 * package offers (q_H = 0.52422 e, sigma_O = 3.16435 Angstrom, epsilon_O = 0.680946 kJ/mol, w_h = 0.106676721) were written
 * down from memory and are UNVERIFIED against OpenMM's tip4pew.xml; no parity with OpenMM is claimed. */
int32_t gamd_water_msite(gamd_handle* h, double w_h);

/* Smooth particle-mesh Ewald (Essmann et al. 1995) for the reciprocal part of the water classical potential: an optional,
 * sticky property of the handle, switched as the M-site is.  order = 4 or 6 (the B-spline order; even orders only: for an odd
 * order the interpolation modulus vanishes at m = n / 2) and a grid of nx x ny x nz points per box, each length one of 8, 16,
 * 32, 64, 128 (every box of the handle has a grid of its own, of the same dimensions).  order = 0 switches PME off: the plain
 * sum of gamd_water_configure is back, served by its own kernels bit for bit.  The setting survives later gamd_water_configure
 * and gamd_water_msite calls.
 * While PME is on the observer's sample, gamd_water_eval and the GAMD_FORCE_WATER_CLASSICAL source replace their three
 * reciprocal launches by ten (clear, spread, three line passes, convolution, three line passes, gather), in double, by
 * hand-written kernels on the caller's stream: the charges in units of q_H are spread with the B-spline weights as 64-bit
 * integers (quantum 2^-50 q_H, so the grid does not depend on the order of the additions, and the same bits come back run
 * after run), transformed by a radix-2 FFT per axis, multiplied by exp(-pi^2 |m|^2 / alpha^2) / (|m|^2 B(m)) with m_d / L_d
 * per component, transformed back and differentiated analytically at the atoms.  U_recip = (C / 2 pi V) q_H^2 sum_m G |Q^|^2
 * stands in column 2 of the row.  k_cut is not read and the limit of 131 072 k-vectors does not apply; alpha, r_cut, the
 * real-space, exclusion and self terms are unchanged.  The accuracy is set by the grid and the order, not by ewald_tol: with
 * alpha = 0.63 / Angstrom (r_cut 6.8, ewald_tol 1e-8) and order 6 a spacing of 0.45 Angstrom leaves an rms force difference of
 * a few 1e-5 of the rms force against the plain sum (profiles/run_water_pme.md).
 * Not built: the PME virial — gamd_water_virial(h, 1) and gamd_water_virial_eval return -22 while PME is on, and gamd_water_pme
 * returns -22 while the virial log is armed (messages name PME).  The minimisers follow PME while gamd_water_minimize_potential
 * is on (below) and return -22 while it is off; start recipe without the switch: minimise under the plain sum, switch PME on,
 * take f from gamd_water_eval.  Nor odd orders, grids that are no power of two,
 * real-to-complex transforms.
 * -22, with a message naming the reason: a null handle or block, a GAMD_KIND_LJ handle, no accepted gamd_water_configure, a
 * pending run, an order other than 0, 4, 6, a grid length outside {8, 16, 32, 64, 128}.  -12 when the grids cannot be
 * allocated (24 B per box and grid point, plus the tables); the handle is then on the plain sum. */
typedef struct gamd_water_pme_params {
    int32_t order;      /* 0 = off, 4, 6 */
    int32_t nx, ny, nz; /* grid points per axis and box */
} gamd_water_pme_params;
int32_t gamd_water_pme(gamd_handle* h, const gamd_water_pme_params* p);

/* The real-space pairs of the water classical potential over a cell table instead of all against all: an optional, sticky
 * property of the handle, switched as the M-site and PME are.  on = 0 (the default): every entry point launches what it
 * launched before this switch existed and gives the same bits.  on = 1: the observer's sample, gamd_water_eval and the
 * GAMD_FORCE_WATER_CLASSICAL source, in the 3-site form and in the M-site form (on the charge sites), replace their pair launch
 * by six (clear, count, scan, fill, rank, pairs) on the caller's stream.  Per sample and box the atoms are ordered by
 * (cell, atom index) — cells of edge >= r_cut / 2, nc_d = min(floor(2 L_d / (r_cut (1 + 2^-20))), 64) per axis from the box's
 * own edges — and every atom walks the 5 x 5 x 5 cells around its own (every cell of an axis with fewer than five), on the
 * positions as they are given, with the all-pairs walk's operations: the set of pairs, the pair count and the charge sum are
 * exactly the all-pairs path's, U_recip and U_self its bits; U_LJ, U_real + U_excl and the forces differ from it in the ORDER
 * of the sums only and lie within the same 1e-12 of their sums of absolute terms of the float64 references.  The same bits come
 * back run after run, from fresh handles, per box of a several-box handle, in chunked runs, and a driven frame still carries
 * fp32(f_cl of gamd_water_eval on its positions).  NOT promised in bits: the same atoms given in other periodic images may
 * fall into a neighbouring cell at a face, which changes the order of the sums (within the bound above).
 * The table costs six launches: below a few thousand atoms all pairs are faster (profiles/run_water_cells.md).
 * Not built, and served all-pairs while the switch is on: the O-O pass of the M-site form, the virial log's own pair walk
 * (which reads the cells' f_cl).  The minimisers walk the table while gamd_water_minimize_potential is on (below); while it is
 * off gamd_water_minimize returns -22 while this switch is on
 * (its f is the all-pairs force bit for bit: minimise with the cells off, switch them on, take f from gamd_water_eval).  Nor a
 * table kept across steps with a skin, nor non-orthorhombic boxes.
 * -22, with a message naming the reason: a null handle, a GAMD_KIND_LJ handle, no accepted gamd_water_configure, a pending
 * run, on not 0 or 1.  -12 when the tables cannot be allocated (44 B per atom, 8 B per box and cell); the switch is then off. */
int32_t gamd_water_cells(gamd_handle* h, int32_t on);

/* Diagnostic: the cell table of box `box` as the last sample, gamd_water_eval call or driven step left it, to the host.
 * nc[3] = the cells per axis; start[nc[0] nc[1] nc[2] + 1] = the first table slot of every cell, cell = (cx nc[1] + cy) nc[2] +
 * cz, and n_atoms per box behind the last; order[n_atoms per box] = the atoms (index inside the box) in table order.  start and
 * order may be NULL.  Synchronises `stream`.  -22 if the switch is off, if nothing has been sampled since it was switched on or
 * since the boxes were last given, or if a buffer is too short. */
int32_t gamd_water_cells_read(gamd_handle* h, void* stream, int32_t box, int32_t* nc, int32_t* start, int64_t max_start,
                              int32_t* order, int64_t max_order);

/* The molecular virial of the water classical potential, and with it the scalar pressure of a box of rigid molecules (with
 * rigid molecules the atomic virial is not the pressure: the constraint forces carry the rest).  Per box, all sums in double,
 * every term in kJ/mol:
 *     W_LJ        = sum over the pairs of U_LJ of -(r u'(r)), u the switched, shifted form in force
 *     W_coul,pair = sum over the pairs of U_real and of U_excl of fs_coul r^2, fs_coul the Coulomb part of the force scalar
 *                   F_ij = fs d: C q_i q_j (erfc(alpha r) / r + g) or C q_i q_j (g - erf(alpha r) / r),
 *                   g = (2 alpha / sqrt(pi)) exp(-alpha^2 r^2); charge sites with an M-site, O-O distances for W_LJ
 *     W_recip     = (4 pi C / V) sum_k A(k) |S(k)|^2 (1 - k^2 / (2 alpha^2)), k-vectors, A and S(k) those of U_recip
 *     W_intra     = sum over molecules and their atoms a of s_a . F_a / length_per_nm, F_a the atom's total classical force
 *                   (kJ/mol/nm, behind the M-site redistribution) and s_a = r_a - R_mol from the minimum-image vectors
 *                   d_k = H_k - O alone: s_O = -(m_H / M)(d_1 + d_2), s_Hk = d_k + s_O, M = m_O + 2 m_H
 *     KE_com      = sum over molecules of |m_O v_O + m_H (v_H1 + v_H2)|^2 / (2 M), velocities over length_per_nm (nm/ps), amu
 *     W_mol       = ((W_LJ + W_coul,pair) + W_recip) - W_intra
 * and P = (2 KE_com + W_mol) / (3 V) (times 16.6053906717 for bar with V in nm^3).  The pressure tensor, a barostat and the
 * atomic virial with constraint forces are not built.
 * gamd_water_virial(h, 1) arms the virial log of the water classical observer, gamd_water_virial(h, 0) switches it off; call it
 * between runs, behind gamd_water_configure.  While it is on, every sample the observer takes also writes a row
 * {W_LJ, W_coul,pair, W_recip, W_intra, KE_com, W_mol} per box in the same slot as its GAMD_WATER_ROW row, from the same frame
 * (x and f_cl of the sample, v behind the step's second half, the run's mass_amu / mass_h_amu: as the run reporter's KE), by
 * four more launches behind the observer's (five with an M-site) that write nothing the observer or a force source reads: rows
 * of gamd_water_read, f_cl and the trajectory are bit for bit what they are with the log off, and with it off every entry point
 * launches exactly what it did.  Same resume rule: a sample evaluated twice writes the same bits twice.  The rows are cleared by
 * gamd_water_configure (interval > 0) and gamd_water_reset, and by switching the log on.
 * -22, with a message: a null handle, a GAMD_KIND_LJ handle, no accepted gamd_water_configure, a pending run (the state is left
 * as it was).  -12 when the buffers cannot be allocated.  Device memory while on: 16 B per atom and pair slice, 8 B per molecule
 * and pair slice with an M-site, 48 B per box and row. */
enum { GAMD_WATER_VIRIAL_ROW = 6 };
int32_t gamd_water_virial(gamd_handle* h, int32_t on);
/* rows HOST double [max_rows][n_boxes][GAMD_WATER_VIRIAL_ROW], slot for slot the samples of gamd_water_read (whose steps are
 * theirs); *n_rows = the rows kept.  A slot sampled while the log was off holds zeros.  -22 while the log has never been on. */
int32_t gamd_water_virial_read(gamd_handle* h, void* stream, double* rows, int64_t max_rows, int64_t* n_rows);
/* The same kernels outside a run, behind those of gamd_water_eval on the same arguments (armed or not): vel_dev float
 * [n_boxes * n_atoms][3] DEVICE in length unit / ps, or NULL (KE_com = 0); mass_o_amu, mass_h_amu > 0; rows HOST double
 * [n_boxes][GAMD_WATER_VIRIAL_ROW]; water_rows HOST double [n_boxes][GAMD_WATER_ROW] or NULL: gamd_water_eval's rows of the same
 * call.  Refusals as gamd_water_eval, and -22 for a mass that is not positive and finite. */
int32_t gamd_water_virial_eval(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev, const float* vel_dev,
                               const float* box, float length_per_nm, double mass_o_amu, double mass_h_amu, double* rows,
                               double* water_rows, void* stream);

/* Energy minimiser: every reference driver relaxes its start in front of the first step (minimizeEnergy(tolerance = 1 kJ/mol),
 * dataset/generate_lj_data.py:83; minimizeEnergy(1e-6), LJ/test_script/test_langevin.py:84, test_nosehoover.py:88).
 * gamd_minimize relaxes the positions of every box of a GAMD_KIND_LJ handle under the classical potential of the last
 * gamd_classical_configure (interval 0 will do) ON THE DEVICE and leaves x and f as a classical-source gamd_md_run /
 * gamd_md_run_nhc expects them on entry.  It is NOT OpenMM's L-BFGS and claims no parity with it: the algorithm is FIRE
 * (Bitzek et al., Phys. Rev. Lett. 97, 170201 (2006)) in the semi-implicit Euler form.  What is matched is the meaning of the
 * tolerance: the root mean square of all 3N force components of a box, in kJ/mol/nm.
 * Per box and iteration, on double positions x (the fp32 input widened) and double velocities v (0 at the start), with the
 * scalars dt = dt_start, alpha = alpha_start, n_pos = 0:
 *   1. F (kJ/mol/nm, through length_per_nm) and U (kJ/mol) at x: the pair term of gamd_classical_configure, operation for
 *      operation, box edges the fp32 edges widened.
 *   2. ff = sum F.F, vf = sum v.F, vv = sum v.v and U in a fixed order; rms = sqrt(ff / 3N).  U or ff not finite: the box stops
 *      as GAMD_MIN_FAILED with the positions of this iteration.  Else rms <= tolerance: it stops as GAMD_MIN_CONVERGED.
 *   3. vf > 0: v = (1 - alpha) v + (alpha sqrt(vv / ff)) F; then, if n_pos > n_min, dt = min(dt f_inc, dt_max) and
 *      alpha = alpha f_alpha; then n_pos += 1.  Otherwise v = 0, alpha = alpha_start, dt = dt f_dec, n_pos = 0.
 *   4. v = v + dt F, dr = dt v, per atom dr *= max_step / |dr| where |dr| > max_step, x = x + dr.
 * F is in kJ/mol/nm while x and max_step are in the handle's length unit: dt is a pseudo-time that absorbs the units (and the
 * mass), so dt_start and dt_max go with the length unit — the defaults are for Angstrom.  After max_iter position updates a
 * box that still runs is evaluated once more (steps 1 and 2) and, unless that converges, stops as GAMD_MIN_MAX_ITER.
 * Everything is in double with fixed summation orders, no floating-point atomics and no contraction: the same bits run after
 * run, whatever check_every is, and every box of a handle gets the bits it gets alone.  The host enqueues check_every
 * iterations at a time and looks at the boxes' states only between such chunks; a box that stopped is skipped on the device.
 * Nothing is allocated between the first and the last enqueue.  O(N^2) per iteration and box.
 * On return (the stream is synchronised):
 *   x_dev        float [n_boxes * n_atoms][3] DEVICE, in and out: the double positions rounded to nearest and wrapped into the
 *                box by the integrators' expression.  A box that was not finite at the start keeps x as given.
 *   f_dev        float [n_boxes * n_atoms][3] DEVICE, out: the classical force at exactly those fp32 positions, by the kernels
 *                of the classical force source — bit for bit the fp32 rounding of gamd_classical_eval's forces on x_dev, the
 *                precondition of a GAMD_FORCE_CLASSICAL run.  Nothing is written for a box that failed.
 *   x64_dev      double [n_boxes * n_atoms][3] DEVICE or NULL: the unrounded, unwrapped positions.
 *   rows_host    double [n_boxes][GAMD_MINIMIZE_ROW] HOST or NULL: state (GAMD_MIN_*), iterations (position updates), U and rms
 *                at the start, U, rms and the largest |force component| at the end, the final dt.
 * Returns 0: every box converged; 1: at least one box stopped at max_iter; 2: at least one box failed (not finite).
 * -22, with a message naming the reason: a null params / x_dev / f_dev / box, a non-positive or non-finite tolerance, negative
 * counts, a constant outside its range (f_dec, f_alpha, alpha_start in (0, 1); f_inc > 1; dt_max >= dt_start > 0;
 * max_step > 0), a null handle, a GAMD_KIND_WATER handle, no accepted gamd_classical_configure, a pending run, a box edge
 * that is not positive or below 2 * r_cut (the message names r_cut).  -12 when an allocation fails; -1 on a handle that a
 * neighbour-buffer overflow of gamd_forces_async left frozen (call gamd_sync_status first).
 * Device memory besides the classical observer's work buffers: 84 B per atom. */
typedef struct gamd_minimize_params {
    double tolerance;        /* kJ/mol/nm, > 0 and finite (the reference's data generator: 1; its rollout drivers: 1e-6) */
    int64_t max_iter;        /* position updates at most; 0 = 10000 */
    int64_t check_every;     /* iterations enqueued between two looks at the boxes' states; 0 = 64 */
    double dt_start;         /* 0 = 0.002 */
    double dt_max;           /* 0 = 0.02 */
    double f_inc;            /* 0 = 1.1 */
    double f_dec;            /* 0 = 0.5 */
    double alpha_start;      /* 0 = 0.1 */
    double f_alpha;          /* 0 = 0.99 */
    double max_step;         /* length unit of the handle; 0 = 0.1 */
    int32_t n_min;           /* 0 = 5 */
    int32_t reserved;        /* 0 */
} gamd_minimize_params;
enum { GAMD_MINIMIZE_ROW = 8 };
enum { GAMD_MIN_CONVERGED = 0, GAMD_MIN_MAX_ITER = 1, GAMD_MIN_FAILED = 2 };
int32_t gamd_minimize(gamd_handle* h, float* x_dev, const float* box, float length_per_nm, float* f_dev, double* x64_dev,
                      const gamd_minimize_params* params, double* rows_host, void* stream);

/* L-BFGS energy minimiser: gamd_minimize's task, arguments and tail with a quasi-Newton algorithm, for the tolerances and sizes
 * at which FIRE's iteration count is what costs (the rollout drivers' minimizeEnergy(1e-6)).  OpenMM's minimizeEnergy is L-BFGS
 * too, but NO parity with its implementation is claimed: the line search and the stopping rule below are this library's own.
 * What is matched is the meaning of the tolerance: the root mean square of all 3N force components of a box, in kJ/mol/nm.
 * gamd_minimize, its parameter block, its states and its bits are untouched by this entry.
 * Per box, in double: x is the fp32 input widened, F in kJ/mol/nm (through length_per_nm) and U in kJ/mol are the pair term of
 * gamd_classical_configure as gamd_minimize evaluates it; x and max_step are in the handle's length unit (the quasi-Newton
 * scaling absorbs the units, as FIRE's dt does).  The history is a ring of at most m pairs (s, y).
 *   1. U and F at the start.  U or F.F not finite: the box stops as GAMD_LBFGS_FAILED and keeps the x it was given.
 *      rms = sqrt(F.F / 3N) <= tolerance: it stops as GAMD_LBFGS_CONVERGED with 0 evaluations.
 *   2. The direction d.  Empty history: d = F max_step / max_i |F_i| (the largest per-atom norm).  Otherwise d = H F by the
 *      two-loop recursion over the ring with H0 = s.y / y.y of the newest pair.  The trial factor t = 1.
 *   3. The trial displacement s_i = t d_i per atom, scaled to length max_step where it is longer; x_t = x + s, and s is from
 *      here on the difference x_t - x as the doubles give it.
 *   4. U_t and F_t at x_t: one evaluation, counted whatever follows.
 *   5. The trial is accepted iff F.s > 0, U_t is finite and U_t <= U - c1 F.s.  Rejected: t = t / 2 and step 3 again; after
 *      max_ls rejections in a row, or at once when F.s <= 0, the search has failed: with a non-empty history the history is
 *      emptied (a reset), d is step 2's steepest direction, t = 1 and step 3 follows; with an empty one the box stops as
 *      GAMD_LBFGS_LINE_SEARCH at x.
 *   6. Accepted: y = F - F_t; the pair (s, y) enters the ring, displacing the oldest of m, iff s.y > curv sqrt(s.s y.y) (else
 *      the push is skipped); x = x_t, F = F_t, U = U_t.  rms <= tolerance: GAMD_LBFGS_CONVERGED.  Else, max_iter evaluations
 *      used up: GAMD_LBFGS_MAX_ITER.  Else step 2.
 *   7. A box that uses up max_iter on a rejected trial stops as GAMD_LBFGS_MAX_ITER at the last accepted x.
 * One evaluation is three launches whatever m is (six more with gamd_classical_cells): the pair pass on x_t, one pass for every
 * inner product, one pass that decides and updates; the recursion runs on the inner products of the ring's vectors alone.
 * Everything is in double with fixed summation orders, no floating-point atomics and no contraction: the same bits run after
 * run, whatever check_every is, and every box of a handle gets the bits it gets alone.  The host enqueues check_every
 * evaluations at a time and looks at the boxes' states only between such chunks; a box that stopped is skipped on the device.
 * Nothing is allocated between the first and the last enqueue.  tests/lbfgs_ref.py is this recipe in float64 on the host.
 * On return (the stream is synchronised) x_dev, f_dev and x64_dev are as gamd_minimize leaves them: the accepted double positions
 * rounded to fp32 and wrapped; the classical force source's force at exactly those fp32 positions; the unrounded positions.
 * Nothing is written for a box that failed.
 *   rows_host    double [n_boxes][GAMD_LBFGS_ROW] HOST or NULL: state (GAMD_LBFGS_*), evaluations (behind the start's), accepted
 *                steps, U and rms at the start, U, rms and the largest per-atom |F_i| at the end, pushes the curvature test
 *                skipped, history resets.
 * Returns 0: every box converged; 1: a box stopped at max_iter; 2: a box failed (not finite); 3: a box stopped in the line
 * search — the largest wins.  -22, with a message naming the reason, before anything is enqueued: what gamd_minimize refuses
 * (null params / x_dev / f_dev / box, tolerance, negative counts, max_step, a null or GAMD_KIND_WATER handle, no accepted
 * gamd_classical_configure, a pending run, a box edge that is not positive or below 2 * r_cut), m outside [1, 8], c1 outside
 * (0, 1), a negative curv or max_ls, a non-zero reserved.  -12 when an allocation fails; -1 on a frozen handle.
 * Device memory besides the classical observer's work buffers: 24 (2 m + 5) + 12 B per atom, the ring sized for the m in force. */
typedef struct gamd_lbfgs_params {
    double tolerance;        /* kJ/mol/nm, > 0 and finite */
    int64_t max_iter;        /* evaluations behind the start's at most; 0 = 10000 */
    int64_t check_every;     /* evaluations enqueued between two looks at the boxes' states; 0 = 64 */
    double max_step;         /* length unit of the handle; 0 = 0.1 */
    double c1;               /* sufficient decrease, in (0, 1); 0 = 1e-4 */
    double curv;             /* curvature test of a push, > 0; 0 = 1e-10 */
    int32_t m;               /* pairs in the ring, 1 .. 8; 0 = 6 */
    int32_t max_ls;          /* rejections in a row that fail a line search; 0 = 20 */
    int64_t reserved;        /* 0 */
} gamd_lbfgs_params;
enum { GAMD_LBFGS_ROW = 10 };
enum { GAMD_LBFGS_CONVERGED = 0, GAMD_LBFGS_MAX_ITER = 1, GAMD_LBFGS_FAILED = 2, GAMD_LBFGS_LINE_SEARCH = 3 };
int32_t gamd_minimize_lbfgs(gamd_handle* h, float* x_dev, const float* box, float length_per_nm, float* f_dev, double* x64_dev,
                            const gamd_lbfgs_params* params, double* rows_host, void* stream);

/* Energy minimiser for rigid 3-site water: every water driver of the reference relaxes its start in front of the first step
 * (minimizeEnergy, dataset/generate_tip3p_data.py:85).  gamd_water_minimize is gamd_minimize for a GAMD_KIND_WATER handle under
 * the potential of the last gamd_water_configure (interval 0 will do), ON THE DEVICE, and leaves x and f as a
 * GAMD_FORCE_WATER_CLASSICAL gamd_md_run / gamd_md_run_nhc with rigid_water expects them on entry.  It is NOT OpenMM's L-BFGS
 * (which treats the constraints by restraints) and claims no parity with it: the algorithm is FIRE on rigid molecules.  What is
 * shared is the meaning of the tolerance — here the root mean square over 3N of the components of the PROJECTED force.
 * Atoms in the caller's order O,H,H, molecule = index / 3, O = species != 0.  r_oh, r_hh: the rigid geometry in the length
 * unit; 0 = TIP3P (0.9572 A, 104.52 degrees: r_hh = 1.5139 A) scaled by length_per_nm / 10.  All constraint arithmetic takes
 * UNIT weights for the three atoms, not their masses: the projection is then the orthogonal one and the projected force F_c is
 * the gradient on the constraint manifold.  The canonical triangle of SETTLE is rc = r_hh / 2, t = sqrt(r_oh^2 - rc^2),
 * ra = 2 t / 3, rb = t / 3.
 * Start: x = the fp32 input widened, then every molecule put on the exact geometry by SETTLE in double with reference = new =
 * the input; v = 0; dt = dt_start, alpha = alpha_start, n_pos = 0.  Per box and iteration:
 *   1. F (kJ/mol/nm) and U (kJ/mol) at x, the terms of gamd_water_configure operation for operation on the double positions:
 *      a same-molecule pair takes the erf branch, another pair with r^2 < r_cut^2 the erfc branch and, O-O, the Lennard-Jones
 *      term; the reciprocal sum over the handle's k-vector list; U = ((U_real + U_excl + U_recip) + U_self) + U_LJ.
 *   2. Per molecule F and v are projected onto the tangent space of the three bond constraints at x (a 3x3 solve): F_c, v.
 *      ff = sum F_c.F_c, vf = sum v.F_c, vv = sum v.v in a fixed order; rms = sqrt(ff / 3N), N atoms.
 *   3. U or ff not finite: the box stops as GAMD_MIN_FAILED.  Else rms <= tolerance: GAMD_MIN_CONVERGED.  Else, in the pass
 *      behind max_iter position updates: GAMD_MIN_MAX_ITER.  A box that stops applies no update.
 *   4. FIRE's mixing and step exactly as gamd_minimize spells them, on F_c: v = v + dt F_c, dr = dt v; per MOLECULE one factor
 *      max_step / max_k |dr_k| where the largest |dr_k| of its three atoms exceeds max_step; x = SETTLE(reference x, new x + dr).
 * gamd_minimize_params and its defaults mean what they mean for gamd_minimize.  Everything is in double with fixed summation
 * orders, no floating-point atomics and no contraction: the same bits run after run, whatever check_every is, and every box of
 * a handle gets the bits it gets alone.  O(N^2 + N K) per iteration and box, six launches.
 * On return (the stream is synchronised):
 *   x_dev        float [n_boxes * n_atoms][3] DEVICE, in and out: molecules whole, the oxygen in [0, L) per component.  Per
 *                molecule and component, with L the fp32 edge widened and xO, xH the double positions:
 *                  s = L floor(xO / L);  if xO - s < 0: s = s - L;  if (float)(xO - s) >= L: s = s + L;
 *                  O = max((float)(xO - s), 0),  H = (float)(xH - s)   (round to nearest)
 *                — an oxygen that rounds up to L goes to 0 and takes its hydrogens along.  A box that was not finite at the
 *                start (two atoms at one point, a molecule SETTLE cannot place) keeps x as given.
 *   f_dev        float [n_boxes * n_atoms][3] DEVICE, out: the water force source's force at exactly those fp32 positions —
 *                bit for bit the fp32 rounding of gamd_water_eval's forces on x_dev.  Nothing is written for a box that failed.
 *   x64_dev      double [n_boxes * n_atoms][3] DEVICE or NULL: the unrounded, unwrapped positions, every molecule exactly
 *                rigid (the input widened for a box that failed at iteration 0).
 *   rows_host    double [n_boxes][GAMD_MINIMIZE_ROW] HOST or NULL: state, iterations, U and rms at the start, U, rms and the
 *                largest |F_c component| at the end, the final dt.
 * Returns 0 / 1 / 2 as gamd_minimize.  -22, with a message naming the reason, before anything is enqueued: what gamd_minimize
 * refuses in the parameter block, a negative or non-finite r_oh / r_hh, r_hh >= 2 r_oh, a null handle, a GAMD_KIND_LJ handle,
 * an atom count per box that is no multiple of 3, no accepted gamd_water_configure, a pending run, a null x_dev / f_dev / box,
 * no species, a box edge that is not positive or below 2 * r_cut (the message names r_cut), a handle that a neighbour-buffer
 * overflow left frozen (call gamd_sync_status first).  -12 when an allocation fails.
 * Device memory besides the water classical observer's work buffers: 84 B per atom (x, v, F_c in double and the fp32 force). */
int32_t gamd_water_minimize(gamd_handle* h, float* x_dev, const uint8_t* species_dev, const float* box, float length_per_nm,
                            double r_oh, double r_hh, float* f_dev, double* x64_dev, const gamd_minimize_params* params,
                            double* rows_host, void* stream);

/* L-BFGS energy minimiser for rigid 3-site water: gamd_water_minimize's task, arguments, return tail and f contract with
 * gamd_minimize_lbfgs's algorithm, parameter block, states and result row, for the tolerances at which FIRE's iteration count is
 * what costs (one water evaluation is six launches with the pair walk and the Ewald sum).  OpenMM's minimizeEnergy is L-BFGS
 * too, with the constraints as restraints: NO parity with it is claimed, what is shared is the meaning of the tolerance — the
 * root mean square over 3N of the components of the PROJECTED force, in kJ/mol/nm.  gamd_water_minimize, gamd_minimize_lbfgs,
 * their parameter blocks, states and bits are untouched by this entry.
 * Per box, in double.  Atoms O,H,H, molecule = index / 3, r_oh, r_hh and the UNIT weights of all constraint arithmetic as for
 * gamd_water_minimize; the iterate lives on the manifold of rigid molecules, SETTLE is the retraction onto it.
 *   0. x = the fp32 input widened, then every molecule put on the exact geometry by SETTLE with reference = new = the input.
 *   1. U and the raw force at x exactly as step 1 of gamd_water_minimize gives them; F is the raw force projected onto the
 *      tangent space of the three bond constraints at x (gamd_water_minimize's F_c), rms = sqrt(F.F / 3N).  U or F.F not
 *      finite: the box stops as GAMD_LBFGS_FAILED and keeps the x it was given.  rms <= tolerance: GAMD_LBFGS_CONVERGED with
 *      0 evaluations.
 *   2. The direction d.  Empty history: d = F max_step / max_i |F_i| (the largest per-atom norm).  Otherwise d = H F by the
 *      two-loop recursion over the ring with H0 = s.y / y.y of the newest pair.  The trial factor t = 1.
 *   3. The trial: s = t d; per MOLECULE one factor max_step / max_k |s_k| where the largest |s_k| of its three atoms exceeds
 *      max_step (gamd_water_minimize's clamp); x_t = SETTLE(reference x, new x + s).  From here on s is x_t - x as the doubles
 *      give it: it includes SETTLE's second-order correction, so a per-atom |s| may exceed max_step by that correction.  A
 *      molecule SETTLE cannot place makes x_t, and with it U_t and F.s, not finite: the trial is rejected, and F.s counts as
 *      not positive in step 5.
 *   4. U_t and F_t at x_t, F_t projected at x_t: one evaluation, counted whatever follows.
 *   5. The trial is accepted iff F.s > 0, U_t is finite and U_t <= U - c1 F.s.  F is tangent at x, so F.s is the directional
 *      derivative along the retraction to first order.  Rejected: t / 2, max_ls, the reset and the GAMD_LBFGS_LINE_SEARCH stop
 *      exactly as step 5 of gamd_minimize_lbfgs.
 *   6. Accepted: y = F - F_t, each projected at its own point; the push test, x = x_t, F = F_t, U = U_t, the stop tests and
 *      GAMD_LBFGS_MAX_ITER exactly as steps 6 and 7 of gamd_minimize_lbfgs.  The ring's vectors are used AS STORED: there is
 *      no vector transport of s and y to the tangent space of the new point.  d is then not exactly tangent at x; SETTLE
 *      removes the normal part of the step, and the sufficient-decrease test guards descent.
 * The DEFAULT Lennard-Jones term of gamd_water_configure is truncated at r_cut without a switch or a shift: U jumps by about
 * 0.03 kJ/mol when an O-O pair crosses r_cut = 6.5 A, and a sufficient-decrease test cannot pass such a jump once the steps
 * gain less than that.  On the default potential the search therefore stops as GAMD_LBFGS_LINE_SEARCH somewhere below a
 * tolerance of about 1 (FIRE never looks at U and does not notice): TOLERANCES BELOW ABOUT 1 NEED r_switch > 0 OR shift = 1.
 * One evaluation is six launches whatever m is: the four force launches of gamd_water_minimize on x_t, one per-molecule pass
 * that projects F_t and forms every inner product, one pass that decides, runs the recursion on the inner products alone and
 * forms the next trial with SETTLE.  Everything is in double with fixed summation orders, no floating-point atomics and no
 * contraction: the same bits run after run, whatever check_every is, and every box of a handle gets the bits it gets alone.  A
 * box that stopped is skipped on the device; nothing is allocated between the first and the last enqueue.
 * tests/water_lbfgs_ref.py is this recipe in float64 on the host.
 * On return (the stream is synchronised) x_dev (molecules whole, the oxygen in [0, L) by gamd_water_minimize's wrap), f_dev (bit
 * for bit the fp32 rounding of gamd_water_eval's forces on x_dev, by the water force source's own kernels) and x64_dev (exactly
 * rigid; the input widened for a failed box) are as gamd_water_minimize leaves them.  Nothing is written for a box that failed.
 *   rows_host    double [n_boxes][GAMD_LBFGS_ROW] HOST or NULL: gamd_minimize_lbfgs's row; the forces in it are F_c, and fmax is
 *                the largest per-atom |F_c,i|.
 * Returns 0 / 1 / 2 / 3 as gamd_minimize_lbfgs, the largest wins.  -22, with a message naming the reason, before anything is
 * enqueued: what gamd_minimize_lbfgs refuses in the parameter block, and everything gamd_water_minimize refuses — a set M-site
 * (gamd_water_msite), particle-mesh Ewald on (gamd_water_pme) and the cell table on (gamd_water_cells) among them while
 * gamd_water_minimize_potential is off — a frozen handle included.  -12 when an allocation fails.
 * Device memory besides the water classical observer's work buffers: 24 (2 m + 5) + 12 B per atom, the ring sized for the
 * largest m a call has asked for (x, x_t, F, F_t, d and the ring in double, the fp32 force). */
int32_t gamd_water_minimize_lbfgs(gamd_handle* h, float* x_dev, const uint8_t* species_dev, const float* box, float length_per_nm,
                                  double r_oh, double r_hh, float* f_dev, double* x64_dev, const gamd_lbfgs_params* params,
                                  double* rows_host, void* stream);

/* The two water minimisers under the potential AS THE HANDLE IS CONFIGURED: an optional, sticky property of the handle, switched
 * as the M-site, PME and the cell table are.  on = 0 (the default): gamd_water_minimize and gamd_water_minimize_lbfgs know the
 * 3-site, plain-sum, all-pairs form alone, refuse the other forms with -22, launch what they launched before this switch
 * existed and give the same bits.  on = 1: both minimise under whatever gamd_water_msite, gamd_water_pme (orders 4 and 6, every
 * offered grid) and gamd_water_cells have set, in any combination, none of them included; with none set the results are the
 * switch-off results bit for bit.  The contract of each entry keeps its shape: x whole molecules with the oxygen in [0, L), x64
 * exactly rigid, nothing written for a failed box, the same states and rows, f bit for bit the fp32 rounding of
 * gamd_water_eval's forces on x UNDER THE CONFIGURATION IN FORCE, and the tolerance bounds the rms over 3N components of the
 * projected force in kJ/mol/nm — the projection of the force on the three real atoms, after M's force has been spread with the
 * weights 1 - 2 w_h, w_h, w_h.  U in the rows is the configured potential's (U_recip by PME where PME is on).
 * Launches per iteration / evaluation on the caller's stream: the pair pass 1 (the cell table: 6), the reciprocal part 3
 * (PME: 10), with the M-site a site prepass on the double positions and the O-O pass on top (+ 2), the per-molecule pass and the
 * update: 6 for the 3-site plain all-pairs form, 25 for M-site + PME + cells.  A box that has stopped is skipped by the
 * minimisers' own kernels; the potential's reused kernels evaluate it again into work buffers nobody reads for it: its x64,
 * state and row stay, and a box gets the bits it gets alone.
 * Still not built: vector transport of the L-BFGS ring, a Wolfe line search, flexible water, minimising inside an enqueued run;
 * the PME virial remains refused.
 * -22, with a message naming the reason: a null handle, a GAMD_KIND_LJ handle, no accepted gamd_water_configure, a pending
 * run, on not 0 or 1.  No device memory of its own. */
int32_t gamd_water_minimize_potential(gamd_handle* h, int32_t on);

/* Event-timed replay of one force evaluation: per-kernel milliseconds of the last gamd_profile call.
 * names: newline-separated kernel labels; ms: one float per label.  For bench.py's roofline block. */
int32_t gamd_profile(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev, const float* box,
                     float* out_norm_dev, void* stream, char* names, size_t names_bytes, float* ms, int32_t max_ms,
                     int32_t* n_out);

/* Live timing of the dominant kernel (conv-layer edge kernel) inside a timed region: while enabled,
 * every conv-edge launch is bracketed by HIP events on the launch stream.  gamd_timing_read
 * synchronises the stream and returns the summed duration and the launch count since the last
 * enable.  Used by bench.py for roofline.achieved. */
int32_t gamd_timing_enable(gamd_handle* h, int32_t enable);
int32_t gamd_timing_read(gamd_handle* h, void* stream, double* total_ms, int64_t* n_launches);
/* The same events split by stage: [0] conv-layer edge kernel (= gamd_timing_read), [1] edge encoder (its own event pair),
 * [2] the node kernel between two conv layers (from the stop event of layer l to the start event of layer l + 1, so it
 * includes the two kernel boundaries around it). */
int32_t gamd_timing_read_stages(gamd_handle* h, void* stream, double total_ms[3], int64_t n_launches[3]);
/* While timing is enabled, gamd_md_run / gamd_md_run_nhc also record one HIP event in front of the first kernel of every MD
 * step (the iteration of the drivers' loop, LJ/test_script/test_langevin.py:95-113) and one behind the last: step_ms[i] =
 * device time between consecutive events, in enqueue order, since the last gamd_timing_enable.  Writes at most max_steps
 * values; *n_steps = intervals available.  K runs of n steps give K * n intervals: the interval between the event behind a run's
 * last step and the first event of the next run (the host's gap between two calls, or the re-allocation of a run that froze
 * on a neighbour-buffer overflow) is not a step and is skipped.  A step that takes far longer than the median is a candidate
 * rebuild or a stall: bench.py reports min / p50 / p99 / max.  The event pools are bounded (65 536 step events): with timing
 * left on across a longer run the remaining steps are not timed. */
int32_t gamd_timing_read_steps(gamd_handle* h, void* stream, float* step_ms, int64_t max_steps, int64_t* n_steps);

#ifdef __cplusplus
}
#endif
#endif /* GAMD_HIP_H */

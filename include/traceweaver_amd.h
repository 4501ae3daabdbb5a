/*
 * traceweaver_amd.h -- C-ABI of the MI355X span->parent assignment engine (libtwgpu.so).
 *
 * The reference (Sachin-A/TraceWeaver) has no FFI; its drop-in boundary is the Python predictor
 * protocol (algorithms/README.md:12-73) as used by the executor:
 *     TraceWeaverV3(all_spans, all_processes).FindAssignments(method, process, in_span_partitions,
 *         out_span_partitions, parallel, instrumented_hops, true_assignments, invocation_graph)
 *     -> (all_assignments, all_topk_assignments, not_best_count, n_in, per_span_candidates,
 *         cnt_unassigned)                       traceweaver_v3.py:1087-1229, executor.py:1172-1175
 * traceweaver_amd/predictor.py mirrors that signature and drives the functions below through
 * ctypes.  Strings and (trace_id, span_id) keys never cross this ABI: the shim maps ids <-> indices.
 *
 * All pointers are plain host pointers unless a function says otherwise; the caller owns every
 * host buffer, the engine owns every device buffer.  Every function returns TW_OK (0) or a negative
 * tw_status; tw_last_error() gives the message.  One engine may be used from one thread at a time.
 *
 * Data model ("batch" = independent service units solved together; "unit" = one call of the
 * reference's FindAssignments):
 *   - incoming spans of a unit sorted by (start, end)                      executor.py:1112
 *   - outgoing endpoints in the topological order of the call-order DAG    traceweaver_v1.py:37-39
 *   - every endpoint's spans sorted by (start, end)
 *   - timestamps are int64 microseconds (Jaeger JSON startTime / startTime+duration)
 * A batch is either a no-skip batch (every endpoint of every unit holds exactly as many outgoing spans as the unit
 * has incoming spans, traceweaver_v3.py:972,1141-1158 "equal_eps": two passes with the mixture refit in between) or a
 * skip-mode batch (tw_batch.skip != NULL; exps/exp2: some requests did not call an endpoint: ONE pass with skip spans,
 * traceweaver_v3.py:820-989,1155-1156).
 */
#ifndef TRACEWEAVER_AMD_H
#define TRACEWEAVER_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TW_MAX_EP 8      /* outgoing endpoints per unit                                     */
#define TW_TOPK 5        /* candidates kept per incoming span        traceweaver_v3.py:1109 */
#define TW_MAX_COMP 5    /* mixture components per edge              traceweaver_v3.py:768  */
#define TW_MAX_WINDOW 32 /* incoming spans per window (reference cap: 31)    */
#define TW_CAND_WORDS 2  /* 64-bit words of the per-(span, endpoint) candidate bitmap       */
#define TW_SKIP_BASE 1024
#define TW_SKIP_STRIDE 128

typedef enum {
    TW_OK = 0,
    TW_ERR_ARG = -1,          /* bad argument / inconsistent sizes                                   */
    TW_ERR_UNSUPPORTED = -2,  /* skip mode (n_out != n_in), E > TW_MAX_EP, topk != TW_TOPK           */
    TW_ERR_DEVICE = -3,       /* HIP runtime error                                                   */
    TW_ERR_STATE = -4,        /* call order violated (e.g. pass 2 before pass 1)                     */
    TW_ERR_WINDOW_WIDTH = -5, /* an incoming span has > 64*TW_CAND_WORDS candidate spans at one      */
                              /* endpoint (the reference's enumeration is infeasible there too)      */
    TW_ERR_WINDOW_SIZE = -6,  /* a window holds more than TW_MAX_WINDOW incoming spans                */
    TW_ERR_NAN_PARAMS = -7,   /* a 100-span block has a single sample: std = NaN, the reference      */
                              /* aborts in the solver (SURVEY.md hazard H3)                          */
    TW_ERR_SKIP_PARAMS = -8,  /* skip mode: the scorer needs a (mean, std) pair BuildDistributions   */
                              /* did not produce (KeyError in the reference, traceweaver_v1.py:118)  */
    TW_ERR_SKIP_REFERENCE_RAISES = -9, /* skip mode: the reference raises on this input (a tuple that */
                              /* skips every endpoint, hazard H7; a score tie whose comparison       */
                              /* reaches a skip span; a skipped predecessor without a called one)    */
    TW_ERR_FIT = -10          /* refit: every model-selection fit of an edge raised in scikit-learn  */
                              /* (covariance <= 0), so the reference's np.argmin([]) raises too      */
                              /* (traceweaver_v3.py:777-780)                                         */
} tw_status;

typedef struct tw_engine tw_engine;

/* Replaces: TraceWeaverV3.__init__ (traceweaver_v3.py:30-54).  device_id = HIP device ordinal. */
int tw_create(int device_id, tw_engine **out);
void tw_destroy(tw_engine *e);
const char *tw_last_error(const tw_engine *e);

/* A batch of independent units in structure-of-arrays form.
 * Replaces: the in_span_partitions / out_span_partitions / invocation_graph arguments of
 * FindAssignments (traceweaver_v3.py:1087) for each unit.
 * Initialise the whole struct to zero (`tw_batch b = {0};` / memset) before filling it in: optional members are NULL = absent,
 * and members added by later versions of this header are appended at the end with zero meaning "as before" -- a caller that
 * leaves them uninitialised hands tw_load_batch a garbage pointer. */
typedef struct {
    int32_t n_units;
    const int64_t *unit_in_off; /* [n_units+1] offsets into in_start/in_end                        */
    const int32_t *unit_E;      /* [n_units]   outgoing endpoints per unit (1..TW_MAX_EP)           */
    const int64_t *ep_off;      /* [sum(E)+1]  offsets into out_start/out_end of every (unit,ep)    */
                                /*             segment, units in order, endpoints in topo order     */
    const uint8_t *dag;         /* concatenated E*E matrices, dag[p*E+e]=1 <=> edge p->e            */
                                /*             (executor.py:214-285 FindOrder, transitively closed) */
    const int32_t *key_rank;    /* [sum(E)]    rank of the endpoint in the partition-key order:     */
                                /*             networkx in_edges() iteration order of predecessors  */
    const int64_t *in_start, *in_end;   /* [unit_in_off[n_units]]                                   */
    const int64_t *out_start, *out_end; /* [ep_off[sum(E)]]                                         */
    int32_t batch_size;     /* 100  traceweaver_v3.py:1107 */
    int32_t batch_size_mis; /* 30   traceweaver_v3.py:1108 */
    int32_t topk;           /* 5    traceweaver_v3.py:1109 */
    /* Load-scaled units (helpers/transforms.py:10-40 repeat_change_spans, called at executor.py:1146-1148 when
     * --compress_factor > 1): the reference's timestamps are Python floats there (start / load_factor).  Such a
     * unit is handed over with its timestamps as exact integers in units of unit_time_scale[u] microseconds (a
     * power of two, e.g. 2^-3): comparisons are then the reference's float comparisons, differences are
     * (double)(t2 - t1) * scale exactly, and the sums of ComputeEpPairDistParams3 (traceweaver_v3.py:593,605)
     * accumulate in binary64 left to right as Python's sum() does over floats.  NULL = every unit holds plain
     * int64 microseconds (exact integer sums, as Python does over ints). */
    const double *unit_time_scale; /* [n_units] or NULL */
    /* Skip mode (NULL = a no-skip batch): one descriptor per unit.  The unit's lists are taken as they are -- after
     * helpers/transforms.py:153-238 (create_cache_hits) they are no longer sorted, and the reference bisects and walks
     * them as handed over (traceweaver_v3.py:1115 runs before the sort of :968-971); endpoints may hold fewer spans
     * than there are incoming spans.  Timestamps must be integer microseconds (unit_time_scale == NULL). */
    const struct tw_skip_unit *skip;
    /* Parts of a service (NULL = every unit is a whole service).  A service solved in parts -- consecutive stretches of its
     * requests, cut at PerfectCuts (traceweaver_v3.py:1024-1039), one unit each, e.g. on several GPUs -- must get the windows
     * of the unsplit run.  CreateWindows2 (:1056-1076) treats the service's first and last request specially: the first one
     * is counted twice towards the size cap (current_count starts at 1, a request after a cut starts at 0), the last one is
     * never tested for a PerfectCut.  unit_part[u] bit 0 (TW_PART_AFTER_CUT): the unit's first request follows a cut -- its
     * first window is counted like a window after a PerfectCut; bit 1 (TW_PART_BEFORE_CUT): a cut follows the unit's last
     * request -- that request is tested for a PerfectCut like any inner one. */
    const uint8_t *unit_part;   /* [n_units] or NULL */
} tw_batch;
#define TW_PART_AFTER_CUT 1
#define TW_PART_BEFORE_CUT 2

/* What TallySkipSpans (traceweaver_v3.py:853-989) and BuildDistributions (:108-172) hand the main loop. */
typedef struct tw_skip_unit {
    int32_t n_tw;            /* time windows of 30 requests (traceweaver_v3.py:976-987), in start order            */
    const int64_t *tw_start; /* [n_tw]                                                                              */
    const int32_t *pool;     /* [E][n_tw] skip spans per (endpoint, window) after water-filling, <= 128             */
    const double *dist;      /* [(E+1)][(E+1)][2] (mean, std) of the delay between two endpoints' spans, NaN where  */
                             /* no sample exists; index 0 = the incoming endpoint, 1 + e = outgoing endpoint e      */
} tw_skip_unit;

/* Copies the batch into HBM (span arrays: 16 B per span).  If `spans_on_device` is non-zero the
 * four span arrays are *device* pointers (already resident, e.g. produced by a device-side loader)
 * and are copied device-to-device; the small descriptor arrays are always host pointers.  A skip-mode batch
 * (tw_batch.skip) takes host span arrays only: TW_ERR_UNSUPPORTED otherwise. */
int tw_load_batch(tw_engine *e, const tw_batch *b, int spans_on_device);

/* Pass 1 (traceweaver_v3.py:1159-1219, iteration 0): windows (CreateWindows2, :1020-1078),
 * per-100-span Gaussian parameters (ComputeEpPairDistParams3, :580-646), candidate enumeration
 * + log-likelihood + top-5 (FindTopKAssignments, :180-465; ScoreAssignmentAsPerInvocationGraph,
 * traceweaver_v1.py:259-361), exact per-window selection (GetAssignmentsMIS, :1237-1281 +
 * Gurobi_MIS :1395-1419) and commit with span consumption (AddAssignment, traceweaver_v1.py:433-463). */
int tw_run_pass1(tw_engine *e);

/* Gap samples implied by the pass-1 assignment, one row of n_in doubles per scored slot of each
 * unit (ComputeEpPairDistParams5's `durations`, traceweaver_v3.py:717-762); entries of unassigned
 * incoming spans and rows of unscored slots are NaN.  Slot order per unit (nslot = E*E + 2E):
 *   [0,E) root(in->e) | E + p*E + e primary(p->e) | E + E*E + e closing(e->in).
 * `gaps` holds sum_u nslot_u * n_in_u doubles, unit after unit. */
int tw_get_gaps(tw_engine *e, double *gaps);

/* The other direction (layout of tw_get_gaps): gap samples for tw_fit_mixtures that were not produced by this engine's
 * pass 1 -- a service whose requests were solved in parts (on several GPUs) is refitted on the union of the parts'
 * samples, exactly as the reference fits one mixture per edge over the whole service (traceweaver_v3.py:1221-1222):
 * load a unit of the service's shape, hand over the gathered rows, tw_fit_mixtures, tw_get_mixtures
 * (traceweaver_amd/sharding.py).  The fit depends on the samples of a row *in request order* (k-means++ seeding): parts that are
 * consecutive stretches of the service's requests are concatenated in that order. */
int tw_set_gaps(tw_engine *e, const double *gaps);

/* The engine's own device buffers of the two exchange steps of a sharded run, so that a collective
 * (ncclAllGather = RCCL over xGMI) works on them in place -- no copy through host memory:
 *   parent  int32 [sum_u E_u * n_in_u]          parent indices of the last pass run, unit after unit, [E][n_in] per unit
 *                                               (the layout of tw_results.parent)
 *   gaps    double [sum_u nslot_u * n_in_u]     gap rows of the pass-1 assignment (the layout of tw_get_gaps)
 * Valid until the next tw_load_batch; every entry point returns with the engine's stream synchronised, so the buffers
 * are complete when the caller reads them.  tw_set_gaps_device is tw_set_gaps with a device pointer (the gathered rows
 * of a split service stay in HBM on their way into the refit). */
typedef struct {
    void *parent;
    int64_t parent_count;
    void *gaps;
    int64_t gaps_count;
    int32_t device;
} tw_device_view;
int tw_device_buffers(tw_engine *e, tw_device_view *out);
int tw_set_gaps_device(tw_engine *e, const double *dev_gaps);

/* Mixtures for pass 2 (the fitted sklearn GaussianMixture objects of traceweaver_v3.py:784-786):
 * mix_n[sum_u nslot_u] components per slot (0 = "(0,0)" fallback, traceweaver_v3.py:765-766),
 * mix_p[sum_u nslot_u][TW_MAX_COMP][3] = weight, mean, precision_cholesky. */
int tw_set_mixtures(tw_engine *e, const int32_t *mix_n, const double *mix_p);

/* Device-side alternative to tw_get_gaps + host fit + tw_set_mixtures: the reference's refit of every scored edge
 * (ComputeEpPairDistParams5, traceweaver_v3.py:764-786) on the GPU, from the pass-1 gap samples: for n = 1..min(5, #unique)
 * `GaussianMixture(n, covariance_type="diag").fit` -- k-means++ seeding on the samples in request order, Lloyd, EM (tol 1e-3,
 * <= 100 iterations, reg_covar 1e-6) --, the n of smallest BIC among the fits that did not raise, then the full-covariance
 * refit with `random_state=100`; see traceweaver_amd/csrc/tw_fit.h.  The only randomness are the uniforms the k-means++
 * seeding draws: 1, 3, 7, 10, 13 doubles for n = 1..5, n after n per edge (TW_FIT_ROW_TAPE = 34 for a row with >= 5 distinct
 * samples), independent of the data.
 *
 * tw_fit_mixtures draws them from the engine's own MT19937 (numpy's RandomState algorithm; tw_set_fit_seed reseeds it,
 * tw_create seeds it with 0, tw_load_batch restarts it; one 34-double block per slot and call): the reference's procedure on *a* random stream, as
 * the reference itself runs it unseeded (SURVEY.md hazard H9).  tw_fit_mixtures_seeded gives every unit a stream of its own,
 * MT19937(unit_seed[u]): a unit's fit is then the same whichever units share its batch (services sharded over GPUs).
 * tw_fit_mixtures_tape takes them from the caller: slot q reads tape[slot_off[q] ...], as many doubles as its fits draw
 * (tw_fit_rows tells: max_n[q] = min(5, #unique) of the row, 0 for a row without samples or an unscored slot; the fits of
 * a row draw 1, 4, 11, 21, 34 doubles for max_n = 1..5).  Handing over the doubles numpy's global RNG produces at that point
 * of a seeded reference run makes the refit the one of that run (traceweaver_amd/predictor.py). */
#define TW_FIT_ROW_TAPE 34
int tw_fit_mixtures(tw_engine *e);
int tw_fit_mixtures_seeded(tw_engine *e, const uint32_t *unit_seed);
int tw_set_fit_seed(tw_engine *e, uint32_t seed);
int tw_fit_rows(tw_engine *e, int32_t *max_n);
int tw_fit_mixtures_tape(tw_engine *e, const double *tape, int64_t tape_len, const int64_t *slot_off);

/* The order tables of the last refit (TW_FIT_ORDER, default 1): its launches hand their fits out longest first -- by distinct
 * values x components of the (row, count) a workgroup serves -- through permutations of their grids, built on the host from the
 * rows' distinct-value counts.  order_seed [4 n_slots] and order_em [5 n_slots]: workgroup b of the model selection's seeding /
 * EM launch serves block order[b] = (5 - count) * n_slots + slot; order_row [n_slots]: the rows of the final fits' launches.
 * Live blocks first, by key descending, then count descending, then slot ascending; blocks without a fit last, in index order.
 * Which workgroup makes a fit does not enter the fit: the mixtures are the same bits under TW_FIT_ORDER=0.  *present = 0 (and
 * nothing written): that refit ran in grid order, or the resident mixtures were set with tw_set_mixtures and come from no refit.
 * For tests and measurements. */
int tw_get_fit_order(tw_engine *e, int32_t *order_seed, int32_t *order_em, int32_t *order_row, int32_t *present);

/* The mixture tables currently resident (layout of tw_set_mixtures). */
int tw_get_mixtures(tw_engine *e, int32_t *mix_n, double *mix_p);

/* Pass 2 (iteration 1): same as pass 1 with GaussianMixture.score terms
 * (traceweaver_v1.py:125-126), reusing the windows. */
int tw_run_pass2(tw_engine *e);

/* Results of pass `pass` (1 or 2), host buffers, any pointer may be NULL.  Per-unit arrays are
 * concatenated unit after unit; within a unit [E][n_in] / [TW_TOPK][E][n_in] / [TW_TOPK][n_in].
 *   parent      int32  chosen outgoing-span index per endpoint, -1 = ("NA","NA"), -2 = ("Skip","Skip")
 *   topk_idx    int32  top-5 tuples on *all* spans (top_k_2, traceweaver_v3.py:1185), -1 padded; skip mode: a skip span
 *                      is -(TW_SKIP_BASE + time window * TW_SKIP_STRIDE + position in the window's pool)
 *   topk_score  double their scores (NaN padded)
 *   topk_n      int32  [n_in] number of valid tuples
 *   chosen      int32  [n_in] rank of the chosen tuple in the span's own candidate list, -1 none
 *   leaves      int64  [n_in] enumerated tuples of the top_k call (per_span_candidates increment)
 *   window_end  uint8  [n_in] 1 where a window closes (traceweaver_v3.py:1192)
 *   unit_stats  int64  [n_units][8]: not_best_count, cnt_unassigned, n_windows, windows re-solved
 *                      because an earlier window consumed one of their candidates, windows whose
 *                      exact selection search hit its node budget (incumbent returned), search nodes /
 *                      states of the selection, windows solved by k_select_dp (a level outgrew the small
 *                      tables of k_select_heavy), components it handed on to the depth-first search */
typedef struct {
    int32_t *parent;
    int32_t *topk_idx;
    double *topk_score;
    int32_t *topk_n;
    int32_t *chosen;
    int64_t *leaves;
    uint8_t *window_end;
    int64_t *unit_stats;
} tw_results;
int tw_get_results(tw_engine *e, int pass, const tw_results *r);

/* Pass-1 Gaussian parameters: gauss[sum_u nblk_u * nslot_u][3] = mean, std, log(std_used);
 * NaN for unscored slots.  nblk_u = ceil(n_in_u / batch_size). */
int tw_get_gauss_params(tw_engine *e, double *gauss);

/* Timing of the last pass, measured with HIP events on the engine's stream:
 * ms[0] whole pass, ms[1] candidate-enumeration kernel, ms[2] selection kernel,
 * ms[3] window construction, ms[4] claim/detect/repair kernels, ms[5] parameter kernels (sort + block
 * sums), ms[6] last tw_fit_mixtures call, ms[7] (a count, not a time) rounds of the span-consumption fixed point,
 * ms[8] / ms[9] host wall clock the last pass spent submitting its first enumeration / in the whole call (a pass of a small
 * batch is bound by that, not by the kernels).
 * Appended: the last tw_stitch_traces (HIP events; with truth set the true forest is built first and is not in these figures):
 * ms[10] links to grouped trees on the device (without the copies to the host), ms[11] link table, ms[12] pointer-doubling
 * rounds (incl. the host's one-word read per round), ms[13] rows per root + scan + scatter, ms[14] per-tree order and figures,
 * ms[15] (a count) doubling rounds.
 * The last tw_attribute_traces (HIP events): ms[16] per-tree kernel, ms[17] selection (flags, sort, mark; incl. the host's
 * read of the eligible count), ms[18] group reduction.
 * The last tw_score_traces (HIP events): ms[19] decision kernel, ms[20] row map + per-tree reduction, ms[21] calibration
 * (tw_get_decisions alone writes ms[19]).
 * The last tw_latency_distributions (HIP events): ms[22] cohorts + the two sweeps over the rows (counts, items; incl. the host's
 * read of the item count), ms[23] sort, offsets and values, ms[24] quantiles and histogram (22 and 23: of the call that built
 * the items).  ms[25..30]: tw_trace_signatures and tw_class_profiles (see there).  ms[31]: the kernel of the last tw_order_bound.
 * ms[32] (a count): class stages of the last pass that were queued behind the stage gate (TW_STAGE_GATE), 0 = the pass was not gated.
 * The last tw_compare_cohorts (HIP events): ms[33] ranks, pool and observed statistics, ms[34] the permutation walk (0 without one).
 * ms[35], ms[36] (counts): rows of the last refit whose final fit ran beside the model selection and was adopted (the row selected
 * the largest admissible count, min(5, #distinct)) / rows that were fitted after the selection; both 0 under TW_FIT_SPEC=0.
 * ms[37]: host wall clock the last refit spent building and queueing its order tables (tw_get_fit_order; 0 under TW_FIT_ORDER=0).
 * The history (HIP events): ms[38] plan and ms[39] merge kernel of the last tw_history_push / tw_history_merge, ms[40] quantiles and
 * histogram of the last tw_history_distributions, ms[41], ms[42] observed statistics and permutation walk of the last tw_history_compare.
 * The class catalogue (HIP events): ms[43] hash and lookup, ms[44] scan, append, insert and any rehash, ms[45] accumulate of the
 * last tw_class_history_push / tw_class_history_merge.
 * The last tw_filter_traces (HIP events): ms[46] the tree kernel (rows, clauses, terms, the bit), ms[47] the list of the matched
 * trees (count, scan, write), ms[48] the copies to the host.
 * The last tw_extract_traces (HIP events): ms[49] selection, sizes and offsets, ms[50] the tree kernel; ms[51] the copies of the
 * last tw_get_extracted. */
int tw_get_timing(tw_engine *e, double *ms, int32_t n);

/* ---- neighbours of the hot path on the same device arrays -------------------------------
 *
 * Replaces: FindOrder (executor.py:214-285), the call-order DAG the scorer is given: dag[a*E+b] = 1 iff in every
 * request the true call to endpoint a ended no later than the true call to endpoint b started.  Works on units
 * *before* they are loaded (endpoints in any order, e.g. partition-key order): unit_in_off / unit_E / ep_off /
 * out_start / out_end as in tw_batch, true_child[sum_u E_u * n_in_u] = per unit [E][n_in] index of the true
 * outgoing span of request i at endpoint e in that endpoint's list (< 0 = unknown).  dag_out[sum_u E_u*E_u]. */
int tw_find_order(tw_engine *e, int32_t n_units, const int64_t *unit_in_off, const int32_t *unit_E,
                  const int64_t *ep_off, const int64_t *out_start, const int64_t *out_end,
                  const int32_t *true_child, uint8_t *dag_out);

/* ---- the call-order DAG without ground truth (traceweaver_amd/csrc/tw_order.h, traceweaver_amd/order.py) ----------
 *
 * Replaces: FindConstraintsUsingFit (executor.py:152-212), the reference's answer for a user who has spans but no true
 * assignment: a greedy search over the ordered endpoint pairs (a, b) in partition-key order -- skip the pair if b -> a is in
 * the graph, else add a -> b, run FindAssignments, keep the edge iff cnt_unassigned <= 0 -- at up to E(E-1) full solves per
 * service.  The loop itself lives in traceweaver_amd/order.py (E^2 small decisions per unit; the refit between the passes is
 * the caller's choice, as everywhere); it runs every unit's next candidate in one batch per round.  The three calls below
 * are what makes a round cheap.  One difference to the reference: a pair that would close a cycle longer than two raises
 * in the reference (nx.topological_sort, traceweaver_v1.py:39); here it is rejected and logged as such.
 *
 * tw_order_bound: a necessary condition from the timestamps alone, on host arrays before any load, like tw_find_order
 * (endpoints in partition-key order, every list sorted by (start, end): TW_ERR_ARG otherwise; E > TW_MAX_EP:
 * TW_ERR_UNSUPPORTED).  viol_out[sum_u E_u*E_u], per unit [E][E]: viol[a][b] = the number of requests r for which no pair
 * (x of a, y of b) has both spans contained in r (in_start <= start, end <= in_end) and end_a[x] <= start_b[y], every
 * comparison non-strict; the diagonal is 0.  Such a request has no feasible tuple under any graph with the
 * edge a -> b and is counted in cnt_unassigned (traceweaver_v3.py:1201-1217): viol[a][b] > 0 proves that the reference's
 * test of a -> b fails, and the solve is not needed.  Lightly interleaved requests: viol == 0 is FindOrder's relation; under
 * load it is an upper bound of it.  Integer arithmetic; independent of scheduling.  Timing: tw_get_timing slot 31 (HIP
 * events, ms, the kernel alone).
 *
 * tw_order_stage: uploads the span table of a no-skip batch once, endpoints in partition-key order, into a staging copy the
 * engine owns (b->dag and b->key_rank are not read).  TW_ERR_UNSUPPORTED: a skip-mode batch (tw_batch.skip, or an endpoint
 * whose span count differs from the unit's requests), load-scaled units (unit_time_scale), split services (unit_part),
 * E > TW_MAX_EP.  The copy lives until the next tw_order_stage or tw_destroy; loads do not touch it.
 *
 * tw_order_load: loads the staged units active_units[0..n_active) (ascending indices into the staged batch) under the
 * candidate graphs dag_key (concatenated E*E matrices of the listed units, endpoints in key order, dag[a*E+b] = 1 <=> edge
 * a -> b; need not be transitively closed).  Per unit: the topological order nx.topological_sort gives for nodes inserted in
 * key order and a node's out-edges in ascending key order (the order the search adds them in); the staged endpoint segments
 * gathered into that order on the device; dag and key_rank (= the endpoint's key index) in that order; then tw_load_batch(...,
 * spans_on_device = 1).  Afterwards the engine is in exactly the state tw_load_batch leaves it in, with the listed units as
 * units 0..n_active-1.  TW_ERR_STATE before tw_order_stage; TW_ERR_ARG for a graph with a cycle. */
int tw_order_bound(tw_engine *e, int32_t n_units, const int64_t *unit_in_off, const int32_t *unit_E, const int64_t *ep_off,
                   const int64_t *in_start, const int64_t *in_end, const int64_t *out_start, const int64_t *out_end,
                   int64_t *viol_out);
int tw_order_stage(tw_engine *e, const tw_batch *b);
int tw_order_load(tw_engine *e, int32_t n_active, const int32_t *active_units, const uint8_t *dag_key);

/* Ground truth of the loaded batch for tw_evaluate: true_child in the layout of tw_results.parent;
 * in_trace[n_in_total] (may be NULL) = trace number in [0, n_traces) of every incoming span, for the per-trace
 * (end-to-end) accuracy.  Call after tw_load_batch. */
int tw_set_truth(tw_engine *e, const int32_t *true_child, const int32_t *in_trace, int64_t n_traces);

/* Replaces: repeat_change_spans (helpers/transforms.py:10-40) -- the load scaling `--compress_factor N` applies to every
 * service before the predictor runs (executor.py:1086-1097,1146-1148) -- on the RESIDENT span table, so that the load levels
 * of one corpus (exps/exp5/run_experiment.sh:60-156 runs six per call graph) share one upload.  Needs an integer-microsecond
 * batch (no unit_time_scale, no skip mode) and tw_set_truth (the requests' own calls pair the spans of a request as the
 * reference's sort by trace id does, helpers/transforms.py:25-29; every endpoint must hold exactly one call per request,
 * otherwise TW_ERR_ARG -- the reference asserts).  Per request with load factor f = unit_factor[u] >= 1 (executor.py:1089-1091):
 * x = in.start / f in binary64, out.start = x + (out.start - in.start), durations kept; every list is re-sorted by
 * (start, end), ties in the order of trace_rank[n_in_total] (rank of the request's trace id inside its unit; NULL = current
 * order); truth and trace numbers follow the spans.  The scaled binary64 timestamps are kept exactly, as int64 multiples of
 * unit_time_scale[u] = 2^-k (written if not NULL; semantics of tw_batch.unit_time_scale).  in_perm[n_in_total] /
 * out_perm[n_out_total] (may be NULL) = list-local old index of every new position.  Always scales the table as uploaded
 * (calls do not compound); afterwards the engine is in the state tw_load_batch leaves it in. */
int tw_scale_load(tw_engine *e, const int32_t *unit_factor, const int32_t *trace_rank, int32_t *in_perm, int32_t *out_perm,
                  double *unit_time_scale);

/* The reference's baseline predictors on the resident table (executor.py:888-900 indices 3, 4, 7 -- what
 * exps/exp1 and exps/exp5 run next to predictor 10), see traceweaver_amd/csrc/tw_baselines.h.  parent_out in the layout of
 * tw_results.parent.  No-skip batches only (the lists of a skip-mode batch are not sorted: TW_ERR_UNSUPPORTED).
 *   tw_run_baseline(TW_BASELINE_FCFS)   algorithms/fcfs.py:10-26: request i takes the i-th call of every endpoint.
 *   tw_run_baseline(TW_BASELINE_VPATH)  algorithms/vpath.py:48-89; needs tw_set_truth (a returning call is followed to the request
 *                                        it truly belongs to, as the reference does through the trace id).
 *   WAP5 (algorithms/wap5.py:257-351) in two steps, because its delay samples accumulate per callee *name* over the services of
 *   a run (the class keeps them; the names live on the host): tw_wap5_delays returns per (unit, endpoint) -- [n_units][TW_MAX_EP] --
 *   the sum (in the unit's timestamp units) and the number of the delay samples of BuildDistributions (:257-275) and the longest
 *   request per unit; the caller adds them up per name in service order, takes the means (statistics.mean: exact) and hands them,
 *   in microseconds, to tw_wap5_parents, which runs ScoreParents (:282-316).  -2 = several calls were given to the request:
 *   the reference's accuracy counts that as wrong (helpers/utils.py:68-73).  call_request (may be NULL; layout of out_start):
 *   the request every call was given to, -1 = none -- the reference's list-valued assignment is its inverse. */
#define TW_BASELINE_FCFS 4
#define TW_BASELINE_VPATH 7
int tw_run_baseline(tw_engine *e, int kind, int32_t *parent_out);
int tw_wap5_delays(tw_engine *e, int64_t *delay_sum, int32_t *delay_cnt, int64_t *unit_maxdur);
int tw_wap5_parents(tw_engine *e, const double *mean, int32_t *parent_out, int32_t *call_request);

/* Replaces: AccuracyForService / TopKAccuracyForService (helpers/utils.py:62-97) and AccuracyEndToEnd /
 * TopKAccuracyEndToEnd (helpers/utils.py:99-145) as reductions over the resident results of the last pass run.
 * per_unit[n_units][4] = requests, requests with every endpoint right, requests whose top-5 list holds the true
 * tuple, requests left unassigned.  trace_flags (may be NULL; needs in_trace): [2][n_traces] uint8, 1 = some span of
 * the trace is wrong (exact / top-5) -- combine across ranks with a MAX all-reduce; e2e[2] (may be NULL) = traces
 * right under the exact / the top-5 criterion on this engine alone. */
int tw_evaluate(tw_engine *e, int64_t *per_unit, uint8_t *trace_flags, int64_t *e2e);

/* ---- from parent arrays to traces (traceweaver_amd/csrc/tw_stitch.h) ---------------------------------------------
 *
 * Replaces: ConstructEndToEndTraces (helpers/utils.py:216-252), which files every predicted span under the TRUE trace id
 * of its request, and the join across services a caller without ground truth otherwise writes on top of the per-service
 * parent arrays.  A trace is made of two kinds of hop over the rows of the span table (tw_corpus_span_table):
 *   server row -> client row of the same RPC   observed: row_link (the table's `parent` column)
 *   client row -> the request that made it     predicted: parent[e][i] = x  =>  link[out_row(e, x)] = in_row(i)
 * The union is a forest; its trees are the reconstructed traces.  A client row that no unit of the batch covers, a call no
 * request took and a skip span are holes, and a hole stays a hole: the rows below it form a tree of their own (a fragment).
 * Ground truth is never used to fill one.
 *
 * tw_set_span_rows hands over, after tw_load_batch: in_row / out_row = span-table row of every incoming / outgoing span of
 * the loaded batch (layouts of in_start / out_start; tw_unit_set has them) and the table itself: n_rows rows with
 *   row_link  >= 0: for a server row the client row of the same RPC; for a client row it is not read (it may hold the true
 *             parent).  -1: the row is a root of the table.  -2: the observed caller is not in the table (a server row whose
 *             client side was deleted): no link, and not a whole trace either
 *   row_kind  1 server, 2 client, 0 absent (a row that takes part in nothing: a tree of its own)
 *   row_start / row_end  microseconds.
 * Checked on the host: ranges, in_row names distinct server rows, out_row distinct client rows, a server row links to a
 * client row, no row links to itself (TW_ERR_ARG).  tw_load_batch and tw_scale_load drop the maps (after load scaling the
 * caller permutes in_row / out_row with the permutations tw_scale_load returns and sets them again).
 *
 * tw_stitch_traces stitches the assignment of pass `pass` (1 or 2; it must be the resident one, as for tw_get_results) or,
 * with use_truth != 0, the true assignment of tw_set_truth (`pass` is not read): the comparison object, not a fallback.
 * Caller-allocated outputs, any may be NULL; trees are numbered in ascending order of their root row:
 *   root, depth    [n_rows]  root row of the row's tree, links between the row and that root
 *   tree_off       [n_rows + 1] capacity, n_trees + 1 entries written: tree k owns tree_rows[tree_off[k] .. tree_off[k + 1])
 *   tree_rows      [n_rows]  rows grouped by tree, ordered by (start, row) inside a tree
 *   tree_root, tree_latency, tree_flags   [n_rows] capacity, n_trees entries written: root row; latest end of the tree's
 *                  rows less the start of its root; bit 0 the root is a root of the table (a whole trace -- every other tree
 *                  is a fragment), bit 1 some request of the tree has an endpoint left unassigned (parent -1; -2, a skip
 *                  span, is an answer), bit 2 (only after tw_set_truth) the tree is whole and its row set is that of the
 *                  tree the true assignment gives
 * counts4 (may be NULL) = whole traces, fragments, trees with an unassigned endpoint, trees with bit 2 (-1 without truth).
 * Only the selected assignment is stitched (not the top-5 alternatives), and one engine's batch: a sharded run gathers the
 * parent arrays first (traceweaver_amd/sharding.py) and stitches on one rank.
 * pass 0 = an assignment handed over with tw_set_parents (layout of tw_results.parent; checked on the host: indices inside
 * the endpoint's list, no call given to two requests): parent arrays that were not produced by this engine's last pass --
 * services solved one after the other, or gathered from the ranks of a sharded run.  Dropped like the row maps.
 * TW_ERR_STATE: before tw_set_span_rows, before the pass named, use_truth without tw_set_truth.  TW_ERR_ARG: the links
 * hold a cycle -- impossible for a table that passes the checks above with valid parent arrays; a malformed one ends
 * here (pointer doubling is capped at 32 rounds), never in a hang.  Timing: tw_get_timing slots 10..15. */
int tw_set_parents(tw_engine *e, const int32_t *parent);
int tw_set_span_rows(tw_engine *e, int64_t n_rows, const int32_t *in_row, const int32_t *out_row, const int32_t *row_link,
                     const uint8_t *row_kind, const int64_t *row_start, const int64_t *row_end);
typedef struct {
    int32_t *root;
    int32_t *depth;
    int64_t *tree_off;
    int32_t *tree_rows;
    int32_t *tree_root;
    int64_t *tree_latency;
    uint8_t *tree_flags;
} tw_stitched;
int tw_stitch_traces(tw_engine *e, int pass, int use_truth, const tw_stitched *out, int64_t *n_trees, int64_t *counts4);

/* ---- latency attribution on the stitched forest (csrc/tw_attr.h) ----------------------------------------------
 *
 * Replaces: the consumer of reconstructed traces, src/query_engine/delay_culprit.py:19-28 -- "FOR all end to end requests
 * WHICH were in the top X %ile response latency bracket AND were initiated after time Y, FIND the worst performing service
 * AND its mean service latency for these requests" -- and its walk over every trace on the host, delay_culprit.py:30-97.
 * Both calls work on the forest of the last tw_stitch_traces call (a pass, pass 0 or the truth), which stays on the device.
 *
 * Definitions (integer microseconds; a row with end < start counts as end = start; the children of row p are the rows c
 * with link[c] == p):
 *   self_time[p]   (end_p - start_p) less the measure of the union of the children's intervals clipped to [start_p, end_p]
 *   path_time[p]   p's share of the critical path of its tree.  walk(p, lo, hi), [lo, hi] inside p's interval, the root walked
 *                  with its own: cursor = hi; among the children with cs = max(start_c, lo) < cursor and end_c > cs the one
 *                  with the greatest ce = min(end_c, cursor) is taken (ties: the smaller cs, then the smaller row);
 *                  path_time[p] += cursor - ce; walk(c, cs, ce); cursor = cs; again.  No such child: path_time[p] +=
 *                  cursor - lo.  Rows never walked have 0, so the path times of a tree sum to its root's duration.
 *   groups         row_group [n_rows] in [0, n_groups), -1 = not counted (normally the span table's interned service).
 *                  tree_top_group = the group with the largest summed path_time among those with a row on the tree's path
 *                  (ties: the smallest id), -1 if there is none.
 *   selection      eligible = trees whose flags hold every bit of need_flags and none of skip_flags (the reference keeps whole
 *                  traces without an unassigned call: need 1, skip 2).  Ordered by (tree_latency, tree), k = (int64)
 *                  (percentile * n_eligible) in binary64 as int(0.95 * len(...)) gives it; the trees of rank >= k whose root
 *                  starts in [start_min, start_max) are selected: the percentile first, the window second, as in the reference.
 *   per group, over the selected trees: path_time, path_rows (rows on a path), self_time, span_time, span_rows (duration and
 *                  count of all the group's rows: span_time / span_rows is the mean service latency), trees (selected trees
 *                  with a row of the group on the path), top_trees (selected trees whose tree_top_group the group is)
 *   summary6       eligible trees, selected trees, k, the latency at rank k (0 without eligible trees), the culprit = the
 *                  group with the largest path_time among those with path_rows > 0 (ties: the smallest id; -1: none), trees
 *
 * tw_set_row_groups: after tw_set_span_rows; ranges are checked on the host; dropped whenever the row maps are dropped.
 * tw_attribute_traces: outputs are caller-allocated, any may be NULL: link, self_time, path_time [n_rows]; tree_* [n_trees of
 * the stitch]; group_* [n_groups].  TW_ERR_STATE: before a stitch, before tw_set_row_groups, after anything that drops the
 * stitched forest (tw_load_batch, tw_scale_load, tw_set_span_rows, tw_run_pass1 / 2).  TW_ERR_ARG: percentile outside [0, 1),
 * start_min > start_max, links that leave their tree (never after a stitch that returned TW_OK).  Covers the selected
 * assignment only and one engine's batch.  Everything is integer arithmetic; the atomics are 64-bit integer adds of which only
 * the sum is read: results do not depend on scheduling.  Timing: tw_get_timing slots 16..18 (per-tree kernel, selection,
 * group reduction; HIP events, ms). */
typedef struct {
    double percentile;
    int64_t start_min, start_max;
    uint32_t need_flags, skip_flags;
} tw_attr_query;
typedef struct {
    int32_t *link;
    int64_t *self_time, *path_time;
    int32_t *tree_top_group;
    uint8_t *tree_selected;
    int32_t *tree_path_rows;
    int64_t *group_path_time, *group_path_rows, *group_self_time, *group_span_time, *group_span_rows, *group_trees, *group_top_trees;
} tw_attribution;
int tw_set_row_groups(tw_engine *e, int32_t n_groups, const int32_t *row_group);
int tw_attribute_traces(tw_engine *e, const tw_attr_query *q, const tw_attribution *out, int64_t *summary6);

/* ---- which of the reconstructed traces can be trusted (csrc/tw_conf.h) -------------------------------------------
 *
 * Replaces: the reference's one figure of trust, not_best_count / num_spans per service -- the requests whose selected tuple
 * is not their own best-scoring one (traceweaver_v3.py:1201-1207), written to confidence_scores_*.pickle (executor.py:
 * 1203-1205,1241) and plotted as 1 - not_best / n against accuracy (utils/plot_accuracy_vs_confidence_multiple_cgs.py:76-84).
 * tw_results.unit_stats[0] is that scalar; here the facts behind it leave the device per request and per stitched trace.
 *
 * Decision of request g (one per incoming span of the loaded batch, of the resident pass).  L = the candidate list the
 * selection chose from, the one chosen[g] indexes: the list enumerated again on the remaining spans where the engine did
 * so, else the first (tw_results.topk_* is always the first).  n = |L|, s[0..n) its scores in list order, c = chosen[g]:
 *   rank      c (-1: none was selected)
 *   list_n    n
 *   margin    binary64, one subtraction: c < 0: NaN.  c == 0: s[0] - s[1], +inf when n == 1.  c > 0: s[c] - s[0].
 *             A NaN that the subtraction itself gives (inf - inf) stays NaN; every NaN is stored as 0x7ff8000000000000.
 *   not_best  c != 0: what unit_stats[0] counts.
 * Per tree k of the stitched forest, over its decisions = the requests g with in_row[g] in the tree:
 *   decisions, not_best, unassigned (c < 0)   int32 counts
 *   min_margin   the minimum over the decisions whose margin is not NaN, in the order -inf < .. < -0 < +0 < .. < +inf;
 *                +inf if there is none
 *   weakest_row  in_row of a decision that attains min_margin (the same bits), the smallest row on ties; -1 if there is none
 *   confident    decisions > 0 && not_best == 0 && min_margin >= threshold
 * TW_TREE_CONFIDENT: after tw_score_traces the forest kept on the device for tw_attribute_traces carries this bit in the
 * flags of its confident trees (need_flags = 1 | 8: whole and confident).  Every tw_score_traces call clears and rewrites
 * it; before the first one it is never set, and the tree_flags tw_stitch_traces returns never show it.
 * Calibration: ascending edges[0..n_edges), n_edges <= 15.  bucket(tree) = 0 if not_best > 0, else 1 + #{j: min_margin >=
 * edges[j]}: n_edges + 2 buckets.  calib[n_edges + 2][3], counted over the whole trees (flag bit 0) with decisions > 0:
 * trees, trees with flag bit 2 (exact; -1 in every row without tw_set_truth), decisions.
 * summary5 = scored trees (decisions > 0), confident trees, decisions, not_best, unassigned (all trees).
 *
 * tw_get_decisions: `pass` (1 or 2) must be the resident one (TW_ERR_STATE otherwise, as for tw_get_results); needs no
 * stitch.  Outputs [requests of the batch] in the layout of in_start, any may be NULL.
 * tw_score_traces: works on the forest of the last tw_stitch_traces(pass = 1 | 2).  Outputs are caller-allocated, any may be
 * NULL: rank, list_n, margin [requests]; row_request [n_rows] (the request whose incoming span the row is, -1 none); tree_*
 * [n_trees of the stitch]; calib [(n_edges + 2) * 3].  TW_ERR_STATE: before a stitch, after anything that drops the stitched
 * forest (see tw_attribute_traces), for a forest stitched from tw_set_parents (pass 0) or from the truth -- they hold no
 * decisions --, when the stitched pass is no longer resident.  TW_ERR_ARG: n_edges outside [0, 15], edges that are NaN or
 * not strictly ascending.
 * Covers the selected assignment only and one engine's batch.  Results do not depend on scheduling: the one floating-point
 * operation is the subtraction that defines a margin, minima are taken on integer keys, the atomic adds are integer adds
 * of which only the sum is read.  Timing: tw_get_timing slots 19..21 (decision kernel, row map + tree reduction,
 * calibration; HIP events, ms). */
#define TW_TREE_CONFIDENT 8
typedef struct {
    double threshold;
    int32_t n_edges;
    const double *edges;
} tw_conf_query;
typedef struct {
    int32_t *rank, *list_n;
    double *margin;
    int32_t *row_request;
    int32_t *tree_decisions, *tree_not_best, *tree_unassigned;
    double *tree_min_margin;
    int32_t *tree_weakest_row;
    uint8_t *tree_confident;
    int64_t *calib;
} tw_confidence;
int tw_get_decisions(tw_engine *e, int pass, int32_t *rank, int32_t *list_n, double *margin);
int tw_score_traces(tw_engine *e, const tw_conf_query *q, const tw_confidence *out, int64_t *summary5);

/* ---- per-service latency distributions and cohorts (csrc/tw_dist.h) -----------------------------------------------
 *
 * Replaces: what the delay-culprit query writes, src/query_engine/delay_culprit.py:80-97 -- per service not a mean but the
 * list of the span latencies (duration_mus) of the selected requests, once for the true and once for the predicted traces,
 * compared afterwards as distributions.  tw_attribute_traces gives seven totals per group; here the populations behind them
 * leave the device sorted, with quantiles and a histogram, and split by cohort (requests served by version A or B of one
 * service, say).  Both entry points work on what the last tw_attribute_traces call left on the device: its selection
 * (tree_selected), its per-row times and the forest it ran on, whether of a pass, of pass 0 or of the truth.
 *
 * Definitions (integer microseconds throughout; a row with end < start counts as end = start, as in the attribution):
 *   cohort     row_cohort [n_rows] in [-1, n_cohorts), -1 = the row says nothing.  tree_cohort[t] = the smallest label >= 0
 *              among the tree's rows, -1 if there is none.  Without tw_set_row_cohorts, or after n_cohorts = 1 with
 *              row_cohort = NULL, every tree has cohort 0.  A tree of cohort -1 is counted in no segment.
 *   items      over the selected trees of cohort c >= 0:
 *                metric 0  span latency   every row with row_group = g >= 0              its duration
 *                metric 1  self time      the same rows                                  self_time
 *                metric 2  path time      those of them on the critical path             path_time
 *                metric 3  trace latency  one item per tree, no group                    tree_latency
 *              Metric 0 is the reference's duration_mus lists.
 *   segments   (c, m, g) for m < 3 and (c, 3): n_seg = n_cohorts * (3 * n_groups + 1), index c * (3 G + 1) + m * G + g, the
 *              trace-latency segment last within a cohort.
 *   outputs    caller-allocated, any may be NULL: tree_cohort [n_trees of the stitch]; seg_count, seg_sum [n_seg]; seg_off
 *              [n_seg + 1] and values [n_items]: segment s owns values[seg_off[s] .. seg_off[s + 1]), ascending in signed
 *              order (ties are equal integers: the array is fully determined); n_items = summary4[0], and a call with
 *              values == NULL returns it, so that the caller can size the array (the sorted items stay on the device until
 *              the next tw_attribute_traces / tw_set_row_cohorts: a second call only gathers and copies).
 *              quantile [n_seg][n_q]: for probs[j] in [0, 1] the value at index min(n - 1, (int64)(probs[j] * (double)n))
 *              of the segment of n items -- the product in binary64, the convention of k = (int64)(percentile * n_eligible)
 *              --, INT64_MIN for an empty segment; n_q <= 32.
 *              hist [n_seg][n_edges + 1]: strictly ascending int64 edges, n_edges <= 63; bin of v = #{j: v >= edges[j]},
 *              the convention of the calibration table.
 *   summary4   items, non-empty segments, selected trees counted (cohort >= 0), selected trees left out (cohort -1)
 *
 * tw_set_row_cohorts: optional; after tw_set_span_rows (TW_ERR_STATE before); ranges are checked on the host (TW_ERR_ARG:
 * n_cohorts < 1, a label outside [-1, n_cohorts), NULL with n_cohorts != 1); dropped with the row maps, like the row groups.
 * tw_latency_distributions: TW_ERR_STATE before a tw_attribute_traces on the current forest (a new tw_stitch_traces, new row
 * groups and everything that drops the forest drop the attribution).  TW_ERR_ARG: a prob that is NaN or outside [0, 1],
 * edges not strictly ascending, n_q outside [0, 32], n_edges outside [0, 63].  TW_ERR_UNSUPPORTED: n_seg > 2^24.
 * No floating point on the device but the one product probs[j] * n (a single binary64 multiplication, built with
 * -ffp-contract=off), equal to the restatement bit for bit.  The atomics are integer adds and minima of which only the
 * result is read; the cursor that hands out item positions decides where an item lies before the sort, never what the
 * output holds: results do not depend on scheduling.  Covers one engine's batch.  Timing: tw_get_timing slots 22..24 (items
 * and counts; sort, offsets and values; quantiles and histogram; HIP events, ms; 22 and 23 are those of the call that
 * built the items). */
typedef struct {
    int32_t n_q;
    const double *probs;
    int32_t n_edges;
    const int64_t *edges;
} tw_dist_query;
typedef struct {
    int32_t *tree_cohort;
    int64_t *seg_count, *seg_sum, *seg_off, *values, *quantile, *hist;
} tw_distributions;
int tw_set_row_cohorts(tw_engine *e, int32_t n_cohorts, const int32_t *row_cohort);
int tw_latency_distributions(tw_engine *e, const tw_dist_query *q, const tw_distributions *out, int64_t *summary4);

/* ---- two cohorts compared: KS, rank sum, quantile shifts, permutation test (csrc/tw_cmp.h) --------------------------
 *
 * Replaces: the reading of the two latency lists the delay-culprit query writes (src/query_engine/delay_culprit.py:80-97),
 * for the case the cohorts exist for: requests served by version a against those served by version b of one service.  It
 * answers "is b slower than a, where, and could that be noise" on the device, from what tw_latency_distributions works on:
 * the last attribution, the cohort labels as they are and the sorted items (built here if they are not resident).  The call
 * drops nothing and keeps no result: tw_latency_distributions answers after it what it answered before.
 *
 * Definitions (integers throughout; latencies are assumed below 2^62 in magnitude):
 *   rows       pairs [n_pairs][2] = (a, b), a != b, both in [0, n_cohorts), 1 <= n_pairs <= 64.  Row pair * (3 G + 1) + r, r =
 *              m * G + g the (metric, group) position inside a cohort (the trace latency last), compares A = the sorted values
 *              of segment (a, r) with B = those of (b, r); n_a, n_b their sizes, N = n_a + n_b, M the N pooled values ascending
 *              (only values matter: M is fully determined).
 *   observed   Where either side is empty: ks_gap = u2 = 0, ks_at = INT64_MIN, every shift 0, every perm_* -1.  Else
 *              ks_gap, ks_at   over the distinct x of M, g(x) = #{A <= x} n_b - #{B <= x} n_a; ks_gap = g at the smallest x
 *                              where |g| is greatest (signed: positive = A's CDF lies above B's there), ks_at that x.  The
 *                              two-sample KS statistic is |ks_gap| / (n_a n_b).
 *              u2              2 #{(i, j): A_i < B_j} + #{(i, j): A_i = B_j}: twice the Mann-Whitney U of B over A;
 *                              u2 / (2 n_a n_b) is the probability that a value of B exceeds one of A (ties count half).
 *              quantile_shift  [n_q], n_q <= 8: Q_B(p_j) - Q_A(p_j), Q(p) the value at index min(n - 1, (int64)(p * (double)n))
 *                              (the index of tw_latency_distributions: one binary64 product, -ffp-contract=off).
 *   permuted   n_perm <= 65536 permutations p of every row with both sides non-empty and (max_pool = 0 or N <= max_pool).
 *              Permutation p hands n_a of the N pooled values to A' by selection sampling along M: with c = items given so
 *              far, item k goes to A' iff (h_k * (N - k)) >> 64 < n_a - c (a 128-bit product), h_k = mix(key + GOLD * (k + 1)),
 *              key = mix(mix(seed + GOLD * (row + 1)) + GOLD * (p + 1)), GOLD = 0x9E3779B97F4A7C15, mix = the finaliser of
 *              splitmix64 (x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31), all
 *              mod 2^64.  Its statistics are the ones above on (A', B'): the gap at the end of every run of equal values, u2
 *              per run as rb * (2 * cA_before_run + ra).  perm_ge_ks = #{p: |gap_p| >= |ks_gap|}, perm_ge_u = #{p: |u2_p - n_a
 *              n_b| >= |u2 - n_a n_b|}, perm_ge_q [n_q] = #{p: |shift_p,j| >= |quantile_shift_j|} (magnitudes as unsigned 64
 *              bit).  A p-value is (1 + ge) / (1 + n_perm), left to the caller.  Rows not permuted hold -1 in all three; with
 *              n_perm = 0 the three arrays are not written.  The draws of different rows are independent.
 *   outputs    caller-allocated, any may be NULL; [n_rows = n_pairs * (3 G + 1)], quantile_shift and perm_ge_q [n_rows][n_q].
 *   summary4   rows with both sides non-empty, rows permuted, pooled items permuted (the sum of N over those rows), n_perm
 *
 * TW_ERR_STATE before a tw_attribute_traces on the current forest.  TW_ERR_ARG: n_pairs outside [1, 64], a label outside
 * [0, n_cohorts) (so every pair while there is one cohort), a = b, n_q outside [0, 8], a prob that is NaN or outside [0, 1],
 * n_perm outside [0, 65536], max_pool < 0.  TW_ERR_UNSUPPORTED: some n_a n_b >= 2^61 or N >= 2^32 (and n_seg > 2^24, as above).
 * All refused on the host.  The atomics are integer adds, maxima and minima of which only the result is read: results do not
 * depend on scheduling.  Limits: one engine's batch; cohort against cohort (predicted against true are two resident states:
 * traces.compare_distributions on the host); the walk of one permutation is sequential in N, so the largest row bounds the
 * call and max_pool is the handle on that.  Timing: tw_get_timing slots 33, 34 (observed statistics; permutation walk). */
#define TW_CMP_MAX_Q 8
typedef struct {
    int32_t n_pairs;
    const int32_t *pairs;
    int32_t n_q;
    const double *probs;
    int32_t n_perm;
    uint64_t seed;
    int64_t max_pool;
} tw_cmp_query;
typedef struct {
    int64_t *n_a, *n_b, *ks_gap, *ks_at, *u2;
    int64_t *quantile_shift;
    int64_t *perm_ge_ks, *perm_ge_u, *perm_ge_q;
} tw_cohort_comparison;
int tw_compare_cohorts(tw_engine *e, const tw_cmp_query *q, const tw_cohort_comparison *out, int64_t *summary4);

/* ---- the distributions of batch after batch: a history on the device (csrc/tw_hist.h) -----------------------------
 *
 * Replaces: the pickle of latency lists the delay-culprit query writes per run and the reading of two runs' files side by
 * side, src/query_engine/delay_culprit.py:32-97 -- yesterday's deployment against today's, a p99 over an hour of batches.
 * tw_latency_distributions and tw_compare_cohorts cover one engine's batch; the history keeps what they work on -- every
 * segment's values ascending, its count and its sum -- beyond the batch, for cohorts of its own, and answers the same two
 * queries over it.  It is device state of the engine and holds copies: tw_load_batch, tw_set_span_rows, tw_stitch_traces,
 * tw_attribute_traces, tw_set_row_groups, tw_set_row_cohorts, a new pass and whatever else drops the forest leave it alone, and
 * none of the calls below drops or rewrites anything of the resident batch.  Only tw_history_reset and tw_destroy end it.
 *
 * Definitions:
 *   history    C_h cohorts x per = 3 G + 1 segments, index h * per + m * G + g, the trace-latency segment last within a cohort
 *              (the layout of tw_latency_distributions).  H[h, r]: the values ascending in signed order; seg_count; seg_sum in
 *              two's complement, wrapping.  Empty after tw_create and tw_history_reset: C_h = 0 and G open.  The first push or
 *              merge fixes G = n_groups; a later one with another n_groups is TW_ERR_ARG.
 *   push       the source is the sorted items of the last tw_attribute_traces, exactly those tw_latency_distributions defines
 *              (built here when they are not resident, as tw_compare_cohorts does, and left resident).  cohort_map [n_map],
 *              n_map = the batch's n_cohorts: source cohort c goes to history cohort cohort_map[c] >= 0, -1 = not kept, NULL =
 *              the identity.  The entries >= 0 must be distinct: a push merges two sorted runs per segment, never more.
 *              Afterwards C_h = max(C_h, 1 + max cohort_map); cohorts nobody was pushed into hold empty segments.  For every c
 *              with h = cohort_map[c] >= 0 and every r < per the new H[h, r] is the ascending multiset union of the old H[h, r]
 *              and the source's segment (c, r); counts and sums are added.  Every other segment is unchanged.
 *   merge      the same from host arrays -- a saved history, another rank's, another engine's tw_latency_distributions output:
 *              n_cohorts_src x (3 n_groups + 1) segments, seg_off_src [n_seg + 1] (first 0, non-decreasing: checked on the host),
 *              values_src [seg_off_src[n_seg]], every segment ascending (checked on the device before anything is merged).
 *              Counts are the differences of the offsets, sums are taken on the device.
 *   summary4   push, merge: items added, items held afterwards, C_h afterwards, pushes and merges since the reset.
 *              tw_history_distributions: items held, non-empty segments, C_h, pushes and merges since the reset.
 *              tw_history_compare: as tw_compare_cohorts.
 *   info       out6 = C_h, G, segments (C_h * per), items held, pushes and merges since the reset, capacity of the value buffer
 *              in items.  All 0 for an empty history (tw_history_reset frees the buffers).
 *
 * tw_history_distributions: the outputs, conventions and argument checks of tw_latency_distributions over the history's
 * segments (n_seg = C_h * per, n_items = items held; out->tree_cohort is ignored); with n_q = n_edges = 0 it is the call that
 * reads the history back.  tw_history_compare: the definitions, limits and argument checks of tw_compare_cohorts over the
 * history's segments, pairs in [0, C_h): batch against batch.  Both run the kernels of their namesakes on a view of the history.
 *
 * TW_ERR_STATE: tw_history_push before a tw_attribute_traces on the current forest; the two queries on an empty history.
 * TW_ERR_ARG: n_map != the batch's n_cohorts; a map entry below -1; two equal entries >= 0; another n_groups than the history's;
 * n_cohorts_src < 1, n_groups < 1; offsets that do not start at 0 or decrease; a source segment that does not ascend; the
 * argument errors of the namesakes.  TW_ERR_UNSUPPORTED: C_h * per (or the source's segments) > 2^24.  TW_ERR_DEVICE: no memory
 * for a buffer.  A call that is refused or fails leaves the history exactly as it was: a push merges into the value buffer that
 * is not in use (two at most; a buffer grows to at least twice its size) and the two are swapped when nothing has failed.
 * Everything runs on the engine's stream; integers throughout but the one product probs[j] * n of the quantile index; the only
 * atomics are the integer adds of the merge's source sums: results do not depend on scheduling.
 * Limits: every push rewrites the whole store (16 B per item held afterwards); no tiers, no eviction, no decay; ranks merge
 * through the host (tw_history_merge), there is no collective.  Timing: tw_get_timing slots 38..42 (HIP events, ms): 38 plan
 * (for a merge with the source's check; the host's read of the plan's counters and the growth of a buffer, where there is one, fall
 * between its events), 39 merge kernel -- of the last push or merge; 40 quantiles and histogram of the last
 * tw_history_distributions; 41, 42 observed statistics and permutation walk of the last tw_history_compare. */
int tw_history_reset(tw_engine *e);
int tw_history_push(tw_engine *e, int32_t n_map, const int32_t *cohort_map, int64_t *summary4);
int tw_history_merge(tw_engine *e, int32_t n_cohorts_src, int32_t n_groups, const int64_t *seg_off_src, const int64_t *values_src,
                     const int32_t *cohort_map, int64_t *summary4);
int tw_history_info(tw_engine *e, int64_t *out6);
int tw_history_distributions(tw_engine *e, const tw_dist_query *q, const tw_distributions *out, int64_t *summary4);
int tw_history_compare(tw_engine *e, const tw_cmp_query *q, const tw_cohort_comparison *out, int64_t *summary4);

/* ---- traces grouped by call-graph signature (csrc/tw_sig.h) -------------------------------------------------------
 *
 * Replaces: AssignCGSignature and FindUniqueCGs (alibaba-analysis/analysis.py:99-126, 214-221) -- per trace and depth the
 * sorted list of the services seen there, and the traces grouped by it; PreparePerCGData (:233-292) then works on one group
 * at a time.  The four sections above treat a trace as a bag of rows with times; this one says what it looks like: which
 * call graphs occur, how often, how slow each is, and whether a reconstructed trace has the call graph its request had.
 * It works on the forest of the last tw_stitch_traces (of a pass, of pass 0 or of the truth) and on row_group / n_groups of
 * tw_set_row_groups.  Everything is integer.
 *
 * Definitions:
 *   level[r]    for a server row (row_kind 1) the number of server rows strictly above it on the way to its tree's root; -1
 *               for every other row.  Server rows link to client rows and client rows to the request's server row, so this
 *               equals depth[r] >> 1.  A fragment rooted at a client row has its server child at level 0.
 *   items       of a tree: its server rows with row_group[r] = g >= 0.  Rows of group -1 are no items, but they count as
 *               ancestors (they are levels, and the cg of their children is -1).
 *   item key    mode 0 ("levels", the reference's signature): (level, 0, g).  Mode 1 ("edges"): (level, cg, g), cg = the
 *               row_group of the nearest server ancestor, -1 if there is none or its group is -1: per level the multiset of
 *               caller -> callee edges, which separates traces that mode 0 merges.
 *   signature   of a tree: its items sorted by key and run-length encoded, a sequence of entries (level, cg, g, count);
 *               fully determined; empty for a tree without items.  Two signatures are equal iff the sequences are equal
 *               entry by entry.  The device decides this exactly: a 64-bit hash of the sequence orders and buckets the
 *               trees, equality is then decided by comparing the entries, never by the hash.
 *   eligible    flags hold every bit of need_flags and none of skip_flags (TW_TREE_CONFIDENT as in the attribution).
 *   classes     rep[t] = the smallest eligible tree index with a signature equal to t's; classes are numbered in ascending
 *               order of their rep: the numbering depends on nothing but the forest and the groups.  tree_class[t] = the
 *               class, -1 for a tree that is not eligible.  tree_items[t] = the number of items, of every tree.
 *   per class   class_rep, class_trees, class_latency_sum / _min / _max over tree_latency, and the signature itself:
 *               class c owns the entries class_off[c] .. class_off[c + 1) of class_entries, four int32 each (level, cg, g,
 *               count).
 *   reference   keep_reference != 0 stores the signatures of this call's eligible trees on the device, keyed by the root
 *               row of their tree.  The set survives a new tw_stitch_traces; it is dropped with the row maps (tw_load_batch,
 *               tw_scale_load, tw_set_span_rows) and with new row groups.
 *   comparison  compare != 0 writes tree_same[t]: 1 if the reference set holds a tree with the same root row and an equal
 *               signature, 0 if it holds one with a different signature, 255 if it holds none or t is not eligible (255
 *               everywhere without compare).  A call with both compares with the set it then replaces.
 *   summary6    eligible trees, classes, items of the eligible trees, entries of all class signatures, compared trees
 *               (tree_same < 255), same trees; the last two are -1 without compare.
 * Against the reference: it also puts the root's `caller` into level 0 (the caller of a root is not in the span table),
 * joins the names into one string before hashing (which can merge distinct multisets) and uses Python's hash, salted per
 * process (analysis.py:111-125).  The classes here are those of the multisets: the reference's apart from these three points.
 *
 * Outputs are caller-allocated, any may be NULL: row_level [n_rows]; tree_class, tree_items, tree_same [n_trees of the
 * stitch]; class_rep, class_trees, class_latency_* with room for n_trees, class_off for n_trees + 1; class_entries [4 *
 * summary6[3]]: a call with class_entries == NULL returns the sizes, the result stays on the device until the forest, the
 * groups, the flags (tw_score_traces) or the query change, and a second call with the same query only copies.
 * TW_ERR_STATE: before a stitch, before tw_set_row_groups, after anything that drops the forest (see tw_attribute_traces);
 * compare without a reference set.  TW_ERR_ARG: mode outside {0, 1}; compare in another mode than the reference set's.
 * TW_ERR_UNSUPPORTED: n_groups > 2^20 or a server row at level >= 2^16: the packed sort key holds 16 bits of level, 21 of
 * cg + 1 and 20 of g.  TW_SIG_HASH_BITS (default 64, read by tw_create) keeps only that many low bits of the hash: with 2,
 * unrelated signatures share a bucket and the exact comparison alone separates them -- the results are the same.
 * Results do not depend on scheduling: no floating point; the atomics are integer adds, minima and maxima of which only the
 * result is read.  Covers one engine's batch.  Timing: tw_get_timing slots 25..27 (items and levels; sort, run lengths and
 * hash; classes, comparison and per-class reduction; HIP events, ms; those of the last call that did not just copy). */
typedef struct {
    int32_t mode;
    uint32_t need_flags, skip_flags;
    int32_t keep_reference, compare;
} tw_sig_query;
typedef struct {
    int32_t *row_level;
    int32_t *tree_class;
    int64_t *tree_items;
    uint8_t *tree_same;
    int32_t *class_rep;
    int64_t *class_trees, *class_latency_sum, *class_latency_min, *class_latency_max;
    int64_t *class_off;
    int32_t *class_entries;
} tw_signatures;
int tw_trace_signatures(tw_engine *e, const tw_sig_query *q, const tw_signatures *out, int64_t *summary6);

/* ---- per-class latency profiles: the aggregate trace of every call-graph class (csrc/tw_prof.h) -------------------
 *
 * Replaces: PreparePerCGData (alibaba-analysis/analysis.py:233-292), which works on the traces of one call graph at a time.
 * tw_trace_signatures says what a trace looks like and gives per class only the latency sum, minimum and maximum;
 * tw_attribute_traces says where every row spends its time, but adds it up per group over all selected traces.  This is the
 * join: of the slow traces of one shape, which call at which level is on the critical path, how long it takes and when it
 * starts -- one node per signature entry, with times.  The call takes no query of its own; it works on what is resident:
 * the forest of the last stitch, the row groups, the result of the last tw_trace_signatures (its mode, tree_class, class_off,
 * class_entries) and the last tw_attribute_traces on the same forest (tree_selected, self_time, path_time).
 *
 * Definitions (integer microseconds; a row with end < start counts as end = start, as in the attribution):
 *   counted     tree t is counted when tree_class[t] = c >= 0 and tree_selected[t] != 0: the attribution's selection (the
 *               slowest X % that started after Y), split by shape.
 *   items       of a counted tree: its signature items, the server rows with row_group >= 0.  Item row r has the key (level,
 *               cg, g) of the resident mode; its entry is the one entry j of class c with that key (it exists: t's signature
 *               is class c's), global entry index i = class_off[c] + j.
 *   per entry i, over the item rows of the counted trees that map to it (int64 [n_entries], n_entries = summary6[3] of the
 *   signature call):
 *     rows                  count
 *     span_time             sum of the durations
 *     span_min, span_max    INT64_MAX / INT64_MIN where rows == 0
 *     self_time, path_time  sums of the attribution's per-row figures
 *     path_rows             rows on the critical path (the rows tw_attribute_traces counts in group_path_rows)
 *     path_trees            counted trees with at least one such row at this entry
 *     offset                sum of start[r] - start[root of t]: where in the trace the entry begins
 *   invariant   rows[i] == class_entries[i].count * class_counted[c].
 *   per class (int64 [n_classes], n_classes = summary6[1] of the signature call):
 *     class_counted         counted trees of the class
 *     class_latency         sum of tree_latency over them
 *     class_path_time       sum of path_time over the class' entries
 *     class_top_entry       the global index of the entry with the largest path_time among those with path_rows > 0 (ties: the
 *                           smallest index), -1 if there is none
 *   summary6    counted trees, classes with a counted tree, counted item rows, entries with rows > 0, trees with a class that
 *               are not selected, selected trees without a class.
 *
 * Outputs are caller-allocated, any may be NULL; the sizes are those the signature call returned.  The result stays on the device
 * until the signature result or the attribution is dropped (and whatever drops either: see both), and a second call only
 * copies.  The call itself drops nothing: tw_latency_distributions and tw_trace_signatures answer after it what they answered
 * before.  TW_ERR_STATE: without a resident signature result (before tw_trace_signatures, after tw_score_traces, new row groups
 * or anything that drops the forest); without a tw_attribute_traces on the current forest.  Both calls have checked their
 * arguments: there is no other status.
 * Covers one engine's batch, the selected assignment and one signature query at a time (a tw_trace_signatures call with another
 * query replaces the result and with it the profile); no quantiles per entry (tw_latency_distributions has them per group).
 * Results do not depend on scheduling: no floating point; the atomics are integer adds, minima, maxima and exchanges -- of an
 * exchange only "was this the first" is used, and only to count: which row counts a tree depends on scheduling, the count does
 * not.  Timing: tw_get_timing slots 28..30 (the sweep over the rows; the per-tree and per-class pass; the copies; HIP events,
 * ms; those of the last call that did not just copy). */
typedef struct {
    int64_t *rows, *span_time, *span_min, *span_max, *self_time, *path_time, *path_rows, *path_trees, *offset;
    int64_t *class_counted, *class_latency, *class_path_time, *class_top_entry;
} tw_class_profile;
int tw_class_profiles(tw_engine *e, const tw_class_profile *out, int64_t *summary6);

/* ---- traces selected by a predicate: a flag bit every stage reads (csrc/tw_filt.h) ------------------------------------
 *
 * Extends: the reference's one hard-coded query (src/query_engine/delay_culprit.py:19-28: whole traces, the slowest X %,
 * started after Y), which is all that the stages above select by.  tw_score_traces already writes one bit
 * (TW_TREE_CONFIDENT) into the device forest's tree_flags that every later stage can select by through need_flags; this is
 * the general form: a predicate over the stitched trees, evaluated on the device, whose result is bit TW_TREE_MATCH.  One
 * call makes tw_attribute_traces, tw_latency_distributions, tw_compare_cohorts, tw_history_push, tw_trace_signatures,
 * tw_class_profiles and tw_class_history_push work on "the traces that match" (need_flags | TW_TREE_MATCH).
 *
 * Definitions (integer microseconds; a row with end < start counts as end = start, as in the attribution; sums wrap in two's
 * complement):
 *   query       n_clauses <= TW_FILT_MAX_CLAUSES clauses, each in one of TW_FILT_MAX_TERMS terms: the predicate is the OR over
 *               the terms that have a clause of the AND over the term's clauses.
 *   value       of clause j on tree t, by subject:
 *                 0 LATENCY  tree_latency[t]
 *                 1 ROWS     tree_off[t + 1] - tree_off[t]
 *                 2 START    row_start of the root
 *                 3 CLASS    tree_class[t] of the resident signature result (-1 for a tree that result did not class)
 *                 4 GROUP    over the tree's rows with row_group == group (group -1: with row_group >= 0) the reduction
 *                            (0 sum, 1 min, 2 max) of the metric: 0 the count, 1 the duration, 2 self_time, 3 path_time, 4 the
 *                            count of those rows that are on the critical path (the rows tw_attribute_traces counts in
 *                            group_path_rows).  Metrics 0 and 4 are sums.
 *                 5 EDGE     the same over the tree's signature items of one edge: the server rows with row_group == group
 *                            whose cg == caller, cg exactly as mode 1 of tw_trace_signatures defines it (the row_group of
 *                            the nearest server ancestor, -1 if there is none or its group is -1).  Metrics 0 (count) and 1
 *                            (duration).
 *               A sum over no rows is 0.  A min or max over no rows is no value: clause_value holds INT64_MIN and the clause
 *               does not hold, negated or not.  group, caller, metric and reduce are read for GROUP and EDGE only.
 *               clause_value is written for every tree, eligible or not.
 *   holds       lo <= value <= hi, then negated when negate != 0.
 *   eligible    flags hold every bit of need_flags and none of skip_flags, as in the attribution (the flags as they are
 *               before the call: a query may name TW_TREE_MATCH and so narrow the last match).
 *   match       an eligible tree matches iff n_clauses == 0 or every clause of some term that has one holds.  A tree that is
 *               not eligible never matches and is counted nowhere.
 *   effect      bit 4 (TW_TREE_MATCH) of the device forest's tree_flags is cleared and rewritten for every tree.  Before the
 *               first call it is never set; a new tw_stitch_traces makes a new forest without it, and the tree_flags that
 *               call returns never show it.  tw_score_traces keeps it (it masks its own bit only).  One bit: a second
 *               filter replaces the first.
 *   outputs     tree_match [n_trees]; match_trees: the matched trees in ascending order, summary6[1] of them (room for
 *               n_trees); clause_value [n_trees][n_clauses]; clause_trees [n_clauses]: eligible trees on which the clause
 *               holds; term_trees [TW_FILT_MAX_TERMS]: eligible trees on which every clause of the term holds, 0 for a term
 *               without a clause.  `out` and any array may be NULL.
 *   summary6    eligible trees, matched trees, the sum / the minimum (INT64_MAX without a match) / the maximum (INT64_MIN
 *               without one) of tree_latency over the matched trees, the rows of the matched trees.
 *
 * TW_ERR_STATE: before a stitch or before tw_set_row_groups (an EDGE clause needs no more than that: the forest and the
 * groups, where tw_trace_signatures refuses without them); a clause of metric 2, 3 or 4 without a resident attribution; a
 * CLASS clause without a resident signature result.  TW_ERR_ARG: n_clauses outside [0, 16]; a term, subject, metric or reduce
 * out of range; a group outside [-1, n_groups) (EDGE: [0, n_groups)) or a caller outside [-1, n_groups); lo > hi; a reduce
 * other than sum on metric 0 or 4.  A refused call leaves the bit and everything resident as it was.
 * Residency: the call reads first and drops afterwards -- the attribution (with the distribution items and the class profile)
 * and the signature result (with the class profile) only where the query they were made with named the bit (need_flags |
 * skip_flags holds TW_TREE_MATCH); a result whose query does not name the bit cannot depend on it and stays.  The history
 * and the class catalogue hold copies and are untouched.
 * Limits: 16 clauses in 8 terms; no clause on a cohort, a decision margin or a catalogue id; no witness row; one bit; one
 * engine's batch and the selected assignment.  Results do not depend on scheduling: no floating point; the atomics are
 * integer adds, minima, maxima and ors of which only the result is read, and the list of the matched trees is written by a
 * scan, not by a cursor.  Timing: tw_get_timing slots 46..48 (the tree kernel; the list; the copies; HIP events, ms). */
#define TW_TREE_MATCH 16
#define TW_FILT_MAX_CLAUSES 16
#define TW_FILT_MAX_TERMS 8
typedef struct {
    int32_t term;      /* 0 .. TW_FILT_MAX_TERMS-1: the conjunction this clause belongs to */
    int32_t subject;   /* 0 LATENCY, 1 ROWS, 2 START, 3 CLASS, 4 GROUP, 5 EDGE */
    int32_t group;     /* GROUP: g in [0, G), or -1 = every row with row_group >= 0.  EDGE: the callee g in [0, G) */
    int32_t caller;    /* EDGE: cg in [-1, G) */
    int32_t metric;    /* GROUP: 0 rows, 1 span (duration), 2 self_time, 3 path_time, 4 rows on the critical path.  EDGE: 0 rows, 1 span */
    int32_t reduce;    /* 0 sum, 1 min, 2 max (metric 0 and 4: sum only) */
    int32_t negate;
    int64_t lo, hi;    /* the clause holds iff lo <= value <= hi, then negated */
} tw_filter_clause;
typedef struct {
    uint32_t need_flags, skip_flags;
    int32_t n_clauses;
    const tw_filter_clause *clauses;
} tw_filter_query;
typedef struct {
    uint8_t *tree_match;      /* [n_trees] */
    int32_t *match_trees;     /* [n_trees] capacity, summary6[1] entries written, ascending */
    int64_t *clause_value;    /* [n_trees][n_clauses], INT64_MIN = no value */
    int64_t *clause_trees;    /* [n_clauses] eligible trees on which the clause holds */
    int64_t *term_trees;      /* [TW_FILT_MAX_TERMS] eligible trees on which every clause of the term holds; 0 for an unused term */
} tw_filter_result;
int tw_filter_traces(tw_engine *e, const tw_filter_query *q, const tw_filter_result *out, int64_t *summary6);

/* ---- reconstructed traces handed out as trees: exemplars, pre-order rows (csrc/tw_extr.h) -------------------------------
 *
 * Extends: the stages above, which answer in aggregates (culprits, distributions, classes, a match bit); the reference walks
 * its traces on the host (src/query_engine/delay_culprit.py:30-97) and hands none out either.  tw_extract_traces selects
 * trees of the device forest of the last tw_stitch_traces and writes them as a packed sub-forest -- every tree in pre-order
 * with local parent indices -- which it keeps on the device; tw_get_extracted copies it out.  Two calls, because the caller
 * cannot know the sizes beforehand: the capacities of tw_get_extracted's arrays are the sizes summary6 returned.
 *
 * Definitions:
 *   eligible    tree_flags hold every bit of need_flags and none of skip_flags: the device forest's flags as they are at the
 *               call, so TW_TREE_CONFIDENT and TW_TREE_MATCH can be named as in tw_attribute_traces.
 *   mode 0 TOP        the eligible trees in the order `order`, the first `limit` of them (limit 0: all of them):
 *                       order 0  by tree ascending
 *                       order 1  slowest first: key (tree_latency descending, tree ascending)
 *                       order 2  fastest first: key (tree_latency ascending, tree ascending)
 *   mode 1 QUANTILES  the eligible trees sorted ascending by (tree_latency, tree), n of them; output tree j is the one at
 *                     index min(n - 1, (int64)(probs[j] * (double)n)), the index rule of tw_latency_distributions and
 *                     tw_compare_cohorts.  A tree chosen twice appears twice; n = 0 selects nothing.
 *   mode 2 LIST       the trees list[0 .. n_list) in the caller's order, duplicates kept; need_flags / skip_flags are not
 *                     applied (match_trees of a filter, one tree of a class).
 *   children(p)  the rows c of p's tree with link[c] == p, ordered by (row_start[c], c); link is the forest's link table, the
 *                one tw_attribute_traces returns.
 *   pre-order    visit(p): emit p, then visit(c) for every c of children(p) in that order; a tree is visit(root).
 *   outputs      output tree j owns the positions out_off[j] .. out_off[j + 1]; a row's local index is its position less
 *                out_off[j].  Per output tree: sel_tree (the source tree), sel_root (its root row), sel_latency, sel_start
 *                (row_start of the root), sel_flags (the device flags, bits 3 and 4 included); out_off has n_sel + 1 entries.
 *                Per position: row (span-table row); parent (local index of link[row], -1 for the root, otherwise smaller
 *                than the row's own local index); depth (the stitch's); subtree (rows of the row's subtree, itself included:
 *                the next sibling or uncle stands at q + subtree[q]); kind (row_kind: 1 the hop above the row was observed, 2
 *                predicted, 0 absent); group (row_group, -1 when no row groups are resident); start, end; self_time,
 *                path_time (gathered from the resident attribution when there is one).
 *   summary6     eligible trees (LIST: n_trees), selected trees, rows of the selected trees, rows of the largest selected
 *                tree, selected trees taken by the single-tree route (more than 256 rows), 1 if an attribution was resident
 *                and the times were gathered, else 0.
 *
 * TW_ERR_STATE: before a stitch or after anything that drops the forest; tw_get_extracted without a result, or with
 * self_time / path_time non-NULL when the result holds no times.  TW_ERR_ARG: mode or order out of range; limit negative; a
 * prob outside [0, 1] or not a number; n_probs outside [0, 32]; n_list outside [0, 2^20] or an id outside [0, n_trees).  A
 * refused call leaves everything resident as it was, the last result included.  The call writes no flag and drops nothing.
 * Residency: the result holds copies in buffers of its own; another extraction replaces it; it goes with the forest (a load,
 * tw_scale_load, tw_set_span_rows, a pass, a new stitch).  A later tw_filter_traces or tw_score_traces does not drop it: it
 * answers the query as the flags stood.
 * Limits: the selected assignment only and one engine's batch; 32 probs; 2^20 list entries; no decision margins per hop (a
 * caller gathers tw_confidence's by `row`).  A tree of more than 256 rows is taken by one wavefront on tables in global
 * memory: rows x preceding rows / 64 steps for the sibling sums and depth x rows / 64 for the sweeps over the levels.
 * Results do not depend on scheduling: integers only; the lists and offsets are written by scans, not by a cursor.  Timing:
 * tw_get_timing slots 49..51 (selection, sizes and offsets; the tree kernel; the copies of tw_get_extracted; HIP events, ms). */
#define TW_EXTR_MAX_PROBS 32
#define TW_EXTR_MAX_LIST (1 << 20)
typedef struct {
    uint32_t need_flags, skip_flags;
    int32_t mode;          /* 0 TOP, 1 QUANTILES, 2 LIST */
    int32_t order;         /* TOP: 0 by tree, 1 slowest first, 2 fastest first */
    int64_t limit;         /* TOP: 0 = every eligible tree */
    int32_t n_probs;       /* QUANTILES: <= TW_EXTR_MAX_PROBS */
    int32_t n_list;        /* LIST: <= TW_EXTR_MAX_LIST */
    const double *probs;
    const int32_t *list;
} tw_extract_query;
typedef struct {
    int32_t *sel_tree, *sel_root;            /* [n_sel] */
    int64_t *sel_latency, *sel_start;        /* [n_sel] */
    uint8_t *sel_flags;                      /* [n_sel] */
    int64_t *out_off;                        /* [n_sel + 1] */
    int32_t *row, *parent, *depth, *subtree; /* [rows of the selected trees] */
    uint8_t *kind;
    int32_t *group;
    int64_t *start, *end;
    int64_t *self_time, *path_time;          /* only where summary6[5] was 1 */
} tw_extracted;
int tw_extract_traces(tw_engine *e, const tw_extract_query *q, int64_t *summary6);
int tw_get_extracted(tw_engine *e, const tw_extracted *out);

/* ---- the classes of batch after batch: a catalogue on the device (csrc/tw_chist.h) --------------------------------
 *
 * Replaces: FindUniqueCGs / PreparePerCGData run over a whole directory of traces (alibaba-analysis/analysis.py:214-221,
 * 233-292).  tw_trace_signatures and tw_class_profiles cover one engine's batch, and their classes are numbered per batch;
 * the catalogue gives classes ids that hold across batches and figures that add up across them: did a call graph appear
 * that was never seen, which shapes became more frequent, where does a shape spend its time over all the batches.  It is
 * device state that outlives loads, stitches, passes and queries, as the history does: none of the calls below drops or
 * rewrites anything of the resident batch.  Only tw_class_history_reset and tw_destroy end it.  Everything is integer.
 *
 * Definitions:
 *   catalogue  empty after tw_create and tw_class_history_reset.  The first push or merge fixes mode (0 levels, 1 edges)
 *              and G = n_groups; a later one with another mode or n_groups is TW_ERR_ARG.  It holds C classes; class k owns
 *              the entries cat_off[k] .. cat_off[k + 1]) of cat_entries, four int32 (level, cg, g, count) in signature
 *              order: the layout of class_off / class_entries.  Two classes are the same iff their entry sequences are
 *              equal entry by entry; a hash of the entries buckets the classes, the comparison of the entries decides.
 *   class ids  a source class whose signature the catalogue holds has that class' id; the source classes it does not hold
 *              get C_before + (the number of such classes with a smaller source index).  An id never changes afterwards:
 *              ids depend on the order of the calls and on nothing else.
 *   per class  (int64) from the signature result, what & 1: trees, latency_sum (wrapping), latency_min / latency_max
 *              (INT64_MAX / INT64_MIN while trees == 0).  From the class profile, what & 2: counted and latency (its
 *              class_counted, class_latency).  Book-keeping: first_epoch = min and last_epoch = max of the epochs, seen = the
 *              number of pushes and merges whose source held the class.  epoch is a label of the caller's (a batch number, a
 *              timestamp) of which the engine only takes minima and maxima.
 *   per entry  (int64, what & 2) the nine fields of tw_class_profile -- rows, span_time, span_min, span_max, self_time,
 *              path_time, path_rows, path_trees, offset -- added, or combined by min / max, at cat_off[id] + j for entry j of
 *              the source class: the entries of equal signatures line up.
 *   derived    on read: class_path_time and class_top_entry by the rule of tw_class_profiles (the largest accumulated
 *              path_time among the class' entries with path_rows > 0, ties to the smallest index, -1 if there is none), with
 *              the catalogue's global entry indices.
 *   push       the source is the resident signature result and, with what & 2, the resident class profile.  what in {1, 2, 3};
 *              with 2 only the profile's figures are added (two attributions of one forest are pushed without counting its
 *              trees twice).  Every class of the source is held afterwards, whatever what is; its seen is incremented and its
 *              epochs are updated.  class_map [the batch's classes] = the catalogue ids.  summary6 = new classes, classes
 *              held, new entries, entries held, pushes and merges since the reset, classes of the source.
 *   match      class_map only, -1 for a class the catalogue does not hold (every class on an empty catalogue, TW_OK); it
 *              changes nothing (a catalogue of the other mode or of other groups holds none of them: -1 everywhere).  With
 *              tree_class of the signature result it names the traces whose shape was never seen.
 *              summary6 as a push would give it, [0] and [2] = the classes and entries not held, [1] and [3] as they are.
 *   merge      a push from host arrays: a saved catalogue, another rank's, another engine's signatures and profile.  The
 *              source is the struct tw_class_history_get fills, with n_classes, n_entries, mode, n_groups set.  A figure
 *              pointer that is NULL adds nothing (zeros, the identities of min and max); first_epoch / last_epoch / seen NULL
 *              = the epoch argument and 1.  class_path_time and class_top_entry are not read.  The host checks that class_off
 *              starts at 0, does not decrease and ends at n_entries; the device, before anything is changed, that every
 *              class' entries ascend strictly by (level, cg, g), count >= 1, 0 <= level < 2^16, 0 <= g < G, cg in [-1, G)
 *              in mode 1 and 0 in mode 0, and that no two source classes have equal signatures.
 *   get        with out == NULL only summary6 (the sizes, as tw_class_history_info); a second call copies.  Every pointer
 *              of out may be NULL; class_off has C + 1 elements, class_entries 4 * entries, the per-class arrays C, the
 *              per-entry arrays `entries` elements.  The scalars of out are not written.
 *   info       out6 = C, entries, pushes and merges since the reset, mode, G, the hash table's capacity in slots; all 0 for
 *              an empty catalogue (tw_class_history_reset frees the buffers).
 *
 * TW_ERR_STATE: push or match without a resident signature result; what & 2 without a resident class profile; get on an
 * empty catalogue.  TW_ERR_ARG: what outside {1, 2, 3}; another mode or n_groups than the catalogue's; the source errors
 * above.  TW_ERR_UNSUPPORTED: more than 2^31 - 1 classes or entries (2^20 groups, as the signatures).  TW_ERR_DEVICE: no
 * memory.  A call that is refused or fails leaves the catalogue exactly as it was -- the store grows by copying and the
 * counts are set last; a merge that finds two equal source classes after they claimed slots refills the table from the
 * store.  Results do not depend on scheduling (where the table put a class does; that is never returned).
 * TW_SIG_HASH_BITS truncates this hash too: with 2 every class shares one of four buckets and the comparison alone
 * separates them.  No eviction; ranks merge through the host.  Timing: tw_get_timing slots 43..45 of the last push or merge
 * (HIP events, ms): 43 hash and lookup (with the source check of a merge), 44 scan, append, insert and any growth and
 * rehash, 45 accumulate. */
typedef struct {
    int64_t n_classes, n_entries;   /* read by tw_class_history_merge only */
    int32_t mode, n_groups;
    int64_t *class_off;
    int32_t *class_entries;
    int64_t *trees, *latency_sum, *latency_min, *latency_max, *counted, *latency, *first_epoch, *last_epoch, *seen;
    int64_t *rows, *span_time, *span_min, *span_max, *self_time, *path_time, *path_rows, *path_trees, *offset;
    int64_t *class_path_time, *class_top_entry;
} tw_class_catalogue;
int tw_class_history_reset(tw_engine *e);
int tw_class_history_push(tw_engine *e, int32_t what, int64_t epoch, int32_t *class_map, int64_t *summary6);
int tw_class_history_match(tw_engine *e, int32_t *class_map, int64_t *summary6);
int tw_class_history_merge(tw_engine *e, const tw_class_catalogue *src, int64_t epoch, int32_t *class_map, int64_t *summary6);
int tw_class_history_info(tw_engine *e, int64_t *out6);
int tw_class_history_get(tw_engine *e, const tw_class_catalogue *out, int64_t *summary6);

/* Replaces: the sweep of BuildDistributions (traceweaver_v3.py:120-169).  The spans of one service merged in start
 * order (stable: incoming spans first, then the endpoints in order): start / dur [n], ep [n] (0 = incoming span,
 * 1 + e = span of outgoing endpoint e), large_delay = the longest incoming span.  Per span: key_out = a * (E + 1) + b
 * of the pair its delay sample belongs to (-1: no qualifying predecessor) and the sample in microseconds.  The
 * (mean, std) per pair are np.mean / np.std of the samples in this order (host, traceweaver_amd/skipmode.py); the
 * durations of the incoming spans form the pair (0, 0), which the scorer never reads. */
int tw_build_distributions(tw_engine *e, int64_t n, const int64_t *start, const int64_t *dur, const uint8_t *ep, int64_t large_delay,
                           int32_t E, int32_t *key_out, int64_t *sample_out);

/* Measurement aid for the roofline figures (bench.py): rate of a plain 16-B-per-lane streaming copy kernel over
 * `bytes` of HBM (read + written bytes per second, in GB/s), `iters` launches timed with HIP events. */
int tw_measure_hbm_copy(tw_engine *e, int64_t bytes, int32_t iters, double *gbps);

/* Page-locked host buffers for the arrays of a tw_batch / tw_results: tw_load_batch and tw_get_results move pinned
 * memory at the full host-link rate (pageable memory is staged by the runtime at a fraction of it). */
int tw_host_alloc(int64_t bytes, void **out);
void tw_host_free(void *p);

/* One-shot convenience for a single unit: load, pass 1, (optional) pass 2 with caller-supplied
 * mixtures, results of the last pass run.  mix_n == NULL => pass 1 only. */
int tw_assign_service(tw_engine *e, int32_t n_in, const int64_t *in_start, const int64_t *in_end,
                      int32_t E, const int64_t *out_off, const int64_t *out_start, const int64_t *out_end,
                      const uint8_t *dag, const int32_t *key_rank, const int32_t *mix_n,
                      const double *mix_p, const tw_results *r);

/* ---- Jaeger-JSON ingest -> structure of arrays (host side) ------------------------------------
 *
 * Replaces the reference's loader for corpora that need no span rewriting: GetAllTracesInDir / TimeOrder
 * (executor.py:287-339), ParseJsonTrace / ParseSpansJson / ParseProcessesJson(2) (executor.py:342-384,451-461,
 * 755-793), ProcessTraceData (executor.py:795-849), PartitionSpansByEndPoint (executor.py:1104-1113),
 * GetGroundTruth (helpers/utils.py:22-32), FindOrder + nx.topological_sort (executor.py:214-285,
 * traceweaver_v1.py:37-39), FixSpans / FixSpans2 (executor.py:505-537,542-645) and the rewrite of the Alibaba parser
 * output (executor.py:377-448).  Names are interned: every *_name / service / span_id field below is a string id for
 * tw_corpus_string().  String ids are handles, not indices of one dense table: service / operation / endpoint names
 * count up from 0 (in order of first use, traces in time order -- the same for any number of parser threads), trace
 * ids are 2^29 + trace number, span ids 2^30 + span-table row (unique per trace: stored, never looked up). */
typedef struct tw_corpus tw_corpus;
int tw_corpus_create(tw_corpus **out);
void tw_corpus_destroy(tw_corpus *c);
const char *tw_corpus_last_error(const tw_corpus *c);   /* first file that failed to parse, if any */

/* Parses one-trace-per-file Jaeger JSON ({"data":[{"traceID","spans":[...],"processes":{...}}]}, or the
 * requestType shape of alibaba-analysis/real-parser.py:308-359), n_threads parser threads (<= 0: up to 32, one per 64 files),
 * orders the traces by the start of their root span and adds those whose root operation is `first_span`
 * (NULL / "" = any; executor.py:757-763,841) until max_traces (> 0; the reference stops at 1001,
 * executor.py:873) traces are held.  Files that do not parse or break an assumption the reference asserts on
 * are counted, not fatal. */
int tw_corpus_add_files(tw_corpus *c, const char *const *paths, int32_t n_paths, const char *first_span,
                        int64_t max_traces, int32_t n_threads, int32_t fix);

/* `fix` = the span surgery the reference applies to some of its corpora before the walk (executor.py:776-779):
 *   TW_FIX_NONE          plain Jaeger exports (hotel; --fix 2..4)
 *   TW_FIX_CLIENT_TWINS  FixSpans (executor.py:505-537; nodejs, --fix 0): every hop is logged once, as a server span;
 *                        each gets a client twin "<id>_client" in the calling service, which is looked up in the
 *                        static service -> caller map given with tw_corpus_set_callers (executor.py:109-115)
 *   TW_FIX_REROOT        FixSpans2 (executor.py:542-645; media, --fix 1): the span named first_span becomes the root,
 *                        same-process children are dropped, every remaining hop gets a client twin in its parent's
 *                        process, spans are ordered by start time
 *   TW_FIX_RPC_TWINS     ParseSpansJson with first_span == None (executor.py:377-448; --fix 5, the output of
 *                        alibaba-analysis/real-parser.py): every call is logged twice under one rpc id, as a server record in
 *                        the callee and a client record in the caller; the client record becomes "<rpc id>.client" and
 *                        the server record is re-pointed at it; a service that calls itself gets a stand-in callee
 *                        "<callee>@<rpc id>-loop" (the reference draws a random name ending in "-loop"), one per rpc id
 *                        for the whole corpus, traces visited in time order; traces in which a child span is not
 *                        contained in its parent are dropped (counted as filtered) */
enum { TW_FIX_NONE = 0, TW_FIX_CLIENT_TWINS = 1, TW_FIX_REROOT = 2, TW_FIX_RPC_TWINS = 3 };
/* serviceLoopMap (executor.py:396): the service a "...-loop" stand-in was split from (its replica count is what the
 * load factor of executor.py:1092-1096 uses), NULL if `service` is not a stand-in. */
const char *tw_corpus_loop_origin(const tw_corpus *c, const char *service);
/* The static service -> caller map of TW_FIX_CLIENT_TWINS. */
int tw_corpus_set_callers(tw_corpus *c, const char *const *service, const char *const *caller, int32_t n);

/* out6 = spans held, traces held, files seen, files that failed to parse, traces filtered out, strings (names + trace
 * ids + span ids held).  tw_corpus_string returns NULL for an id that names nothing. */
int tw_corpus_counts(const tw_corpus *c, int64_t *out6);
const char *tw_corpus_string(const tw_corpus *c, int32_t id);
int tw_corpus_trace_names(const tw_corpus *c, int32_t *out);   /* string id of the traceID of trace 0 .. traces-1 */

/* The span table (one row per span reached from its trace's root, in walk order); caller-allocated columns of
 * tw_corpus_counts()[0] entries, any may be NULL.  parent = row of the referenced span (-1 for roots),
 * kind: 1 server (incoming), 2 client (outgoing). */
typedef struct {
    int32_t *trace, *span_id, *service, *op_name, *parent;
    int64_t *start, *duration;
    uint8_t *kind;
} tw_span_table;
int tw_corpus_span_table(const tw_corpus *c, tw_span_table *t);

/* Every service with a single caller whose endpoints each hold one call per request becomes a unit, in the
 * layout tw_load_batch takes (first nine fields = tw_batch's); pointers stay owned by the corpus and are valid
 * until the next call.  true_child / in_trace as in tw_find_order / tw_set_truth; in_row / out_row = span-table
 * row of every incoming / outgoing span (to translate results back to (trace id, span id)); skipped[4] =
 * services left out because they have several callers (executor.py:1126-1128), because an endpoint's span count
 * differs from the number of requests (skip mode) or E > TW_MAX_EP, because they hold < 2 requests, because the
 * call-order relation has a cycle. */
typedef struct {
    int32_t n_units;
    const int64_t *unit_in_off;
    const int32_t *unit_E;
    const int64_t *ep_off;
    const uint8_t *dag;
    const int32_t *key_rank;
    const int64_t *in_start, *in_end, *out_start, *out_end;
    const int32_t *true_child, *in_trace, *in_row, *out_row;
    const int32_t *unit_service, *ep_name, *in_ep_name;
    const int32_t *unit_order;   /* position of the unit's service among the services that make calls (the executor's process_id, executor.py:1079) */
    int64_t n_traces;
    int32_t skipped[4];
} tw_unit_set;
int tw_corpus_build_units(tw_corpus *c, tw_unit_set *out);

#ifdef __cplusplus
}
#endif
#endif /* TRACEWEAVER_AMD_H */

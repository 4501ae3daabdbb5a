// tw_engine.hip -- host side of libtwgpu.so: the C-ABI of include/traceweaver_amd.h on top of the
// kernels in tw_kernels.h.  One engine = one HIP device + one stream; inputs stay resident in HBM
// between the two passes (spans are read from host memory exactly once, in tw_load_batch).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "traceweaver_amd.h"
#include "tw_kernels.h"
#include "tw_fit.h"
#include "tw_eval.h"
#include "tw_skip.h"
#include "tw_load.h"
#include "tw_baselines.h"
#include "tw_stitch.h"
#include "tw_attr.h"
#include "tw_conf.h"
#include "tw_dist.h"
#include "tw_cmp.h"
#include "tw_hist.h"
#include "tw_sig.h"
#include "tw_prof.h"
#include "tw_filt.h"
#include "tw_extr.h"
#include "tw_chist.h"
#include "tw_order.h"

using namespace tw;

namespace {

constexpr int kMaxRepairRounds = 1 << 20;
enum { ST_EMPTY = 0, ST_LOADED = 1, ST_PASS1 = 2, ST_MIX = 3, ST_PASS2 = 4 };
enum { EV_BEGIN = 0, EV_PARAMS, EV_ENUM0, EV_ENUM1, EV_WIN, EV_SEL, EV_REPAIR, EV_END, EV_COUNT };
enum { SE_STITCH = 0, SE_ATTR = 5, SE_CONF = 9, SE_DIST = 13, SE_SIG = 18, SE_PROF = 22, SE_CMP = 26, SE_HIST = 29, SE_CHIST = 37, SE_FILT = 41, SE_EXTR = 45, SE_COUNT = 50 };   // stage events: 5 + 4 + 4 + 5 + 4 + 4 + 3 + 8 + 4 + 4 + 5

int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

// Every TW_* variable of the engine.  read_knobs, called by tw_create, is the only reader of the environment: a knob has the
// engine's lifetime, and a variable set after tw_create does not reach that engine.
struct Knobs {
    int tile;                 // TW_TILE: incoming spans (threads) per workgroup of the per-span kernels
    int tile_threads;         // TW_TILE_THREADS: threads per incoming span of k_enumerate_tile (its items and tuples are spread over all of them)
    int tile_single;          // TW_TILE_SINGLE: the one-endpoint class takes the lean path of k_enumerate_tile (0 = the general path: A/B runs, bisection)
    int tile_single_threads;  // TW_TILE_SINGLE_THREADS: threads per incoming span on that path (media shape: 19.3-19.4 ms per step with one, 19.5-19.6 with two)
    int tile_pair;            // TW_TILE_PAIR: the two-endpoint class takes the pair path of k_enumerate_tile (0 = the general path: A/B runs, bisection)
    int tile_pair_threads;    // TW_TILE_PAIR_THREADS: threads per incoming span on that path (1 or 2)
    int tile_rank;            // TW_TILE_RANK: the general path of k_enumerate_tile ranks long spans among their compacted survivors (0 = the all-pairs loop: A/B runs, bisection)
    int block_params;         // TW_BLOCK_PARAMS: pass-1 block parameters by a wavefront per group of blocks (0 = the thread-per-slot kernel: A/B runs, bisection)
    int coop;                 // TW_COOP_THREADS: threads of the per-unit cooperative kernels
    int set_hw_queues;        // TW_SET_HW_QUEUES: tw_create exports GPU_MAX_HW_QUEUES when it is still unset (see there)
    int pipeline;             // TW_CLASS_PIPELINE=0: every class joins the engine's stream after its enumeration (measurements, tests)
    int sig_hash_bits;        // TW_SIG_HASH_BITS: bits of the signature hash that tw_trace_signatures keeps (tests: collisions)
    int debug_lists;          // TW_DEBUG_LISTS=1: the list counters of the first enumeration are copied to the host per class (tw_debug_worklists)
    int stage_min_tiles;      // TW_STAGE_MIN_TILES: batches of fewer tiles per class on average join the classes after the enumeration (a stage is 17 small
                              // launches per class: the 1 M-span Alibaba-shape slice, eight classes of 300 tiles, takes 7.8 ms per step staged and 6.4 joined)
    int tile_sub;             // TW_TILE_SUB: workgroups per tile for classes of few tiles (1 = never)
    int lean_pool;            // TW_LEAN_POOL: doubles of LDS for the pair tables of k_enumerate_lean
    int split_twins, defer_min_e, lean_min_e, lean_grid, tile_max_deep;   // TW_SPLIT_TWINS .. TW_TILE_MAX_DEEP: handed to the kernels in Dev (tw_load_batch)
    int64_t part_slots_max;   // TW_PART_SLOTS_MAX: most scratch slots of the split enumerations, whatever the batch (tw_load_batch)
    int part_budget_deep;     // TW_PART_BUDGET_DEEP: extra work-list entries per span of the classes of five and more endpoints (part_extra)
    int fit_sort;             // TW_FIT_SORT=1: the gap rows go the sort route (fit_prepare)
    int stage_gate;           // TW_STAGE_GATE: the stages of the shorter classes wait for the critical class' tile kernel (launch_class_stage; 0 = they do not: A/B runs, bisection)
    int fit_spec;             // TW_FIT_SPEC: the final fit of the likeliest count runs beside the model selection (fit_run; 0 = after it, five launches on one stream: A/B runs, bisection)
    int fit_order;            // TW_FIT_ORDER: the refit's launches hand their fits out longest first, by order tables built on the host (fit_order; 0 = in grid order: A/B runs, bisection)
};

Knobs read_knobs() {
    Knobs K;
    K.tile = std::min(std::max(env_int("TW_TILE", kTile), 1), kTile);
    K.tile_threads = std::min(std::max(env_int("TW_TILE_THREADS", 2), 1), 4);
    K.tile_single = env_int("TW_TILE_SINGLE", 1);
    K.tile_single_threads = std::min(std::max(env_int("TW_TILE_SINGLE_THREADS", 1), 1), 4);
    K.tile_pair = env_int("TW_TILE_PAIR", 1);
    K.tile_pair_threads = std::min(std::max(env_int("TW_TILE_PAIR_THREADS", 2), 1), 2);
    K.tile_rank = env_int("TW_TILE_RANK", 1) != 0 ? 1 : 0;
    K.block_params = env_int("TW_BLOCK_PARAMS", 1);
    K.coop = std::min(std::max(env_int("TW_COOP_THREADS", kCoop), 1), kCoop);
    K.set_hw_queues = env_int("TW_SET_HW_QUEUES", 0);
    K.pipeline = env_int("TW_CLASS_PIPELINE", 1);
    K.sig_hash_bits = std::min(std::max(env_int("TW_SIG_HASH_BITS", 64), 1), 64);
    K.debug_lists = env_int("TW_DEBUG_LISTS", 0);
    K.stage_min_tiles = env_int("TW_STAGE_MIN_TILES", 1024);
    K.tile_sub = std::max(env_int("TW_TILE_SUB", 8), 1);
    K.lean_pool = std::min(std::max(env_int("TW_LEAN_POOL", 512), 1), 4096);
    K.split_twins = env_int("TW_SPLIT_TWINS", 2);
    K.defer_min_e = env_int("TW_DEFER_MIN_E", 5);
    K.lean_min_e = env_int("TW_LEAN_MIN_E", 5);
    K.lean_grid = std::max(env_int("TW_LEAN_GRID", TW_LEAN_GRID), 1);
    K.tile_max_deep = std::min(std::max(env_int("TW_TILE_MAX_DEEP", kTileMax), 0), kTileMax);
    K.part_slots_max = (int64_t)std::max(env_int("TW_PART_SLOTS_MAX", 16 << 20), 1024);
    K.part_budget_deep = env_int("TW_PART_BUDGET_DEEP", 2);
    K.fit_sort = env_int("TW_FIT_SORT", 0);
    K.stage_gate = env_int("TW_STAGE_GATE", 1);
    K.fit_spec = env_int("TW_FIT_SPEC", 1) != 0 ? 1 : 0;
    K.fit_order = env_int("TW_FIT_ORDER", 1) != 0 ? 1 : 0;
    return K;
}

// MT19937 as numpy's RandomState runs it (the published reference algorithm of Matsumoto & Nishimura; seeding of an integer
// seed = init_genrand, `random_sample` = (a >> 5, b >> 6) -> (a * 2^26 + b) / 2^53): `Mt19937(s).random_sample()` yields the
// doubles of `np.random.RandomState(s).random_sample()`.  Used for the k-means++ draws of the mixture refit (tw_fit.h).
struct Mt19937 {
    uint32_t mt[624];
    int idx = 624;
    explicit Mt19937(uint32_t seed = 0u) {
        mt[0] = seed;
        for (int i = 1; i < 624; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    }
    uint32_t next() {
        if (idx >= 624) {
            for (int i = 0; i < 624; i++) {
                const uint32_t y = (mt[i] & 0x80000000u) | (mt[(i + 1) % 624] & 0x7fffffffu);
                mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            idx = 0;
        }
        uint32_t y = mt[idx++];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= y >> 18;
        return y;
    }
    double random_sample() {
        const uint32_t a = next() >> 5, b = next() >> 6;
        return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
    }
};

}  // namespace

struct tw_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t cls_stream[kMaxEp + 1] = {};   // one stream per endpoint count: the enumeration kernels of different classes overlap
    hipEvent_t cls_ev[kMaxEp + 2] = {};        // [0] fork, [E] class E's enumeration done
    // the window / selection stage of a class follows its enumeration on the class' stream (run_pass): the three instantiations of
    // k_select_heavy on streams of their own beside it, forked from and joined to the class' stream
    hipStream_t sel_stream[3] = {};
    // the stage gate (launch_enumerate_all, launch_class_stage): the critical class of the pass being queued (0 = none), the event
    // behind its k_enumerate_tile, and how many stages of the last pass were queued behind that event (tw_get_timing slot 32)
    int gate_cls = 0, gate_waits = 0;
    hipEvent_t tile_done = nullptr;
    hipEvent_t prep_ev = nullptr;              // the per-pass fills the selection stage needs (main stream, beside the enumerations)
    hipEvent_t post_fork[kMaxEp + 1] = {}, post_join[kMaxEp + 1][3] = {}, post_done[kMaxEp + 1] = {};
    Knobs K{};                                 // the TW_* variables as tw_create found them (read_knobs)
    int32_t first_lists[3][kMaxEp + 1] = {};   // K.debug_lists: the list counters of the first enumeration per class -- narrow, wide, long enumerations
    int32_t *rank_in = nullptr, *rank_out = nullptr;   // scratch of sort_ends: rank of a span's end time less its index
    bool class_params = false;                 // pass 1 of a staged batch: sort_ends / k_block_params per class on the class' stream
    std::string err;
    int state = ST_EMPTY;
    std::vector<UnitDev> units;
    std::vector<TileDev> tiles;
    std::vector<int64_t> gs_off_h;
    std::vector<void*> allocs;
    // the arrays of a batch live in one device allocation that is kept (and grown) across tw_load_batch calls:
    // ~60 hipMalloc / hipFree pairs per batch otherwise cost as much as the transfer itself
    void* arena = nullptr;
    size_t arena_cap = 0;
    bool arena_open = false;
    std::vector<std::pair<std::function<void(void*)>, size_t>> arena_req;
    Dev P{};
    int64_t n_ie = 0, n_gp = 0, n_slots = 0, n_gaps = 0;
    // scratch for scans / sort
    PairVI* agg_pair = nullptr;
    int32_t *agg_i32 = nullptr, *agg_i32b = nullptr;
    uint32_t *seg_in = nullptr, *seg_out = nullptr;
    int n_seg_out = 0;
    void* sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
    double* mix_p_dev = nullptr;
    int32_t* mix_n_dev = nullptr;
    double* mix_c_dev = nullptr;
    double* gaps_sorted = nullptr;
    double* fit_models = nullptr;
    double* fit_uval = nullptr;
    int32_t *fit_ustart = nullptr, *fit_row_n = nullptr, *fit_row_uniq = nullptr;
    double* fit_centres = nullptr;
    // the speculative final fit (fit_run, tw_fit.h): forked from and joined to the engine's stream; its results; hits and misses of
    // the last refit (tw_get_timing slots 35, 36)
    hipEvent_t fit_fork = nullptr, fit_join = nullptr;
    double *fit_spec_centres = nullptr, *fit_spec_p = nullptr;
    int32_t *fit_spec_failed = nullptr, *fit_spec_ctr = nullptr;
    int32_t fit_spec_count[2] = {0, 0};
    double *fit_tape = nullptr, *fit_tape100 = nullptr;   // uniforms of the k-means++ seedings: model-selection fits / the refit (MT19937(100))
    int64_t* fit_tape_off = nullptr;
    int64_t fit_tape_cap = 0;
    bool fit_runs_pending = false;          // k_fit_runs is queued, its refusal flag not read yet (fit_prepare_launch / fit_prepare)
    bool fit_prepared = false;              // the gap rows of the resident pass-1 result are sorted and run-length compressed
    int32_t hard_pass1[kMaxEp + 1] = {};    // per class: windows its stage listed for k_select_dp in pass 1 (-1 not known)
    int8_t wide_pass1[kMaxEp + 1] = {};     // per class: -1 not known, 0 / 1 = the first enumeration of pass 1 listed no / some span with wide windows
    int32_t split_pass1[kMaxEp + 1] = {};   // per class: spans the first enumeration of pass 1 cut into parts (-1 not known): sizes the merge launch of pass 2 (a guess that only costs time when wrong)
    bool pass1_done = false;                // tw_run_pass1 has run on the resident batch (tw_run_pass2 reads its cut-offs, windows, tuple counts)
    std::vector<int32_t> fit_rows_h;        // host copy of fit_row_n, fit_row_uniq and the refusal flag of k_fit_runs, one block on the device too (fit_prepare): tw_fit_rows and the order tables read it
    bool fit_rows_h_valid = false;          // ... of the rows that are prepared now (cleared with fit_prepared)
    // The order tables of the last refit (fit_order; TW_FIT_ORDER): permutations of the grids of k_fit_seed<false> [4 n_slots] and
    // k_fit_em<false> [5 n_slots] and of the rows [n_slots] for the four kFull launches, behind one another; empty = grid order
    std::vector<int32_t> fit_order_h;
    int32_t* fit_order_dev = nullptr;
    double fit_order_host_ms = 0.0;         // host wall clock of building them (tw_get_timing slot 37)
    Mt19937 fit_rng;                        // stream of tw_fit_mixtures (tw_set_fit_seed; restarted by every tw_load_batch)
    uint32_t fit_seed = 0;
    int32_t* slot_unit = nullptr;
    int32_t* tile_ids = nullptr;            // tiles grouped by the unit's endpoint count
    // The small counters of a pass in one block, so that a pass (and a repair round) starts with one fill instead of a dozen:
    // [work-list counters .. frontier cursors] are what a repair round resets, the whole block what a pass resets.
    int32_t* ctr = nullptr;
    int64_t ctr_round_ints = 0, ctr_pass_ints = 0;
    int32_t tile_cls_off[kMaxEp + 2] = {};  // class E owns tile_ids[tile_cls_off[E] .. tile_cls_off[E+1])
    BlockRef* blk_tab = nullptr;            // the groups of blocks k_block_params_wave is launched over (a wavefront each), in unit order: those of every unit, then class by class
    int32_t blk_cls_off[kMaxEp + 2] = {};   // slot 0 (every unit) and class E own blk_tab[blk_cls_off[E] .. blk_cls_off[E+1])
    uint32_t *seg_gap = nullptr, *seg_gap_end = nullptr, *seg_gap_dst = nullptr;
    unsigned long long *comp_a = nullptr, *comp_b = nullptr;  // composite keys of sort_rows
    int64_t comp_cap = 0, n_gap_scored = 0;
    int32_t *truth = nullptr, *in_trace = nullptr;  // tw_set_truth
    uint8_t* trace_bad = nullptr;           // [2][n_traces]
    unsigned long long* eval_counts = nullptr;  // [n_units][4] + [2]
    int64_t n_traces = 0, trace_cap = 0;
    uint8_t* slot_scored = nullptr;
    int64_t n_gap_rows = 0;
    unsigned long long* key_acc = nullptr;  // [2] scratch of k_key_bits
    double fit_ms = 0.0;
    int rounds = 0;                         // repair rounds of the last pass
    bool skip_mode = false;                 // skip-mode batch (tw_batch.skip): one pass with skip spans
    SkipUnitDev* skip_units = nullptr;
    int32_t* skip_perm = nullptr; int64_t* skip_tw = nullptr; int32_t* skip_pool = nullptr; double* skip_dist = nullptr; long long* skip_fetch = nullptr;
    int64_t skip_fetch_n = 0;
    // tw_scale_load: the table as uploaded (kept so that every load level starts from it)
    int64_t *orig_is = nullptr, *orig_ie = nullptr, *orig_os = nullptr, *orig_oe = nullptr;
    int32_t *orig_truth = nullptr, *orig_trace = nullptr;
    bool scaled_upload = false;             // the batch was uploaded with unit_time_scale (already load-scaled by the caller)
    hipEvent_t ev[EV_COUNT] = {};
    double ms[6] = {0, 0, 0, 0, 0, 0};
    // The trace stages (tw_set_span_rows .. tw_class_profiles).  What is resident, what it needs and what drops it: the residency
    // model below the helpers (drop_*); the flags and capacities here are assigned there and at the one place that makes each resident.
    StitchDev S{};                          // tw_set_span_rows / tw_stitch_traces (tw_stitch.h): row maps, scratch and forest of a stitch
    int32_t* given_parent = nullptr;        // tw_set_parents: an assignment handed over by the caller (stitched as pass 0)
    bool rows_set = false, parents_given = false, stitched = false;
    int64_t rows_cap = 0, st_trees = 0;
    int stitched_pass = -1;                 // the forest is that of pass 1 | 2 (only such a forest can be scored), 0 = of tw_set_parents, -1 = of the truth
    bool stitched_truth = false;            // ground truth was set when the forest was stitched: its flags carry bit 2
    AttrDev A{};                            // tw_set_row_groups / tw_attribute_traces (tw_attr.h)
    bool groups_set = false, attributed = false;
    uint32_t attr_need = 0, attr_skip = 0;  // the flags the resident attribution selected by (tw_filter_traces drops it where they name its bit)
    int64_t groups_cap = 0, attr_rows_cap = 0;
    ConfDev C{};                            // tw_get_decisions / tw_score_traces (tw_conf.h): the decisions are those of the resident pass
    int64_t conf_rows_cap = 0;
    DistDev D{};                            // tw_set_row_cohorts / tw_latency_distributions (tw_dist.h); dist_ready: the sorted items of the
    bool cohorts_set = false, dist_ready = false;   // last attribution and the current labels are resident, a further call only gathers
    int64_t cohort_rows_cap = 0, dist_trees_cap = 0, dist_seg_cap = 0, dist_out_cap = 0 /* segments */, dist_items = 0;
    DistKeyDev dist_key{};
    CmpDev M{};                             // tw_compare_cohorts (tw_cmp.h): scratch of a call (the pool, the per-row results); nothing of it
    int64_t cmp_rows_cap = 0, cmp_items_cap = 0;    // outlives the call but the buffers
    // tw_history_* (tw_hist.h): the distributions of batch after batch.  Owned by the engine, not by a load: free_all leaves the
    // history alone, only tw_history_reset and tw_destroy end it.  side[cur] holds it; a push merges into the other side and swaps.
    struct HistSide {
        int64_t* values = nullptr; int64_t cap = 0;                       // items
        int64_t* off = nullptr; unsigned long long *count = nullptr, *sum = nullptr; int64_t seg_cap = 0;
    } hist_side[2];
    int hist_cur = 0;
    int32_t hist_C = 0, hist_G = 0;          // C_h; G, 0 = open (fixed by the first push or merge after a reset)
    int64_t hist_items = 0, hist_pushes = 0;
    int64_t* hist_tile_off = nullptr; int32_t* hist_inv = nullptr; int64_t hist_plan_cap = 0 /* segments */, hist_inv_cap = 0;
    unsigned long long* hist_counters = nullptr;
    int64_t *hist_src_off = nullptr, *hist_src_values = nullptr; unsigned long long *hist_src_count = nullptr, *hist_src_sum = nullptr;
    int64_t hist_src_seg_cap = 0, hist_src_cap = 0;   // the uploaded source of tw_history_merge
    // tw_class_history_* (tw_chist.h): the call-graph classes of batch after batch.  Owned by the engine like the history: free_all
    // leaves the catalogue alone, only tw_class_history_reset and tw_destroy end it.  CH.C / CH.E: classes and entries held.
    ChistDev CH{};
    int32_t ch_mode = 0, ch_G = 0;          // G, 0 = empty (mode and G are fixed by the first push or merge after a reset)
    int64_t ch_pushes = 0, ch_src_cap = 0 /* source classes the scratch holds */;
    void* ch_up = nullptr; size_t ch_up_bytes = 0;   // the uploaded source of tw_class_history_merge
    SigDev G{};                             // tw_trace_signatures (tw_sig.h); sig_ready: the result of sig_q on the forest is resident, a further
    bool sig_ready = false, ref_set = false;        // call with the same query only copies; ref_set: the reference set, keyed by root row
    tw_sig_query sig_q{};
    int32_t ref_mode = 0;
    int64_t sig_rows_cap = 0, sig_trees_cap = 0, sig_ent_cap = 0, sig_ref_cap = 0, sig_summary[6] = {0, 0, 0, 0, 0, 0};
    ProfDev F{};                            // tw_class_profiles (tw_prof.h); prof_ready: the profile of the resident signature result and the
    bool prof_ready = false;                // resident attribution is resident, a further call only copies
    int64_t prof_ent_cap = 0, prof_cls_cap = 0, prof_rows_cap = 0, prof_summary[6] = {0, 0, 0, 0, 0, 0};
    FiltDev FL{};                           // tw_filter_traces (tw_filt.h): scratch of a call; what outlives it is bit TW_TREE_MATCH of S.tree_flags
    int64_t filt_trees_cap = 0, filt_val_cap = 0;
    ExtrDev X{};                            // tw_extract_traces / tw_get_extracted (tw_extr.h); extr_ready: the result (copies in buffers of
    bool extr_ready = false, extr_times = false;   // its own) is resident, extr_times: with the self and path times of an attribution
    int64_t extr_sort_cap = 0, extr_sel_cap = 0, extr_rows_cap = 0, extr_pos_cap = 0, extr_sel = 0, extr_rows = 0;
    // HIP events around the parts of a stage (SE_*: a stage's first event; created by tw_create) and what tw_get_timing reports of them
    hipEvent_t stage_ev[SE_COUNT] = {};
    double st_ms[6] = {0, 0, 0, 0, 0, 0};   // whole call on the device, links, jump rounds, count + scan + scatter, group + figures; [5] = rounds
    double at_ms[3] = {0, 0, 0};            // per-tree kernel, selection (flags, sort, mark), group reduction
    double cf_ms[3] = {0, 0, 0};            // decision kernel, row map + per-tree reduction, calibration
    double ds_ms[3] = {0, 0, 0};            // items and counts; sort, offsets and values; quantiles and histogram
    double sg_ms[3] = {0, 0, 0};            // items and levels; sort, run lengths and hash; classes, comparison and per-class reduction
    double pf_ms[3] = {0, 0, 0};            // the sweep over the rows; the per-tree and per-class pass; the copies
    double fl_ms[3] = {0, 0, 0};            // trace filter: the tree kernel; the list of the matched trees; the copies
    double ex_ms[3] = {0, 0, 0};            // extraction: selection, sizes and offsets; the tree kernel; the copies of tw_get_extracted
    double cm_ms[2] = {0, 0};               // ranks, pool and observed statistics; the permutation walk
    double hs_ms[5] = {0, 0, 0, 0, 0};      // history: plan (with the source check of a merge), merge; quantiles and histogram; observed statistics, permutation walk
    double ch_ms[3] = {0, 0, 0};            // class catalogue: hash and lookup; scan, append, insert and any rehash; accumulate
    double host_ms[2] = {0, 0};             // host wall clock of the last pass: submitting the first enumeration / the whole tw_run_pass call
    // tw_order_stage / tw_order_load (tw_order.h): the span table of a batch in partition-key order, staged once, and the buffers a
    // candidate's permuted copy is gathered into before tw_load_batch takes it device to device.  Owned by the engine, not by a
    // load: free_all leaves them alone, tw_order_stage replaces them, tw_destroy frees them.
    int64_t* ord_stage[4] = {};             // in_start, in_end, out_start, out_end as staged
    int64_t* ord_gather[4] = {};            // ... of the units of the last tw_order_load, endpoints in topological order
    int64_t* ord_seg = nullptr;             // segment descriptors of k_order_gather: src, dst, len [ord_seg_cap each]
    int64_t ord_seg_cap = 0;
    bool ord_staged = false;
    std::vector<int64_t> ord_in_off, ord_ep_off, ord_ep_base;
    std::vector<int32_t> ord_E;
    int32_t ord_batch_size = 0, ord_batch_mis = 0;
    double ob_ms = 0;                       // the last k_order_bound (HIP events)
};

namespace {

int fail(tw_engine* e, int code, const std::string& msg) {
    e->err = msg;
    return code;
}

#define HIPCHK(call)                                                                               \
    do {                                                                                           \
        hipError_t _s = (call);                                                                    \
        if (_s != hipSuccess)                                                                      \
            return fail(e, TW_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(_s));      \
    } while (0)

#define TWCHK(call)                                                                                \
    do {                                                                                           \
        const int _rc = (call);                                                                    \
        if (_rc != TW_OK) return _rc;                                                              \
    } while (0)

template <class T>
int dev_alloc(tw_engine* e, T** p, int64_t count) {
    const size_t bytes = (size_t)std::max<int64_t>(count, 1) * sizeof(T);
    if (e->arena_open) {  // tw_load_batch: collected, placed by arena_commit
        *p = nullptr;
        e->arena_req.emplace_back([p](void* q) { *p = (T*)q; }, (bytes + 255) / 256 * 256);
        return TW_OK;
    }
    void* q = nullptr;
    HIPCHK(hipMalloc(&q, bytes));
    e->allocs.push_back(q);
    *p = (T*)q;
    return TW_OK;
}

#define DEV_ALLOC(ptr, count) TWCHK(dev_alloc(e, &(ptr), (count)))

int ensure_sort_tmp(tw_engine* e, size_t bytes) {
    if (bytes > e->sort_tmp_bytes) {
        void* q = nullptr;
        HIPCHK(hipMalloc(&q, bytes));
        e->allocs.push_back(q);
        e->sort_tmp = q;
        e->sort_tmp_bytes = bytes;
    }
    return TW_OK;
}

// rocprim's two-step call: call(nullptr, bytes) asks for the size of the temporary, call(e->sort_tmp, bytes) runs.  `at_least`: room
// that a call right after this one needs (the temporary grows before this one is queued, not between the two).
template <class F>
int rocprim_call(tw_engine* e, F call, size_t at_least = 0) {
    size_t bytes = 0;
    HIPCHK(call(nullptr, bytes));
    TWCHK(ensure_sort_tmp(e, std::max(bytes, at_least)));
    bytes = e->sort_tmp_bytes;
    HIPCHK(call(e->sort_tmp, bytes));
    return TW_OK;
}

// an output array the caller may leave out: `count` elements of the device array `src` (queued on the engine's stream)
template <class T, class U>
int copy_out(tw_engine* e, T* dst, const U* src, size_t count) {
    static_assert(sizeof(T) == sizeof(U), "copy_out: the host and the device array differ in element size");
    if (dst != nullptr) HIPCHK(hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyDeviceToHost, e->stream));
    return TW_OK;
}

// launch shapes.  Flat kernels: a thread per item, workgroups of 256.  Persistent wavefronts that take `per_wave` items at a time:
// workgroups of `waves` wavefronts, at most 8192 of them.  (TW_COOP_THREADS < 64, the emulation of the tests: that many threads.)
unsigned flat_threads(const tw_engine* e) { return (unsigned)(e->K.coop >= 64 ? 256 : e->K.coop); }
unsigned flat_grid(int64_t n, unsigned threads) { return (unsigned)((n + threads - 1) / threads); }
struct WaveShape { dim3 grid, block; };
WaveShape wave_shape(const tw_engine* e, int64_t n, int per_wave, int waves) {
    const int64_t want = (n / per_wave + 1 + waves - 1) / waves;
    return WaveShape{dim3((unsigned)std::min<int64_t>(want, 8192)), dim3(e->K.coop >= 64 ? 64u * (unsigned)waves : (unsigned)e->K.coop)};
}

// stage events: milliseconds between events a and b of the stage whose first event is `stage` (SE_*)
int stage_elapsed(tw_engine* e, int stage, int a, int b, double* ms) {
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, e->stage_ev[stage + a], e->stage_ev[stage + b]));
    *ms = f;
    return TW_OK;
}

/* ---- residency of the trace stages -----------------------------------------------------------------------------------
   What the engine holds beyond the batch and the results of a pass, what each item needs (<-) and what drops it besides the
   items it needs.  Dropping an item drops everything that needs it: the functions below are the only code that clears a flag,
   so a flag is set only while everything it needs is set, and a consumer tests the items it reads directly.

     row maps         rows_set       tw_set_span_rows     <- the loaded batch.  Dropped by a load and by tw_scale_load (the lists
                                                             are re-sorted: the caller permutes the maps and sets them again)
     given parents    parents_given  tw_set_parents       <- the loaded batch.  Dropped like the row maps
     row groups       groups_set     tw_set_row_groups    <- row maps
     cohort labels    cohorts_set    tw_set_row_cohorts   <- row maps.  Not set = one cohort that holds every tree
     reference set    ref_set        tw_trace_signatures  <- row maps, row groups (keyed by root row: it survives a new stitch)
     forest           stitched       tw_stitch_traces     <- row maps and the parent arrays it was made from.  Dropped by a new pass
                                                             (it overwrites them) and by a new stitch
     attribution      attributed     tw_attribute_traces  <- forest, row groups
     distribution     dist_ready     tw_latency_distributions <- attribution, the cohort labels as they are (set or not)
       items
     signature        sig_ready      tw_trace_signatures  <- forest, row groups.  Dropped by tw_score_traces (it rewrites the CONFIDENT
       result                                                bit that a query may select by) and by a call with another query
     class profile    prof_ready     tw_class_profiles    <- signature result, attribution
     match bit        (bit 4 of the    tw_filter_traces     <- forest, row groups: it lives in the forest's tree_flags and goes with the
                      forest's flags)                          forest (a new stitch writes new flags without it).  A call rewrites it
                                                             for every tree, after it has read what its clauses name, and then drops
                                                             the attribution and the signature result where the query they were made
                                                             with named the bit (need_flags | skip_flags & 16): a result whose query
                                                             does not name the bit cannot depend on it and stays
     extracted        extr_ready     tw_extract_traces    <- forest.  Copies in buffers of its own: it answers the query as the flags, the
       traces                                                 row groups and the attribution stood, so tw_filter_traces, tw_score_traces,
                                                             new row groups and a new attribution leave it; another extraction
                                                             replaces it
     history          hist_C > 0     tw_history_push / tw_history_merge <- nothing: it holds copies.  Dropped by tw_history_reset and
                                                             tw_destroy only (its buffers are not a load's: free_all leaves them)
     class catalogue  ch_G > 0       tw_class_history_push / tw_class_history_merge <- nothing: it holds copies.  Dropped by
                                                             tw_class_history_reset and tw_destroy only (buffers of its own, as the
                                                             history's; no drop_* function touches it)
   An API function drops what it is about to replace with one call, before it overwrites anything, and sets its own flag last, when
   everything has succeeded (tw_trace_signatures owns two items: its result and, with keep_reference, the reference set). */
void drop_dist(tw_engine* e) { e->dist_ready = false; }
void drop_prof(tw_engine* e) { e->prof_ready = false; }
void drop_sig(tw_engine* e) { e->sig_ready = false; drop_prof(e); }
void drop_ref(tw_engine* e) { e->ref_set = false; }
void drop_attribution(tw_engine* e) { e->attributed = false; drop_dist(e); drop_prof(e); }
void drop_extr(tw_engine* e) { e->extr_ready = false; }
void drop_forest(tw_engine* e) { e->stitched = false; drop_attribution(e); drop_sig(e); drop_extr(e); }
void drop_groups(tw_engine* e) { e->groups_set = false; drop_attribution(e); drop_sig(e); drop_ref(e); }
void drop_cohorts(tw_engine* e) { e->cohorts_set = false; drop_dist(e); }
void drop_rows(tw_engine* e) { e->rows_set = false; drop_forest(e); drop_groups(e); drop_cohorts(e); }
void drop_batch_order(tw_engine* e) { drop_rows(e); e->parents_given = false; }   // a load, tw_scale_load: whatever names spans by position
// ... and a load frees every buffer with the batch (free_all): the arrays and what was known of their sizes go with the flags
void drop_buffers(tw_engine* e) {
    drop_batch_order(e);
    e->S = StitchDev{}; e->rows_cap = 0; e->given_parent = nullptr;                                    // row maps, forest, given parents
    e->A = AttrDev{}; e->groups_cap = 0; e->attr_rows_cap = 0;                                         // row groups, attribution
    e->C = ConfDev{}; e->conf_rows_cap = 0;                                                            // decisions, confidence
    e->D = DistDev{}; e->cohort_rows_cap = 0; e->dist_trees_cap = 0; e->dist_seg_cap = 0; e->dist_out_cap = 0; e->dist_items = 0;   // cohort labels, items
    e->G = SigDev{}; e->sig_rows_cap = 0; e->sig_trees_cap = 0; e->sig_ent_cap = 0; e->sig_ref_cap = 0;   // signatures, reference set
    e->F = ProfDev{}; e->prof_ent_cap = 0; e->prof_cls_cap = 0; e->prof_rows_cap = 0;                  // class profile
    e->FL = FiltDev{}; e->filt_trees_cap = 0; e->filt_val_cap = 0;                                     // scratch of the trace filter
    e->X = ExtrDev{}; e->extr_sort_cap = 0; e->extr_sel_cap = 0; e->extr_rows_cap = 0; e->extr_pos_cap = 0;   // extracted traces and their scratch
    e->M = CmpDev{}; e->cmp_rows_cap = 0; e->cmp_items_cap = 0;                                        // scratch of the cohort comparison
}

bool pass_resident(const tw_engine* e, int pass) {
    return (pass == 1 && (e->state == ST_PASS1 || e->state == ST_MIX)) || (pass == 2 && e->state == ST_PASS2);
}

// what the consumers of the forest say when there is none
int need_forest(tw_engine* e, const char* fn) {
    if (e->stitched) return TW_OK;
    return fail(e, TW_ERR_STATE, std::string(fn) + " needs the forest of a tw_stitch_traces call (a load, tw_scale_load, new row maps and a new pass drop it)");
}

int ensure_class_stream(tw_engine* e, int E) {
    if (e->cls_stream[E] != nullptr) return TW_OK;
    HIPCHK(hipStreamCreate(&e->cls_stream[E]));
    return TW_OK;
}

int arena_commit(tw_engine* e) {
    e->arena_open = false;
    size_t total = 0;
    for (const auto& r : e->arena_req) total += r.second;
    if (total > e->arena_cap) {
        if (e->arena != nullptr) (void)hipFree(e->arena);
        e->arena = nullptr;
        e->arena_cap = 0;
        HIPCHK(hipMalloc(&e->arena, total));
        e->arena_cap = total;
    }
    size_t off = 0;
    for (const auto& r : e->arena_req) { r.first((char*)e->arena + off); off += r.second; }
    e->arena_req.clear();
    return TW_OK;
}

void order_unstage(tw_engine* e) {   // (the staged table of tw_order_stage: not a load's, free_all leaves it alone)
    for (int k = 0; k < 4; k++) {
        if (e->ord_stage[k]) (void)hipFree(e->ord_stage[k]);
        if (e->ord_gather[k]) (void)hipFree(e->ord_gather[k]);
        e->ord_stage[k] = e->ord_gather[k] = nullptr;
    }
    if (e->ord_seg) (void)hipFree(e->ord_seg);
    e->ord_seg = nullptr; e->ord_seg_cap = 0; e->ord_staged = false;
}

void hist_free(tw_engine* e) {   // (the history of tw_history_*: not a load's, free_all leaves it alone)
    for (auto& side : e->hist_side) {
        if (side.values) (void)hipFree(side.values);
        if (side.off) (void)hipFree(side.off);
        if (side.count) (void)hipFree(side.count);
        if (side.sum) (void)hipFree(side.sum);
        side = tw_engine::HistSide{};
    }
    void* rest[] = {e->hist_tile_off, e->hist_inv, e->hist_counters, e->hist_src_off, e->hist_src_values, e->hist_src_count, e->hist_src_sum};
    for (void* q : rest)
        if (q) (void)hipFree(q);
    e->hist_tile_off = nullptr; e->hist_inv = nullptr; e->hist_counters = nullptr; e->hist_plan_cap = 0; e->hist_inv_cap = 0;
    e->hist_src_off = e->hist_src_values = nullptr; e->hist_src_count = e->hist_src_sum = nullptr; e->hist_src_seg_cap = 0; e->hist_src_cap = 0;
    e->hist_cur = 0; e->hist_C = 0; e->hist_G = 0; e->hist_items = 0; e->hist_pushes = 0;
}

void chist_free(tw_engine* e) {   // (the catalogue of tw_class_history_*: not a load's, free_all leaves it alone)
    ChistDev& H = e->CH;
    void* all[] = {H.table, H.off, H.entries, H.hash, H.stamp, H.cls, H.cell, H.src_hash, H.src_id, H.new_src, H.chunk_sum, H.counters, e->ch_up};
    for (void* q : all)
        if (q) (void)hipFree(q);
    H = ChistDev{};
    e->ch_mode = 0; e->ch_G = 0; e->ch_pushes = 0; e->ch_src_cap = 0; e->ch_up = nullptr; e->ch_up_bytes = 0;
}

void free_all(tw_engine* e) {
    for (void* q : e->allocs) (void)hipFree(q);
    e->allocs.clear();
    e->orig_is = e->orig_ie = e->orig_os = e->orig_oe = nullptr; e->orig_truth = e->orig_trace = nullptr;
    e->truth = nullptr; e->in_trace = nullptr; e->trace_bad = nullptr; e->eval_counts = nullptr; e->n_traces = 0; e->trace_cap = 0;
    drop_buffers(e);
    e->state = ST_EMPTY;
}

const char* kernel_error_text(int code) {
    switch (code) {
        case TW_ERR_WINDOW_WIDTH: return "an incoming span has more candidate spans at one endpoint than the candidate bitmap holds";
        case TW_ERR_WINDOW_SIZE: return "a window holds more than TW_MAX_WINDOW incoming spans";
        case TW_ERR_NAN_PARAMS: return "a parameter block holds a single sample (std = NaN); the reference aborts here (n_in % 100 == 1)";
        case TW_ERR_SKIP_PARAMS: return "skip mode: the scorer needs a (mean, std) pair that BuildDistributions did not produce (the reference raises KeyError)";
        case TW_ERR_SKIP_REFERENCE_RAISES: return "skip mode: the reference raises on this input (all endpoints skipped, or a score tie compared through a skip span)";
        case TW_ERR_ARG: return "skip mode: a request starts before the first time window";
        default: return "kernel reported an error";
    }
}

// (S: all tiles or the tiles of one endpoint-count class, TileSet in tw_device.h)
template <class Tr>
int run_scan(tw_engine* e, const TileSet& S, hipStream_t st, typename Tr::T* agg) {
    const Dev& P = e->P;
    hipLaunchKernelGGL((k_scan_local<Tr>), dim3(S.n), dim3(e->K.tile), 0, st, P, S, agg);
    hipLaunchKernelGGL((k_scan_spine<Tr>), dim3(P.n_units), dim3(e->K.coop), 0, st, P, S, agg);
    hipLaunchKernelGGL((k_scan_fix<Tr>), dim3(S.n), dim3(e->K.tile), 0, st, P, S, agg);
    HIPCHK(hipGetLastError());
    return TW_OK;
}

TileSet all_tiles_host(const tw_engine* e) { return TileSet{nullptr, 0, e->P.n_tiles, 0}; }
TileSet class_tiles(const tw_engine* e, int E) { return TileSet{e->tile_ids + e->tile_cls_off[E], e->tile_cls_off[E], e->tile_cls_off[E + 1] - e->tile_cls_off[E], E}; }

// (no-skip batches: every endpoint list holds one span per incoming span, all lists sorted by (start, end))
int sort_ends(tw_engine* e, const TileSet& S, hipStream_t st) {   // (the counters e->rank_in / rank_out zeroed by the caller)
    const Dev& P = e->P;
    const dim3 tiles(S.n), tb(e->K.tile);
    hipLaunchKernelGGL(k_rank_ends, tiles, tb, 0, st, P, S, e->rank_in, e->rank_out);
    hipLaunchKernelGGL(k_place_ends, tiles, tb, 0, st, P, S, (const int32_t*)e->rank_in, (const int32_t*)e->rank_out);
    HIPCHK(hipGetLastError());
    return TW_OK;
}

// ComputeEpPairDistParams3 behind sort_ends: the blocks of every unit (cls = 0) or of the units of one endpoint-count class
void launch_block_params(tw_engine* e, int cls, hipStream_t st) {
    const Dev& P = e->P;
    if (e->K.block_params == 0) {
        const int64_t total = e->n_gp;
        hipLaunchKernelGGL(k_block_params, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, P, total, cls);
        return;
    }
    const int n = e->blk_cls_off[cls + 1] - e->blk_cls_off[cls];
    if (n <= 0) return;
    const int threads = e->K.coop >= 64 ? 64 * std::min(e->K.coop / 64, kParamWaves) : e->K.coop, waves = std::max(threads / 64, 1);
    hipLaunchKernelGGL(k_block_params_wave, dim3((unsigned)((n + waves - 1) / waves)), dim3(threads), 0, st, P, (const BlockRef*)(e->blk_tab + e->blk_cls_off[cls]), n);
}

// mode 0: first solve on all spans (per-thread kernel, then the wavefront kernel for the spans it deferred);
// mode 1: the spans listed by k_detect_gone, without the candidate spans earlier windows took
// The classes (units of one endpoint count) are independent of one another and every class' kernels end in a long tail
// (work per span spans four orders of magnitude): each class runs on a stream of its own, forked from and joined to the
// engine's stream by events, so that the tails overlap.  The wide instantiation of a class owns the big-list pool slots
// together with the narrow one (one counter): no conflict, they only ever add.
// Extra work-list entries of a class for the parts of its split enumerations.  Up to four endpoints few spans are split (an eighth of
// the class + 64 was never short); in the deep call graphs most wavefront-enumerated spans are, and a budget that runs out leaves
// whichever spans come last unsplit -- single wavefronts then hold the class' kernel for milliseconds (round 5: 3 of its 4 ms).
// One-endpoint classes never split: no budget.
int64_t part_extra(const tw_engine* e, int cls, int64_t n_cls) {
    if (n_cls <= 0) return 0;
    if (cls <= 1) return 64;
    const int deep = e->K.part_budget_deep;
    return (cls >= 5 && deep > 0 ? n_cls * deep : n_cls / 8) + 64;
}

constexpr int pair_pool(int E) { return E > 4 ? 2048 : (E > 1 ? kPairPoolPerEp * E : 1); }   // doubles of pair-term tables per wavefront of k_enumerate_heavy<E>

// `listed` (mode 1 only): the class' entries of heavy_in_count as the host read them with the round's change count -- a class, or an
// instantiation, with nothing listed is not launched at all.
// The whole chain of a class on the class' stream: tile kernel, wavefront kernels (k_enumerate_heavy<E>; from lean_min_e endpoints on
// k_enumerate_lean), k_merge_parts.  (k_enumerate_lean and k_merge_parts can serve several classes in one launch; measured on the
// Alibaba-shape slice, one launch per phase for the four deep classes: 2.5 ms per pass instead of 1.9 -- the phases of different classes
// no longer overlap, and every phase ends with its longest item.)
template <int E>
void launch_enumerate(tw_engine* e, int pass, int mode, const int32_t* listed) {
    const int nt = e->tile_cls_off[E + 1] - e->tile_cls_off[E];
    if (nt == 0) return;
    // (-1: not known.  The first enumeration of pass 2 lists the spans pass 1 listed: a class without wide windows then has none now)
    const int n_narrow = listed != nullptr ? listed[E] : -1, n_wide = listed != nullptr ? listed[kMaxEp + 1 + E] : ((pass == 2 && mode == 0 && e->wide_pass1[E] == 0) ? 0 : -1);
    if (n_narrow == 0 && n_wide == 0) return;
    hipStream_t st = e->cls_stream[E];
    (void)hipStreamWaitEvent(st, e->cls_ev[0], 0);
    const Dev& P = e->P;
    const dim3 hb(std::min(e->K.coop, kHeavyThreads));
    constexpr int pool = pair_pool(E);
    const size_t pool_bytes = sizeof(double) * (size_t)pool;
    // (k_enumerate_lean: root / closing term tables + an LDS pool of pair tables for the common case, larger pair tables in global memory)
    const size_t lean_bytes = sizeof(double) * (size_t)(2 * kMaxEp * kNarrow + e->K.lean_pool), lean_bytes_w = sizeof(double) * (size_t)(2 * kMaxEp * 64 * kCandWords + e->K.lean_pool);
    const bool lean = E >= P.lean_min_e && !e->skip_mode;   // the deep call graphs: k_enumerate_lean; what it hands on to k_enumerate_heavy is launched by launch_enumerate_all
    const int cap = P.heavy_in_off[E + 1] - P.heavy_in_off[E];
    auto grid_for = [&](int known, int most) { return std::max(std::min(((known >= 0 ? known : cap) + kWorkChunk - 1) / kWorkChunk, most), 1); };   // persistent wavefronts pulling spans from the work list
    auto narrow = [&](int part, int g) {
        if (lean) hipLaunchKernelGGL((k_enumerate_lean<kNarrow>), dim3(g), hb, lean_bytes, st, P, pass, mode, part, e->K.lean_pool, E, E);
        else hipLaunchKernelGGL((k_enumerate_heavy<E, kNarrow>), dim3(g), hb, pool_bytes, st, P, pass, mode, part, pool);
    };
    auto wide = [&](int part, int g) {
        if (lean) hipLaunchKernelGGL((k_enumerate_lean<64 * kCandWords>), dim3(g), hb, lean_bytes_w, st, P, pass, mode, part, e->K.lean_pool, E, E);
        else hipLaunchKernelGGL((k_enumerate_heavy<E, 64 * kCandWords>), dim3(g), hb, pool_bytes, st, P, pass, mode, part, pool);
    };
    if (mode == 0 && pass == 1 && e->class_params) {   // the class' sorted end times and block parameters (run_pass)
        const TileSet S = class_tiles(e, E);
        (void)sort_ends(e, S, st);
        launch_block_params(e, E, st);
    }
    if (mode == 0) {
        // cut-offs and work lists, the short enumerations: the tile kernel.  A class of few tiles: several workgroups per tile, until
        // the class fills the CUs twice over
        const bool single = E == 1 && e->K.tile_single != 0;
        const bool pair = E == 2 && e->K.tile_pair != 0;
        const dim3 tile_block(e->K.tile >= 64 ? e->K.tile * (single ? e->K.tile_single_threads : (pair ? e->K.tile_pair_threads : e->K.tile_threads)) : e->K.tile);
        int sub = 1;
        while (sub < e->K.tile_sub && nt * sub < 512 && (e->K.tile / (sub * 2)) * (sub * 2) == e->K.tile && e->K.tile / (sub * 2) >= 8) sub *= 2;
        const bool sub_tile = e->K.tile == kTile && e->K.tile / sub == kSubTileSpans;   // (the instantiation with tables for a sub-tile's 16 spans: a third of the LDS)
        auto tile = [&](auto spans, auto lean_single, auto lean_pair) {
            hipLaunchKernelGGL((k_enumerate_tile<E, decltype(spans)::value, decltype(lean_single)::value, decltype(lean_pair)::value>), dim3(nt * sub), tile_block, 0, st,
                               P, pass, (const int32_t*)(e->tile_ids + e->tile_cls_off[E]), nt, sub);
        };
        auto tile_path = [&](auto spans) {   // (the lean paths: instantiated for one and for two endpoints only)
            if constexpr (E == 1) { if (single) return tile(spans, std::true_type{}, std::false_type{}); }
            if constexpr (E == 2) { if (pair) return tile(spans, std::false_type{}, std::true_type{}); }
            tile(spans, std::false_type{}, std::false_type{});
        };
        if (sub_tile) tile_path(std::integral_constant<int, kSubTileSpans>{});
        else tile_path(std::integral_constant<int, kTile>{});
        if (E == e->gate_cls) (void)hipEventRecord(e->tile_done, st);   // (who waits for it: launch_class_stage of the other classes, queued after every class' chain)
    }
    // the wavefront kernels of the class: the spans the tile kernel handed over (mode 1: the spans k_detect_gone listed), the long
    // enumerations first; the list parts of the spans those launches deferred (kListSplitFlag); the parts combined, the few spans whose
    // order of equal scores the parts left undecided enumerated whole.  Every launch of the chain has a work-list cursor of its own
    // (enum_cursor): nothing is reset in between.
    if (n_narrow != 0) narrow(0, grid_for(n_narrow, kHeavyGrid));
    if (n_wide != 0) wide(0, grid_for(n_wide, 1024));
    if (mode == 0 && E >= 3 && E >= P.defer_min_e) { narrow(3, grid_for(-1, 4096)); if (n_wide != 0) wide(3, grid_for(-1, 1024)); }
    if (mode == 0 && E > 1) {
        // (34 KB of LDS a workgroup: a thousand of them ask for all there is -- and wait for it while the selection kernels of other
        // classes hold the CUs' LDS: the launch for the two-endpoint class of the nodejs shape at 14.4 M spans, which has nothing to merge,
        // lasted 0.9-2.3 ms.  Pass 2 cuts the same spans as pass 1 -- the cuts follow the candidates' containment and the tuple counts --:
        // its launch is sized by pass 1's count; the workgroups stride over the records, so a wrong guess only costs time)
        const int nsplit = (pass == 2 && mode == 0) ? e->split_pass1[E] : -1;
        const int merge_grid = nsplit < 0 ? (cap >= (1 << 20) ? 1024 : 256) : std::max(std::min(nsplit, 1024), 8);
        hipLaunchKernelGGL(k_merge_parts, dim3(merge_grid), dim3(std::min(e->K.coop, 64)), 0, st, P, pass, E, E);
        narrow(1, nsplit == 0 ? 8 : 256); if (n_wide != 0) wide(1, nsplit == 0 ? 8 : 64);
    }
    if (e->K.debug_lists != 0 && mode == 0) {
        (void)hipMemcpyAsync(&e->first_lists[0][E], P.heavy_in_count + E, sizeof(int32_t), hipMemcpyDeviceToHost, st);
        (void)hipMemcpyAsync(&e->first_lists[1][E], P.heavy_in_count + kMaxEp + 1 + E, sizeof(int32_t), hipMemcpyDeviceToHost, st);
        (void)hipMemcpyAsync(&e->first_lists[2][E], P.heavy_big_count + E, sizeof(int32_t), hipMemcpyDeviceToHost, st);
    }
    (void)hipEventRecord(e->cls_ev[E], st);   // (who waits for it: launch_enumerate_all)
}

// What k_enumerate_lean handed on (whole spans only: P.fb_*), class by class, by k_enumerate_heavy (part 4).  Rare at scale, and a launch
// of that kernel -- 256 + 256 registers for eight endpoints: it needs a SIMD to itself -- waits for one even when its list is empty: the
// host reads the counts (one small copy, the enumeration has to be complete anyway) and launches only what has entries.
template <int E>
void launch_fallback(tw_engine* e, int pass, int mode, const int32_t* fb) {
    if (fb[E] <= 0) return;
    hipStream_t st = e->cls_stream[E];
    (void)hipStreamWaitEvent(st, e->cls_ev[0], 0);
    const dim3 hb(std::min(e->K.coop, kHeavyThreads));
    constexpr int pool = pair_pool(E);
    const int grid = std::max(std::min((fb[E] + kWorkChunk - 1) / kWorkChunk, 1024), 1);
    hipLaunchKernelGGL((k_enumerate_heavy<E, kNarrow>), dim3(grid), hb, sizeof(double) * (size_t)pool, st, e->P, pass, mode, 4, pool);
    hipLaunchKernelGGL((k_enumerate_heavy<E, 64 * kCandWords>), dim3(grid), hb, sizeof(double) * (size_t)pool, st, e->P, pass, mode, 4, pool);
    (void)hipEventRecord(e->cls_ev[E], st);
}


// CreateWindows2 + PerfectCut (traceweaver_v3.py:1020-1078) over the tiles of S on stream st: needs the candidate sets of S's spans.
// (the running maximum of the request ends -- PerfectCut's prev_index -- depends on the spans alone: run_pass computes it over all
// tiles on the engine's stream beside the enumerations.  The rest in five launches, k_cut_scan .. k_index_fix in tw_kernels.h)
int launch_windows(tw_engine* e, const TileSet& S, hipStream_t st) {
    const Dev& P = e->P;
    const dim3 tiles(S.n), tb(e->K.tile);
    hipLaunchKernelGGL(k_cut_scan, tiles, tb, 0, st, P, S, e->agg_i32);
    hipLaunchKernelGGL((k_scan_spine<ScanSegStart>), dim3(P.n_units), dim3(e->K.coop), 0, st, P, S, e->agg_i32);
    hipLaunchKernelGGL(k_flags_scan, tiles, tb, 0, st, P, S, (const int32_t*)e->agg_i32, e->agg_i32b);
    hipLaunchKernelGGL((k_scan_spine<ScanWinId>), dim3(P.n_units), dim3(e->K.coop), 0, st, P, S, e->agg_i32b);
    hipLaunchKernelGGL(k_index_fix, tiles, tb, 0, st, P, S, (const int32_t*)e->agg_i32b);
    HIPCHK(hipGetLastError());
    return TW_OK;
}

// The listed windows of the tile set S: those of up to kBruteMax spans (nearly all of them) by k_select_tiny, whose workgroups hold 1 KB
// of LDS and fill the SIMDs, on stream st; the middle ones (up to kBigWindow - 1 spans: one-word masks, 7 KB) and the long ones (22 KB:
// seven wavefronts per CU, ends with its longest search) by the instantiations of k_select_heavy -- each on a stream of its own,
// forked from and joined to st by events, so that the many short windows run beside the long searches' tail instead of before it.
// What the searches give up on goes to one list for k_select_dp (the caller launches it when every set has joined).
// (fork = false: everything on st, one after the other -- the stages of the classes that end before the last one have the time, and the
// three selection streams stay free for the class whose stage ends the pass)
// the three instantiations of k_select_heavy with room for EMAX endpoints per candidate (SelectLdsT: what a workgroup holds in LDS decides
// how many windows the GPU searches at a time)
// Persistent workgroups of one wavefront each, as many as the CUs hold at a time by the layout's LDS (the window's data + the small tables
// of the level solver): 2 800 / 4 300 / 6 100 for the three layouts of a two-endpoint class.  (One figure for all three, 4 096, left the
// small layouts short of wavefronts and gave the large one a second round: nodejs shape at 14.4 M spans 40.9 -> 39.2 ms with 6 144, 41.4
// with 8 192.)
template <class LDS>
unsigned select_heavy_grid(const tw_engine* e, dim3 most) {
    const size_t lds = sizeof(LDS) + sizeof(SelectDpT<LDS::kW, kDpCapSmall, kDpSlotsSmall>) + 512;
    const unsigned resident = 256u * (unsigned)std::max<size_t>((160u * 1024u) / lds, 1);
    return std::max(std::min(most.x, std::min(resident, 8192u)), 1u);
}
template <int EMAX>
void launch_select_heavy3(tw_engine* e, const TileSet& S, dim3 most, dim3 wave, hipStream_t s0, hipStream_t s1, hipStream_t s2) {
    hipLaunchKernelGGL((k_select_heavy<SelectLdsLvlE<EMAX>, 3>), dim3(select_heavy_grid<SelectLdsLvlE<EMAX>>(e, most)), wave, 0, s0, e->P, S);      // the longest searches first
    hipLaunchKernelGGL((k_select_heavy<SelectLdsBigLvlE<EMAX>, 1>), dim3(select_heavy_grid<SelectLdsBigLvlE<EMAX>>(e, most)), wave, 0, s1, e->P, S);
    hipLaunchKernelGGL((k_select_heavy<SelectLdsMidLvlE<EMAX>, 2>), dim3(select_heavy_grid<SelectLdsMidLvlE<EMAX>>(e, most)), wave, 0, s2, e->P, S);
}
void launch_select_heavy3(tw_engine* e, const TileSet& S, dim3 most, dim3 wave, hipStream_t s0, hipStream_t s1, hipStream_t s2) {
    int emax = S.slot;   // a class' tile set: its endpoint count; all tiles: the batch's largest
    if (emax == 0)
        for (int c = 1; c <= kMaxEp; c++) if (e->tile_cls_off[c + 1] > e->tile_cls_off[c]) emax = c;
    if (emax <= 2) launch_select_heavy3<2>(e, S, most, wave, s0, s1, s2);
    else if (emax <= 4) launch_select_heavy3<4>(e, S, most, wave, s0, s1, s2);
    else launch_select_heavy3<kMaxEp>(e, S, most, wave, s0, s1, s2);
}

void launch_select_listed(tw_engine* e, const TileSet& S, hipStream_t st, int64_t n_spans, bool fork = true) {
    const Dev& P = e->P;
    const dim3 wave(std::min(e->K.coop, 64));
    const dim3 grid((unsigned)std::min<int64_t>(n_spans / 2 + 1, 1 << 20));   // (what the set could need at most; launch_select_heavy3 sizes each layout's launch)
    if (!fork) {
        hipLaunchKernelGGL(k_select_tiny, dim3((unsigned)std::min<int64_t>(n_spans / 2 + 1, 8192)), wave, 0, st, P, S);
        launch_select_heavy3(e, S, grid, wave, st, st, st);
        return;
    }
    hipStream_t* ss = e->sel_stream;
    (void)hipEventRecord(e->post_fork[S.slot], st);
    for (int j = 0; j < 3; j++) (void)hipStreamWaitEvent(ss[j], e->post_fork[S.slot], 0);
    launch_select_heavy3(e, S, grid, wave, ss[0], ss[1], ss[2]);
    for (int j = 0; j < 3; j++) (void)hipEventRecord(e->post_join[S.slot][j], ss[j]);
    hipLaunchKernelGGL(k_select_tiny, dim3((unsigned)std::min<int64_t>(n_spans / 2 + 1, 8192)), wave, 0, st, P, S);
    for (int j = 0; j < 3; j++) (void)hipStreamWaitEvent(st, e->post_join[S.slot][j], 0);
}

// the windows the searches gave up on (kDpNodes), level by level over 256 lanes each; nothing listed: the workgroups leave at once
// (`few`: the set listed no such window in pass 1 -- pass 2 rarely differs, and 512 workgroups of 70 KB of LDS take 0.1-0.2 ms to come and
// go with nothing to do; the workgroups are persistent, a small grid is only slower when the guess is wrong)
void launch_select_hard(tw_engine* e, const TileSet& S, hipStream_t st, bool few = false) {
    hipLaunchKernelGGL(k_select_dp, dim3(few ? 32 : (kDpCap <= 384 ? 512 : 256)), dim3(std::min(e->K.coop, kDpThreads)), 0, st, e->P, S);   // (one / two workgroups per CU by their LDS)
}

// What follows a class' first enumeration, on the class' stream: its windows (pass 1), the first selection of its windows, the first
// round of the span consumption (claim, detect) and -- in anticipation of that round finding nothing to repair, the usual case --
// the parents and gap samples of its units (run_pass runs both again over all tiles when a repair round changed something).  Units
// of different classes are independent (traceweaver_v3.py:1182-1193 runs per service): nothing here waits for another class.
// The stage gate.  e->gate_cls (0 = no gate) is the class whose chain is the pass and whose tile kernel takes the general path of
// k_enumerate_tile (launch_enumerate_all).  That kernel fills every CU's LDS, four workgroups of 39 KB, and is bound by instruction
// issue: what runs beside it makes the pass longer, while behind it the machine runs that class' wavefront kernels and a stage of few
// wavefronts with room to spare.  The other classes therefore hold the persistent, LDS-sized part of their stage -- the listed and the
// hard windows, claim, detect -- until that tile kernel has ended; windows and k_select_fast, plain throughput kernels, run at once.
// (The wait is on an event of the critical class' stream that was recorded when the chains were queued: before this wait in
// submission order, so streams that share a hardware queue cannot wait on one another.)
int launch_class_stage(tw_engine* e, int pass, int E, int deepest) {
    const TileSet S = class_tiles(e, E);
    if (S.n == 0) return TW_OK;
    hipStream_t st = e->cls_stream[E];
    (void)hipStreamWaitEvent(st, e->prep_ev, 0);
    if (pass == 1) { int rc = launch_windows(e, S, st); if (rc != TW_OK) return rc; }
    hipLaunchKernelGGL(k_select_fast, dim3(S.n), dim3(e->K.tile), 0, st, e->P, S);
    if (e->gate_cls > 0 && E != e->gate_cls) { (void)hipStreamWaitEvent(st, e->tile_done, 0); e->gate_waits++; }
    const int64_t n_cls = (int64_t)e->P.heavy_in_off[E + 1] - e->P.heavy_in_off[E];
    launch_select_listed(e, S, st, n_cls, E == deepest);
    launch_select_hard(e, S, st, pass == 2 && e->hard_pass1[E] == 0);
    const dim3 tiles(S.n), tb(e->K.tile);
    hipLaunchKernelGGL(k_claim, tiles, tb, 0, st, e->P, S, E);
    hipLaunchKernelGGL(k_detect_gone, tiles, tb, 0, st, e->P, S, 0, pass == 1 ? 2 : 1);
    (void)hipEventRecord(e->post_done[E], st);
    return TW_OK;
}

// mode 0 with `staged`: every class goes on to its windows and first selection on its own stream (launch_class_stage); the engine's
// stream waits for the enumerations (EV_ENUM1: the group's timer), then for the stages.
template <class Prep>
int launch_enumerate_all(tw_engine* e, int pass, int mode, const int32_t* listed, bool staged, Prep prep) {
    // (the work-list cursors were reset with the counter block of the pass / the repair round)
    (void)hipEventRecord(e->cls_ev[0], e->stream);
    auto has = [&](int E) { return e->tile_cls_off[E + 1] > e->tile_cls_off[E]; };
    auto is_lean = [&](int E) { return E >= e->P.lean_min_e && !e->skip_mode; };
    int deepest = 0;
    for (int E = 1; E <= kMaxEp; E++) if (has(E)) deepest = E;
    // The stage gate's critical class: the deepest class of a staged batch (media shape: four endpoints), where the general path of the
    // tile kernel serves it.  Not where k_enumerate_lean does (Alibaba shape: the pass is as long as the deep classes' chains, whenever
    // the shallower tile kernels end), and not where the tile kernel takes one of its lean paths (nodejs shape: the pair path; the
    // single-endpoint services' stages are the longer part of the pass there and the gate serialises them -- profiles/HISTORY.md, round
    // 12).  Measured on those three shapes only: a deepest class of three endpoints, or of one or two with TW_TILE_SINGLE / TW_TILE_PAIR
    // = 0, is gated by the same reasoning, without a measurement of its own.
    e->gate_cls = 0;
    if (staged && e->K.stage_gate != 0 && !is_lean(deepest) && !(deepest == 1 && e->K.tile_single != 0) && !(deepest == 2 && e->K.tile_pair != 0)) e->gate_cls = deepest;
    if (mode == 0) e->gate_waits = 0;
    // the classes with the most endpoints first: their enumerations are the longest and end the group (each class runs on a
    // stream of its own; what is launched first is dispatched first)
    launch_enumerate<8>(e, pass, mode, listed); launch_enumerate<7>(e, pass, mode, listed); launch_enumerate<6>(e, pass, mode, listed); launch_enumerate<5>(e, pass, mode, listed);
    launch_enumerate<4>(e, pass, mode, listed); launch_enumerate<3>(e, pass, mode, listed); launch_enumerate<2>(e, pass, mode, listed); launch_enumerate<1>(e, pass, mode, listed);
    { int rc = prep(); if (rc != TW_OK) return rc; }   // (fills on the engine's stream, beside the enumerations)
    bool any_lean = false;
    for (int E = 1; E <= kMaxEp; E++) any_lean |= has(E) && is_lean(E);
    // the classes that are complete with their chain go on at once -- those expected to end first first (the selection streams serve
    // the classes in this order): the fewest endpoints
    if (staged)
        for (int E = 1; E <= kMaxEp; E++)
            if (has(E) && !is_lean(E)) { int rc = launch_class_stage(e, pass, E, deepest); if (rc != TW_OK) return rc; }
    if (any_lean) {
        // what k_enumerate_lean handed on: the host reads the counts when the lean classes' chains have ended
        int32_t fb[kMaxEp + 1] = {};
        int first_lean = 0;
        for (int E = kMaxEp; E >= 1; E--)
            if (has(E) && is_lean(E)) {
                if (listed == nullptr || listed[E] != 0 || listed[kMaxEp + 1 + E] != 0) HIPCHK(hipEventSynchronize(e->cls_ev[E]));
                first_lean = E;
            }
        HIPCHK(hipMemcpyAsync(fb, e->P.fb_count, sizeof(fb), hipMemcpyDeviceToHost, e->cls_stream[first_lean]));
        HIPCHK(hipStreamSynchronize(e->cls_stream[first_lean]));
        launch_fallback<8>(e, pass, mode, fb); launch_fallback<7>(e, pass, mode, fb); launch_fallback<6>(e, pass, mode, fb); launch_fallback<5>(e, pass, mode, fb);
        launch_fallback<4>(e, pass, mode, fb); launch_fallback<3>(e, pass, mode, fb); launch_fallback<2>(e, pass, mode, fb); launch_fallback<1>(e, pass, mode, fb);
        if (staged)
            for (int E = 1; E <= kMaxEp; E++)
                if (has(E) && is_lean(E)) { int rc = launch_class_stage(e, pass, E, deepest); if (rc != TW_OK) return rc; }   // (a batch with lean classes has no gate)
    }
    for (int E = 1; E <= kMaxEp; E++)
        if (has(E)) (void)hipStreamWaitEvent(e->stream, e->cls_ev[E], 0);
    HIPCHK(hipEventRecord(e->ev[EV_ENUM1], e->stream));
    if (staged) {
        HIPCHK(hipEventRecord(e->ev[EV_WIN], e->stream));   // (the windows are inside the class stages: what the timers show after this point is the part of the stages that outlasts the enumerations)
        for (int E = 1; E <= kMaxEp; E++)
            if (has(E)) (void)hipStreamWaitEvent(e->stream, e->post_done[E], 0);
    }
    return TW_OK;
}

// OR of (key ^ first key) and of the keys themselves over a set of index ranges (see k_key_bits)
int key_bits(tw_engine* e, const void* keys, const uint32_t* seg_begin, const uint32_t* seg_end, int nseg, int64_t total,
             unsigned long long out[2]) {
    out[0] = out[1] = 0;
    if (nseg <= 0 || total <= 0) return TW_OK;
    HIPCHK(hipMemsetAsync(e->key_acc, 0, 2 * sizeof(unsigned long long), e->stream));
    const int bx = (int)std::min<int64_t>(std::max<int64_t>(2048 / nseg, 1), total / nseg / 2048 + 1);  // ~2k workgroups at most
    hipLaunchKernelGGL(k_key_bits, dim3((unsigned)bx, (unsigned)std::min(nseg, 1024)), dim3(flat_threads(e)), 0, e->stream,
                       (const unsigned long long*)keys, seg_begin, seg_end, nseg, e->key_acc);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, e->key_acc, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TW_OK;
}

unsigned bit_length(unsigned long long x) {
    unsigned n = 0;
    while (x) { n++; x >>= 1; }
    return n;
}

// Sorts every row [seg_begin[s], seg_end[s]) of 64-bit keys ascending into `out` (same positions).  Only the bits
// [begin_bit, end_bit) differ between keys and none of them is a sign bit that is set (callers check); `fixed` holds
// the common bits.  dst_off[s] = position of row s in the packed array (rows back to back), `packed` = its size.
// One device-wide radix sort over composite keys (see k_rows_pack); rows too many / keys too wide for 64 bits fall
// back to rocprim's segmented sort on the raw keys.
template <class Key>
int sort_rows(tw_engine* e, const Key* keys, Key* out, unsigned size, const uint32_t* seg_begin, const uint32_t* seg_end,
              const uint32_t* dst_off, int nseg, int64_t packed, unsigned begin_bit, unsigned end_bit, unsigned long long fixed) {
    if (nseg <= 0 || packed <= 0) return TW_OK;
    unsigned segbits = 0;
    while ((1u << segbits) < (unsigned)nseg) segbits++;
    const unsigned kb = end_bit - begin_bit;
    const bool mixed_signs = std::is_signed<Key>::value && end_bit >= 64;  // composite keys compare unsigned
    if (kb + segbits > 64 || kb == 0 || packed > e->comp_cap || mixed_signs) {
        return rocprim_call(e, [&](void* tmp, size_t& bytes) {
            return rocprim::segmented_radix_sort_keys(tmp, bytes, keys, out, size, (unsigned)nseg, seg_begin, seg_end, begin_bit, end_bit, e->stream);
        });
    }
    const int bx = (int)std::min<int64_t>(std::max<int64_t>(4096 / nseg, 1), packed / nseg / 1024 + 1);
    const dim3 grid((unsigned)bx, (unsigned)std::min(nseg, 1024)), block(flat_threads(e));
    hipLaunchKernelGGL(k_rows_pack, grid, block, 0, e->stream, (const unsigned long long*)keys, seg_begin, seg_end, dst_off, nseg,
                       (int)begin_bit, (int)kb, e->comp_a);
    TWCHK(rocprim_call(e, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_keys(tmp, bytes, e->comp_a, e->comp_b, (size_t)packed, 0u, kb + segbits, e->stream); }));
    hipLaunchKernelGGL(k_rows_unpack, grid, block, 0, e->stream, (const unsigned long long*)e->comp_b, seg_begin, seg_end, dst_off, nseg,
                       (int)begin_bit, (int)kb, fixed, (unsigned long long*)out);
    HIPCHK(hipGetLastError());
    return TW_OK;
}

// (no-skip batches: every endpoint list holds one span per incoming span, all lists sorted by (start, end).  The counters
// borrow two per-span words that the pass writes only later: the window ids and the owner words)
int run_pass(tw_engine* e, int pass) {
    const Dev& P = e->P;
    const dim3 tiles(P.n_tiles), tb(e->K.tile);
    const auto host_t0 = std::chrono::steady_clock::now();
    HIPCHK(hipEventRecord(e->ev[EV_BEGIN], e->stream));
    HIPCHK(hipMemsetAsync(e->ctr, 0, sizeof(int32_t) * (size_t)e->ctr_pass_ints, e->stream));   // error flag, statistics, every work-list counter
#ifdef TW_PROFILE
    HIPCHK(hipMemsetAsync(P.prof + 5, 0, sizeof(unsigned long long) * 3, e->stream));    // the longest item / wavefront of THIS pass (the sums run on)
    HIPCHK(hipMemsetAsync(P.prof + 10, 0, sizeof(unsigned long long) * 3, e->stream));
#endif
    // Every class on its own stream: enumeration, then (staged) its windows and the first selection of its windows, while the longer
    // enumerations of other classes are still running.  TW_CLASS_PIPELINE=0 / skip mode / small batches: the classes join after the enumeration.
    int n_cls = 0;
    for (int E = 1; E <= kMaxEp; E++) n_cls += e->tile_cls_off[E + 1] > e->tile_cls_off[E] ? 1 : 0;
    const bool staged = !e->skip_mode && e->K.pipeline != 0 && P.n_tiles >= (int64_t)e->K.stage_min_tiles * std::max(n_cls, 1);
    // pass 1, ComputeEpPairDistParams3: sorted end times and block parameters -- staged: per class, at the head of the class' chain
    // (launch_enumerate: the class with the longest chain does not wait for the parameters of the others)
    e->class_params = false;
    if (pass == 1 && !e->skip_mode) {
        HIPCHK(hipMemsetAsync(e->rank_in, 0, sizeof(int32_t) * (size_t)std::max<int64_t>(P.n_in_total, 1), e->stream));
        HIPCHK(hipMemsetAsync(e->rank_out, 0, sizeof(int32_t) * (size_t)std::max<int64_t>(P.n_out_total, 1), e->stream));
        if (staged) e->class_params = true;
        else {
            int rc = sort_ends(e, all_tiles_host(e), e->stream);
            if (rc != TW_OK) return rc;
            launch_block_params(e, 0, e->stream);
        }
    }
    if (e->skip_mode) {
        // ComputeEpPairDistParams3 is not called when an endpoint is short of spans (traceweaver_v3.py:1177-1178); the first
        // enumeration only serves the candidate sets of the windows (DfsTraverse3), its scores are not used: neutral parameters
        const int64_t total = e->n_gp;
        hipLaunchKernelGGL(k_neutral_params, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, e->stream, P.gparam, total);
    }
    HIPCHK(hipEventRecord(e->ev[EV_PARAMS], e->stream));
    HIPCHK(hipEventRecord(e->ev[EV_ENUM0], e->stream));
    const auto host_t1 = std::chrono::steady_clock::now();
    {
        // what the selection stage and the repair rounds start from: filled on the engine's stream beside the enumerations
        int rc = launch_enumerate_all(e, pass, 0, nullptr, staged, [&]() -> int {
            if (pass == 1) { int rs = run_scan<ScanMaxEnd>(e, all_tiles_host(e), e->stream, e->agg_pair); if (rs != TW_OK) return rs; }
            if (e->skip_mode) { HIPCHK(hipEventRecord(e->prep_ev, e->stream)); return TW_OK; }
            HIPCHK(hipMemsetAsync(P.w_conf, 0, sizeof(int32_t) * (size_t)P.n_in_total, e->stream));
            HIPCHK(hipMemsetAsync(P.gone_valid, 0, (size_t)P.n_in_total, e->stream));   // (P.gone itself is not filled: k_detect_gone)
            HIPCHK(hipMemsetAsync(P.w_dirty, 0, (size_t)P.n_in_total, e->stream));
            HIPCHK(hipMemsetAsync(P.owner, 0x7f, sizeof(int32_t) * std::max<int64_t>(P.n_out_total, 1), e->stream));
            HIPCHK(hipEventRecord(e->prep_ev, e->stream));
            return TW_OK;
        });
        if (rc != TW_OK) return rc;
    }
    e->host_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t1).count();
    if (pass == 1 && !staged) {
        int rc = launch_windows(e, all_tiles_host(e), e->stream);
        if (rc != TW_OK) return rc;
    }
    if (!staged) HIPCHK(hipEventRecord(e->ev[EV_WIN], e->stream));
    if (e->skip_mode) {   // the reference's loop in its own order, one wavefront per unit (tw_skip.h)
        HIPCHK(hipMemsetAsync(P.owner, 0x7f, sizeof(int32_t) * std::max<int64_t>(P.n_out_total, 1), e->stream));
        HIPCHK(hipMemsetAsync(e->skip_fetch, 0, sizeof(long long) * (size_t)std::max<int64_t>(e->skip_fetch_n, 1), e->stream));
        HIPCHK(hipMemsetAsync(P.w_dirty, 0, (size_t)P.n_in_total, e->stream));
        hipLaunchKernelGGL(k_skip_walk, dim3(P.n_units), dim3(std::min(e->K.coop, 64)), 0, e->stream, P, (const SkipUnitDev*)e->skip_units);
        HIPCHK(hipEventRecord(e->ev[EV_SEL], e->stream));
        HIPCHK(hipEventRecord(e->ev[EV_REPAIR], e->stream));
        hipLaunchKernelGGL(k_finalize, tiles, tb, 0, e->stream, P, all_tiles_host(e));
        HIPCHK(hipEventRecord(e->ev[EV_END], e->stream));
        HIPCHK(hipGetLastError());
        int32_t kerr0 = 0;
        HIPCHK(hipMemcpyAsync(&kerr0, P.err, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        if (kerr0 != 0) return fail(e, kerr0, kernel_error_text(kerr0));
        return TW_OK;
    }
    if (!staged) {
        hipLaunchKernelGGL(k_select_fast, tiles, tb, 0, e->stream, P, all_tiles_host(e));
        launch_select_listed(e, all_tiles_host(e), e->stream, P.n_in_total);
        launch_select_hard(e, all_tiles_host(e), e->stream);
    }
    HIPCHK(hipEventRecord(e->ev[EV_SEL], e->stream));
    // span consumption: rounds of claim / detect / re-enumerate / re-select until no span's set of taken candidates changes
    e->rounds = 0;
    for (int round = 0;; round++) {
        if (!(staged && round == 0)) {   // (staged: the first round ran class by class, launch_class_stage)
            if (round > 0) HIPCHK(hipMemsetAsync(P.owner, 0x7f, sizeof(int32_t) * std::max<int64_t>(P.n_out_total, 1), e->stream));
            hipLaunchKernelGGL(k_claim, tiles, tb, 0, e->stream, P, all_tiles_host(e), 0);
            HIPCHK(hipMemsetAsync(e->ctr, 0, sizeof(int32_t) * (size_t)e->ctr_round_ints, e->stream));   // work lists, round_changed, frontier cursors
            hipLaunchKernelGGL(k_detect_gone, tiles, tb, 0, e->stream, P, all_tiles_host(e), round, 0);
        }
        int32_t changed = 0, listed[2 * (kMaxEp + 1)] = {};
        HIPCHK(hipMemcpyAsync(&changed, P.round_changed, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(listed, P.heavy_in_count, sizeof(listed), hipMemcpyDeviceToHost, e->stream));   // (what k_detect_gone listed, per class and instantiation)
        HIPCHK(hipStreamSynchronize(e->stream));
        if (changed == 0) break;
        if (round >= kMaxRepairRounds) return fail(e, TW_ERR_DEVICE, "span consumption did not settle (more repair rounds than windows)");
        e->rounds = round + 1;
        { int rc = launch_enumerate_all(e, pass, 1, listed, false, []() { return (int)TW_OK; }); if (rc != TW_OK) return rc; }
        launch_select_listed(e, all_tiles_host(e), e->stream, P.n_in_total);
        launch_select_hard(e, all_tiles_host(e), e->stream);
    }
    HIPCHK(hipEventRecord(e->ev[EV_REPAIR], e->stream));
    if (!(staged && e->rounds == 0)) {   // (staged and nothing repaired: the classes' stages have written parents and gap samples)
        if (staged) hipLaunchKernelGGL(k_reset_stats, dim3((unsigned)((P.n_units + 255) / 256)), dim3(256), 0, e->stream, P);
        hipLaunchKernelGGL(k_finalize, tiles, tb, 0, e->stream, P, all_tiles_host(e));
        if (pass == 1) hipLaunchKernelGGL(k_gaps, tiles, tb, 0, e->stream, P, all_tiles_host(e));
    }
    HIPCHK(hipEventRecord(e->ev[EV_END], e->stream));
    HIPCHK(hipGetLastError());
    int32_t kerr = 0, aw[kMaxEp + 1] = {}, hn[kSelSlots * 8] = {}, sc[kMaxEp + 1] = {};
    HIPCHK(hipMemcpyAsync(&kerr, P.err, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (pass == 1) HIPCHK(hipMemcpyAsync(aw, P.any_wide, sizeof(aw), hipMemcpyDeviceToHost, e->stream));   // (which classes listed spans with wide windows: pass 2 lists the same spans)
    if (pass == 1) HIPCHK(hipMemcpyAsync(hn, P.heavy_next, sizeof(hn), hipMemcpyDeviceToHost, e->stream));
    if (pass == 1) HIPCHK(hipMemcpyAsync(sc, P.split_count, sizeof(sc), hipMemcpyDeviceToHost, e->stream));   // (the pass' total per class: not reset by the repair rounds)
    HIPCHK(hipStreamSynchronize(e->stream));
    if (pass == 1) for (int E = 1; E <= kMaxEp; E++) e->wide_pass1[E] = aw[E] != 0 ? 1 : 0;
    if (pass == 1) for (int E = 1; E <= kMaxEp; E++) e->split_pass1[E] = sc[E];
    // (a repair round's fill of the counter block takes the stages' counts with it: not known then)
    if (pass == 1) for (int E = 1; E <= kMaxEp; E++) e->hard_pass1[E] = (staged && e->rounds == 0) ? hn[E * 8 + kHardCount] : -1;
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, e->ev[EV_BEGIN], e->ev[EV_END])); e->ms[0] = f;
    HIPCHK(hipEventElapsedTime(&f, e->ev[EV_ENUM0], e->ev[EV_ENUM1])); e->ms[1] = f;
    HIPCHK(hipEventElapsedTime(&f, e->ev[EV_WIN], e->ev[EV_SEL])); e->ms[2] = f;
    HIPCHK(hipEventElapsedTime(&f, e->ev[EV_ENUM1], e->ev[EV_WIN])); e->ms[3] = f;
    HIPCHK(hipEventElapsedTime(&f, e->ev[EV_SEL], e->ev[EV_REPAIR])); e->ms[4] = f;
    HIPCHK(hipEventElapsedTime(&f, e->ev[EV_BEGIN], e->ev[EV_PARAMS])); e->ms[5] = f;
    e->host_ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count();
    if (kerr != 0) return fail(e, kerr, kernel_error_text(kerr));
    return TW_OK;
}

}  // namespace

namespace {
// One stable pass of the (start, end, trace order) sort: keys gathered through the current permutation, pairs sorted
// on the bits that differ at all.
template <class Src>
int load_sort_pass(tw_engine* e, const Src* src, int64_t n, unsigned bits, unsigned long long* ka, unsigned long long* kb, uint32_t** perm, uint32_t** perm_alt) {
    if (n <= 0 || bits == 0) return TW_OK;
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 8192), block = flat_threads(e);
    if (sizeof(Src) == 8) hipLaunchKernelGGL(k_load_keys64, dim3(grid), dim3(block), 0, e->stream, (const int64_t*)src, (const uint32_t*)*perm, n, ka);
    else hipLaunchKernelGGL(k_load_keys32, dim3(grid), dim3(block), 0, e->stream, (const int32_t*)src, (const uint32_t*)*perm, n, ka);
    TWCHK(rocprim_call(e, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_pairs(tmp, bytes, ka, kb, *perm, *perm_alt, (size_t)n, 0u, bits, e->stream); }));
    std::swap(*perm, *perm_alt);
    return TW_OK;
}

// number of low bits in which the int64 values of an array differ (64 if signs differ)
int differing_bits(tw_engine* e, const int64_t* v, int64_t n, unsigned* bits) {
    *bits = 0;
    if (n <= 0) return TW_OK;
    std::vector<uint32_t> seg = {0u, (uint32_t)n};
    uint32_t* d = nullptr;
    HIPCHK(hipMalloc((void**)&d, sizeof(uint32_t) * 2));
    hipError_t st = hipMemcpy(d, seg.data(), sizeof(uint32_t) * 2, hipMemcpyHostToDevice);
    unsigned long long out[2] = {0, 0};
    int rc = st == hipSuccess ? key_bits(e, v, d, d + 1, 1, n, out) : TW_ERR_DEVICE;
    (void)hipFree(d);
    if (rc != TW_OK) return rc == TW_ERR_DEVICE ? fail(e, TW_ERR_DEVICE, "differing_bits: copy failed") : rc;
    *bits = std::min(64u, std::max(1u, bit_length(out[0])));
    return TW_OK;
}
}  // namespace

extern "C" int tw_scale_load(tw_engine* e, const int32_t* unit_factor, const int32_t* trace_rank, int32_t* in_perm, int32_t* out_perm, double* unit_time_scale) {
    if (e == nullptr || unit_factor == nullptr) return TW_ERR_ARG;
    if (e->state < ST_LOADED) return fail(e, TW_ERR_STATE, "tw_scale_load before tw_load_batch");
    if (e->skip_mode) return fail(e, TW_ERR_UNSUPPORTED, "load scaling of a skip-mode batch (skip mode takes integer microseconds)");
    if (e->scaled_upload) return fail(e, TW_ERR_UNSUPPORTED, "the batch was uploaded with unit_time_scale: it is load-scaled already");
    if (e->truth == nullptr) return fail(e, TW_ERR_STATE, "tw_scale_load needs the requests' own calls (tw_set_truth): helpers/transforms.py:25-29 pairs them by trace id");
    HIPCHK(hipSetDevice(e->device));
    Dev& P = e->P;
    const int64_t n_in = P.n_in_total, n_out = P.n_out_total;
    for (int u = 0; u < P.n_units; u++)
        if (unit_factor[u] < 1) return fail(e, TW_ERR_ARG, "tw_scale_load: load factors are integers >= 1 (executor.py:1089-1091)");
    int rc;
    const bool has_trace = e->n_traces > 0 && e->in_trace != nullptr;
    if (e->orig_is == nullptr) {   // first load level: keep the table as uploaded
        rc = dev_alloc(e, &e->orig_is, n_in); if (rc != TW_OK) return rc;
        rc = dev_alloc(e, &e->orig_ie, n_in); if (rc != TW_OK) return rc;
        rc = dev_alloc(e, &e->orig_os, n_out); if (rc != TW_OK) return rc;
        rc = dev_alloc(e, &e->orig_oe, n_out); if (rc != TW_OK) return rc;
        rc = dev_alloc(e, &e->orig_truth, e->n_ie); if (rc != TW_OK) return rc;
        rc = dev_alloc(e, &e->orig_trace, n_in); if (rc != TW_OK) return rc;
        HIPCHK(hipMemcpyAsync(e->orig_is, P.in_start, sizeof(int64_t) * n_in, hipMemcpyDeviceToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->orig_ie, P.in_end, sizeof(int64_t) * n_in, hipMemcpyDeviceToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->orig_os, P.out_start, sizeof(int64_t) * n_out, hipMemcpyDeviceToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->orig_oe, P.out_end, sizeof(int64_t) * n_out, hipMemcpyDeviceToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->orig_truth, e->truth, sizeof(int32_t) * e->n_ie, hipMemcpyDeviceToDevice, e->stream));
        if (has_trace) HIPCHK(hipMemcpyAsync(e->orig_trace, e->in_trace, sizeof(int32_t) * n_in, hipMemcpyDeviceToDevice, e->stream));
    }
    // scratch of this call (freed on return): binary64 / int64 images, tie ranks, row ids, sort keys and permutations
    const int64_t n_max = std::max(n_in, n_out);
    std::vector<void*> tmp;
    auto scratch = [&](size_t bytes) -> void* { void* q = nullptr; if (hipMalloc(&q, std::max<size_t>(bytes, 8)) != hipSuccess) return nullptr; tmp.push_back(q); return q; };
    struct Free { std::vector<void*>& v; ~Free() { for (void* q : v) (void)hipFree(q); } } free_tmp{tmp};
    LoadDev L{};
    L.units = P.units; L.tiles = P.tiles;
    L.is = e->orig_is; L.ie = e->orig_ie; L.os = e->orig_os; L.oe = e->orig_oe; L.truth = e->orig_truth; L.in_trace = e->orig_trace;
    L.x = (double*)scratch(8 * n_in); L.xe = (double*)scratch(8 * n_in); L.y = (double*)scratch(8 * n_out); L.ye = (double*)scratch(8 * n_out);
    L.rank_in = (int32_t*)scratch(4 * n_in); L.rank_out = (int32_t*)scratch(4 * n_out); L.row_in = (int32_t*)scratch(4 * n_in); L.row_out = (int32_t*)scratch(4 * n_out);
    L.owner_req = (int32_t*)scratch(4 * n_out); L.kmax = (int32_t*)scratch(4 * P.n_units); L.err = (int32_t*)scratch(4);
    int32_t* d_factor = (int32_t*)scratch(4 * P.n_units); int32_t* d_segbase = (int32_t*)scratch(4 * P.n_units);
    int32_t* d_rank = trace_rank != nullptr ? (int32_t*)scratch(4 * n_in) : nullptr;
    unsigned long long *ka = (unsigned long long*)scratch(8 * n_max), *kb = (unsigned long long*)scratch(8 * n_max);
    uint32_t *perm = (uint32_t*)scratch(4 * n_max), *perm_alt = (uint32_t*)scratch(4 * n_max);
    uint32_t* perm_in = (uint32_t*)scratch(4 * n_in);
    int32_t *pos_in = (int32_t*)scratch(4 * n_in), *pos_out = (int32_t*)scratch(4 * n_out);
    if (!L.x || !L.xe || !L.y || !L.ye || !L.rank_in || !L.rank_out || !L.row_in || !L.row_out || !L.owner_req || !L.kmax || !L.err || !d_factor ||
        !d_segbase || (trace_rank != nullptr && !d_rank) || !ka || !kb || !perm || !perm_alt || !perm_in || !pos_in || !pos_out)
        return fail(e, TW_ERR_DEVICE, "tw_scale_load: out of device memory");
    std::vector<int32_t> segbase_h((size_t)P.n_units);
    { int32_t acc = 0; for (int u = 0; u < P.n_units; u++) { segbase_h[(size_t)u] = acc; acc += e->units[(size_t)u].E; } }
    HIPCHK(hipMemcpyAsync(d_factor, unit_factor, sizeof(int32_t) * P.n_units, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_segbase, segbase_h.data(), sizeof(int32_t) * P.n_units, hipMemcpyHostToDevice, e->stream));
    if (d_rank != nullptr) HIPCHK(hipMemcpyAsync(d_rank, trace_rank, sizeof(int32_t) * n_in, hipMemcpyHostToDevice, e->stream));
    L.factor = d_factor; L.seg_base = d_segbase; L.trace_rank = d_rank;
    HIPCHK(hipMemsetAsync(L.kmax, 0, sizeof(int32_t) * P.n_units, e->stream));
    HIPCHK(hipMemsetAsync(L.err, 0, sizeof(int32_t), e->stream));
    HIPCHK(hipMemsetAsync(L.owner_req, 0xff, sizeof(int32_t) * n_out, e->stream));
    hipLaunchKernelGGL(k_load_scale_in, dim3(P.n_tiles), dim3(e->K.tile), 0, e->stream, L);
    hipLaunchKernelGGL(k_load_scale_out, dim3(P.n_tiles), dim3(e->K.tile), 0, e->stream, L);
    hipLaunchKernelGGL(k_load_to_int, dim3(P.n_tiles), dim3(e->K.tile), 0, e->stream, L);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> kmax_h((size_t)P.n_units);
    int32_t err_h = 0;
    HIPCHK(hipMemcpyAsync(kmax_h.data(), L.kmax, sizeof(int32_t) * P.n_units, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(&err_h, L.err, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (err_h != 0)
        return fail(e, TW_ERR_ARG, "tw_scale_load: the requests' own calls are not one call per request at every endpoint (helpers/transforms.py:25-29 asserts it), "
                                   "or the scaled timestamps span too many binades for int64");
    // stable least-significant-key-first passes: trace order, end, start, list
    const unsigned grid_in = (unsigned)std::min<int64_t>((n_in + 255) / 256, 8192), grid_out = (unsigned)std::min<int64_t>((n_out + 255) / 256, 8192);
    const unsigned block = flat_threads(e);
    int64_t* d_is = const_cast<int64_t*>(P.in_start); int64_t* d_ie = const_cast<int64_t*>(P.in_end);
    int64_t* d_os = const_cast<int64_t*>(P.out_start); int64_t* d_oe = const_cast<int64_t*>(P.out_end);
    for (int side = 0; side < 2; side++) {
        const int64_t n = side == 0 ? n_in : n_out;
        const int64_t* vs = (const int64_t*)(side == 0 ? L.x : L.y); const int64_t* ve = (const int64_t*)(side == 0 ? L.xe : L.ye);
        const int32_t* rank = side == 0 ? L.rank_in : L.rank_out; const int32_t* row = side == 0 ? L.row_in : L.row_out;
        const int nrows = side == 0 ? P.n_units : e->n_seg_out;
        unsigned bs = 0, be = 0;
        rc = differing_bits(e, vs, n, &bs); if (rc != TW_OK) return rc;
        rc = differing_bits(e, ve, n, &be); if (rc != TW_OK) return rc;
        hipLaunchKernelGGL(k_load_iota, dim3(side == 0 ? grid_in : grid_out), dim3(block), 0, e->stream, perm, n);
        rc = load_sort_pass(e, rank, n, 32u, ka, kb, &perm, &perm_alt); if (rc != TW_OK) return rc;
        rc = load_sort_pass(e, ve, n, be, ka, kb, &perm, &perm_alt); if (rc != TW_OK) return rc;
        rc = load_sort_pass(e, vs, n, bs, ka, kb, &perm, &perm_alt); if (rc != TW_OK) return rc;
        rc = load_sort_pass(e, row, n, std::max(1u, bit_length((unsigned long long)std::max(nrows - 1, 1))), ka, kb, &perm, &perm_alt); if (rc != TW_OK) return rc;
        hipLaunchKernelGGL(k_load_place, dim3(side == 0 ? grid_in : grid_out), dim3(block), 0, e->stream, (const uint32_t*)perm, n, vs, ve,
                           side == 0 ? d_is : d_os, side == 0 ? d_ie : d_oe, side == 0 ? pos_in : pos_out);
        hipLaunchKernelGGL(k_load_local, dim3(side == 0 ? grid_in : grid_out), dim3(block), 0, e->stream, perm, row, (const uint32_t*)(side == 0 ? e->seg_in : e->seg_out), n);
        HIPCHK(hipGetLastError());
        int32_t* host = side == 0 ? in_perm : out_perm;
        if (host != nullptr) HIPCHK(hipMemcpyAsync(host, perm, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    hipLaunchKernelGGL(k_load_retruth, dim3(P.n_tiles), dim3(e->K.tile), 0, e->stream, L, (const int32_t*)pos_in, (const int32_t*)pos_out, e->truth,
                       has_trace ? e->in_trace : nullptr);
    HIPCHK(hipGetLastError());
    for (int u = 0; u < P.n_units; u++) {
        UnitDev& U = e->units[(size_t)u];
        U.tscale = std::ldexp(1.0, -kmax_h[(size_t)u]);
        U.float_time = 1;
        if (unit_time_scale != nullptr) unit_time_scale[u] = U.tscale;
    }
    HIPCHK(hipMemcpyAsync(const_cast<UnitDev*>(P.units), e->units.data(), sizeof(UnitDev) * e->units.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->state = ST_LOADED; e->pass1_done = false;
    drop_batch_order(e);   // every list was re-sorted: in_row / out_row and the given parents no longer name the spans at these positions
    for (int E = 0; E <= kMaxEp; E++) { e->wide_pass1[E] = -1; e->hard_pass1[E] = -1; e->split_pass1[E] = -1; }
    return TW_OK;
}

extern "C" {

int tw_create(int device_id, tw_engine** out) {
    if (out == nullptr) return TW_ERR_ARG;
    *out = nullptr;
    tw_engine* e = new tw_engine();
    e->device = device_id;
    e->K = read_knobs();
    // The engine runs its endpoint-count classes and window classes on streams of their own (up to 8 + 3 beside its own).  The
    // runtime multiplexes a process' streams onto GPU_MAX_HW_QUEUES hardware queues, 4 by default: classes that share a queue run one
    // after the other (Alibaba-shape slice, eight classes: 9.5 / 11.2 ms per pass with 4 or 8 queues, 6.3 / 7.0 ms with 12 or 16;
    // three classes: the same either way).  The variable is read when the runtime initialises and belongs to the whole process
    // (torch, RCCL, other HIP libraries in it): the library does not touch it.  The applications of this repository export it
    // before anything initialises HIP (bench.py, python -m traceweaver_amd.executor); other hosts do the same, or set
    // TW_SET_HW_QUEUES=1 to let this call export it when it is still unset (effective if the engine is the process' first user of HIP).
    if (e->K.set_hw_queues != 0) setenv("GPU_MAX_HW_QUEUES", "12", 0);
    hipError_t s = hipSetDevice(device_id);
    if (s == hipSuccess) s = hipStreamCreate(&e->stream);
    if (s == hipSuccess) s = hipEventCreateWithFlags(&e->fit_fork, hipEventDisableTiming);
    if (s == hipSuccess) s = hipEventCreateWithFlags(&e->fit_join, hipEventDisableTiming);
    for (int i = 0; i < EV_COUNT && s == hipSuccess; i++) s = hipEventCreate(&e->ev[i]);
    for (int i = 0; i < SE_COUNT && s == hipSuccess; i++) s = hipEventCreate(&e->stage_ev[i]);
    // (the class streams are created when a batch first holds the class, tw_load_batch: the streams of a process share its hardware
    // queues, and a queue shared by two busy streams runs their kernels one after the other -- an engine that only ever sees three
    // classes owns seven streams, not twelve)
    for (int i = 0; i <= kMaxEp + 1 && s == hipSuccess; i++) s = hipEventCreateWithFlags(&e->cls_ev[i], hipEventDisableTiming);
    if (s == hipSuccess) s = hipEventCreateWithFlags(&e->prep_ev, hipEventDisableTiming);
    if (s == hipSuccess) s = hipEventCreateWithFlags(&e->tile_done, hipEventDisableTiming);
    for (int i = 0; i <= kMaxEp && s == hipSuccess; i++) {
        s = hipEventCreateWithFlags(&e->post_fork[i], hipEventDisableTiming);
        if (s == hipSuccess) s = hipEventCreateWithFlags(&e->post_done[i], hipEventDisableTiming);
        for (int j = 0; j < 3 && s == hipSuccess; j++) s = hipEventCreateWithFlags(&e->post_join[i][j], hipEventDisableTiming);
    }
    if (s != hipSuccess) {
        fprintf(stderr, "tw_create: %s\n", hipGetErrorString(s));
        delete e;
        return TW_ERR_DEVICE;
    }
    *out = e;
    return TW_OK;
}

void tw_destroy(tw_engine* e) {
    if (e == nullptr) return;
    (void)hipSetDevice(e->device);
    free_all(e);
    order_unstage(e);
    hist_free(e);
    chist_free(e);
    if (e->arena != nullptr) (void)hipFree(e->arena);
    for (int i = 0; i < EV_COUNT; i++)
        if (e->ev[i]) (void)hipEventDestroy(e->ev[i]);
    for (int i = 0; i <= kMaxEp + 1; i++)
        if (e->cls_ev[i]) (void)hipEventDestroy(e->cls_ev[i]);
    for (int i = 1; i <= kMaxEp; i++)
        if (e->cls_stream[i]) (void)hipStreamDestroy(e->cls_stream[i]);
    for (int i = 0; i < 3; i++)
        if (e->sel_stream[i]) (void)hipStreamDestroy(e->sel_stream[i]);
    if (e->prep_ev) (void)hipEventDestroy(e->prep_ev);
    if (e->tile_done) (void)hipEventDestroy(e->tile_done);
    if (e->fit_fork) (void)hipEventDestroy(e->fit_fork);
    if (e->fit_join) (void)hipEventDestroy(e->fit_join);
    for (int i = 0; i <= kMaxEp; i++) {
        if (e->post_fork[i]) (void)hipEventDestroy(e->post_fork[i]);
        if (e->post_done[i]) (void)hipEventDestroy(e->post_done[i]);
        for (int j = 0; j < 3; j++)
            if (e->post_join[i][j]) (void)hipEventDestroy(e->post_join[i][j]);
    }
    for (int i = 0; i < SE_COUNT; i++)
        if (e->stage_ev[i]) (void)hipEventDestroy(e->stage_ev[i]);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

const char* tw_last_error(const tw_engine* e) { return e ? e->err.c_str() : "null engine"; }

int tw_load_batch(tw_engine* e, const tw_batch* b, int spans_on_device) {
    if (e == nullptr || b == nullptr) return TW_ERR_ARG;
    HIPCHK(hipSetDevice(e->device));
    if (b->n_units <= 0) return fail(e, TW_ERR_ARG, "n_units must be positive");
    if (b->topk != TW_TOPK) return fail(e, TW_ERR_UNSUPPORTED, "topk must be 5 (traceweaver_v3.py:1109)");
    if (b->skip != nullptr && spans_on_device)   // the start-ordered views and the pool checks of a skip-mode batch are built on the host
        return fail(e, TW_ERR_UNSUPPORTED, "a skip-mode batch takes its span arrays from host memory (spans_on_device = 0)");
    if (b->batch_size <= 0 || b->batch_size_mis <= 0) return fail(e, TW_ERR_ARG, "batch sizes must be positive");
    free_all(e);
    e->fit_rng = Mt19937(e->fit_seed);   // a batch's refit does not depend on what the engine solved before
    e->fit_prepared = false; e->fit_runs_pending = false; e->fit_rows_h_valid = false;
    e->units.assign((size_t)b->n_units, UnitDev{});
    e->tiles.clear();
    e->gs_off_h.assign((size_t)b->n_units, 0);
    int64_t ie = 0, gp = 0, slots = 0, gaps = 0, epi = 0, dagi = 0;
    std::vector<uint32_t> seg_in((size_t)b->n_units + 1), seg_out;
    for (int u = 0; u < b->n_units; u++) {
        UnitDev& U = e->units[(size_t)u];
        const int E = b->unit_E[u];
        const int64_t n = b->unit_in_off[u + 1] - b->unit_in_off[u];
        if (E < 1 || E > TW_MAX_EP) return fail(e, TW_ERR_UNSUPPORTED, "unit has E outside [1, TW_MAX_EP]");
        if (n < 2) return fail(e, TW_ERR_ARG, "a unit needs at least 2 incoming spans (the reference raises on max([]) for 1, traceweaver_v3.py:1119)");
        if (n > (1 << 26)) return fail(e, TW_ERR_ARG, "unit too large (more than 2^26 incoming spans: the selection work lists address a window's first span in 26 bits)");
        U.in_off = b->unit_in_off[u];
        U.tscale = b->unit_time_scale != nullptr ? b->unit_time_scale[u] : 1.0;
        U.float_time = b->unit_time_scale != nullptr ? 1 : 0;
        U.part = b->unit_part != nullptr ? (int32_t)b->unit_part[u] : 0;
        {
            int ex = 0;
            if (!(U.tscale > 0.0) || std::frexp(U.tscale, &ex) != 0.5) return fail(e, TW_ERR_ARG, "unit_time_scale must be a positive power of two");
        }
        U.n_in = (int32_t)n;
        U.E = E;
        U.ie_off = ie;
        U.nblk = (int32_t)((n + b->batch_size - 1) / b->batch_size);
        U.nslot = E * E + 2 * E;
        U.gp_off = gp;
        U.slot_off = (int32_t)slots;
        U.tile_off = (int32_t)e->tiles.size();
        U.ntile = (int32_t)((n + e->K.tile - 1) / e->K.tile);
        for (int t = 0; t < U.ntile; t++) e->tiles.push_back(TileDev{u, t * e->K.tile});
        seg_in[(size_t)u] = (uint32_t)U.in_off;
        const uint8_t* dag = b->dag + dagi;
        for (int k = 0; k <= E; k++) U.ep_off[k] = b->ep_off[epi + k];
        U.skip = b->skip != nullptr ? 1 : 0;
        for (int k = 0; k < E; k++) {
            const int64_t m = U.ep_off[k + 1] - U.ep_off[k];
            if (b->skip == nullptr && m != n)
                return fail(e, TW_ERR_UNSUPPORTED, "an endpoint's span count differs from the number of incoming spans: a skip-mode unit (traceweaver_v3.py:972,1155-1156) needs tw_batch.skip");
            if (b->skip != nullptr && (m > n || m < 0)) return fail(e, TW_ERR_ARG, "skip mode: an endpoint holds more spans than there are incoming spans");
            seg_out.push_back((uint32_t)U.ep_off[k]);
        }
        if (b->skip != nullptr) {
            if (b->unit_time_scale != nullptr) return fail(e, TW_ERR_UNSUPPORTED, "skip mode takes integer microseconds");
            const tw_skip_unit& K = b->skip[u];
            if (K.n_tw < 1 || !K.tw_start || !K.pool || !K.dist) return fail(e, TW_ERR_ARG, "skip mode: incomplete tw_skip_unit");
            if (K.n_tw > (0x7fffffff - TW_SKIP_BASE) / TW_SKIP_STRIDE) return fail(e, TW_ERR_ARG, "skip mode: too many time windows");
            for (int64_t q = 0; q < (int64_t)E * K.n_tw; q++)
                if (K.pool[q] < 0 || K.pool[q] > TW_SKIP_STRIDE) return fail(e, TW_ERR_ARG, "skip mode: a pool holds more than TW_SKIP_STRIDE skip spans");
        }
        for (int q = 0; q < E; q++) {
            uint8_t pm = 0, sm = 0;
            int np = 0;
            for (int p = 0; p < E; p++) {
                if (dag[p * E + q]) {
                    if (p >= q) return fail(e, TW_ERR_ARG, "endpoints are not in topological order of the DAG");
                    pm |= (uint8_t)(1u << p);
                    U.pred_list[q][np++] = (uint8_t)p;
                }
                if (dag[q * E + p]) sm |= (uint8_t)(1u << p);
            }
            U.pred_mask[q] = pm;
            U.key_rank[q] = (uint8_t)b->key_rank[epi + q];
            U.succ_mask[q] = sm;
            U.npred[q] = (uint8_t)np;
            // networkx in_edges(): predecessors in partition-key (insertion) order, executor.py:223-236
            std::stable_sort(U.pred_list[q], U.pred_list[q] + np, [&](uint8_t x, uint8_t y) {
                return b->key_rank[epi + x] < b->key_rank[epi + y];
            });
            for (int j = 0; j < np; j++) {  // primary <=> no 2-hop alternative (traceweaver_v1.py:245-254)
                const int p = U.pred_list[q][j];
                bool prim = true;
                for (int m = 0; m < E; m++)
                    if (m != p && m != q && dag[p * E + m] && dag[m * E + q]) prim = false;
                U.pred_prim[q][j] = prim ? 1 : 0;
            }
        }
        e->gs_off_h[(size_t)u] = gaps;
        ie += n * E;
        gp += (int64_t)U.nblk * U.nslot;
        slots += U.nslot;
        gaps += (int64_t)U.nslot * n;
        epi += E;
        dagi += E * E;
    }
    std::vector<int32_t> tile_ids_h;
    int32_t heavy_off_h[kMaxEp + 2] = {};
    for (int cls = 0; cls <= kMaxEp; cls++) {
        e->tile_cls_off[cls] = (int32_t)tile_ids_h.size();
        heavy_off_h[cls + 1] = heavy_off_h[cls];
        for (size_t tix = 0; tix < e->tiles.size(); tix++)
            if (e->units[(size_t)e->tiles[tix].unit].E == cls) tile_ids_h.push_back((int32_t)tix);
        for (int u = 0; u < b->n_units; u++)
            if (e->units[(size_t)u].E == cls) heavy_off_h[cls + 1] += e->units[(size_t)u].n_in;
    }
    e->tile_cls_off[kMaxEp + 1] = (int32_t)tile_ids_h.size();
    std::vector<BlockRef> blk_tab_h;   // (8 B per group of blocks and table: every unit's groups, then each class' own)
    for (int cls = 0; cls <= kMaxEp; cls++) {
        e->blk_cls_off[cls] = (int32_t)blk_tab_h.size();
        for (int u = 0; u < b->n_units; u++)
            if (cls == 0 || e->units[(size_t)u].E == cls)
                for (int k = 0; k < e->units[(size_t)u].nblk; k += param_group(e->units[(size_t)u].E)) blk_tab_h.push_back(BlockRef{u, k});
    }
    e->blk_cls_off[kMaxEp + 1] = (int32_t)blk_tab_h.size();
    for (int cls = 1; cls <= kMaxEp; cls++)
        if (e->tile_cls_off[cls + 1] > e->tile_cls_off[cls]) {
            int rs = ensure_class_stream(e, cls); if (rs != TW_OK) return rs;
        }
    for (int j = 0; j < 3; j++)
        if (e->sel_stream[j] == nullptr) HIPCHK(hipStreamCreate(&e->sel_stream[j]));
    const int64_t n_in_total = b->unit_in_off[b->n_units], n_out_total = b->ep_off[epi];
    if (n_in_total >= (1ll << 31) || n_out_total >= (1ll << 31)) return fail(e, TW_ERR_ARG, "batch exceeds 2^31 spans");
    if (gaps >= (1ll << 31)) return fail(e, TW_ERR_ARG, "batch too large: sum of nslot*n_in must stay below 2^31");
    std::vector<int32_t> slot_unit_h;
    std::vector<uint8_t> slot_scored_h;
    std::vector<uint32_t> seg_gap_h, seg_gap_end_h;  // gap rows of the scored slots only (the others stay NaN and are never fitted)
    for (int u = 0; u < b->n_units; u++) {
        const UnitDev& U = e->units[(size_t)u];
        const int E = U.E;
        for (int q = 0; q < U.nslot; q++) {
            bool scored;
            if (q < E) scored = U.npred[q] == 0;
            else if (q < E + E * E) {
                const int p = (q - E) / E, en = (q - E) % E;
                scored = false;
                for (int j = 0; j < U.npred[en]; j++) scored |= (U.pred_list[en][j] == p && U.pred_prim[en][j]);
            } else scored = true;
            slot_unit_h.push_back(u);
            slot_scored_h.push_back(scored ? 1 : 0);
            if (scored) {
                seg_gap_h.push_back((uint32_t)(e->gs_off_h[(size_t)u] + (int64_t)q * U.n_in));
                seg_gap_end_h.push_back((uint32_t)(e->gs_off_h[(size_t)u] + (int64_t)(q + 1) * U.n_in));
            }
        }
    }
    e->n_gap_rows = (int64_t)seg_gap_h.size();
    std::vector<uint32_t> seg_gap_dst_h(seg_gap_h.size());
    e->n_gap_scored = 0;
    for (size_t r = 0; r < seg_gap_h.size(); r++) { seg_gap_dst_h[r] = (uint32_t)e->n_gap_scored; e->n_gap_scored += seg_gap_end_h[r] - seg_gap_h[r]; }
    seg_in[(size_t)b->n_units] = (uint32_t)n_in_total;
    seg_out.push_back((uint32_t)n_out_total);
    e->n_seg_out = (int)seg_out.size() - 1;
    e->n_ie = ie; e->n_gp = gp; e->n_slots = slots; e->n_gaps = gaps;

    Dev& P = e->P;
    P = Dev{};
    P.n_units = b->n_units;
    P.n_tiles = (int32_t)e->tiles.size();
    P.tile_spans = e->K.tile;
    P.n_in_total = n_in_total;
    P.n_out_total = n_out_total;
    P.batch_size = b->batch_size;
    P.batch_mis = b->batch_size_mis;
    P.split_twins = e->K.split_twins;
    P.defer_min_e = e->K.defer_min_e;
    P.lean_min_e = e->K.lean_min_e;
    P.lean_grid = e->K.lean_grid;
    P.tile_max_deep = e->K.tile_max_deep;
    P.tile_rank = e->K.tile_rank;
    int rc;
    e->arena_req.clear();
    e->arena_open = true;
    UnitDev* d_units; TileDev* d_tiles; int64_t *d_is, *d_ie, *d_os, *d_oe, *d_gs;
    DEV_ALLOC(d_units, P.n_units); DEV_ALLOC(d_tiles, P.n_tiles);
    DEV_ALLOC(d_is, n_in_total); DEV_ALLOC(d_ie, n_in_total); DEV_ALLOC(d_os, n_out_total); DEV_ALLOC(d_oe, n_out_total);
    DEV_ALLOC(d_gs, P.n_units);
    DEV_ALLOC(P.in_end_sorted, n_in_total); DEV_ALLOC(P.out_end_sorted, n_out_total);
    DEV_ALLOC(P.gparam, gp * 4);
    DEV_ALLOC(e->mix_n_dev, slots); DEV_ALLOC(e->mix_p_dev, slots * kMaxComp * 3); DEV_ALLOC(e->mix_c_dev, slots * kMaxComp * 4);
    DEV_ALLOC(P.pm_val, n_in_total); DEV_ALLOC(P.pm_idx, n_in_total); DEV_ALLOC(P.pc, n_in_total + 1); DEV_ALLOC(P.seg, n_in_total);
    DEV_ALLOC(P.win_end, n_in_total); DEV_ALLOC(P.wid, n_in_total); DEV_ALLOC(P.w_last, n_in_total);
    DEV_ALLOC(P.unit_nwin, P.n_units); DEV_ALLOC(P.w_dirty, n_in_total); DEV_ALLOC(P.w_conf, n_in_total);
    DEV_ALLOC(P.tk_n, n_in_total); DEV_ALLOC(P.leaves, n_in_total); DEV_ALLOC(P.leaves0, n_in_total); DEV_ALLOC(P.chosen, n_in_total); DEV_ALLOC(P.rep, n_in_total);
    DEV_ALLOC(P.tkr_n, n_in_total);
    DEV_ALLOC(P.tk_idx, ie * kTopK); DEV_ALLOC(P.tkr_idx, ie * kTopK);
    DEV_ALLOC(P.tk_score, n_in_total * kTopK); DEV_ALLOC(P.tkr_score, n_in_total * kTopK);
    DEV_ALLOC(P.c_lo, ie); DEV_ALLOC(P.c_hi, ie); DEV_ALLOC(P.c_bits, ie * kCandWords); DEV_ALLOC(P.parent, ie);
    DEV_ALLOC(P.gone, ie * kCandWords); DEV_ALLOC(P.gone_valid, n_in_total); DEV_ALLOC(P.leaves_r, n_in_total);
    DEV_ALLOC(P.frontier, (int64_t)kFrontierSlots * 2 * kFrontierCap); 
    // long tuple lists: a pool that grows with the batch (one list per 16 k incoming spans, 48 ... 512 of 32 MB each; recycled)
    P.frontier_big_slots = (int32_t)std::min<int64_t>(std::max<int64_t>(n_in_total / 16384, kFrontierBigSlots), std::max(kFrontierBigSlots, 512));
    DEV_ALLOC(P.frontier_big, (int64_t)P.frontier_big_slots * 2 * kFrontierBigCap);
    DEV_ALLOC(P.pair_pool, (int64_t)kPairSlots * kPairSpill);
    DEV_ALLOC(P.owner, n_out_total);
    DEV_ALLOC(P.gaps, gaps);
    DEV_ALLOC(e->tile_ids, (int64_t)tile_ids_h.size());
    DEV_ALLOC(e->blk_tab, (int64_t)blk_tab_h.size());
    DEV_ALLOC(P.heavy_in_unit, n_in_total); DEV_ALLOC(P.heavy_in_idx, n_in_total);
    {   // long enumerations: a list entry per span plus the extra entries of the split ones (an eighth of the class + 64), two
        // scratch slots per extra entry
        int64_t big_total = 0, slots = 0, want = 0;
        for (int cls = 0; cls <= kMaxEp; cls++) want += 2 * part_extra(e, cls, heavy_off_h[cls + 1] - heavy_off_h[cls]);
        // (a scratch slot is 4.4 KB, most of it the log of a part in log mode: at most TW_PART_SLOTS_MAX slots, 16 M = 70 GB, whatever the batch)
        const int64_t slots_max = e->K.part_slots_max;
        for (int cls = 0; cls <= kMaxEp; cls++) {
            const int64_t n_cls = heavy_off_h[cls + 1] - heavy_off_h[cls];
            int64_t extra = part_extra(e, cls, n_cls);
            if (want > slots_max && extra > 64) extra = std::max<int64_t>((int64_t)((double)extra * (double)slots_max / (double)want), std::min<int64_t>(n_cls / 8 + 64, extra));
            P.heavy_big_off[cls] = (int32_t)big_total; P.part_off[cls] = (int32_t)slots;
            big_total += n_cls + extra; slots += 2 * extra;
        }
        P.heavy_big_off[kMaxEp + 1] = (int32_t)big_total; P.part_off[kMaxEp + 1] = (int32_t)slots;
        DEV_ALLOC(P.heavy_big_unit, big_total); DEV_ALLOC(P.heavy_big_idx, big_total);
        DEV_ALLOC(P.heavy_big_part, big_total); DEV_ALLOC(P.heavy_big_slot, big_total);
        DEV_ALLOC(P.fb_unit, big_total); DEV_ALLOC(P.fb_idx, big_total); DEV_ALLOC(P.fb_part, big_total); DEV_ALLOC(P.fb_slot, big_total);
        DEV_ALLOC(P.split_unit, slots); DEV_ALLOC(P.split_idx, slots); DEV_ALLOC(P.split_slot, slots); DEV_ALLOC(P.split_parts, slots);
        DEV_ALLOC(P.part_n, slots); DEV_ALLOC(P.part_leaves, slots); DEV_ALLOC(P.part_score, slots * kTopK); DEV_ALLOC(P.part_idx, slots * kTopK * kMaxEp);
        DEV_ALLOC(P.part_bits, slots * kMaxEp * kCandWords);
        DEV_ALLOC(P.part_logn, slots); DEV_ALLOC(P.part_log_sc, slots * kPartLogCap); DEV_ALLOC(P.part_log_ix, slots * kPartLogCap);
        DEV_ALLOC(P.part_lo, slots); DEV_ALLOC(P.part_hi, slots); DEV_ALLOC(P.part_lvl, slots);
        // the arena of the deferred spans' prefix lists: a few thousand entries per span that defers, recycled every pass
        int64_t deep = 0;
        for (int cls = std::max(P.defer_min_e, 3); cls <= kMaxEp; cls++) deep += heavy_off_h[cls + 1] - heavy_off_h[cls];
        P.defer_cap = (int32_t)(deep > 0 ? std::min<int64_t>(std::max<int64_t>(deep * kDeferListPerSpan, kDeferListMin), 1ll << 28) : 1);
        DEV_ALLOC(P.defer_list, P.defer_cap);
    }
    for (int cls = 0; cls <= kMaxEp + 1; cls++) P.heavy_in_off[cls] = heavy_off_h[cls];
    DEV_ALLOC(P.prof, 32); DEV_ALLOC(e->key_acc, 2);
    const int64_t sel_cap = (int64_t)P.n_tiles * e->K.tile + 1;   // every segment of the selection lists has room for all windows of its tiles
    {   // the counter block (every array on a 128-byte line of its own: their atomics come from different kernels)
        int64_t at = 0;
        auto take = [&](int64_t ints) { const int64_t o = at; at += (ints + 31) / 32 * 32; return o; };
        const int64_t o_hc = take(kSelSlots * 4 * kSelSeg * kCtrStride), o_hn = take(kSelSlots * 8), o_ic = take(2 * (kMaxEp + 1)), o_in = take(8 * (kMaxEp + 1)), o_bc = take(kMaxEp + 1),
                      o_rc = take(1), o_rd = take(kMaxEp + 1), o_fc = take(kMaxEp + 1);
        e->ctr_round_ints = at;
        const int64_t o_pu = take(kMaxEp + 1), o_sc = take(kMaxEp + 1), o_dc = take(kMaxEp + 1), o_du = take(1), o_err = take(1), o_nd = take(P.n_units), o_us = take((int64_t)P.n_units * 16);
        const int64_t o_dr = take(kMaxEp + 1), o_ft = take(kMaxEp + 1), o_aw = take(kMaxEp + 1);
        const int64_t o_fn = take(kFrontierSlots), o_fb = take(P.frontier_big_slots), o_pb = take(kPairSlots);   // flags of the tuple-list pools (given back by the kernels themselves)
        e->ctr_pass_ints = at;
        auto place = [=](void* q) {
            Dev& D = e->P;
            int32_t* c = e->ctr = (int32_t*)q;
            D.heavy_count = c + o_hc; D.heavy_next = c + o_hn; D.heavy_in_count = c + o_ic; D.heavy_in_next = c + o_in; D.heavy_big_count = c + o_bc;
            D.round_changed = c + o_rc; D.frontier_busy = c + o_fn; D.frontier_big_busy = c + o_fb;
            D.defer_count = c + o_dc; D.defer_used = c + o_du;
            D.part_used = c + o_pu; D.split_count = c + o_sc; D.err = c + o_err; D.unit_ndirty = c + o_nd;
            D.redo_count = c + o_rd; D.fb_count = c + o_fc; D.defer_refused = c + o_dr; D.fb_total = c + o_ft; D.pair_busy = c + o_pb; D.any_wide = c + o_aw;
            D.unit_stats = (int64_t*)(c + o_us);
        };
        if (e->arena_open) e->arena_req.emplace_back(place, ((size_t)at * sizeof(int32_t) + 255) / 256 * 256);   // (placed by arena_commit, like the rest)
        else { DEV_ALLOC(e->ctr, at); place(e->ctr); }
    }
    DEV_ALLOC(P.heavy_unit, sel_cap); DEV_ALLOC(P.heavy_win, sel_cap);
    DEV_ALLOC(P.tiny_unit, sel_cap); DEV_ALLOC(P.tiny_win, sel_cap);
    DEV_ALLOC(P.rheavy_unit, sel_cap); DEV_ALLOC(P.rheavy_win, sel_cap); DEV_ALLOC(P.rtiny_unit, sel_cap); DEV_ALLOC(P.rtiny_win, sel_cap);
    DEV_ALLOC(P.hard_unit, sel_cap / (kBruteMax + 1) + 1 + kSelSlots); DEV_ALLOC(P.hard_win, sel_cap / (kBruteMax + 1) + 1 + kSelSlots);   // (a searched window holds more than kBruteMax spans)
    DEV_ALLOC(e->rank_in, n_in_total); DEV_ALLOC(e->rank_out, n_out_total);
    DEV_ALLOC(e->agg_pair, P.n_tiles); DEV_ALLOC(e->agg_i32, P.n_tiles); DEV_ALLOC(e->agg_i32b, P.n_tiles);
    DEV_ALLOC(e->seg_in, (int64_t)seg_in.size()); DEV_ALLOC(e->seg_out, (int64_t)seg_out.size());
    DEV_ALLOC(e->gaps_sorted, gaps); DEV_ALLOC(e->fit_models, slots * kMaxComp * kModelStride);
    DEV_ALLOC(e->fit_uval, gaps); DEV_ALLOC(e->fit_ustart, gaps); DEV_ALLOC(e->fit_row_n, 2 * slots + 1);   // samples, distinct values (fit_row_uniq, set behind arena_commit) and the refusal flag of k_fit_runs: one copy to the host, fit_prepare
    DEV_ALLOC(e->fit_tape, slots * kFitRowTape); DEV_ALLOC(e->fit_tape_off, slots); DEV_ALLOC(e->fit_tape100, kMaxComp * 13);
    e->fit_tape_cap = slots * kFitRowTape;
    DEV_ALLOC(e->fit_centres, slots * kMaxComp * (kMaxComp + 1));
    DEV_ALLOC(e->fit_spec_centres, slots * (kMaxComp + 1)); DEV_ALLOC(e->fit_spec_p, slots * kMaxComp * 3);
    DEV_ALLOC(e->fit_spec_failed, slots); DEV_ALLOC(e->fit_spec_ctr, 2);
    DEV_ALLOC(e->fit_order_dev, slots * (2 * kMaxComp));
    e->fit_order_h.clear();
    DEV_ALLOC(e->slot_unit, slots); DEV_ALLOC(e->slot_scored, slots);
    DEV_ALLOC(e->seg_gap, (int64_t)seg_gap_h.size()); DEV_ALLOC(e->seg_gap_end, (int64_t)seg_gap_end_h.size()); DEV_ALLOC(e->seg_gap_dst, (int64_t)seg_gap_dst_h.size());
    e->comp_cap = std::max(std::max(n_in_total, n_out_total), e->n_gap_scored);
    DEV_ALLOC(e->comp_a, e->comp_cap); DEV_ALLOC(e->comp_b, e->comp_cap);
    // skip mode: per unit the start-ordered view of every endpoint list (TallySkipSpans sorts the lists in place,
    // traceweaver_v3.py:968-971; the top_k_2 enumeration walks that order), time windows, pools, (mean, std) table, draw counters
    e->skip_mode = b->skip != nullptr;
    std::vector<int32_t> perm_h, pool_h;
    std::vector<int64_t> tw_h;
    std::vector<double> dist_h;
    std::vector<SkipUnitDev> skip_h;
    std::vector<int64_t> sk_tw_off, sk_pool_off, sk_dist_off;
    if (e->skip_mode) {
        perm_h.resize((size_t)n_out_total);
        for (int u = 0; u < b->n_units; u++) {
            const UnitDev& U = e->units[(size_t)u];
            const tw_skip_unit& K = b->skip[u];
            for (int k = 0; k < U.E; k++) {
                const int64_t a = U.ep_off[k], m = U.ep_off[k + 1] - a;
                std::vector<int32_t> idx((size_t)m);
                for (int64_t q = 0; q < m; q++) idx[(size_t)q] = (int32_t)q;
                std::stable_sort(idx.begin(), idx.end(), [&](int32_t x, int32_t y) { return b->out_start[a + x] < b->out_start[a + y]; });
                std::copy(idx.begin(), idx.end(), perm_h.begin() + a);
            }
            sk_tw_off.push_back((int64_t)tw_h.size()); sk_pool_off.push_back((int64_t)pool_h.size()); sk_dist_off.push_back((int64_t)dist_h.size());
            tw_h.insert(tw_h.end(), K.tw_start, K.tw_start + K.n_tw);
            pool_h.insert(pool_h.end(), K.pool, K.pool + (int64_t)U.E * K.n_tw);
            dist_h.insert(dist_h.end(), K.dist, K.dist + (int64_t)(U.E + 1) * (U.E + 1) * 2);
        }
        e->skip_fetch_n = (int64_t)pool_h.size();
        DEV_ALLOC(e->skip_units, b->n_units); DEV_ALLOC(e->skip_perm, n_out_total); DEV_ALLOC(e->skip_tw, (int64_t)tw_h.size());
        DEV_ALLOC(e->skip_pool, (int64_t)pool_h.size()); DEV_ALLOC(e->skip_dist, (int64_t)dist_h.size()); DEV_ALLOC(e->skip_fetch, e->skip_fetch_n);
    }
    rc = arena_commit(e);
    if (rc != TW_OK) return rc;
    e->fit_row_uniq = e->fit_row_n + slots;   // (one block; the arena has placed it only now)
    if (e->skip_mode) {
        for (int u = 0; u < b->n_units; u++) {
            SkipUnitDev K{};
            K.perm = e->skip_perm; K.tw_start = e->skip_tw + sk_tw_off[(size_t)u]; K.pool = e->skip_pool + sk_pool_off[(size_t)u];
            K.dist = e->skip_dist + sk_dist_off[(size_t)u]; K.fetches = e->skip_fetch + sk_pool_off[(size_t)u]; K.n_tw = b->skip[u].n_tw;
            skip_h.push_back(K);
        }
        HIPCHK(hipMemcpyAsync(e->skip_units, skip_h.data(), sizeof(SkipUnitDev) * skip_h.size(), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->skip_perm, perm_h.data(), sizeof(int32_t) * perm_h.size(), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->skip_tw, tw_h.data(), sizeof(int64_t) * tw_h.size(), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->skip_pool, pool_h.data(), sizeof(int32_t) * pool_h.size(), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->skip_dist, dist_h.data(), sizeof(double) * dist_h.size(), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));   // the staging vectors go out of scope
    }
    HIPCHK(hipMemsetAsync(P.prof, 0, sizeof(unsigned long long) * 32, e->stream));
    HIPCHK(hipMemsetAsync(P.prof + 10, 0xff, sizeof(unsigned long long), e->stream));
    P.units = d_units; P.tiles = d_tiles;
    P.in_start = d_is; P.in_end = d_ie; P.out_start = d_os; P.out_end = d_oe;
    P.gs_off = d_gs;
    P.mix_n = e->mix_n_dev; P.mix_c = e->mix_c_dev;
    e->sort_tmp = nullptr; e->sort_tmp_bytes = 0;
    const hipMemcpyKind kind = spans_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIPCHK(hipMemcpyAsync(d_is, b->in_start, sizeof(int64_t) * n_in_total, kind, e->stream));
    HIPCHK(hipMemcpyAsync(d_ie, b->in_end, sizeof(int64_t) * n_in_total, kind, e->stream));
    HIPCHK(hipMemcpyAsync(d_os, b->out_start, sizeof(int64_t) * n_out_total, kind, e->stream));
    HIPCHK(hipMemcpyAsync(d_oe, b->out_end, sizeof(int64_t) * n_out_total, kind, e->stream));
    HIPCHK(hipMemcpyAsync(d_units, e->units.data(), sizeof(UnitDev) * e->units.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_tiles, e->tiles.data(), sizeof(TileDev) * e->tiles.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_gs, e->gs_off_h.data(), sizeof(int64_t) * e->gs_off_h.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->seg_in, seg_in.data(), sizeof(uint32_t) * seg_in.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->seg_out, seg_out.data(), sizeof(uint32_t) * seg_out.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->tile_ids, tile_ids_h.data(), sizeof(int32_t) * tile_ids_h.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->blk_tab, blk_tab_h.data(), sizeof(BlockRef) * blk_tab_h.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->slot_unit, slot_unit_h.data(), sizeof(int32_t) * slot_unit_h.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->seg_gap, seg_gap_h.data(), sizeof(uint32_t) * seg_gap_h.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->seg_gap_end, seg_gap_end_h.data(), sizeof(uint32_t) * seg_gap_end_h.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->seg_gap_dst, seg_gap_dst_h.data(), sizeof(uint32_t) * seg_gap_dst_h.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->slot_scored, slot_scored_h.data(), slot_scored_h.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(P.gaps, 0xff, sizeof(double) * std::max<int64_t>(gaps, 1), e->stream));  // all-ones = NaN: rows of unscored slots
    HIPCHK(hipMemsetAsync(P.pc, 0, (size_t)n_in_total + 1, e->stream));
    // top-5 lists: all-ones = index -1 / score NaN; the enumeration kernels write only the entries a span has
    HIPCHK(hipMemsetAsync(P.tk_idx, 0xff, sizeof(int32_t) * (size_t)std::max<int64_t>(ie * kTopK, 1), e->stream));
    HIPCHK(hipMemsetAsync(P.tk_score, 0xff, sizeof(double) * (size_t)std::max<int64_t>(n_in_total * kTopK, 1), e->stream));
    HIPCHK(hipMemsetAsync(e->mix_n_dev, 0, sizeof(int32_t) * std::max<int64_t>(slots, 1), e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->scaled_upload = b->unit_time_scale != nullptr;
    e->state = ST_LOADED; e->pass1_done = false;
    for (int E = 0; E <= kMaxEp; E++) { e->wide_pass1[E] = -1; e->hard_pass1[E] = -1; e->split_pass1[E] = -1; }
    return TW_OK;
}

int tw_run_pass1(tw_engine* e) {
    if (e == nullptr) return TW_ERR_ARG;
    if (e->state < ST_LOADED) return fail(e, TW_ERR_STATE, "tw_run_pass1 before tw_load_batch");
    HIPCHK(hipSetDevice(e->device));
    drop_forest(e);   // (the parent arrays a stitched forest was made from are overwritten)
    const int rc = run_pass(e, 1);
    e->fit_prepared = false; e->fit_runs_pending = false; e->fit_rows_h_valid = false;
    if (rc == TW_OK) { e->state = ST_PASS1; e->pass1_done = true; }
    return rc;
}

int tw_get_gaps(tw_engine* e, double* gaps) {
    if (e == nullptr || gaps == nullptr) return TW_ERR_ARG;
    if (e->state != ST_PASS1) return fail(e, TW_ERR_STATE, "tw_get_gaps is valid right after tw_run_pass1");
    if (e->skip_mode) return fail(e, TW_ERR_STATE, "a skip-mode batch runs one pass (traceweaver_v3.py:1155-1156): there is no refit");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(gaps, e->P.gaps, sizeof(double) * e->n_gaps, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TW_OK;
}

int tw_set_gaps(tw_engine* e, const double* gaps) {
    if (e == nullptr || gaps == nullptr) return TW_ERR_ARG;
    if (e->state < ST_LOADED) return fail(e, TW_ERR_STATE, "tw_set_gaps before tw_load_batch");
    if (e->skip_mode) return fail(e, TW_ERR_STATE, "a skip-mode batch runs one pass (traceweaver_v3.py:1155-1156): there is no refit");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(e->P.gaps, gaps, sizeof(double) * e->n_gaps, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->fit_prepared = false; e->fit_runs_pending = false; e->fit_rows_h_valid = false;
    e->state = ST_PASS1;
    return TW_OK;
}

int tw_device_buffers(tw_engine* e, tw_device_view* out) {
    if (e == nullptr || out == nullptr) return TW_ERR_ARG;
    if (e->state < ST_LOADED) return fail(e, TW_ERR_STATE, "tw_device_buffers before tw_load_batch");
    out->parent = e->P.parent; out->parent_count = e->n_ie;
    out->gaps = e->P.gaps; out->gaps_count = e->n_gaps;
    out->device = e->device;
    return TW_OK;
}

int tw_set_gaps_device(tw_engine* e, const double* dev_gaps) {
    if (e == nullptr || dev_gaps == nullptr) return TW_ERR_ARG;
    if (e->state < ST_LOADED) return fail(e, TW_ERR_STATE, "tw_set_gaps_device before tw_load_batch");
    if (e->skip_mode) return fail(e, TW_ERR_STATE, "a skip-mode batch runs one pass (traceweaver_v3.py:1155-1156): there is no refit");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(e->P.gaps, dev_gaps, sizeof(double) * e->n_gaps, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->fit_prepared = false; e->fit_runs_pending = false; e->fit_rows_h_valid = false;
    e->state = ST_PASS1;
    return TW_OK;
}

int tw_set_mixtures(tw_engine* e, const int32_t* mix_n, const double* mix_p) {
    if (e == nullptr || mix_n == nullptr || mix_p == nullptr) return TW_ERR_ARG;
    if (e->state < ST_PASS1) return fail(e, TW_ERR_STATE, "tw_set_mixtures before tw_run_pass1");
    if (e->skip_mode) return fail(e, TW_ERR_STATE, "a skip-mode batch runs one pass (traceweaver_v3.py:1155-1156): there is no second pass");
    HIPCHK(hipSetDevice(e->device));
    for (int64_t q = 0; q < e->n_slots; q++)
        if (mix_n[q] < 0 || mix_n[q] > TW_MAX_COMP) return fail(e, TW_ERR_ARG, "mixture component count outside [0, TW_MAX_COMP]");
    HIPCHK(hipMemcpyAsync(e->mix_n_dev, mix_n, sizeof(int32_t) * e->n_slots, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->mix_p_dev, mix_p, sizeof(double) * e->n_slots * kMaxComp * 3, hipMemcpyHostToDevice, e->stream));
    const int64_t total = e->n_slots * kMaxComp;
    hipLaunchKernelGGL(k_mix_consts, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, e->stream, (const double*)e->mix_p_dev, (const int32_t*)e->mix_n_dev, (const int32_t*)e->slot_unit, e->P.units, e->mix_c_dev, total);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    e->fit_order_h.clear();   // (these mixtures come from no refit: tw_get_fit_order reports none)
    e->state = ST_MIX;
    return TW_OK;
}

namespace {

FitDev fit_dev(tw_engine* e) {
    FitDev F{};
    F.units = e->P.units; F.n_units = e->P.n_units; F.n_slots = e->n_slots; F.gaps = e->P.gaps; F.sorted = e->gaps_sorted;
    F.gs_off = e->P.gs_off; F.slot_unit = e->slot_unit; F.slot_scored = e->slot_scored; F.models = e->fit_models; F.mix_n = e->mix_n_dev; F.mix_p = e->mix_p_dev;
    F.uval = e->fit_uval; F.ustart = e->fit_ustart; F.row_n = e->fit_row_n; F.row_uniq = e->fit_row_uniq;
    F.tape = e->fit_tape; F.tape_off = e->fit_tape_off; F.tape100 = e->fit_tape100; F.err = e->P.err; F.centres = e->fit_centres;
    F.full_mode = FIT_FINAL; F.spec_centres = e->fit_spec_centres; F.spec_p = e->fit_spec_p; F.spec_failed = e->fit_spec_failed; F.spec_ctr = e->fit_spec_ctr;
    return F;
}

// Turns every scored gap row into (value, multiplicity) runs; idempotent per pass-1 result.  Default route: k_fit_runs (a hash
// table per row in LDS, the row read once); rows it cannot take -- and TW_FIT_SORT=1 -- go the sort route below: composite-key
// radix sort of all rows + k_fit_compress.  Both leave the same arrays (uval, ustart, row_n, row_uniq).
// (in two halves: fit_prepare_launch queues k_fit_runs and returns -- the caller has host work of its own to do meanwhile, the
// uniforms of the k-means++ draws -- and fit_prepare waits for it, reads whether a row was refused and runs the sort route then)
int fit_prepare_launch(tw_engine* e) {
    e->fit_runs_pending = false;
    if (e->fit_prepared || e->K.fit_sort != 0) return TW_OK;
    int32_t* flag = e->fit_row_n + 2 * e->n_slots;
    HIPCHK(hipMemsetAsync(flag, 0, sizeof(int32_t), e->stream));
#ifdef TW_HOST_EMULATION
    const int runs_threads = e->K.coop;
#else
    const int runs_threads = e->K.coop >= 64 ? kRunsThreads : e->K.coop;
#endif
    hipLaunchKernelGGL(k_fit_runs, dim3((unsigned)e->n_slots), dim3(runs_threads), 0, e->stream, fit_dev(e), flag);
    HIPCHK(hipGetLastError());
    e->fit_runs_pending = true;
    return TW_OK;
}
// The rows' sample and distinct-value counts for the host (tw_fit_rows, fit_order), with the refusal flag of k_fit_runs behind them
// (the three are one block): one copy queued behind the kernel that leaves them, where the hash route copied the flag alone.
int fit_rows_to_host(tw_engine* e) {
    e->fit_rows_h.resize((size_t)(2 * e->n_slots + 1));
    HIPCHK(hipMemcpyAsync(e->fit_rows_h.data(), e->fit_row_n, sizeof(int32_t) * e->fit_rows_h.size(), hipMemcpyDeviceToHost, e->stream));
    return TW_OK;
}
int fit_prepare(tw_engine* e) {
    if (e->fit_prepared) return TW_OK;
    if (e->K.fit_sort == 0) {
        if (!e->fit_runs_pending) { int rl = fit_prepare_launch(e); if (rl != TW_OK) return rl; }
        e->fit_runs_pending = false;
        TWCHK(fit_rows_to_host(e));
        HIPCHK(hipStreamSynchronize(e->stream));
        if (!e->fit_rows_h[(size_t)(2 * e->n_slots)]) {   // no row was refused
            e->fit_prepared = true;
            e->fit_rows_h_valid = true;
            return TW_OK;
        }
    }
    const unsigned size = (unsigned)e->n_gaps, nseg = (unsigned)e->n_gap_rows;
    // gap samples are non-negative integers (and NaN = 0x7ff8...0) stored as doubles: their low mantissa bits
    // are all zero, the sort starts at the lowest bit set anywhere.  A negative key (none can occur: children
    // lie inside their parent and follow their predecessors) would flip rocprim's key transform -> full width.
    unsigned long long kb[2];
    int rck = key_bits(e, e->P.gaps, e->seg_gap, e->seg_gap_end, (int)nseg, e->n_gaps, kb);
    if (rck != TW_OK) return rck;
    unsigned begin_bit = 0;
    if (kb[1] != 0 && !(kb[1] >> 63)) while (!((kb[1] >> begin_bit) & 1)) begin_bit++;
    if (kb[1] >> 63) {  // a negative sample: leave the key transform to rocprim (never seen; see above)
        TWCHK(rocprim_call(e, [&](void* tmp, size_t& bytes) {
            return rocprim::segmented_radix_sort_keys(tmp, bytes, (const double*)e->P.gaps, e->gaps_sorted, size, nseg, e->seg_gap, e->seg_gap_end, 0, 64, e->stream);
        }));
    } else {  // non-negative doubles order like their bit patterns
        int rcs = sort_rows(e, (const unsigned long long*)e->P.gaps, (unsigned long long*)e->gaps_sorted, size, e->seg_gap, e->seg_gap_end,
                            e->seg_gap_dst, (int)nseg, e->n_gap_scored, begin_bit, 64, 0ull);
        if (rcs != TW_OK) return rcs;
    }
    FitDev F = fit_dev(e);
#ifdef TW_HOST_EMULATION   // (the lane-threaded emulation of the tests runs a host thread per lane: the cooperative size there)
    const int compress_threads = e->K.coop;
#else
    const int compress_threads = e->K.coop >= 64 ? kCompressThreads : e->K.coop;
#endif
    hipLaunchKernelGGL(k_fit_compress, dim3((unsigned)e->n_slots), dim3(compress_threads), 0, e->stream, F);
    HIPCHK(hipGetLastError());
    TWCHK(fit_rows_to_host(e));   // (the rare route: a wait of its own)
    HIPCHK(hipStreamSynchronize(e->stream));
    e->fit_prepared = true;
    e->fit_rows_h_valid = true;
    return TW_OK;
}

// The order tables of a refit (TW_FIT_ORDER).  A workgroup is one whole fit, and a fit's length goes with distinct values x
// components: 10-30 times as long on a row of 10^4 distinct values as on one of 10^3.  The hardware hands workgroups out in index
// order, so in grid order the long fits of the smaller counts start late and end the launch alone; longest first, the span of a
// launch approaches work / CUs.  Every table is a full permutation of its grid -- a dead workgroup keeps its side effects
// (k_fit_em<false> marks a fit that is not made) --: key = distinct values x count of a live block (fit_row's predicate), -1 of a dead
// one; by key descending, then count descending, then slot ascending, so dead blocks come last in index order.
void fit_order(const int32_t* row_uniq, const int32_t* row_n, int64_t n_slots, std::vector<int32_t>& out) {
    out.resize((size_t)(n_slots * 2 * kMaxComp));
    // The rows with a fit, by distinct values descending, then slot ascending: the order of the kFull launches (their key, distinct
    // values x fit_spec_k, grows with the distinct values), and per count k the rows of that count's live blocks -- a prefix, the
    // rows of at least k distinct values -- in the order of their keys.  The model selection's tables merge the counts' lists: the
    // largest key next, of equal keys the larger count; a row sort and a merge of five lists instead of a sort of all blocks.
    // (A row has a fit <=> it has samples: k_fit_runs and k_fit_compress leave row_n = row_uniq = 0 for a slot that is not scored, so
    // fit_row's slot_scored is implied here.)
    std::vector<int32_t> rows;
    rows.reserve((size_t)n_slots);
    for (int64_t q = 0; q < n_slots; q++)
        if (row_n[q] > 0 && row_uniq[q] >= 1) rows.push_back((int32_t)q);
    std::stable_sort(rows.begin(), rows.end(), [&](int32_t a, int32_t b) { return row_uniq[a] > row_uniq[b]; });
    int64_t len[kMaxComp + 1];   // rows of at least k distinct values
    for (int k = 1; k <= kMaxComp; k++)
        len[k] = std::partition_point(rows.begin(), rows.end(), [&](int32_t q) { return row_uniq[q] >= k; }) - rows.begin();
    const auto merge = [&](int32_t* tab, int k_min) {   // the grid of counts 5..k_min: block (5 - k) * n_slots + q
        int64_t at = 0, pos[kMaxComp + 1] = {};
        for (;;) {
            int best = 0;
            int64_t best_key = -1;
            for (int k = kMaxComp; k >= k_min; k--) {
                if (pos[k] >= len[k]) continue;
                const int64_t key = (int64_t)row_uniq[rows[(size_t)pos[k]]] * k;
                if (key > best_key) { best_key = key; best = k; }
            }
            if (best == 0) break;
            tab[at++] = (int32_t)((kMaxComp - best) * n_slots + rows[(size_t)pos[best]++]);
        }
        for (int k = kMaxComp; k >= k_min; k--)   // the blocks without a fit, in index order
            for (int64_t q = 0; q < n_slots; q++)
                if (!(row_n[q] > 0 && k <= row_uniq[q])) tab[at++] = (int32_t)((kMaxComp - k) * n_slots + q);
    };
    merge(out.data(), 2);                                  // k_fit_seed<false>
    merge(out.data() + n_slots * (kMaxComp - 1), 1);       // k_fit_em<false>
    int32_t* tab = out.data() + n_slots * (2 * kMaxComp - 1);
    int64_t at = 0;
    for (const int32_t q : rows) tab[at++] = q;
    for (int64_t q = 0; q < n_slots; q++)
        if (!(row_n[q] > 0 && row_uniq[q] >= 1)) tab[at++] = (int32_t)q;
}

// The fits themselves; the tape and the slots' offsets are resident in e->fit_tape / e->fit_tape_off.
int fit_run(tw_engine* e) {
    static const std::vector<double> tape100 = [] {   // GaussianMixture(n, random_state=100): a fresh MT19937(100) per fit
        std::vector<double> t((size_t)kMaxComp * 13, 0.0);
        for (int k = 1; k <= kMaxComp; k++) {
            Mt19937 r(100u);
            for (int j = 0; j < fit_draws(k); j++) t[(size_t)(k - 1) * 13 + j] = r.random_sample();
        }
        return t;
    }();
    HIPCHK(hipMemcpyAsync(e->fit_tape100, tape100.data(), sizeof(double) * tape100.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(e->P.err, 0, sizeof(int32_t), e->stream));
    FitDev F = fit_dev(e);
    const int threads = e->K.coop >= 64 ? kFitThreads : e->K.coop;
    // The order tables (fit_order), uploaded with the tapes: null = every launch in grid order
    const int32_t *order_seed = nullptr, *order_em = nullptr, *order_row = nullptr;
    e->fit_order_h.clear();
    e->fit_order_host_ms = 0.0;
    if (e->K.fit_order != 0) {
        if (!e->fit_rows_h_valid) return fail(e, TW_ERR_STATE, "refit: the rows' counts are not on the host (fit_prepare leaves them there)");
        const auto h0 = std::chrono::steady_clock::now();
        fit_order(e->fit_rows_h.data() + e->n_slots, e->fit_rows_h.data(), e->n_slots, e->fit_order_h);
        HIPCHK(hipMemcpyAsync(e->fit_order_dev, e->fit_order_h.data(), sizeof(int32_t) * e->fit_order_h.size(), hipMemcpyHostToDevice, e->stream));
        e->fit_order_host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
        order_seed = e->fit_order_dev;
        order_em = order_seed + e->n_slots * (kMaxComp - 1);
        order_row = order_em + e->n_slots * kMaxComp;
    }
    // The second stream of the refit is the stream of the batch's first class, idle between the passes: every batch has one
    // (tw_load_batch), and its work is joined to the engine's stream below.  A stream of the refit's own, created in tw_create, took
    // the hardware queue that the class streams created after it would have had (the runtime deals a process' streams onto four
    // queues by default): the deepest class then shared the engine's queue and each pass of the headline was 1 ms longer
    // (profiles/HISTORY.md, round 13).  Borrowed, the streams' queues are those of an engine without the speculative fit; the
    // headline gains the same 1.1 ms with 4 and with 12 hardware queues.  (side_cls = 0 cannot occur for a loaded batch: every unit
    // has at least one endpoint, so some class has tiles and tw_load_batch created its stream; such a refit would run unforked.)
    int side_cls = 0;
    for (int E = kMaxEp; E >= 1; E--)
        if (e->tile_cls_off[E + 1] > e->tile_cls_off[E]) side_cls = E;
    const hipStream_t side = e->cls_stream[side_cls];
    const bool spec = e->K.fit_spec != 0 && side_cls > 0;
    e->fit_spec_count[0] = e->fit_spec_count[1] = 0;
    if (spec) {
        // The final fit GaussianMixture(n_selected, random_state=100) depends on the model selection only through the count; the
        // row, its runs and the tape are fixed by now.  The likeliest count (fit_spec_k) is fitted on the second stream beside
        // the selection, into buffers of its own: the two nearly empty launches behind k_fit_select (one workgroup per row on
        // 256 CUs, as long as the longest fit) leave the chain and their workgroups fill the tails of the two busy ones.  (Queued
        // first: the long rows' fits of the largest count are the longest workgroups of the refit.)
        HIPCHK(hipMemsetAsync(e->fit_spec_ctr, 0, 2 * sizeof(int32_t), e->stream));
        HIPCHK(hipEventRecord(e->fit_fork, e->stream));   // (behind the tapes, the prepared rows and the reset of err)
        HIPCHK(hipStreamWaitEvent(side, e->fit_fork, 0));
        FitDev S = F;
        S.full_mode = FIT_SPEC;
        S.order = order_row;
        hipLaunchKernelGGL(k_fit_seed<true>, dim3((unsigned)e->n_slots), dim3(threads), 0, side, S);
        hipLaunchKernelGGL(k_fit_em<true>, dim3((unsigned)e->n_slots), dim3(threads), 0, side, S);
        HIPCHK(hipEventRecord(e->fit_join, side));
    }
    // Model selection: two launches over all counts, the largest count (the longest fits) first (fit_row)
    F.order = order_seed;
    hipLaunchKernelGGL(k_fit_seed<false>, dim3((unsigned)(e->n_slots * (kMaxComp - 1))), dim3(threads), 0, e->stream, F);
    F.order = order_em;
    hipLaunchKernelGGL(k_fit_em<false>, dim3((unsigned)(e->n_slots * kMaxComp)), dim3(threads), 0, e->stream, F);
    F.order = order_row;
    hipLaunchKernelGGL(k_fit_select, dim3((unsigned)((e->n_slots + 63) / 64)), dim3(64), 0, e->stream, F);
    if (spec) {   // rows that selected the count fitted ahead adopt its result (k_fit_em), the others are fitted now
        HIPCHK(hipStreamWaitEvent(e->stream, e->fit_join, 0));
        F.full_mode = FIT_ADOPT;
    }
    hipLaunchKernelGGL(k_fit_seed<true>, dim3((unsigned)e->n_slots), dim3(threads), 0, e->stream, F);
    hipLaunchKernelGGL(k_fit_em<true>, dim3((unsigned)e->n_slots), dim3(threads), 0, e->stream, F);
    const int64_t total = e->n_slots * kMaxComp;
    hipLaunchKernelGGL(k_mix_consts, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, e->stream, (const double*)e->mix_p_dev, (const int32_t*)e->mix_n_dev, (const int32_t*)e->slot_unit, e->P.units, e->mix_c_dev, total);
    HIPCHK(hipEventRecord(e->ev[EV_END], e->stream));
    HIPCHK(hipGetLastError());
    int32_t kerr = 0;
    HIPCHK(hipMemcpyAsync(&kerr, e->P.err, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (spec) HIPCHK(hipMemcpyAsync(e->fit_spec_count, e->fit_spec_ctr, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, e->ev[EV_BEGIN], e->ev[EV_END]));
    e->fit_ms = f;
    if (kerr != 0)
        return fail(e, kerr, "refit: every model-selection fit of an edge ended in a covariance <= 0 (scikit-learn's ValueError); the reference "
                             "raises there as well (np.argmin of an empty list, traceweaver_v3.py:777-780)");
    e->state = ST_MIX;
    return TW_OK;
}

int fit_check_state(tw_engine* e, const char* who) {
    if (e->state != ST_PASS1) return fail(e, TW_ERR_STATE, std::string(who) + " is valid right after tw_run_pass1");
    if (e->skip_mode) return fail(e, TW_ERR_STATE, "a skip-mode batch runs one pass (traceweaver_v3.py:1155-1156): there is no refit");
    return TW_OK;
}

}  // namespace

int tw_set_fit_seed(tw_engine* e, uint32_t seed) {
    if (e == nullptr) return TW_ERR_ARG;
    e->fit_seed = seed;
    e->fit_rng = Mt19937(seed);
    return TW_OK;
}

int tw_fit_rows(tw_engine* e, int32_t* max_n) {
    if (e == nullptr || max_n == nullptr) return TW_ERR_ARG;
    int rc = fit_check_state(e, "tw_fit_rows");
    if (rc != TW_OK) return rc;
    HIPCHK(hipSetDevice(e->device));
    rc = fit_prepare(e);
    if (rc != TW_OK) return rc;
    for (int64_t q = 0; q < e->n_slots; q++) max_n[q] = std::min<int32_t>(e->fit_rows_h[(size_t)(e->n_slots + q)], kMaxComp);   // (fit_prepare's host copy)
    return TW_OK;
}

int tw_get_fit_order(tw_engine* e, int32_t* order_seed, int32_t* order_em, int32_t* order_row, int32_t* present) {
    if (e == nullptr || order_seed == nullptr || order_em == nullptr || order_row == nullptr || present == nullptr) return TW_ERR_ARG;
    if (e->state < ST_MIX) return fail(e, TW_ERR_STATE, "tw_get_fit_order: no refit has run on the resident batch");
    *present = e->fit_order_h.empty() ? 0 : 1;
    if (*present) {
        const size_t ns = (size_t)e->n_slots, k = (size_t)kMaxComp;
        std::copy_n(e->fit_order_h.data(), ns * (k - 1), order_seed);
        std::copy_n(e->fit_order_h.data() + ns * (k - 1), ns * k, order_em);
        std::copy_n(e->fit_order_h.data() + ns * (2 * k - 1), ns, order_row);
    }
    return TW_OK;
}

int tw_fit_mixtures_tape(tw_engine* e, const double* tape, int64_t tape_len, const int64_t* slot_off) {
    if (e == nullptr || tape == nullptr || slot_off == nullptr || tape_len < 0) return TW_ERR_ARG;
    int rc = fit_check_state(e, "tw_fit_mixtures_tape");
    if (rc != TW_OK) return rc;
    HIPCHK(hipSetDevice(e->device));
    rc = fit_prepare(e);
    if (rc != TW_OK) return rc;
    static const int need[kMaxComp + 1] = {0, 1, 4, 11, 21, 34};
    for (int64_t q = 0; q < e->n_slots; q++) {
        const int m = std::min<int32_t>(e->fit_rows_h[(size_t)(e->n_slots + q)], kMaxComp);
        if (m > 0 && (slot_off[q] < 0 || slot_off[q] + need[m] > tape_len))
            return fail(e, TW_ERR_ARG, "tw_fit_mixtures_tape: the tape does not hold the draws of slot " + std::to_string(q));
    }
    HIPCHK(hipEventRecord(e->ev[EV_BEGIN], e->stream));
    if (tape_len > e->fit_tape_cap) {
        double* p = nullptr;
        rc = dev_alloc(e, &p, tape_len);
        if (rc != TW_OK) return rc;
        e->fit_tape = p;
        e->fit_tape_cap = tape_len;
    }
    HIPCHK(hipMemcpyAsync(e->fit_tape, tape, sizeof(double) * (size_t)std::max<int64_t>(tape_len, 0), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->fit_tape_off, slot_off, sizeof(int64_t) * e->n_slots, hipMemcpyHostToDevice, e->stream));
    return fit_run(e);
}

int tw_fit_mixtures_seeded(tw_engine* e, const uint32_t* unit_seed) {
    if (e == nullptr) return TW_ERR_ARG;
    int rc = fit_check_state(e, "tw_fit_mixtures");
    if (rc != TW_OK) return rc;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipEventRecord(e->ev[EV_BEGIN], e->stream));
    rc = fit_prepare_launch(e);   // (the rows become runs while the host draws the uniforms; fit_prepare below waits for both)
    if (rc != TW_OK) return rc;
    // one block of 34 uniforms per slot: no look at the rows needed, no host round trip.  With unit seeds every unit draws from
    // a stream of its own, so its fit does not depend on which other units share the batch (sharded runs);
    // otherwise all slots draw from the engine's stream in slot order.
    static thread_local std::vector<double> tape;
    static thread_local std::vector<int64_t> off;
    tape.resize((size_t)e->n_slots * kFitRowTape);
    off.resize((size_t)e->n_slots);
    for (int64_t q = 0; q < e->n_slots; q++) off[(size_t)q] = q * kFitRowTape;
    if (unit_seed == nullptr) {
        for (size_t i = 0; i < tape.size(); i++) tape[i] = e->fit_rng.random_sample();
    } else {
        for (size_t u = 0; u < e->units.size(); u++) {
            Mt19937 r(unit_seed[u]);
            const size_t lo = (size_t)e->units[u].slot_off * kFitRowTape, hi = lo + (size_t)e->units[u].nslot * kFitRowTape;
            for (size_t i = lo; i < hi; i++) tape[i] = r.random_sample();
        }
    }
    if ((int64_t)tape.size() > e->fit_tape_cap) return fail(e, TW_ERR_STATE, "tw_fit_mixtures: tape buffer smaller than the batch");
    HIPCHK(hipMemcpyAsync(e->fit_tape, tape.data(), sizeof(double) * tape.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->fit_tape_off, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice, e->stream));
    if (e->fit_prepared) HIPCHK(hipStreamSynchronize(e->stream));   // (the host vectors are reused by the next call; else fit_prepare's wait covers it)
    rc = fit_prepare(e);
    if (rc != TW_OK) return rc;
    return fit_run(e);
}

int tw_fit_mixtures(tw_engine* e) { return tw_fit_mixtures_seeded(e, nullptr); }

int tw_get_mixtures(tw_engine* e, int32_t* mix_n, double* mix_p) {
    if (e == nullptr || mix_n == nullptr || mix_p == nullptr) return TW_ERR_ARG;
    if (e->state < ST_MIX) return fail(e, TW_ERR_STATE, "no mixtures resident (tw_fit_mixtures / tw_set_mixtures first)");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(mix_n, e->mix_n_dev, sizeof(int32_t) * e->n_slots, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(mix_p, e->mix_p_dev, sizeof(double) * e->n_slots * kMaxComp * 3, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TW_OK;
}

int tw_run_pass2(tw_engine* e) {
    if (e == nullptr) return TW_ERR_ARG;
    if (e->state != ST_MIX && e->state != ST_PASS2) return fail(e, TW_ERR_STATE, "tw_run_pass2 needs tw_run_pass1 and tw_set_mixtures first");
    // (tw_set_gaps* + tw_set_mixtures reach ST_MIX on a batch that never ran pass 1 -- an engine that only serves the refit; the second
    // pass reads what the first left behind: cut-offs, window flags, tuple counts)
    if (!e->pass1_done) return fail(e, TW_ERR_STATE, "tw_run_pass2 on a batch whose first pass has not run (tw_run_pass1 first)");
    HIPCHK(hipSetDevice(e->device));
    drop_forest(e);
    const int rc = run_pass(e, 2);
    if (rc == TW_OK) e->state = ST_PASS2;
    return rc;
}

int tw_get_results(tw_engine* e, int pass, const tw_results* r) {
    if (e == nullptr || r == nullptr) return TW_ERR_ARG;
    const bool ok = (pass == 1 && (e->state == ST_PASS1 || e->state == ST_MIX)) || (pass == 2 && e->state == ST_PASS2);
    if (!ok) return fail(e, TW_ERR_STATE, "results of that pass are not resident (fetch pass-1 results before running pass 2)");
    HIPCHK(hipSetDevice(e->device));
    const Dev& P = e->P;
    const int64_t n = P.n_in_total;
    TWCHK(copy_out(e, r->parent, P.parent, e->n_ie));
    TWCHK(copy_out(e, r->topk_idx, P.tk_idx, e->n_ie * kTopK));
    TWCHK(copy_out(e, r->topk_score, P.tk_score, n * kTopK));
    TWCHK(copy_out(e, r->topk_n, P.tk_n, n));
    TWCHK(copy_out(e, r->chosen, P.chosen, n));
    TWCHK(copy_out(e, r->leaves, P.leaves, n));
    TWCHK(copy_out(e, r->window_end, P.win_end, n));
    TWCHK(copy_out(e, r->unit_stats, P.unit_stats, 8 * P.n_units));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TW_OK;
}

int tw_get_gauss_params(tw_engine* e, double* gauss) {
    if (e == nullptr || gauss == nullptr) return TW_ERR_ARG;
    if (e->state < ST_PASS1) return fail(e, TW_ERR_STATE, "tw_get_gauss_params before tw_run_pass1");
    HIPCHK(hipSetDevice(e->device));
    std::vector<double> tmp((size_t)e->n_gp * 4);
    HIPCHK(hipMemcpyAsync(tmp.data(), e->P.gparam, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int64_t q = 0; q < e->n_gp; q++)
        for (int k = 0; k < 3; k++) gauss[q * 3 + k] = tmp[(size_t)q * 4 + k];
    for (const UnitDev& U : e->units)  // the device keeps the means in timestamp units (k_block_params)
        for (int64_t q = U.gp_off; q < U.gp_off + (int64_t)U.nblk * U.nslot; q++) gauss[q * 3] *= U.tscale;
    return TW_OK;
}

int tw_get_timing(tw_engine* e, double* ms, int32_t n) {
    if (e == nullptr || ms == nullptr) return TW_ERR_ARG;
    for (int i = 0; i < n && i < 6; i++) ms[i] = e->ms[i];
    if (n > 6) ms[6] = e->fit_ms;
    if (n > 7) ms[7] = (double)e->rounds;
    if (n > 8) ms[8] = e->host_ms[0];
    if (n > 9) ms[9] = e->host_ms[1];
    for (int i = 0; i < 6 && 10 + i < n; i++) ms[10 + i] = e->st_ms[i];   // the last tw_stitch_traces
    for (int i = 0; i < 3 && 16 + i < n; i++) ms[16 + i] = e->at_ms[i];   // the last tw_attribute_traces
    for (int i = 0; i < 3 && 19 + i < n; i++) ms[19 + i] = e->cf_ms[i];   // the last tw_score_traces
    for (int i = 0; i < 3 && 22 + i < n; i++) ms[22 + i] = e->ds_ms[i];   // the last tw_latency_distributions
    for (int i = 0; i < 3 && 25 + i < n; i++) ms[25 + i] = e->sg_ms[i];   // the last tw_trace_signatures that ran kernels
    for (int i = 0; i < 3 && 28 + i < n; i++) ms[28 + i] = e->pf_ms[i];   // the last tw_class_profiles that ran kernels
    if (n > 31) ms[31] = e->ob_ms;                                        // the last tw_order_bound
    if (n > 32) ms[32] = (double)e->gate_waits;                           // class stages of the last pass that were queued behind the stage gate
    for (int i = 0; i < 2 && 33 + i < n; i++) ms[33 + i] = e->cm_ms[i];   // the last tw_compare_cohorts
    for (int i = 0; i < 2 && 35 + i < n; i++) ms[35 + i] = (double)e->fit_spec_count[i];   // the last refit: rows that adopted the fit made ahead / that were fitted after the selection
    if (n > 37) ms[37] = e->fit_order_host_ms;                            // ... and the host's time for its order tables
    for (int i = 0; i < 3 && 43 + i < n; i++) ms[43 + i] = e->ch_ms[i];   // the last tw_class_history_push / _merge
    for (int i = 0; i < 3 && 46 + i < n; i++) ms[46 + i] = e->fl_ms[i];   // the last tw_filter_traces
    for (int i = 0; i < 3 && 49 + i < n; i++) ms[49 + i] = e->ex_ms[i];   // the last tw_extract_traces (49, 50) / tw_get_extracted (51)
    for (int i = 0; i < 5 && 38 + i < n; i++) ms[38 + i] = e->hs_ms[i];   // the last tw_history_push / _merge (38, 39), _distributions (40), _compare (41, 42)
    return TW_OK;
}

/* Debug aid, not part of the public header: phase timers of -DTW_PROFILE builds (zeros otherwise). */
int tw_debug_profile_hist(tw_engine* e, unsigned long long* out16) {   // item durations of the profiled kernel, by powers of two (TW_ITEM_END)
    if (e == nullptr || out16 == nullptr || e->state < ST_LOADED) return TW_ERR_ARG;
    HIPCHK(hipMemcpyAsync(out16, e->P.prof + 16, sizeof(unsigned long long) * 16, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TW_OK;
}

int tw_debug_profile(tw_engine* e, unsigned long long* out16) {
    if (e == nullptr || out16 == nullptr || e->state < ST_LOADED) return TW_ERR_ARG;
    HIPCHK(hipMemcpyAsync(out16, e->P.prof, sizeof(unsigned long long) * 16, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TW_OK;
}

int tw_find_order(tw_engine* e, int32_t n_units, const int64_t* unit_in_off, const int32_t* unit_E, const int64_t* ep_off,
                  const int64_t* out_start, const int64_t* out_end, const int32_t* true_child, uint8_t* dag_out) {
    if (e == nullptr || n_units <= 0 || !unit_in_off || !unit_E || !ep_off || !out_start || !out_end || !true_child || !dag_out) return TW_ERR_ARG;
    HIPCHK(hipSetDevice(e->device));
    std::vector<int64_t> ep_base((size_t)n_units), ie_off((size_t)n_units);
    int64_t epi = 0, ie = 0, max_n = 0;
    for (int u = 0; u < n_units; u++) {
        if (unit_E[u] < 1 || unit_E[u] > TW_MAX_EP) return fail(e, TW_ERR_UNSUPPORTED, "unit has E outside [1, TW_MAX_EP]");
        const int64_t n = unit_in_off[u + 1] - unit_in_off[u];
        ep_base[(size_t)u] = epi; ie_off[(size_t)u] = ie;
        epi += unit_E[u]; ie += n * unit_E[u];
        max_n = std::max(max_n, n);
    }
    const int64_t n_out = ep_off[epi];
    std::vector<void*> tmp;
    auto up = [&](const void* src, size_t bytes, void** dst) -> hipError_t {
        hipError_t s = hipMalloc(dst, std::max<size_t>(bytes, 8));
        if (s != hipSuccess) return s;
        tmp.push_back(*dst);
        return hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, e->stream);
    };
    OrderDev O{};
    O.n_units = n_units;
    void *d_io, *d_E, *d_eb, *d_eo, *d_ie, *d_os, *d_oe, *d_tr, *d_v;
    hipError_t s = up(unit_in_off, sizeof(int64_t) * (size_t)(n_units + 1), &d_io);
    if (s == hipSuccess) s = up(unit_E, sizeof(int32_t) * (size_t)n_units, &d_E);
    if (s == hipSuccess) s = up(ep_base.data(), sizeof(int64_t) * (size_t)n_units, &d_eb);
    if (s == hipSuccess) s = up(ep_off, sizeof(int64_t) * (size_t)(epi + 1), &d_eo);
    if (s == hipSuccess) s = up(ie_off.data(), sizeof(int64_t) * (size_t)n_units, &d_ie);
    if (s == hipSuccess) s = up(out_start, sizeof(int64_t) * (size_t)n_out, &d_os);
    if (s == hipSuccess) s = up(out_end, sizeof(int64_t) * (size_t)n_out, &d_oe);
    if (s == hipSuccess) s = up(true_child, sizeof(int32_t) * (size_t)ie, &d_tr);
    if (s == hipSuccess) { s = hipMalloc(&d_v, sizeof(unsigned long long) * (size_t)n_units); if (s == hipSuccess) tmp.push_back(d_v); }
    if (s == hipSuccess) s = hipMemsetAsync(d_v, 0, sizeof(unsigned long long) * (size_t)n_units, e->stream);
    std::vector<unsigned long long> viol((size_t)n_units, 0ull);
    if (s == hipSuccess) {
        O.unit_in_off = (const int64_t*)d_io; O.unit_E = (const int32_t*)d_E; O.ep_base = (const int64_t*)d_eb; O.ep_off = (const int64_t*)d_eo;
        O.ie_off = (const int64_t*)d_ie; O.out_start = (const int64_t*)d_os; O.out_end = (const int64_t*)d_oe; O.truth = (const int32_t*)d_tr;
        O.viol = (unsigned long long*)d_v;
        const int threads = (int)flat_threads(e);
        const unsigned bx = (unsigned)std::min<int64_t>((max_n + threads - 1) / threads + 1, 1024);
        for (int u0 = 0; u0 < n_units && s == hipSuccess; u0 += 32768) {  // grid.y is limited to 65535
            OrderDev Q = O;
            Q.unit_in_off += u0; Q.unit_E += u0; Q.ep_base += u0; Q.ie_off += u0; Q.viol += u0;
            hipLaunchKernelGGL(k_find_order, dim3(bx, (unsigned)std::min(n_units - u0, 32768)), dim3((unsigned)threads), 0, e->stream, Q);
            s = hipGetLastError();
        }
        if (s == hipSuccess) s = hipMemcpyAsync(viol.data(), d_v, sizeof(unsigned long long) * (size_t)n_units, hipMemcpyDeviceToHost, e->stream);
        if (s == hipSuccess) s = hipStreamSynchronize(e->stream);
    }
    for (void* q : tmp) (void)hipFree(q);
    if (s != hipSuccess) return fail(e, TW_ERR_DEVICE, std::string("tw_find_order: ") + hipGetErrorString(s));
    int64_t di = 0;
    for (int u = 0; u < n_units; u++) {
        const int E = unit_E[u];
        for (int a = 0; a < E; a++)
            for (int b = 0; b < E; b++) dag_out[di + a * E + b] = (a != b && !((viol[(size_t)u] >> (a * TW_MAX_EP + b)) & 1ull)) ? 1 : 0;
        di += E * E;
    }
    return TW_OK;
}

int tw_order_bound(tw_engine* e, int32_t n_units, const int64_t* unit_in_off, const int32_t* unit_E, const int64_t* ep_off,
                   const int64_t* in_start, const int64_t* in_end, const int64_t* out_start, const int64_t* out_end, int64_t* viol_out) {
    if (e == nullptr || n_units <= 0 || !unit_in_off || !unit_E || !ep_off || !in_start || !in_end || !out_start || !out_end || !viol_out) return TW_ERR_ARG;
    HIPCHK(hipSetDevice(e->device));
    std::vector<int64_t> ep_base((size_t)n_units), viol_off((size_t)n_units);
    int64_t epi = 0, vi = 0, max_n = 0;
    auto sorted = [](const int64_t* s, const int64_t* t, int64_t a, int64_t b) {   // by (start, end)
        for (int64_t i = a + 1; i < b; i++)
            if (s[i - 1] > s[i] || (s[i - 1] == s[i] && t[i - 1] > t[i])) return false;
        return true;
    };
    for (int u = 0; u < n_units; u++) {
        const int E = unit_E[u];
        if (E < 1 || E > TW_MAX_EP) return fail(e, TW_ERR_UNSUPPORTED, "unit has E outside [1, TW_MAX_EP]");
        const int64_t n = unit_in_off[u + 1] - unit_in_off[u];
        if (n < 0) return fail(e, TW_ERR_ARG, "tw_order_bound: unit_in_off is not ascending");
        if (!sorted(in_start, in_end, unit_in_off[u], unit_in_off[u + 1])) return fail(e, TW_ERR_ARG, "tw_order_bound: incoming spans are not sorted by (start, end)");
        for (int k = 0; k < E; k++) {
            if (ep_off[epi + k + 1] < ep_off[epi + k]) return fail(e, TW_ERR_ARG, "tw_order_bound: ep_off is not ascending");
            if (!sorted(out_start, out_end, ep_off[epi + k], ep_off[epi + k + 1])) return fail(e, TW_ERR_ARG, "tw_order_bound: an endpoint's spans are not sorted by (start, end)");
        }
        ep_base[(size_t)u] = epi; viol_off[(size_t)u] = vi;
        epi += E; vi += (int64_t)E * E;
        max_n = std::max(max_n, n);
    }
    if (unit_in_off[0] != 0 || ep_off[0] != 0) return fail(e, TW_ERR_ARG, "tw_order_bound: offsets start at 0");
    const int64_t n_in = unit_in_off[n_units], n_out = ep_off[epi];
    std::vector<void*> tmp;
    auto up = [&](const void* src, size_t bytes, void** dst) -> hipError_t {
        hipError_t s = hipMalloc(dst, std::max<size_t>(bytes, 8));
        if (s != hipSuccess) return s;
        tmp.push_back(*dst);
        return bytes ? hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, e->stream) : hipSuccess;
    };
    void *d_io, *d_E, *d_eb, *d_eo, *d_vo, *d_is, *d_ie, *d_os, *d_oe, *d_v = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipError_t s = up(unit_in_off, sizeof(int64_t) * (size_t)(n_units + 1), &d_io);
    if (s == hipSuccess) s = up(unit_E, sizeof(int32_t) * (size_t)n_units, &d_E);
    if (s == hipSuccess) s = up(ep_base.data(), sizeof(int64_t) * (size_t)n_units, &d_eb);
    if (s == hipSuccess) s = up(ep_off, sizeof(int64_t) * (size_t)(epi + 1), &d_eo);
    if (s == hipSuccess) s = up(viol_off.data(), sizeof(int64_t) * (size_t)n_units, &d_vo);
    if (s == hipSuccess) s = up(in_start, sizeof(int64_t) * (size_t)n_in, &d_is);
    if (s == hipSuccess) s = up(in_end, sizeof(int64_t) * (size_t)n_in, &d_ie);
    if (s == hipSuccess) s = up(out_start, sizeof(int64_t) * (size_t)n_out, &d_os);
    if (s == hipSuccess) s = up(out_end, sizeof(int64_t) * (size_t)n_out, &d_oe);
    if (s == hipSuccess) { s = hipMalloc(&d_v, sizeof(unsigned long long) * (size_t)vi); if (s == hipSuccess) tmp.push_back(d_v); }
    if (s == hipSuccess) s = hipMemsetAsync(d_v, 0, sizeof(unsigned long long) * (size_t)vi, e->stream);
    if (s == hipSuccess) s = hipEventCreate(&ev0);
    if (s == hipSuccess) s = hipEventCreate(&ev1);
    if (s == hipSuccess) {
        OrderBoundDev O{};
        O.unit_in_off = (const int64_t*)d_io; O.unit_E = (const int32_t*)d_E; O.ep_base = (const int64_t*)d_eb; O.ep_off = (const int64_t*)d_eo;
        O.viol_off = (const int64_t*)d_vo; O.in_start = (const int64_t*)d_is; O.in_end = (const int64_t*)d_ie;
        O.out_start = (const int64_t*)d_os; O.out_end = (const int64_t*)d_oe; O.viol = (unsigned long long*)d_v;
        const int threads = (int)flat_threads(e);
        const unsigned bx = (unsigned)std::max<int64_t>((max_n + threads - 1) / threads, 1);   // a lane per request
        s = hipEventRecord(ev0, e->stream);
        for (int u0 = 0; u0 < n_units && s == hipSuccess; u0 += 32768) {  // grid.y is limited to 65535
            OrderBoundDev Q = O;
            Q.unit_in_off += u0; Q.unit_E += u0; Q.ep_base += u0; Q.viol_off += u0;
            hipLaunchKernelGGL(k_order_bound, dim3(bx, (unsigned)std::min(n_units - u0, 32768)), dim3((unsigned)threads), 0, e->stream, Q);
            s = hipGetLastError();
        }
        if (s == hipSuccess) s = hipEventRecord(ev1, e->stream);
        static_assert(sizeof(unsigned long long) == sizeof(int64_t), "viol table");
        if (s == hipSuccess) s = hipMemcpyAsync(viol_out, d_v, sizeof(int64_t) * (size_t)vi, hipMemcpyDeviceToHost, e->stream);
        if (s == hipSuccess) s = hipStreamSynchronize(e->stream);
        float ms = 0.f;
        if (s == hipSuccess && hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) e->ob_ms = (double)ms;
    }
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    for (void* q : tmp) (void)hipFree(q);
    if (s != hipSuccess) return fail(e, TW_ERR_DEVICE, std::string("tw_order_bound: ") + hipGetErrorString(s));
    return TW_OK;
}

int tw_order_stage(tw_engine* e, const tw_batch* b) {
    if (e == nullptr || b == nullptr) return TW_ERR_ARG;
    HIPCHK(hipSetDevice(e->device));
    if (b->n_units <= 0 || !b->unit_in_off || !b->unit_E || !b->ep_off || !b->in_start || !b->in_end || !b->out_start || !b->out_end)
        return fail(e, TW_ERR_ARG, "tw_order_stage: incomplete batch");
    if (b->skip != nullptr) return fail(e, TW_ERR_UNSUPPORTED, "tw_order_stage: skip-mode batches are not searched (one pass, no cnt_unassigned test of a candidate)");
    if (b->unit_time_scale != nullptr) return fail(e, TW_ERR_UNSUPPORTED, "tw_order_stage: load-scaled units (unit_time_scale) are not supported");
    if (b->unit_part != nullptr) return fail(e, TW_ERR_UNSUPPORTED, "tw_order_stage: split services (unit_part) are not supported");
    if (b->topk != TW_TOPK) return fail(e, TW_ERR_UNSUPPORTED, "topk must be 5 (traceweaver_v3.py:1109)");
    if (b->batch_size <= 0 || b->batch_size_mis <= 0) return fail(e, TW_ERR_ARG, "batch sizes must be positive");
    if (b->unit_in_off[0] != 0 || b->ep_off[0] != 0) return fail(e, TW_ERR_ARG, "tw_order_stage: offsets start at 0");
    int64_t epi = 0;
    std::vector<int64_t> ep_base((size_t)b->n_units);
    for (int u = 0; u < b->n_units; u++) {
        const int E = b->unit_E[u];
        if (E < 1 || E > TW_MAX_EP) return fail(e, TW_ERR_UNSUPPORTED, "unit has E outside [1, TW_MAX_EP]");
        const int64_t n = b->unit_in_off[u + 1] - b->unit_in_off[u];
        if (n < 2) return fail(e, TW_ERR_ARG, "a unit needs at least 2 incoming spans");
        for (int k = 0; k < E; k++)
            if (b->ep_off[epi + k + 1] - b->ep_off[epi + k] != n)
                return fail(e, TW_ERR_UNSUPPORTED, "tw_order_stage: an endpoint's span count differs from the number of incoming spans (a skip-mode unit)");
        ep_base[(size_t)u] = epi;
        epi += E;
    }
    const int64_t n_in = b->unit_in_off[b->n_units], n_out = b->ep_off[epi];
    if (n_in >= (1ll << 31) || n_out >= (1ll << 31)) return fail(e, TW_ERR_ARG, "batch exceeds 2^31 spans");
    order_unstage(e);
    const int64_t counts[4] = {n_in, n_in, n_out, n_out};
    const int64_t* src[4] = {b->in_start, b->in_end, b->out_start, b->out_end};
    for (int k = 0; k < 4; k++) {
        HIPCHK(hipMalloc((void**)&e->ord_stage[k], sizeof(int64_t) * (size_t)std::max<int64_t>(counts[k], 1)));
        HIPCHK(hipMalloc((void**)&e->ord_gather[k], sizeof(int64_t) * (size_t)std::max<int64_t>(counts[k], 1)));
        HIPCHK(hipMemcpyAsync(e->ord_stage[k], src[k], sizeof(int64_t) * (size_t)counts[k], hipMemcpyHostToDevice, e->stream));
    }
    e->ord_seg_cap = std::max<int64_t>(epi, b->n_units);
    HIPCHK(hipMalloc((void**)&e->ord_seg, sizeof(int64_t) * 3 * (size_t)e->ord_seg_cap));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->ord_in_off.assign(b->unit_in_off, b->unit_in_off + b->n_units + 1);
    e->ord_ep_off.assign(b->ep_off, b->ep_off + epi + 1);
    e->ord_E.assign(b->unit_E, b->unit_E + b->n_units);
    e->ord_ep_base = ep_base;
    e->ord_batch_size = b->batch_size; e->ord_batch_mis = b->batch_size_mis;
    e->ord_staged = true;
    return TW_OK;
}

int tw_order_load(tw_engine* e, int32_t n_active, const int32_t* active_units, const uint8_t* dag_key) {
    if (e == nullptr || n_active <= 0 || active_units == nullptr || dag_key == nullptr) return TW_ERR_ARG;
    if (!e->ord_staged) return fail(e, TW_ERR_STATE, "tw_order_load before tw_order_stage");
    HIPCHK(hipSetDevice(e->device));
    const int32_t n_staged = (int32_t)e->ord_E.size();
    std::vector<int64_t> in_off{0}, ep_off{0}, seg_in_src, seg_in_dst, seg_in_len, seg_out_src, seg_out_dst, seg_out_len;
    std::vector<int32_t> unit_E, key_rank;
    std::vector<uint8_t> dag;
    int64_t di = 0, max_len = 0;
    for (int k = 0; k < n_active; k++) {
        const int32_t u = active_units[k];
        if (u < 0 || u >= n_staged || (k > 0 && u <= active_units[k - 1])) return fail(e, TW_ERR_ARG, "tw_order_load: active_units must be ascending indices of staged units");
        const int E = e->ord_E[(size_t)u];
        const uint8_t* dk = dag_key + di;
        // nx.topological_sort (traceweaver_v1.py:37-39) on arrays: generation after generation, a generation in the order in which
        // its nodes lost their last predecessor -- the nodes in insertion (key) order, a node's successors in the order its edges
        // were added, which is ascending key order for the search (it walks the pairs (a, b) in key order)
        int indeg[TW_MAX_EP] = {}, order[TW_MAX_EP], n_ord = 0;
        for (int a = 0; a < E; a++)
            for (int c = 0; c < E; c++)
                if (dk[a * E + c]) {
                    if (a == c) return fail(e, TW_ERR_ARG, "tw_order_load: the candidate graph has a self loop");
                    indeg[c]++;
                }
        for (int a = 0; a < E; a++) if (indeg[a] == 0) order[n_ord++] = a;
        for (int h = 0; h < n_ord; h++)
            for (int c = 0; c < E; c++)
                if (dk[order[h] * E + c] && --indeg[c] == 0) order[n_ord++] = c;
        if (n_ord != E) return fail(e, TW_ERR_ARG, "tw_order_load: the candidate graph has a cycle");
        const int64_t n = e->ord_in_off[(size_t)u + 1] - e->ord_in_off[(size_t)u];
        seg_in_src.push_back(e->ord_in_off[(size_t)u]); seg_in_dst.push_back(in_off.back()); seg_in_len.push_back(n);
        in_off.push_back(in_off.back() + n);
        max_len = std::max(max_len, n);
        const int64_t eb = e->ord_ep_base[(size_t)u];
        for (int p = 0; p < E; p++) {
            const int64_t a = e->ord_ep_off[(size_t)(eb + order[p])], len = e->ord_ep_off[(size_t)(eb + order[p] + 1)] - a;
            seg_out_src.push_back(a); seg_out_dst.push_back(ep_off.back()); seg_out_len.push_back(len);
            ep_off.push_back(ep_off.back() + len);
            key_rank.push_back(order[p]);
            for (int q = 0; q < E; q++) dag.push_back(dk[order[p] * E + order[q]]);
        }
        unit_E.push_back(E);
        di += (int64_t)E * E;
    }
    const unsigned threads = flat_threads(e);
    const unsigned bx = (unsigned)std::min<int64_t>(std::max<int64_t>((max_len + threads - 1) / threads, 1), 1024);
    auto gather = [&](const std::vector<int64_t>& src, const std::vector<int64_t>& dst, const std::vector<int64_t>& len, int first) -> int {
        const int64_t n_seg = (int64_t)src.size();   // (<= ord_seg_cap: the listed units are distinct staged units)
        HIPCHK(hipMemcpyAsync(e->ord_seg, src.data(), sizeof(int64_t) * (size_t)n_seg, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->ord_seg + e->ord_seg_cap, dst.data(), sizeof(int64_t) * (size_t)n_seg, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->ord_seg + 2 * e->ord_seg_cap, len.data(), sizeof(int64_t) * (size_t)n_seg, hipMemcpyHostToDevice, e->stream));
        for (int64_t g0 = 0; g0 < n_seg; g0 += 32768) {  // grid.y is limited to 65535
            OrderGatherDev G{e->ord_seg + g0, e->ord_seg + e->ord_seg_cap + g0, e->ord_seg + 2 * e->ord_seg_cap + g0,
                             e->ord_stage[first], e->ord_stage[first + 1], e->ord_gather[first], e->ord_gather[first + 1]};
            hipLaunchKernelGGL(k_order_gather, dim3(bx, (unsigned)std::min<int64_t>(n_seg - g0, 32768)), dim3(threads), 0, e->stream, G);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamSynchronize(e->stream));   // (the descriptor block is written again by the next call)
        return TW_OK;
    };
    TWCHK(gather(seg_in_src, seg_in_dst, seg_in_len, 0));
    TWCHK(gather(seg_out_src, seg_out_dst, seg_out_len, 2));
    tw_batch b{};
    b.n_units = n_active;
    b.unit_in_off = in_off.data(); b.unit_E = unit_E.data(); b.ep_off = ep_off.data(); b.dag = dag.data(); b.key_rank = key_rank.data();
    b.in_start = e->ord_gather[0]; b.in_end = e->ord_gather[1]; b.out_start = e->ord_gather[2]; b.out_end = e->ord_gather[3];
    b.batch_size = e->ord_batch_size; b.batch_size_mis = e->ord_batch_mis; b.topk = TW_TOPK;
    return tw_load_batch(e, &b, 1);
}

int tw_set_truth(tw_engine* e, const int32_t* true_child, const int32_t* in_trace, int64_t n_traces) {
    if (e == nullptr || true_child == nullptr) return TW_ERR_ARG;
    if (e->state < ST_LOADED) return fail(e, TW_ERR_STATE, "tw_set_truth before tw_load_batch");
    if (in_trace != nullptr && n_traces <= 0) return fail(e, TW_ERR_ARG, "in_trace given without n_traces");
    HIPCHK(hipSetDevice(e->device));
    // k_evaluate indexes trace_bad[] with in_trace and compares parents with true_child: both are checked here, once,
    // on the host (an out-of-range trace number would be an out-of-bounds store on the device)
    for (const UnitDev& U : e->units) {
        const int32_t* t = true_child + U.ie_off;
        for (int64_t k = 0; k < (int64_t)U.E * U.n_in; k++)
            if (t[k] < (e->skip_mode ? -2 : -1) || t[k] >= U.n_in) return fail(e, TW_ERR_ARG, "tw_set_truth: true_child outside [-1, n_in) (-2 = skipped, skip-mode batches only)");
    }
    if (in_trace != nullptr)
        for (int64_t k = 0; k < e->P.n_in_total; k++)
            if (in_trace[k] < -1 || in_trace[k] >= n_traces) return fail(e, TW_ERR_ARG, "tw_set_truth: in_trace outside [-1, n_traces)");
    int rc;
    if (e->truth == nullptr) {
        rc = dev_alloc(e, &e->truth, e->n_ie); if (rc != TW_OK) return rc;
        rc = dev_alloc(e, &e->eval_counts, (int64_t)e->P.n_units * 4 + 2); if (rc != TW_OK) return rc;
    }
    HIPCHK(hipMemcpyAsync(e->truth, true_child, sizeof(int32_t) * e->n_ie, hipMemcpyHostToDevice, e->stream));
    e->n_traces = 0;
    if (in_trace != nullptr) {  // (buffers are freed with the batch)
        if (e->in_trace == nullptr) { rc = dev_alloc(e, &e->in_trace, e->P.n_in_total); if (rc != TW_OK) return rc; }
        if (e->trace_bad == nullptr || n_traces > e->trace_cap) {
            rc = dev_alloc(e, &e->trace_bad, 2 * n_traces); if (rc != TW_OK) return rc;
            e->trace_cap = n_traces;
        }
        HIPCHK(hipMemcpyAsync(e->in_trace, in_trace, sizeof(int32_t) * e->P.n_in_total, hipMemcpyHostToDevice, e->stream));
        e->n_traces = n_traces;
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return TW_OK;
}

int tw_evaluate(tw_engine* e, int64_t* per_unit, uint8_t* trace_flags, int64_t* e2e) {
    if (e == nullptr || per_unit == nullptr) return TW_ERR_ARG;
    if (e->state != ST_PASS1 && e->state != ST_MIX && e->state != ST_PASS2) return fail(e, TW_ERR_STATE, "tw_evaluate needs the results of a pass");
    if (e->truth == nullptr) return fail(e, TW_ERR_STATE, "tw_evaluate before tw_set_truth");
    if ((trace_flags != nullptr || e2e != nullptr) && e->n_traces == 0) return fail(e, TW_ERR_STATE, "per-trace accuracy needs in_trace (tw_set_truth)");
    HIPCHK(hipSetDevice(e->device));
    const Dev& P = e->P;
    const int64_t nc = (int64_t)P.n_units * 4 + 2;
    HIPCHK(hipMemsetAsync(e->eval_counts, 0, sizeof(unsigned long long) * nc, e->stream));
    if (e->n_traces > 0) HIPCHK(hipMemsetAsync(e->trace_bad, 0, (size_t)(2 * e->n_traces), e->stream));
    hipLaunchKernelGGL(k_evaluate, dim3(P.n_tiles), dim3(e->K.tile), 0, e->stream, P, (const int32_t*)e->truth,
                       (const int32_t*)(e->n_traces > 0 ? e->in_trace : nullptr), e->eval_counts, e->trace_bad,
                       e->n_traces > 0 ? e->trace_bad + e->n_traces : nullptr);
    if (e->n_traces > 0 && e2e != nullptr)
        hipLaunchKernelGGL(k_count_flags, dim3((unsigned)std::min<int64_t>(e->n_traces / 1024 + 1, 1024)), dim3(flat_threads(e)), 0, e->stream,
                           (const uint8_t*)e->trace_bad, (const uint8_t*)(e->trace_bad + e->n_traces), e->n_traces, e->eval_counts + (nc - 2));
    HIPCHK(hipGetLastError());
    std::vector<unsigned long long> h((size_t)nc);
    HIPCHK(hipMemcpyAsync(h.data(), e->eval_counts, sizeof(unsigned long long) * nc, hipMemcpyDeviceToHost, e->stream));
    if (trace_flags != nullptr) HIPCHK(hipMemcpyAsync(trace_flags, e->trace_bad, (size_t)(2 * e->n_traces), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int u = 0; u < P.n_units; u++) {
        const int64_t n = e->units[(size_t)u].n_in;
        per_unit[u * 4 + 0] = n;
        per_unit[u * 4 + 1] = n - (int64_t)h[(size_t)u * 4 + 1];
        per_unit[u * 4 + 2] = n - (int64_t)h[(size_t)u * 4 + 2];
        per_unit[u * 4 + 3] = (int64_t)h[(size_t)u * 4 + 3];
    }
    if (e2e != nullptr) { e2e[0] = (int64_t)h[(size_t)nc - 2]; e2e[1] = (int64_t)h[(size_t)nc - 1]; }
    return TW_OK;
}

/* ---- from parent arrays to traces (tw_stitch.h) ------------------------------------------------------------------- */
int tw_set_span_rows(tw_engine* e, int64_t n_rows, const int32_t* in_row, const int32_t* out_row, const int32_t* row_link,
                     const uint8_t* row_kind, const int64_t* row_start, const int64_t* row_end) {
    if (e == nullptr || !in_row || !out_row || !row_link || !row_kind || !row_start || !row_end) return TW_ERR_ARG;
    if (e->state < ST_LOADED) return fail(e, TW_ERR_STATE, "tw_set_span_rows before tw_load_batch");
    if (n_rows < 1 || n_rows > 0x7ffffff0ll) return fail(e, TW_ERR_ARG, "tw_set_span_rows: n_rows outside [1, 2^31 - 16]");
    HIPCHK(hipSetDevice(e->device));
    const Dev& P = e->P;
    // the kernels index the row arrays with these values: range, kind and uniqueness are checked here, once, on the host
    for (int64_t r = 0; r < n_rows; r++) {
        if (row_kind[r] > 2) return fail(e, TW_ERR_ARG, "tw_set_span_rows: row_kind outside {0 absent, 1 server, 2 client}");
        const int32_t l = row_link[r];
        if (l < -2 || l >= n_rows || l == r) return fail(e, TW_ERR_ARG, "tw_set_span_rows: row_link outside [-2, n_rows) or a row linked to itself");
        if (row_kind[r] == 1 && l >= 0 && row_kind[l] != 2)
            return fail(e, TW_ERR_ARG, "tw_set_span_rows: a server row's link must name a client row (the caller's side of the same RPC)");
    }
    std::vector<uint8_t> seen((size_t)n_rows, 0);
    for (int64_t k = 0; k < P.n_in_total + P.n_out_total; k++) {
        const bool in = k < P.n_in_total;
        const int32_t r = in ? in_row[k] : out_row[k - P.n_in_total];
        if (r < 0 || r >= n_rows || row_kind[r] != (in ? 1 : 2) || seen[(size_t)r])
            return fail(e, TW_ERR_ARG, in ? "tw_set_span_rows: in_row must name distinct server rows of the table" : "tw_set_span_rows: out_row must name distinct client rows of the table");
        seen[(size_t)r] = 1;
    }
    drop_rows(e);   // (the groups, the cohort labels and the reference set name rows of the old maps)
    StitchDev& S = e->S;
    if (S.link == nullptr || n_rows > e->rows_cap) {   // (freed with the batch)
        int32_t *in_d, *out_d, *link_d; uint8_t* kind_d; int64_t *start_d, *end_d;
        DEV_ALLOC(in_d, P.n_in_total); DEV_ALLOC(out_d, P.n_out_total); DEV_ALLOC(link_d, n_rows); DEV_ALLOC(kind_d, n_rows); DEV_ALLOC(start_d, n_rows); DEV_ALLOC(end_d, n_rows);
        S.in_row = in_d; S.out_row = out_d; S.row_link = link_d; S.row_kind = kind_d; S.row_start = start_d; S.row_end = end_d;
        DEV_ALLOC(S.link, n_rows); DEV_ALLOC(S.state_a, n_rows); DEV_ALLOC(S.state_b, n_rows);
        DEV_ALLOC(S.root, n_rows); DEV_ALLOC(S.depth, n_rows); DEV_ALLOC(S.true_root, n_rows); DEV_ALLOC(S.una, n_rows); DEV_ALLOC(S.bad, n_rows);
        DEV_ALLOC(S.cursor, n_rows); DEV_ALLOC(S.chunk_sum, n_rows / kStitchScanItems + 2);
        DEV_ALLOC(S.rows_tmp, n_rows); DEV_ALLOC(S.tree_rows, n_rows); DEV_ALLOC(S.tree_root, n_rows);
        DEV_ALLOC(S.tree_off, n_rows + 1); DEV_ALLOC(S.tree_latency, n_rows); DEV_ALLOC(S.tree_flags, n_rows);
        DEV_ALLOC(S.totals, 4); DEV_ALLOC(S.changed, kStitchMaxRounds); DEV_ALLOC(S.err, 1);
        e->rows_cap = n_rows;
    }
    S.n_rows = n_rows;
    HIPCHK(hipMemcpyAsync(const_cast<int32_t*>(S.in_row), in_row, sizeof(int32_t) * (size_t)P.n_in_total, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(const_cast<int32_t*>(S.out_row), out_row, sizeof(int32_t) * (size_t)P.n_out_total, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(const_cast<int32_t*>(S.row_link), row_link, sizeof(int32_t) * (size_t)n_rows, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(const_cast<uint8_t*>(S.row_kind), row_kind, (size_t)n_rows, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(const_cast<int64_t*>(S.row_start), row_start, sizeof(int64_t) * (size_t)n_rows, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(const_cast<int64_t*>(S.row_end), row_end, sizeof(int64_t) * (size_t)n_rows, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->rows_set = true;
    return TW_OK;
}

int tw_set_parents(tw_engine* e, const int32_t* parent) {
    if (e == nullptr || parent == nullptr) return TW_ERR_ARG;
    if (e->state < ST_LOADED) return fail(e, TW_ERR_STATE, "tw_set_parents before tw_load_batch");
    HIPCHK(hipSetDevice(e->device));
    // k_stitch_links indexes out_row with these values and relies on a call being given to one request at most
    std::vector<uint8_t> taken;
    for (const UnitDev& U : e->units)
        for (int ep = 0; ep < U.E; ep++) {
            const int64_t len = U.ep_off[ep + 1] - U.ep_off[ep];
            taken.assign((size_t)len, 0);
            const int32_t* p = parent + U.ie_off + (int64_t)ep * U.n_in;
            for (int64_t i = 0; i < U.n_in; i++) {
                if (p[i] < -2 || p[i] >= len) return fail(e, TW_ERR_ARG, "tw_set_parents: parent outside [-2, spans of the endpoint)");
                if (p[i] >= 0 && taken[(size_t)p[i]]++) return fail(e, TW_ERR_ARG, "tw_set_parents: a call is given to two requests");
            }
        }
    if (e->given_parent == nullptr) DEV_ALLOC(e->given_parent, e->n_ie);
    HIPCHK(hipMemcpyAsync(e->given_parent, parent, sizeof(int32_t) * (size_t)e->n_ie, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->parents_given = true;
    return TW_OK;
}

namespace {

// link table of `src` (parent arrays of a pass, or the true ones) -> root of every row in root_out (and its depth); `final`: the
// forest that is grouped afterwards (rows per root are counted, trees compared with true_root if given).  *rounds = jump rounds run.
int stitch_forest(tw_engine* e, const int32_t* src, int32_t* root_out, int32_t* depth_out, bool final, const int32_t* true_root, int* rounds) {
    const Dev& P = e->P;
    const StitchDev& S = e->S;
    const unsigned threads = flat_threads(e);
    const dim3 rows(flat_grid(S.n_rows, threads)), tb(threads);
    HIPCHK(hipMemsetAsync(S.changed, 0, sizeof(int32_t) * kStitchMaxRounds, e->stream));
    hipLaunchKernelGGL(k_stitch_init, rows, tb, 0, e->stream, S);
    int max_e = 1;
    for (const UnitDev& U : e->units) max_e = std::max(max_e, (int)U.E);
    hipLaunchKernelGGL(k_stitch_links, dim3((unsigned)P.n_tiles, (unsigned)max_e), dim3((unsigned)e->K.tile), 0, e->stream, P, S, src);
    HIPCHK(hipGetLastError());
    if (final) HIPCHK(hipEventRecord(e->stage_ev[SE_STITCH + 1], e->stream));
    unsigned long long *a = S.state_a, *b = S.state_b;
    int round = 0;
    for (;; round++) {
        if (round == kStitchMaxRounds)
            return fail(e, TW_ERR_ARG, "tw_stitch_traces: the links do not settle in 32 doubling rounds: row_link holds a cycle");
        hipLaunchKernelGGL(k_stitch_jump, rows, tb, 0, e->stream, S, (const unsigned long long*)a, b, round == 0 ? 1 : 0, round);
        HIPCHK(hipGetLastError());
        int32_t moved = 0;   // one word per round: the loop ends at the first quiet one
        HIPCHK(hipMemcpyAsync(&moved, S.changed + round, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        std::swap(a, b);
        if (!moved) break;
    }
    *rounds = round + 1;
    if (final) HIPCHK(hipEventRecord(e->stage_ev[SE_STITCH + 2], e->stream));
    hipLaunchKernelGGL(k_stitch_count, rows, tb, 0, e->stream, S, (const unsigned long long*)a, root_out, depth_out, final ? 1 : 0, true_root);
    HIPCHK(hipGetLastError());
    return TW_OK;
}

}  // namespace

int tw_stitch_traces(tw_engine* e, int pass, int use_truth, const tw_stitched* out, int64_t* n_trees, int64_t* counts4) {
    if (e == nullptr || out == nullptr || n_trees == nullptr) return TW_ERR_ARG;
    if (!e->rows_set)
        return fail(e, TW_ERR_STATE, "tw_stitch_traces before tw_set_span_rows (tw_load_batch and tw_scale_load drop the row maps)");
    if (use_truth) {
        if (e->truth == nullptr) return fail(e, TW_ERR_STATE, "tw_stitch_traces(use_truth) before tw_set_truth");
    } else {
        if (!(pass == 0 && e->parents_given) && !pass_resident(e, pass)) return fail(e, TW_ERR_STATE, "tw_stitch_traces: the results of that pass are not resident (pass 0: tw_set_parents first)");
    }
    HIPCHK(hipSetDevice(e->device));
    drop_forest(e);
    const StitchDev& S = e->S;
    const bool has_truth = e->truth != nullptr;
    const unsigned threads = flat_threads(e);
    const dim3 rows(flat_grid(S.n_rows, threads)), tb(threads);
    HIPCHK(hipMemsetAsync(S.totals, 0, sizeof(unsigned long long) * 4, e->stream));
    HIPCHK(hipMemsetAsync(S.err, 0, sizeof(int32_t), e->stream));
    HIPCHK(hipEventRecord(e->stage_ev[SE_STITCH], e->stream));
    int rounds = 0;
    if (has_truth && !use_truth) {   // the true forest first: what bit 2 of the flags compares with
        TWCHK(stitch_forest(e, e->truth, S.true_root, nullptr, false, nullptr, &rounds));
        HIPCHK(hipEventRecord(e->stage_ev[SE_STITCH], e->stream));   // (timed: the stitch of the assignment alone)
    }
    TWCHK(stitch_forest(e, use_truth ? e->truth : (pass == 0 ? e->given_parent : e->P.parent), S.root, S.depth, true, (has_truth && !use_truth) ? S.true_root : nullptr, &rounds));
    const int64_t n_chunks = (S.n_rows + (int64_t)threads * kStitchScanItems - 1) / ((int64_t)threads * kStitchScanItems);
    hipLaunchKernelGGL(k_stitch_scan_sums, dim3((unsigned)n_chunks), tb, 0, e->stream, S);
    hipLaunchKernelGGL(k_stitch_scan_chunks, dim3(1), tb, 0, e->stream, S, n_chunks);
    hipLaunchKernelGGL(k_stitch_scan_write, dim3((unsigned)n_chunks), tb, 0, e->stream, S);
    hipLaunchKernelGGL(k_stitch_scatter, rows, tb, 0, e->stream, S);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->stage_ev[SE_STITCH + 3], e->stream));
    const WaveShape group = wave_shape(e, S.n_rows, kStitchTrees, kStitchWaves);   // (the trees are not counted yet: as if every row were one)
    hipLaunchKernelGGL(k_stitch_group, group.grid, group.block, 0, e->stream, S, has_truth ? 1 : 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->stage_ev[SE_STITCH + 4], e->stream));
    unsigned long long totals[4] = {0, 0, 0, 0};
    int32_t err = 0;
    HIPCHK(hipMemcpyAsync(totals, S.totals, sizeof(totals), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(&err, S.err, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (err != 0) return fail(e, TW_ERR_ARG, "tw_stitch_traces: the links hold a cycle (a row is its own ancestor): malformed row_link / row maps");
    TWCHK(stage_elapsed(e, SE_STITCH, 0, 4, &e->st_ms[0]));
    for (int i = 1; i <= 4; i++) TWCHK(stage_elapsed(e, SE_STITCH, i - 1, i, &e->st_ms[i]));
    e->st_ms[5] = (double)rounds;
    const int64_t nt = (int64_t)(totals[0] >> 32);
    *n_trees = nt;
    if (counts4 != nullptr) {
        counts4[0] = (int64_t)totals[1]; counts4[1] = nt - (int64_t)totals[1]; counts4[2] = (int64_t)totals[2];
        counts4[3] = has_truth ? (int64_t)totals[3] : -1;
    }
    TWCHK(copy_out(e, out->root, S.root, S.n_rows));
    TWCHK(copy_out(e, out->depth, S.depth, S.n_rows));
    TWCHK(copy_out(e, out->tree_off, S.tree_off, nt + 1));
    TWCHK(copy_out(e, out->tree_rows, S.tree_rows, S.n_rows));
    TWCHK(copy_out(e, out->tree_root, S.tree_root, nt));
    TWCHK(copy_out(e, out->tree_latency, S.tree_latency, nt));
    TWCHK(copy_out(e, out->tree_flags, S.tree_flags, nt));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->stitched = true; e->st_trees = nt;
    e->stitched_pass = use_truth ? -1 : pass; e->stitched_truth = has_truth;
    return TW_OK;
}

/* ---- latency attribution on the stitched forest (tw_attr.h) ------------------------------------------------------- */
int tw_set_row_groups(tw_engine* e, int32_t n_groups, const int32_t* row_group) {
    if (e == nullptr || row_group == nullptr) return TW_ERR_ARG;
    if (!e->rows_set) return fail(e, TW_ERR_STATE, "tw_set_row_groups before tw_set_span_rows (tw_load_batch and tw_scale_load drop the row maps)");
    if (n_groups < 1) return fail(e, TW_ERR_ARG, "tw_set_row_groups: n_groups must be positive");
    const int64_t n_rows = e->S.n_rows;
    for (int64_t r = 0; r < n_rows; r++)   // k_attr_reduce indexes the totals with these values
        if (row_group[r] < -1 || row_group[r] >= n_groups) return fail(e, TW_ERR_ARG, "tw_set_row_groups: row_group outside [-1, n_groups)");
    HIPCHK(hipSetDevice(e->device));
    drop_groups(e);   // (the per-row flags of the last attribution name the old groups, and so do the signatures, the reference set's among them)
    AttrDev& A = e->A;
    if (A.self_time == nullptr || n_rows > e->attr_rows_cap) {   // (freed with the batch)
        int32_t* group_d;
        DEV_ALLOC(group_d, n_rows); A.row_group = group_d;
        DEV_ALLOC(A.self_time, n_rows); DEV_ALLOC(A.path_time, n_rows); DEV_ALLOC(A.row_tree, n_rows); DEV_ALLOC(A.row_flag, n_rows);
        DEV_ALLOC(A.tree_top, n_rows); DEV_ALLOC(A.tree_path_rows, n_rows); DEV_ALLOC(A.tree_sel, n_rows);
        DEV_ALLOC(A.key_a, n_rows); DEV_ALLOC(A.key_b, n_rows); DEV_ALLOC(A.val_a, n_rows); DEV_ALLOC(A.val_b, n_rows);
        DEV_ALLOC(A.counters, 4); DEV_ALLOC(A.err, 1);
        e->attr_rows_cap = n_rows;
    }
    if (A.totals == nullptr || n_groups > e->groups_cap) {
        DEV_ALLOC(A.totals, (int64_t)kAttrCols * n_groups);
        e->groups_cap = n_groups;
    }
    A.n_groups = n_groups;
    HIPCHK(hipMemcpyAsync(const_cast<int32_t*>(A.row_group), row_group, sizeof(int32_t) * (size_t)n_rows, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->groups_set = true;
    return TW_OK;
}

namespace {

// The trees in order of (latency, tree), the eligible ones first, into V.val_b with their keys in V.key_b: the selection of the
// attribution, which the extraction reads too (on sort buffers of its own: it needs no row groups).  Counts into V.counters[0 .. 2).
int trees_by_latency(tw_engine* e, const AttrDev& V, const AttrQueryDev& Q, int64_t nt) {
    const unsigned threads = flat_threads(e);
    hipLaunchKernelGGL(k_attr_flags, dim3(flat_grid(nt, threads)), dim3(threads), 0, e->stream, e->S, V, Q, nt);
    HIPCHK(hipGetLastError());
    return rocprim_call(e, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_pairs(tmp, bytes, V.key_a, V.key_b, V.val_a, V.val_b, (size_t)nt, 0u, 64u, e->stream); });
}

}  // namespace

int tw_attribute_traces(tw_engine* e, const tw_attr_query* q, const tw_attribution* out, int64_t* summary) {
    if (e == nullptr || q == nullptr) return TW_ERR_ARG;
    TWCHK(need_forest(e, "tw_attribute_traces"));
    if (!e->groups_set) return fail(e, TW_ERR_STATE, "tw_attribute_traces before tw_set_row_groups (dropped with the row maps)");
    if (!(q->percentile >= 0.0 && q->percentile < 1.0)) return fail(e, TW_ERR_ARG, "tw_attribute_traces: percentile outside [0, 1)");
    if (q->start_min > q->start_max) return fail(e, TW_ERR_ARG, "tw_attribute_traces: start_min > start_max");
    HIPCHK(hipSetDevice(e->device));
    drop_attribution(e);
    const StitchDev& S = e->S;
    AttrDev& A = e->A;
    const int64_t nt = e->st_trees, G = A.n_groups;
    const unsigned threads = flat_threads(e);
    const dim3 tb(threads), trees(flat_grid(nt, threads)), rows(flat_grid(S.n_rows, threads));
    AttrQueryDev Q{q->start_min, q->start_max, 0, q->need_flags, q->skip_flags};
    // selection: eligible trees in order of (latency, tree), those of rank >= k inside the start window
    HIPCHK(hipMemsetAsync(A.counters, 0, sizeof(unsigned long long) * 4, e->stream));
    HIPCHK(hipMemsetAsync(A.err, 0, sizeof(int32_t), e->stream));
    HIPCHK(hipMemsetAsync(A.totals, 0, sizeof(unsigned long long) * (size_t)(kAttrCols * G), e->stream));
    HIPCHK(hipEventRecord(e->stage_ev[SE_ATTR + 0], e->stream));
    TWCHK(trees_by_latency(e, A, Q, nt));
    unsigned long long counters[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(counters, A.counters, sizeof(counters), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int64_t n_eligible = (int64_t)counters[0], big_rows = (int64_t)counters[1];
    Q.k = (int64_t)(q->percentile * (double)n_eligible);   // int(0.95 * len(...)) of the reference, in binary64
    hipLaunchKernelGGL(k_attr_mark, trees, tb, 0, e->stream, S, A, Q, nt, n_eligible);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->stage_ev[SE_ATTR + 1], e->stream));
    if (big_rows > A.big_cap) {   // tables of the trees that outgrow a wavefront's LDS (freed with the batch)
        DEV_ALLOC(A.g_s, big_rows); DEV_ALLOC(A.g_e, big_rows); DEV_ALLOC(A.g_s2, big_rows); DEV_ALLOC(A.g_e2, big_rows); DEV_ALLOC(A.g_row, big_rows);
        DEV_ALLOC(A.g_par, big_rows); DEV_ALLOC(A.g_rank, big_rows); DEV_ALLOC(A.g_row2, big_rows); DEV_ALLOC(A.g_par2, big_rows);
        A.big_cap = big_rows;
    }
    const WaveShape per_tree = wave_shape(e, nt, kAttrTrees, kAttrWaves);
    hipLaunchKernelGGL(k_attr_tree, per_tree.grid, per_tree.block, 0, e->stream, S, A, nt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->stage_ev[SE_ATTR + 2], e->stream));
    hipLaunchKernelGGL(k_attr_reduce, rows, tb, 0, e->stream, S, A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->stage_ev[SE_ATTR + 3], e->stream));
    std::vector<unsigned long long> totals((size_t)(kAttrCols * G));
    unsigned long long key_k = 1ull << 63;
    int32_t err = 0;
    HIPCHK(hipMemcpyAsync(totals.data(), A.totals, sizeof(unsigned long long) * totals.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(counters, A.counters, sizeof(counters), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(&err, A.err, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (n_eligible > 0) HIPCHK(hipMemcpyAsync(&key_k, A.key_b + Q.k, sizeof(key_k), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (err == TW_ERR_DEVICE) return fail(e, TW_ERR_DEVICE, "tw_attribute_traces: the tables of the large trees are smaller than the trees");
    if (err != 0) return fail(e, TW_ERR_ARG, "tw_attribute_traces: a row is linked to a row outside its tree: not the forest tw_stitch_traces left behind");
    TWCHK(stage_elapsed(e, SE_ATTR, 1, 2, &e->at_ms[0]));
    TWCHK(stage_elapsed(e, SE_ATTR, 0, 1, &e->at_ms[1]));
    TWCHK(stage_elapsed(e, SE_ATTR, 2, 3, &e->at_ms[2]));
    if (summary != nullptr) {
        int64_t culprit = -1;   // the group with the largest path time among those with a row on a selected path; ties: the smallest id
        for (int64_t g = 0; g < G; g++)
            if (totals[(size_t)(G + g)] != 0 && (culprit < 0 || (int64_t)totals[(size_t)g] > (int64_t)totals[(size_t)culprit])) culprit = g;
        summary[0] = n_eligible; summary[1] = (int64_t)counters[2]; summary[2] = Q.k;
        summary[3] = (int64_t)(key_k ^ (1ull << 63)); summary[4] = culprit; summary[5] = nt;
    }
    if (out != nullptr) {
        TWCHK(copy_out(e, out->link, S.link, S.n_rows));
        TWCHK(copy_out(e, out->self_time, A.self_time, S.n_rows));
        TWCHK(copy_out(e, out->path_time, A.path_time, S.n_rows));
        TWCHK(copy_out(e, out->tree_top_group, A.tree_top, nt));
        TWCHK(copy_out(e, out->tree_selected, A.tree_sel, nt));
        TWCHK(copy_out(e, out->tree_path_rows, A.tree_path_rows, nt));
        HIPCHK(hipStreamSynchronize(e->stream));
        int64_t* cols[kAttrCols] = {out->group_path_time, out->group_path_rows, out->group_self_time, out->group_span_time, out->group_span_rows,
                                    out->group_trees, out->group_top_trees};
        for (int c = 0; c < kAttrCols; c++)
            if (cols[c] != nullptr)
                for (int64_t g = 0; g < G; g++) cols[c][g] = (int64_t)totals[(size_t)(c * G + g)];
    }
    e->attr_need = q->need_flags; e->attr_skip = q->skip_flags;
    e->attributed = true;
    return TW_OK;
}

/* ---- which of the reconstructed traces can be trusted (tw_conf.h) -------------------------------------------------- */
namespace {

// rank, list_n and margin of the resident pass into e->C (freed with the batch); the first two events of SE_CONF around the kernel
int conf_decisions(tw_engine* e) {
    const Dev& P = e->P;
    ConfDev& C = e->C;
    if (C.rank == nullptr) {
        int rc;
        if ((rc = dev_alloc(e, &C.rank, P.n_in_total)) != TW_OK || (rc = dev_alloc(e, &C.list_n, P.n_in_total)) != TW_OK ||
            (rc = dev_alloc(e, &C.margin, P.n_in_total)) != TW_OK || (rc = dev_alloc(e, &C.cells, kConfCells)) != TW_OK) {
            C.rank = nullptr;
            return rc;
        }
    }
    HIPCHK(hipEventRecord(e->stage_ev[SE_CONF + 0], e->stream));
    hipLaunchKernelGGL(k_conf_requests, dim3((unsigned)P.n_tiles), dim3((unsigned)e->K.tile), 0, e->stream, P, C);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->stage_ev[SE_CONF + 1], e->stream));
    return TW_OK;
}

}  // namespace

int tw_get_decisions(tw_engine* e, int pass, int32_t* rank, int32_t* list_n, double* margin) {
    if (e == nullptr) return TW_ERR_ARG;
    if (!pass_resident(e, pass)) return fail(e, TW_ERR_STATE, "tw_get_decisions: the results of that pass are not resident");
    HIPCHK(hipSetDevice(e->device));
    TWCHK(conf_decisions(e));
    const ConfDev& C = e->C;
    const size_t n = (size_t)e->P.n_in_total;
    TWCHK(copy_out(e, rank, C.rank, n));
    TWCHK(copy_out(e, list_n, C.list_n, n));
    TWCHK(copy_out(e, margin, C.margin, n));
    HIPCHK(hipStreamSynchronize(e->stream));
    return stage_elapsed(e, SE_CONF, 0, 1, &e->cf_ms[0]);
}

int tw_score_traces(tw_engine* e, const tw_conf_query* q, const tw_confidence* out, int64_t* summary) {
    if (e == nullptr || q == nullptr) return TW_ERR_ARG;
    TWCHK(need_forest(e, "tw_score_traces"));
    if (e->stitched_pass != 1 && e->stitched_pass != 2)
        return fail(e, TW_ERR_STATE, "tw_score_traces: the forest was stitched from tw_set_parents or from the truth: it holds no decisions of this engine");
    if (!pass_resident(e, e->stitched_pass)) return fail(e, TW_ERR_STATE, "tw_score_traces: the pass the forest was stitched from is no longer resident");
    if (q->n_edges < 0 || q->n_edges > kConfMaxEdges || (q->n_edges > 0 && q->edges == nullptr))
        return fail(e, TW_ERR_ARG, "tw_score_traces: n_edges outside [0, 15]");
    ConfQueryDev Q{};
    Q.threshold = q->threshold;
    Q.n_edges = q->n_edges;
    for (int j = 0; j < q->n_edges; j++) {
        if (!(q->edges[j] == q->edges[j]) || (j > 0 && !(q->edges[j] > q->edges[j - 1])))
            return fail(e, TW_ERR_ARG, "tw_score_traces: the edges must be ascending and not NaN");
        Q.edges[j] = q->edges[j];
    }
    HIPCHK(hipSetDevice(e->device));
    const Dev& P = e->P;
    const StitchDev& S = e->S;
    ConfDev& C = e->C;
    const int64_t nt = e->st_trees;
    if (C.row_request == nullptr || S.n_rows > e->conf_rows_cap) {   // (freed with the batch)
        DEV_ALLOC(C.row_request, S.n_rows); DEV_ALLOC(C.decisions, S.n_rows); DEV_ALLOC(C.not_best, S.n_rows); DEV_ALLOC(C.unassigned, S.n_rows);
        DEV_ALLOC(C.weakest_row, S.n_rows); DEV_ALLOC(C.min_margin, S.n_rows); DEV_ALLOC(C.confident, S.n_rows);
        e->conf_rows_cap = S.n_rows;
    }
    TWCHK(conf_decisions(e));
    drop_sig(e);   // (the CONFIDENT bit of the flags is rewritten: the eligible trees of a resident signature result may change)
    const unsigned threads = flat_threads(e);
    const dim3 tb(threads), trees(flat_grid(nt, threads)), reqs(flat_grid(P.n_in_total, threads));
    HIPCHK(hipMemsetAsync(C.row_request, 0xff, sizeof(int32_t) * (size_t)S.n_rows, e->stream));
    hipLaunchKernelGGL(k_conf_scatter, reqs, tb, 0, e->stream, S, C, P.n_in_total);
    const WaveShape per_tree = wave_shape(e, nt, kConfTrees, kConfWaves);
    hipLaunchKernelGGL(k_conf_trees, per_tree.grid, per_tree.block, 0, e->stream, S, C, Q, nt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->stage_ev[SE_CONF + 2], e->stream));
    HIPCHK(hipMemsetAsync(C.cells, 0, sizeof(unsigned long long) * kConfCells, e->stream));
    hipLaunchKernelGGL(k_conf_calib, trees, tb, 0, e->stream, S, C, Q, nt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->stage_ev[SE_CONF + 3], e->stream));
    unsigned long long cells[kConfCells];
    HIPCHK(hipMemcpyAsync(cells, C.cells, sizeof(cells), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int i = 0; i < 3; i++) TWCHK(stage_elapsed(e, SE_CONF, i, i + 1, &e->cf_ms[i]));
    if (summary != nullptr)
        for (int k = 0; k < 5; k++) summary[k] = (int64_t)cells[(kConfMaxEdges + 2) * kConfCalibCols + k];
    if (out != nullptr) {
        if (out->calib != nullptr)
            for (int b = 0; b < q->n_edges + 2; b++)
                for (int c = 0; c < kConfCalibCols; c++)
                    out->calib[b * kConfCalibCols + c] = (c == 1 && !e->stitched_truth) ? -1 : (int64_t)cells[b * kConfCalibCols + c];
        const size_t n = (size_t)P.n_in_total;
        TWCHK(copy_out(e, out->rank, C.rank, n));
        TWCHK(copy_out(e, out->list_n, C.list_n, n));
        TWCHK(copy_out(e, out->margin, C.margin, n));
        TWCHK(copy_out(e, out->row_request, C.row_request, S.n_rows));
        TWCHK(copy_out(e, out->tree_decisions, C.decisions, nt));
        TWCHK(copy_out(e, out->tree_not_best, C.not_best, nt));
        TWCHK(copy_out(e, out->tree_unassigned, C.unassigned, nt));
        TWCHK(copy_out(e, out->tree_min_margin, C.min_margin, nt));
        TWCHK(copy_out(e, out->tree_weakest_row, C.weakest_row, nt));
        TWCHK(copy_out(e, out->tree_confident, C.confident, nt));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return TW_OK;
}

/* ---- per-service latency distributions and cohorts (tw_dist.h) ----------------------------------------------------- */
int tw_set_row_cohorts(tw_engine* e, int32_t n_cohorts, const int32_t* row_cohort) {
    if (e == nullptr) return TW_ERR_ARG;
    if (!e->rows_set) return fail(e, TW_ERR_STATE, "tw_set_row_cohorts before tw_set_span_rows (tw_load_batch and tw_scale_load drop the row maps)");
    if (n_cohorts < 1) return fail(e, TW_ERR_ARG, "tw_set_row_cohorts: n_cohorts must be positive");
    if (row_cohort == nullptr && n_cohorts != 1) return fail(e, TW_ERR_ARG, "tw_set_row_cohorts: no labels with n_cohorts != 1");
    const int64_t n_rows = e->S.n_rows;
    if (row_cohort != nullptr)
        for (int64_t r = 0; r < n_rows; r++)   // k_dist_items indexes the segments with the trees' cohorts
            if (row_cohort[r] < -1 || row_cohort[r] >= n_cohorts) return fail(e, TW_ERR_ARG, "tw_set_row_cohorts: row_cohort outside [-1, n_cohorts)");
    HIPCHK(hipSetDevice(e->device));
    DistDev& D = e->D;
    drop_cohorts(e);
    if (row_cohort == nullptr) return TW_OK;   // back to one cohort that holds every tree
    if (D.row_cohort == nullptr || n_rows > e->cohort_rows_cap) {   // (freed with the batch)
        int32_t* label_d;
        DEV_ALLOC(label_d, n_rows);
        D.row_cohort = label_d;
        e->cohort_rows_cap = n_rows;
    }
    HIPCHK(hipMemcpyAsync(const_cast<int32_t*>(D.row_cohort), row_cohort, sizeof(int32_t) * (size_t)n_rows, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    D.n_cohorts = n_cohorts;
    e->cohorts_set = true;
    return TW_OK;
}

namespace {

int dist_bits(unsigned long long x) {   // bits needed to write x
    int b = 0;
    while (x != 0) { b++; x >>= 1; }
    return b;
}

// Cohorts, counts, items, sort, offsets and values of the resident attribution into e->D; the first three events of SE_DIST around the two halves.
int dist_build(tw_engine* e) {
    const StitchDev& S = e->S;
    const AttrDev& A = e->A;
    DistDev D = e->D;   // (the kernels' view: row_cohort is null without labels)
    const int64_t nt = e->st_trees;
    if (!e->cohorts_set) { D.row_cohort = nullptr; D.n_cohorts = 1; }
    D.n_seg = (int64_t)D.n_cohorts * (3 * (int64_t)A.n_groups + 1);
    if (D.counters == nullptr) DEV_ALLOC(D.counters, kDistCounters);   // (all of them freed with the batch)
    if (D.tree_cohort == nullptr || nt > e->dist_trees_cap) { DEV_ALLOC(D.tree_cohort, nt); e->dist_trees_cap = nt; }
    if (D.seg_count == nullptr || D.n_seg > e->dist_seg_cap) {
        DEV_ALLOC(D.seg_count, D.n_seg); DEV_ALLOC(D.seg_sum, D.n_seg); DEV_ALLOC(D.seg_off, D.n_seg + 1);
        e->dist_seg_cap = D.n_seg;
    }
    const unsigned threads = flat_threads(e);
    const dim3 tb(threads);
    // workgroups stride over the rows: at most 2048 of them clear and add up an LDS table
    const dim3 rows(std::min(flat_grid(S.n_rows, threads), 2048u));
    unsigned long long counters[kDistCounters] = {0, ~0ull, 0, 0, 0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(D.counters, counters, sizeof(counters), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(D.seg_count, 0, sizeof(unsigned long long) * (size_t)D.n_seg, e->stream));
    HIPCHK(hipMemsetAsync(D.seg_sum, 0, sizeof(unsigned long long) * (size_t)D.n_seg, e->stream));
    HIPCHK(hipEventRecord(e->stage_ev[SE_DIST + 0], e->stream));
    if (D.row_cohort != nullptr) {
        const WaveShape per_tree = wave_shape(e, nt, kDistTrees, kDistWaves);
        hipLaunchKernelGGL(k_dist_cohort, per_tree.grid, per_tree.block, 0, e->stream, S, D, nt);
    } else {
        HIPCHK(hipMemsetAsync(D.tree_cohort, 0, sizeof(int32_t) * (size_t)std::max<int64_t>(nt, 1), e->stream));
    }
    DistKeyDev K{};
    hipLaunchKernelGGL(k_dist_items<false>, rows, tb, 0, e->stream, S, A, D, K);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(counters, D.counters, sizeof(counters), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int64_t n_items = (int64_t)counters[0];
    int seg_bits = dist_bits((unsigned long long)(D.n_seg - 1));
    if (n_items > 0) {
        K.vmin = counters[1] ^ (1ull << 63);
        K.vbits = dist_bits(counters[2] - counters[1]);
        K.wide = seg_bits + K.vbits > 64 ? 1 : 0;
    }
    if (D.key_a == nullptr || n_items > D.items_cap) {
        DEV_ALLOC(D.key_a, n_items); DEV_ALLOC(D.key_b, n_items); DEV_ALLOC(D.values, n_items);
        D.seg_a = nullptr; D.seg_b = nullptr;
        D.items_cap = std::max<int64_t>(n_items, 1);
    }
    if (K.wide && D.seg_a == nullptr) { DEV_ALLOC(D.seg_a, D.items_cap); DEV_ALLOC(D.seg_b, D.items_cap); }
    if (n_items > 0) hipLaunchKernelGGL(k_dist_items<true>, rows, tb, 0, e->stream, S, A, D, K);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->stage_ev[SE_DIST + 1], e->stream));
    const unsigned long long* sorted = D.key_a;
    if (n_items > 0 && !K.wide) {
        const unsigned end_bit = (unsigned)std::max(seg_bits + K.vbits, 1);
        TWCHK(rocprim_call(e, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_keys(tmp, bytes, D.key_a, D.key_b, (size_t)n_items, 0u, end_bit, e->stream); }));
        sorted = D.key_b;
    } else if (n_items > 0) {   // stable: by value, then by segment (the temporary is sized for both before the first is queued)
        auto by_value = [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_pairs(tmp, bytes, D.key_a, D.key_b, D.seg_a, D.seg_b, (size_t)n_items, 0u, (unsigned)K.vbits, e->stream); };
        auto by_segment = [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_pairs(tmp, bytes, D.seg_b, D.seg_a, D.key_b, D.key_a, (size_t)n_items, 0u, (unsigned)seg_bits, e->stream); };
        size_t bytes2 = 0;
        HIPCHK(by_segment(nullptr, bytes2));
        TWCHK(rocprim_call(e, by_value, bytes2));
        TWCHK(rocprim_call(e, by_segment));
    }
    hipLaunchKernelGGL(k_dist_scan, dim3(1), tb, 0, e->stream, D);
    if (n_items > 0) hipLaunchKernelGGL(k_dist_unpack, dim3(flat_grid(n_items, threads)), tb, 0, e->stream, D, K, sorted, n_items);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->stage_ev[SE_DIST + 2], e->stream));
    HIPCHK(hipMemcpyAsync(counters, D.counters, sizeof(counters), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (counters[7] != 0 || (int64_t)counters[6] != n_items) return fail(e, TW_ERR_DEVICE, "tw_latency_distributions: the two sweeps over the rows disagree on the number of items");
    for (int i = 0; i < 2; i++) TWCHK(stage_elapsed(e, SE_DIST, i, i + 1, &e->ds_ms[i]));
    const int32_t* labels = e->D.row_cohort;
    const int32_t n_cohorts = e->D.n_cohorts;
    e->D = D;
    e->D.row_cohort = labels; e->D.n_cohorts = n_cohorts;   // (the labels stay set whether or not this call used them)
    e->dist_key = K;
    e->dist_items = n_items;
    e->dist_ready = true;
    return TW_OK;
}

}  // namespace

namespace {

// the checks of a tw_dist_query, and the query as the kernels read it
int dist_query(tw_engine* e, const tw_dist_query* q, DistQueryDev& Q, const std::string& fn) {
    if (q->n_q < 0 || q->n_q > kDistMaxQ || (q->n_q > 0 && q->probs == nullptr)) return fail(e, TW_ERR_ARG, fn + ": n_q outside [0, 32]");
    if (q->n_edges < 0 || q->n_edges > kDistMaxEdges || (q->n_edges > 0 && q->edges == nullptr)) return fail(e, TW_ERR_ARG, fn + ": n_edges outside [0, 63]");
    Q.n_q = q->n_q;
    Q.n_edges = q->n_edges;
    for (int j = 0; j < q->n_q; j++) {
        if (!(q->probs[j] >= 0.0 && q->probs[j] <= 1.0)) return fail(e, TW_ERR_ARG, fn + ": a prob outside [0, 1]");
        Q.probs[j] = q->probs[j];
    }
    for (int j = 0; j < q->n_edges; j++) {
        if (j > 0 && !(q->edges[j] > q->edges[j - 1])) return fail(e, TW_ERR_ARG, fn + ": the edges must be strictly ascending");
        Q.edges[j] = q->edges[j];
    }
    return TW_OK;
}

// Quantiles, histogram and the copies to the host of the segments V views (the resident items, or the history): the scratch of the
// two kernels is that of e->D whichever it is (freed with the batch).  Events ev, ev + 1 around the kernels; the stream is left
// with the copies queued.
int dist_answer(tw_engine* e, DistDev V, int64_t n_items, const DistQueryDev& Q, const tw_distributions* out, int ev) {
    const int64_t n_seg = V.n_seg;
    const int bins = Q.n_edges + 1;
    const bool want_q = out != nullptr && out->quantile != nullptr && Q.n_q > 0, want_h = out != nullptr && out->hist != nullptr;
    if ((want_q || want_h) && (e->D.quant == nullptr || n_seg > e->dist_out_cap)) {   // room for any query on these segments
        DEV_ALLOC(e->D.quant, n_seg * kDistMaxQ); DEV_ALLOC(e->D.hist, n_seg * (kDistMaxEdges + 1));
        e->dist_out_cap = n_seg;
    }
    V.quant = e->D.quant; V.hist = e->D.hist;
    const unsigned threads = flat_threads(e);
    const dim3 tb(threads);
    HIPCHK(hipEventRecord(e->stage_ev[ev], e->stream));
    if (want_q) hipLaunchKernelGGL(k_dist_quantiles, dim3(flat_grid(n_seg * Q.n_q, threads)), tb, 0, e->stream, V, Q);
    if (want_h) hipLaunchKernelGGL(k_dist_hist, dim3(flat_grid(n_seg * bins, threads)), tb, 0, e->stream, V, Q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->stage_ev[ev + 1], e->stream));
    if (out != nullptr) {
        TWCHK(copy_out(e, out->seg_count, V.seg_count, n_seg));
        TWCHK(copy_out(e, out->seg_sum, V.seg_sum, n_seg));
        TWCHK(copy_out(e, out->seg_off, V.seg_off, n_seg + 1));
        TWCHK(copy_out(e, out->values, V.values, n_items));
        if (want_q) TWCHK(copy_out(e, out->quantile, V.quant, n_seg * Q.n_q));
        if (want_h) TWCHK(copy_out(e, out->hist, V.hist, n_seg * bins));
    }
    return TW_OK;
}

}  // namespace

int tw_latency_distributions(tw_engine* e, const tw_dist_query* q, const tw_distributions* out, int64_t* summary) {
    if (e == nullptr || q == nullptr) return TW_ERR_ARG;
    if (!e->attributed)
        return fail(e, TW_ERR_STATE, "tw_latency_distributions needs a tw_attribute_traces call on the current forest (a new tw_stitch_traces, new row groups and "
                                     "whatever drops the forest drop the attribution)");
    DistQueryDev Q{};
    TWCHK(dist_query(e, q, Q, "tw_latency_distributions"));
    const int64_t n_seg = (int64_t)(e->cohorts_set ? e->D.n_cohorts : 1) * (3 * (int64_t)e->A.n_groups + 1);
    if (n_seg > kDistMaxSeg) return fail(e, TW_ERR_UNSUPPORTED, "tw_latency_distributions: more than 2^24 segments (n_cohorts * (3 * n_groups + 1))");
    HIPCHK(hipSetDevice(e->device));
    if (!e->dist_ready) TWCHK(dist_build(e));
    const int64_t nt = e->st_trees, n_items = e->dist_items;
    TWCHK(dist_answer(e, e->D, n_items, Q, out, SE_DIST + 3));
    unsigned long long counters[kDistCounters];
    HIPCHK(hipMemcpyAsync(counters, e->D.counters, sizeof(counters), hipMemcpyDeviceToHost, e->stream));
    if (out != nullptr) TWCHK(copy_out(e, out->tree_cohort, e->D.tree_cohort, nt));
    HIPCHK(hipStreamSynchronize(e->stream));
    TWCHK(stage_elapsed(e, SE_DIST, 3, 4, &e->ds_ms[2]));
    if (summary != nullptr) {
        summary[0] = n_items; summary[1] = (int64_t)counters[5]; summary[2] = (int64_t)counters[3]; summary[3] = (int64_t)counters[4];
    }
    return TW_OK;
}

/* ---- two cohorts compared: KS, rank sum, quantile shifts, permutation test (tw_cmp.h) -------------------------------- */
namespace {

// The comparison of the cohorts [0, n_cohorts) of the segments D views (the resident items, or the history): the checks of the
// query, the kernels, the copies and the summary.  Events ev .. ev + 2, the two times into ms[0], ms[1].
int cmp_run(tw_engine* e, const DistDev& D, int32_t n_cohorts, int64_t per, const tw_cmp_query* q, const tw_cohort_comparison* out, int64_t* summary,
            const std::string& fn, int ev, double* ms, bool checks_only) {
    if (q->n_pairs < 1 || q->n_pairs > kCmpMaxPairs || q->pairs == nullptr) return fail(e, TW_ERR_ARG, fn + ": n_pairs outside [1, 64]");
    for (int i = 0; i < q->n_pairs; i++) {
        const int32_t a = q->pairs[2 * i], b = q->pairs[2 * i + 1];
        if (a < 0 || a >= n_cohorts || b < 0 || b >= n_cohorts) return fail(e, TW_ERR_ARG, fn + ": a pair names a cohort outside [0, n_cohorts)");
        if (a == b) return fail(e, TW_ERR_ARG, fn + ": a pair compares a cohort with itself");
    }
    if (q->n_q < 0 || q->n_q > kCmpMaxQ || (q->n_q > 0 && q->probs == nullptr)) return fail(e, TW_ERR_ARG, fn + ": n_q outside [0, 8]");
    for (int j = 0; j < q->n_q; j++)
        if (!(q->probs[j] >= 0.0 && q->probs[j] <= 1.0)) return fail(e, TW_ERR_ARG, fn + ": a prob outside [0, 1]");
    if (q->n_perm < 0 || q->n_perm > kCmpMaxPerm) return fail(e, TW_ERR_ARG, fn + ": n_perm outside [0, 65536]");
    if (q->max_pool < 0) return fail(e, TW_ERR_ARG, fn + ": max_pool below 0");
    const int64_t n_seg = (int64_t)n_cohorts * per;
    if (n_seg > kDistMaxSeg) return fail(e, TW_ERR_UNSUPPORTED, fn + ": more than 2^24 segments (n_cohorts * (3 * n_groups + 1))");
    if (checks_only) return TW_OK;
    // the sizes of the rows: limits, pool offsets and the summary on the host
    std::vector<unsigned long long> count((size_t)n_seg);
    HIPCHK(hipMemcpyAsync(count.data(), D.seg_count, sizeof(unsigned long long) * (size_t)n_seg, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int64_t n_rows = (int64_t)q->n_pairs * per;
    std::vector<int64_t> row_off((size_t)n_rows + 1, 0);
    int64_t both = 0, permuted = 0, permuted_items = 0;
    for (int64_t row = 0; row < n_rows; row++) {
        const int64_t pi = row / per, r = row - pi * per;
        const unsigned long long na = count[(size_t)(q->pairs[2 * pi] * per + r)], nb = count[(size_t)(q->pairs[2 * pi + 1] * per + r)];
        int64_t n = 0;
        if (na > 0 && nb > 0) {
            if (na + nb >= (1ull << 32)) return fail(e, TW_ERR_UNSUPPORTED, fn + ": a row pools 2^32 values or more");
            if (na * nb >= (1ull << 61)) return fail(e, TW_ERR_UNSUPPORTED, fn + ": n_a * n_b of a row is 2^61 or more");
            n = (int64_t)(na + nb);
            both++;
            if (q->n_perm > 0 && (q->max_pool == 0 || n <= q->max_pool)) { permuted++; permuted_items += n; }
        }
        row_off[(size_t)row + 1] = row_off[(size_t)row] + n;
    }
    const int64_t n_items = row_off[(size_t)n_rows];
    CmpDev& M = e->M;
    if (M.pairs == nullptr) { int32_t* pairs_d; DEV_ALLOC(pairs_d, 2 * kCmpMaxPairs); M.pairs = pairs_d; }   // (all of them freed with the batch)
    if (M.row_off == nullptr || n_rows > e->cmp_rows_cap) {
        int64_t* off_d;
        DEV_ALLOC(off_d, n_rows + 1);
        M.row_off = off_d;
        DEV_ALLOC(M.ks_abs, n_rows); DEV_ALLOC(M.ks_pos, n_rows); DEV_ALLOC(M.u2_acc, n_rows);
        DEV_ALLOC(M.n_a, n_rows); DEV_ALLOC(M.n_b, n_rows); DEV_ALLOC(M.ks_gap, n_rows); DEV_ALLOC(M.ks_at, n_rows); DEV_ALLOC(M.u2, n_rows);
        DEV_ALLOC(M.ge_ks, n_rows); DEV_ALLOC(M.ge_u, n_rows);
        DEV_ALLOC(M.shift, n_rows * kCmpMaxQ); DEV_ALLOC(M.ge_q, n_rows * kCmpMaxQ);
        e->cmp_rows_cap = n_rows;
    }
    if (M.pool == nullptr || n_items > e->cmp_items_cap) {
        DEV_ALLOC(M.pool, n_items); DEV_ALLOC(M.gabs, n_items);
        e->cmp_items_cap = std::max<int64_t>(n_items, 1);
    }
    M.n_pairs = q->n_pairs; M.n_q = q->n_q; M.n_perm = q->n_perm;
    M.per = per; M.n_rows = n_rows; M.n_items = n_items;
    M.max_pool = q->max_pool; M.seed = q->seed;
    for (int j = 0; j < kCmpMaxQ; j++) M.probs[j] = j < q->n_q ? q->probs[j] : 0.0;
    HIPCHK(hipMemcpyAsync(const_cast<int32_t*>(M.pairs), q->pairs, sizeof(int32_t) * 2 * (size_t)q->n_pairs, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(const_cast<int64_t*>(M.row_off), row_off.data(), sizeof(int64_t) * ((size_t)n_rows + 1), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(M.ks_abs, 0, sizeof(unsigned long long) * (size_t)n_rows, e->stream));
    HIPCHK(hipMemsetAsync(M.u2_acc, 0, sizeof(unsigned long long) * (size_t)n_rows, e->stream));
    HIPCHK(hipMemsetAsync(M.ks_pos, 0xFF, sizeof(unsigned long long) * (size_t)n_rows, e->stream));
    const unsigned threads = flat_threads(e);
    const dim3 tb(threads);
    HIPCHK(hipEventRecord(e->stage_ev[ev + 0], e->stream));
    if (n_items > 0) {
        const dim3 items((unsigned)std::min<int64_t>(flat_grid(n_items, threads), 1 << 20));
        hipLaunchKernelGGL(k_cmp_rank, items, tb, 0, e->stream, D, M);
        hipLaunchKernelGGL(k_cmp_at, items, tb, 0, e->stream, M);
    }
    hipLaunchKernelGGL(k_cmp_final, dim3(flat_grid(n_rows, threads)), tb, 0, e->stream, D, M);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->stage_ev[ev + 1], e->stream));
    if (permuted > 0) {
        const WaveShape per_block = wave_shape(e, n_rows * ((q->n_perm + 63) / 64), 1, kCmpWaves);
        hipLaunchKernelGGL(k_cmp_perm, per_block.grid, per_block.block, 0, e->stream, M);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(e->stage_ev[ev + 2], e->stream));
    if (out != nullptr) {
        const size_t nr = (size_t)n_rows, nrq = nr * (size_t)q->n_q;
        TWCHK(copy_out(e, out->n_a, M.n_a, nr));
        TWCHK(copy_out(e, out->n_b, M.n_b, nr));
        TWCHK(copy_out(e, out->ks_gap, M.ks_gap, nr));
        TWCHK(copy_out(e, out->ks_at, M.ks_at, nr));
        TWCHK(copy_out(e, out->u2, M.u2, nr));
        if (nrq > 0) TWCHK(copy_out(e, out->quantile_shift, M.shift, nrq));
        if (q->n_perm > 0) {
            TWCHK(copy_out(e, out->perm_ge_ks, M.ge_ks, nr));
            TWCHK(copy_out(e, out->perm_ge_u, M.ge_u, nr));
            if (nrq > 0) TWCHK(copy_out(e, out->perm_ge_q, M.ge_q, nrq));
        }
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int i = 0; i < 2; i++) TWCHK(stage_elapsed(e, ev, i, i + 1, &ms[i]));
    if (summary != nullptr) { summary[0] = both; summary[1] = permuted; summary[2] = permuted_items; summary[3] = q->n_perm; }
    return TW_OK;
}

}  // namespace

int tw_compare_cohorts(tw_engine* e, const tw_cmp_query* q, const tw_cohort_comparison* out, int64_t* summary) {
    if (e == nullptr || q == nullptr) return TW_ERR_ARG;
    if (!e->attributed)
        return fail(e, TW_ERR_STATE, "tw_compare_cohorts needs a tw_attribute_traces call on the current forest (a new tw_stitch_traces, new row groups and "
                                     "whatever drops the forest drop the attribution)");
    const int32_t n_cohorts = e->cohorts_set ? e->D.n_cohorts : 1;
    const int64_t per = 3 * (int64_t)e->A.n_groups + 1;
    TWCHK(cmp_run(e, e->D, n_cohorts, per, q, out, summary, "tw_compare_cohorts", SE_CMP, e->cm_ms, true));   // refused before the items are built
    HIPCHK(hipSetDevice(e->device));
    if (!e->dist_ready) TWCHK(dist_build(e));
    return cmp_run(e, e->D, n_cohorts, per, q, out, summary, "tw_compare_cohorts", SE_CMP, e->cm_ms, false);
}

/* ---- the distributions of batch after batch: a history on the device (tw_hist.h) ---------------------------------------- */
namespace {

// A buffer of the history's own (not a load's): the new one first, so that a failure leaves the old one and the history intact.
extern "C++" {
template <class T>
int hist_grow(tw_engine* e, T** p, int64_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, (size_t)std::max<int64_t>(count, 1) * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(e, TW_ERR_DEVICE, "tw_history: no device memory for " + std::to_string(count) + " elements (the history is as it was)");
    }
    if (*p != nullptr) (void)hipFree(*p);
    *p = (T*)q;
    return TW_OK;
}
}

struct HistSource {                  // sorted segments on the device: the resident items of a batch, or an uploaded source
    int32_t n_cohorts, n_groups;
    const int64_t* off;
    const unsigned long long *count, *sum;
    const int64_t* values;
};

// The checks of a cohort map (NULL = the identity) against the history as it is; inv[h] = the source cohort that goes to history
// cohort h, C_new = the history's cohorts afterwards.
int hist_map(tw_engine* e, const std::string& fn, int32_t n_cohorts, int32_t n_groups, const int32_t* cohort_map, std::vector<int32_t>& inv, int32_t& C_new) {
    if (n_groups < 1) return fail(e, TW_ERR_ARG, fn + ": n_groups must be positive");
    if (e->hist_G != 0 && n_groups != e->hist_G)
        return fail(e, TW_ERR_ARG, fn + ": the history holds " + std::to_string(e->hist_G) + " groups, the source " + std::to_string(n_groups) + " (tw_history_reset opens it again)");
    std::vector<int32_t> seen;
    int64_t top = -1;
    for (int32_t c = 0; c < n_cohorts; c++) {
        const int32_t h = cohort_map != nullptr ? cohort_map[c] : c;
        if (h < -1) return fail(e, TW_ERR_ARG, fn + ": cohort_map holds an entry below -1");
        if (h >= 0) seen.push_back(h);
        top = std::max<int64_t>(top, h);
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
        return fail(e, TW_ERR_ARG, fn + ": two cohorts of the source go to one cohort of the history (a push merges two sorted runs per segment, never more)");
    const int64_t c_new = std::max<int64_t>(e->hist_C, top + 1), per = 3 * (int64_t)n_groups + 1;
    if (c_new * per > kDistMaxSeg) return fail(e, TW_ERR_UNSUPPORTED, fn + ": more than 2^24 segments in the history (C_h * (3 * n_groups + 1))");
    C_new = (int32_t)c_new;
    inv.assign((size_t)c_new, -1);
    for (int32_t c = 0; c < n_cohorts; c++) {
        const int32_t h = cohort_map != nullptr ? cohort_map[c] : c;
        if (h >= 0) inv[(size_t)h] = c;
    }
    return TW_OK;
}

// Plan and merge of `src` into the side of the history that is not in use, and the swap when nothing has failed.  Events
// SE_HIST + 0 (recorded here unless the caller has: `started`) .. + 2.
int hist_absorb(tw_engine* e, const HistSource& src, const std::vector<int32_t>& inv, int32_t C_new, int64_t* summary, bool started) {
    const int64_t per = 3 * (int64_t)src.n_groups + 1, n_seg = (int64_t)C_new * per, n_old = (int64_t)e->hist_C * per;
    const tw_engine::HistSide& from = e->hist_side[e->hist_cur];
    tw_engine::HistSide& to = e->hist_side[e->hist_cur ^ 1];
    if (n_seg > to.seg_cap || to.off == nullptr) {
        to.seg_cap = 0;
        TWCHK(hist_grow(e, &to.off, n_seg + 1)); TWCHK(hist_grow(e, &to.count, n_seg)); TWCHK(hist_grow(e, &to.sum, n_seg));
        to.seg_cap = n_seg;
    }
    if (n_seg > e->hist_plan_cap || e->hist_tile_off == nullptr) {
        e->hist_plan_cap = 0;
        TWCHK(hist_grow(e, &e->hist_tile_off, n_seg + 1));
        e->hist_plan_cap = n_seg;
    }
    if (C_new > e->hist_inv_cap || e->hist_inv == nullptr) {
        e->hist_inv_cap = 0;
        TWCHK(hist_grow(e, &e->hist_inv, (int64_t)C_new));
        e->hist_inv_cap = C_new;
    }
    if (e->hist_counters == nullptr) TWCHK(hist_grow(e, &e->hist_counters, (int64_t)kHistCounters));
    HistDev H{};
    H.per = per; H.n_seg = n_seg; H.n_old = n_old;
    H.old_off = from.off; H.old_count = from.count; H.old_sum = from.sum; H.old_values = from.values;
    H.inv = e->hist_inv;
    H.src_off = src.off; H.src_count = src.count; H.src_sum = src.sum; H.src_values = src.values;
    H.new_off = to.off; H.new_count = to.count; H.new_sum = to.sum;
    H.tile_off = e->hist_tile_off; H.counters = e->hist_counters;
    if (!started) HIPCHK(hipEventRecord(e->stage_ev[SE_HIST + 0], e->stream));
    if (C_new > 0) HIPCHK(hipMemcpyAsync(e->hist_inv, inv.data(), sizeof(int32_t) * (size_t)C_new, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(e->hist_counters, 0, sizeof(unsigned long long) * kHistCounters, e->stream));
    hipLaunchKernelGGL(k_hist_plan, dim3(1), dim3(flat_threads(e)), 0, e->stream, H);
    HIPCHK(hipGetLastError());
    unsigned long long counters[kHistCounters];
    HIPCHK(hipMemcpyAsync(counters, e->hist_counters, sizeof(counters), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int64_t added = (int64_t)counters[0], held = (int64_t)counters[1], n_tiles = (int64_t)counters[2];
    if (held > to.cap || to.values == nullptr) {   // geometric: at least twice what this side held
        const int64_t cap = std::max<int64_t>(std::max<int64_t>(held, 2 * to.cap), 1);
        to.cap = 0;
        TWCHK(hist_grow(e, &to.values, cap));
        to.cap = cap;
    }
    H.new_values = to.values;
    HIPCHK(hipEventRecord(e->stage_ev[SE_HIST + 1], e->stream));
    if (n_tiles > 0) {
        const unsigned threads = e->K.coop >= 64 ? (unsigned)kHistThreads : (unsigned)e->K.coop;
        hipLaunchKernelGGL(k_hist_merge, dim3((unsigned)std::min<int64_t>(n_tiles, 1 << 24)), dim3(threads), 0, e->stream, H, n_tiles);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(e->stage_ev[SE_HIST + 2], e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int i = 0; i < 2; i++) TWCHK(stage_elapsed(e, SE_HIST, i, i + 1, &e->hs_ms[i]));
    // nothing has failed: the other side is the history now
    e->hist_cur ^= 1;
    e->hist_C = C_new; e->hist_G = src.n_groups; e->hist_items = held; e->hist_pushes++;
    if (summary != nullptr) { summary[0] = added; summary[1] = held; summary[2] = C_new; summary[3] = e->hist_pushes; }
    return TW_OK;
}

// the history as the quantile, histogram and comparison kernels read it
DistDev hist_view(const tw_engine* e) {
    const tw_engine::HistSide& side = e->hist_side[e->hist_cur];
    DistDev V{};
    V.n_cohorts = e->hist_C;
    V.n_seg = (int64_t)e->hist_C * (3 * (int64_t)e->hist_G + 1);
    V.seg_count = side.count; V.seg_sum = side.sum; V.seg_off = side.off; V.values = side.values;
    V.items_cap = side.cap;
    return V;
}

int need_history(tw_engine* e, const char* fn) {
    if (e->hist_C > 0) return TW_OK;
    return fail(e, TW_ERR_STATE, std::string(fn) + " on an empty history (tw_history_push or tw_history_merge first; tw_history_reset empties it)");
}

}  // namespace

int tw_history_reset(tw_engine* e) {
    if (e == nullptr) return TW_ERR_ARG;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    hist_free(e);
    return TW_OK;
}

int tw_history_push(tw_engine* e, int32_t n_map, const int32_t* cohort_map, int64_t* summary) {
    if (e == nullptr) return TW_ERR_ARG;
    if (!e->attributed)
        return fail(e, TW_ERR_STATE, "tw_history_push needs a tw_attribute_traces call on the current forest (a new tw_stitch_traces, new row groups and "
                                     "whatever drops the forest drop the attribution)");
    const int32_t n_cohorts = e->cohorts_set ? e->D.n_cohorts : 1, G = e->A.n_groups;
    if (n_map != n_cohorts) return fail(e, TW_ERR_ARG, "tw_history_push: n_map must be the batch's n_cohorts (" + std::to_string(n_cohorts) + ")");
    std::vector<int32_t> inv;
    int32_t C_new = 0;
    TWCHK(hist_map(e, "tw_history_push", n_cohorts, G, cohort_map, inv, C_new));
    if ((int64_t)n_cohorts * (3 * (int64_t)G + 1) > kDistMaxSeg) return fail(e, TW_ERR_UNSUPPORTED, "tw_history_push: more than 2^24 segments in the batch (n_cohorts * (3 * n_groups + 1))");
    HIPCHK(hipSetDevice(e->device));
    if (!e->dist_ready) TWCHK(dist_build(e));
    const HistSource src{n_cohorts, G, e->D.seg_off, e->D.seg_count, e->D.seg_sum, e->D.values};
    return hist_absorb(e, src, inv, C_new, summary, false);
}

int tw_history_merge(tw_engine* e, int32_t n_cohorts_src, int32_t n_groups, const int64_t* seg_off_src, const int64_t* values_src, const int32_t* cohort_map,
                     int64_t* summary) {
    if (e == nullptr) return TW_ERR_ARG;
    if (n_cohorts_src < 1 || seg_off_src == nullptr) return fail(e, TW_ERR_ARG, "tw_history_merge: n_cohorts_src must be positive, seg_off_src given");
    std::vector<int32_t> inv;
    int32_t C_new = 0;
    TWCHK(hist_map(e, "tw_history_merge", n_cohorts_src, n_groups, cohort_map, inv, C_new));
    const int64_t n_seg = (int64_t)n_cohorts_src * (3 * (int64_t)n_groups + 1);
    if (n_seg > kDistMaxSeg) return fail(e, TW_ERR_UNSUPPORTED, "tw_history_merge: more than 2^24 segments in the source (n_cohorts_src * (3 * n_groups + 1))");
    if (seg_off_src[0] != 0) return fail(e, TW_ERR_ARG, "tw_history_merge: seg_off_src must start at 0");
    for (int64_t s = 0; s < n_seg; s++)
        if (seg_off_src[s + 1] < seg_off_src[s]) return fail(e, TW_ERR_ARG, "tw_history_merge: seg_off_src must not decrease");
    const int64_t n_items = seg_off_src[n_seg];
    if (n_items > 0 && values_src == nullptr) return fail(e, TW_ERR_ARG, "tw_history_merge: no values_src for " + std::to_string(n_items) + " items");
    HIPCHK(hipSetDevice(e->device));
    if (n_seg > e->hist_src_seg_cap || e->hist_src_off == nullptr) {
        e->hist_src_seg_cap = 0;
        TWCHK(hist_grow(e, &e->hist_src_off, n_seg + 1)); TWCHK(hist_grow(e, &e->hist_src_count, n_seg)); TWCHK(hist_grow(e, &e->hist_src_sum, n_seg));
        e->hist_src_seg_cap = n_seg;
    }
    if (n_items > e->hist_src_cap || e->hist_src_values == nullptr) {
        e->hist_src_cap = 0;
        TWCHK(hist_grow(e, &e->hist_src_values, n_items));
        e->hist_src_cap = std::max<int64_t>(n_items, 1);
    }
    if (e->hist_counters == nullptr) TWCHK(hist_grow(e, &e->hist_counters, (int64_t)kHistCounters));
    HIPCHK(hipMemcpyAsync(e->hist_src_off, seg_off_src, sizeof(int64_t) * ((size_t)n_seg + 1), hipMemcpyHostToDevice, e->stream));
    if (n_items > 0) HIPCHK(hipMemcpyAsync(e->hist_src_values, values_src, sizeof(int64_t) * (size_t)n_items, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(e->hist_src_sum, 0, sizeof(unsigned long long) * (size_t)n_seg, e->stream));
    HIPCHK(hipMemsetAsync(e->hist_counters, 0, sizeof(unsigned long long) * kHistCounters, e->stream));
    // every segment ascending, checked before anything is merged; the counts and the sums beside it
    HIPCHK(hipEventRecord(e->stage_ev[SE_HIST + 0], e->stream));
    const HistSrcDev S{n_seg, n_items, e->hist_src_off, e->hist_src_values, e->hist_src_count, e->hist_src_sum, e->hist_counters};
    const unsigned threads = flat_threads(e);
    hipLaunchKernelGGL(k_hist_source, dim3((unsigned)std::min<int64_t>(flat_grid(std::max(n_items, n_seg), threads), 1 << 20)), dim3(threads), 0, e->stream, S);
    HIPCHK(hipGetLastError());
    unsigned long long counters[kHistCounters];
    HIPCHK(hipMemcpyAsync(counters, e->hist_counters, sizeof(counters), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (counters[3] != 0) return fail(e, TW_ERR_ARG, "tw_history_merge: a segment of values_src does not ascend");
    const HistSource src{n_cohorts_src, n_groups, e->hist_src_off, e->hist_src_count, e->hist_src_sum, e->hist_src_values};
    return hist_absorb(e, src, inv, C_new, summary, true);
}

int tw_history_info(tw_engine* e, int64_t* out6) {
    if (e == nullptr || out6 == nullptr) return TW_ERR_ARG;
    out6[0] = e->hist_C; out6[1] = e->hist_G; out6[2] = (int64_t)e->hist_C * (e->hist_G > 0 ? 3 * (int64_t)e->hist_G + 1 : 0);
    out6[3] = e->hist_items; out6[4] = e->hist_pushes; out6[5] = e->hist_side[e->hist_cur].cap;
    return TW_OK;
}

int tw_history_distributions(tw_engine* e, const tw_dist_query* q, const tw_distributions* out, int64_t* summary) {
    if (e == nullptr || q == nullptr) return TW_ERR_ARG;
    TWCHK(need_history(e, "tw_history_distributions"));
    DistQueryDev Q{};
    TWCHK(dist_query(e, q, Q, "tw_history_distributions"));
    HIPCHK(hipSetDevice(e->device));
    const DistDev V = hist_view(e);
    TWCHK(dist_answer(e, V, e->hist_items, Q, out, SE_HIST + 3));
    std::vector<unsigned long long> count((size_t)V.n_seg);
    HIPCHK(hipMemcpyAsync(count.data(), V.seg_count, sizeof(unsigned long long) * (size_t)V.n_seg, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    TWCHK(stage_elapsed(e, SE_HIST, 3, 4, &e->hs_ms[2]));
    if (summary != nullptr) {
        int64_t filled = 0;
        for (unsigned long long c : count) filled += c != 0 ? 1 : 0;
        summary[0] = e->hist_items; summary[1] = filled; summary[2] = e->hist_C; summary[3] = e->hist_pushes;
    }
    return TW_OK;
}

int tw_history_compare(tw_engine* e, const tw_cmp_query* q, const tw_cohort_comparison* out, int64_t* summary) {
    if (e == nullptr || q == nullptr) return TW_ERR_ARG;
    TWCHK(need_history(e, "tw_history_compare"));
    HIPCHK(hipSetDevice(e->device));
    return cmp_run(e, hist_view(e), e->hist_C, 3 * (int64_t)e->hist_G + 1, q, out, summary, "tw_history_compare", SE_HIST + 5, e->hs_ms + 3, false);
}

/* ---- traces grouped by call-graph signature (tw_sig.h) --------------------------------------------------------------- */
int tw_trace_signatures(tw_engine* e, const tw_sig_query* q, const tw_signatures* out, int64_t* summary) {
    if (e == nullptr || q == nullptr) return TW_ERR_ARG;
    TWCHK(need_forest(e, "tw_trace_signatures"));
    if (!e->groups_set) return fail(e, TW_ERR_STATE, "tw_trace_signatures before tw_set_row_groups (dropped with the row maps)");
    if (q->mode != 0 && q->mode != 1) return fail(e, TW_ERR_ARG, "tw_trace_signatures: mode outside {0 levels, 1 edges}");
    if ((int64_t)e->A.n_groups > ((int64_t)1 << kSigGroupBits)) return fail(e, TW_ERR_UNSUPPORTED, "tw_trace_signatures: more than 2^20 groups (the packed key holds 20 bits of group)");
    if (q->compare != 0 && !e->ref_set)
        return fail(e, TW_ERR_STATE, "tw_trace_signatures: compare without a reference set (keep_reference first; new row maps and new row groups drop the set)");
    if (q->compare != 0 && e->ref_mode != q->mode) return fail(e, TW_ERR_ARG, "tw_trace_signatures: the reference set was kept in the other mode");
    HIPCHK(hipSetDevice(e->device));
    const StitchDev& S = e->S;
    SigDev& D = e->G;
    const int64_t nt = e->st_trees, n_rows = S.n_rows;
    const bool same_query = e->sig_ready && e->sig_q.mode == q->mode && e->sig_q.need_flags == q->need_flags && e->sig_q.skip_flags == q->skip_flags &&
                            (e->sig_q.keep_reference != 0) == (q->keep_reference != 0) && (e->sig_q.compare != 0) == (q->compare != 0);
    if (!same_query) {
        drop_sig(e);
        if (D.counters == nullptr) DEV_ALLOC(D.counters, kSigCounters);   // (all of them freed with the batch)
        if (D.key_a == nullptr || n_rows > e->sig_rows_cap) {
            DEV_ALLOC(D.row_level, n_rows); DEV_ALLOC(D.key_a, n_rows); DEV_ALLOC(D.key_b, n_rows); DEV_ALLOC(D.ent_cnt, n_rows);
            DEV_ALLOC(D.big_begin, n_rows / kSigCap + 1); DEV_ALLOC(D.big_end, n_rows / kSigCap + 1);
            e->sig_rows_cap = n_rows;
        }
        if (D.hkey_a == nullptr || nt > e->sig_trees_cap) {
            DEV_ALLOC(D.hkey_a, nt); DEV_ALLOC(D.hkey_b, nt); DEV_ALLOC(D.val_a, nt); DEV_ALLOC(D.val_b, nt); DEV_ALLOC(D.tree_ent, nt); DEV_ALLOC(D.rep, nt);
            DEV_ALLOC(D.tree_class, nt); DEV_ALLOC(D.tree_items, nt); DEV_ALLOC(D.elig, nt); DEV_ALLOC(D.tree_same, nt); DEV_ALLOC(D.chunk_sum, nt / kSigScanItems + 2);
            DEV_ALLOC(D.class_rep, nt); DEV_ALLOC(D.class_trees, nt); DEV_ALLOC(D.class_sum, nt); DEV_ALLOC(D.class_min, nt); DEV_ALLOC(D.class_max, nt);
            DEV_ALLOC(D.class_off, nt + 1);
            e->sig_trees_cap = nt;
        }
        if (q->keep_reference != 0 && (D.ref_key == nullptr || n_rows > e->sig_ref_cap)) {
            DEV_ALLOC(D.ref_key, n_rows); DEV_ALLOC(D.ref_cnt, n_rows); DEV_ALLOC(D.ref_n, n_rows); DEV_ALLOC(D.ref_pos, n_rows);
            e->sig_ref_cap = n_rows;
            drop_ref(e);   // (new arrays: the set in the old ones is out of reach)
        }
        D.mode = q->mode; D.hash_bits = e->K.sig_hash_bits; D.need_flags = q->need_flags; D.skip_flags = q->skip_flags;
        D.row_group = e->A.row_group;
        const unsigned threads = flat_threads(e);
        const dim3 tb(threads), trees(flat_grid(nt, threads)), rows(flat_grid(n_rows, threads));
        unsigned long long counters[kSigCounters] = {0, 0, 0, 0, 0, 0, 0, 0};
        HIPCHK(hipMemsetAsync(D.counters, 0, sizeof(counters), e->stream));
        HIPCHK(hipEventRecord(e->stage_ev[SE_SIG + 0], e->stream));
        hipLaunchKernelGGL(k_sig_items, rows, tb, 0, e->stream, S, D);
        hipLaunchKernelGGL(k_sig_trees, trees, tb, 0, e->stream, S, D, nt);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(e->stage_ev[SE_SIG + 1], e->stream));
        HIPCHK(hipMemcpyAsync(counters, D.counters, sizeof(counters), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        if (counters[3] != 0) return fail(e, TW_ERR_UNSUPPORTED, "tw_trace_signatures: a server row lies 2^16 or more levels deep (the packed key holds 16 bits of level)");
        const int64_t n_big = (int64_t)counters[2];
        if (n_big > 0) {   // the trees beyond a wavefront's LDS table: sorted before k_sig_sign reads them
            TWCHK(rocprim_call(e, [&](void* tmp, size_t& bytes) {
                return rocprim::segmented_radix_sort_keys(tmp, bytes, (const unsigned long long*)D.key_a, D.key_b, (unsigned)n_rows, (unsigned)n_big, D.big_begin,
                                                          D.big_end, 0u, 64u, e->stream);
            }));
        }
        const WaveShape per_tree = wave_shape(e, nt, kSigTrees, kSigWaves);
        hipLaunchKernelGGL(k_sig_sign, per_tree.grid, per_tree.block, 0, e->stream, S, D, nt);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(e->stage_ev[SE_SIG + 2], e->stream));
        TWCHK(rocprim_call(e, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_pairs(tmp, bytes, D.hkey_a, D.hkey_b, D.val_a, D.val_b, (size_t)nt, 0u, 64u, e->stream); }));
        hipLaunchKernelGGL(k_sig_rep, trees, tb, 0, e->stream, S, D, nt);
        const int64_t n_chunks = (nt + (int64_t)threads * kSigScanItems - 1) / ((int64_t)threads * kSigScanItems);
        hipLaunchKernelGGL(k_sig_scan_sums<SigScan>, dim3((unsigned)n_chunks), tb, 0, e->stream, SigScan{D}, nt);
        hipLaunchKernelGGL(k_sig_scan_chunks<SigScan>, dim3(1), tb, 0, e->stream, SigScan{D}, n_chunks);
        hipLaunchKernelGGL(k_sig_scan_write<SigScan>, dim3((unsigned)n_chunks), tb, 0, e->stream, SigScan{D}, nt);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(counters, D.counters, sizeof(counters), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        const int64_t n_classes = (int64_t)(counters[6] >> 32), n_entries = (int64_t)(counters[6] & 0xffffffffull);
        if (D.class_entries == nullptr || n_entries > e->sig_ent_cap) {
            DEV_ALLOC(D.class_entries, 4 * n_entries);
            e->sig_ent_cap = std::max<int64_t>(n_entries, 1);
        }
        hipLaunchKernelGGL(k_sig_classes, trees, tb, 0, e->stream, S, D, nt);
        if (q->compare != 0) hipLaunchKernelGGL(k_sig_compare, trees, tb, 0, e->stream, S, D, nt);
        else HIPCHK(hipMemsetAsync(D.tree_same, 0xff, (size_t)nt, e->stream));
        if (q->keep_reference != 0) {   // (after the comparison: a call with both compares with the set it replaces)
            drop_ref(e);
            HIPCHK(hipMemsetAsync(D.ref_n, 0xff, sizeof(int32_t) * (size_t)n_rows, e->stream));
            HIPCHK(hipMemcpyAsync(D.ref_key, D.key_a, sizeof(unsigned long long) * (size_t)n_rows, hipMemcpyDeviceToDevice, e->stream));
            HIPCHK(hipMemcpyAsync(D.ref_cnt, D.ent_cnt, sizeof(int32_t) * (size_t)n_rows, hipMemcpyDeviceToDevice, e->stream));
            hipLaunchKernelGGL(k_sig_keep, trees, tb, 0, e->stream, S, D, nt);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(e->stage_ev[SE_SIG + 3], e->stream));
        HIPCHK(hipMemcpyAsync(counters, D.counters, sizeof(counters), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        for (int i = 0; i < 3; i++) TWCHK(stage_elapsed(e, SE_SIG, i, i + 1, &e->sg_ms[i]));
        e->sig_summary[0] = (int64_t)counters[0]; e->sig_summary[1] = n_classes; e->sig_summary[2] = (int64_t)counters[1]; e->sig_summary[3] = n_entries;
        e->sig_summary[4] = q->compare != 0 ? (int64_t)counters[4] : -1; e->sig_summary[5] = q->compare != 0 ? (int64_t)counters[5] : -1;
        if (q->keep_reference != 0) { e->ref_set = true; e->ref_mode = q->mode; }
        e->sig_q = *q;
        e->sig_ready = true;
    }
    if (summary != nullptr)
        for (int k = 0; k < 6; k++) summary[k] = e->sig_summary[k];
    if (out != nullptr) {
        const size_t nc = (size_t)e->sig_summary[1], ne = (size_t)e->sig_summary[3];
        TWCHK(copy_out(e, out->row_level, D.row_level, n_rows));
        TWCHK(copy_out(e, out->tree_class, D.tree_class, nt));
        TWCHK(copy_out(e, out->tree_items, D.tree_items, nt));
        TWCHK(copy_out(e, out->tree_same, D.tree_same, nt));
        TWCHK(copy_out(e, out->class_rep, D.class_rep, nc));
        TWCHK(copy_out(e, out->class_trees, D.class_trees, nc));
        TWCHK(copy_out(e, out->class_latency_sum, D.class_sum, nc));
        TWCHK(copy_out(e, out->class_latency_min, D.class_min, nc));
        TWCHK(copy_out(e, out->class_latency_max, D.class_max, nc));
        TWCHK(copy_out(e, out->class_off, D.class_off, nc + 1));
        if (ne > 0) TWCHK(copy_out(e, out->class_entries, D.class_entries, 4 * ne));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return TW_OK;
}

/* ---- per-class latency profiles (tw_prof.h) ----------------------------------------------------------------------------- */
int tw_class_profiles(tw_engine* e, const tw_class_profile* out, int64_t* summary) {
    if (e == nullptr) return TW_ERR_ARG;
    if (!e->sig_ready)
        return fail(e, TW_ERR_STATE, "tw_class_profiles needs the result of a tw_trace_signatures call (tw_score_traces, new row groups and whatever drops the "
                                     "forest drop it)");
    if (!e->attributed)
        return fail(e, TW_ERR_STATE, "tw_class_profiles needs a tw_attribute_traces call on the current forest (a new tw_stitch_traces, new row groups and "
                                     "whatever drops the forest drop the attribution)");
    HIPCHK(hipSetDevice(e->device));
    const StitchDev& S = e->S;
    ProfDev& P = e->F;
    const int64_t nt = e->st_trees, n_rows = S.n_rows, nc = e->sig_summary[1], ne = e->sig_summary[3];
    const bool built = !e->prof_ready;
    if (built) {
        if (P.counters == nullptr) DEV_ALLOC(P.counters, kProfCounters);   // (all of them freed with the batch)
        if (P.cells == nullptr || ne > e->prof_ent_cap) { DEV_ALLOC(P.cells, (int64_t)kProfCols * ne); e->prof_ent_cap = std::max<int64_t>(ne, 1); }
        if (P.seen == nullptr || n_rows > e->prof_rows_cap) { DEV_ALLOC(P.seen, n_rows); e->prof_rows_cap = n_rows; }
        if (P.class_counted == nullptr || nc > e->prof_cls_cap) {
            DEV_ALLOC(P.class_counted, nc); DEV_ALLOC(P.class_latency, nc); DEV_ALLOC(P.class_path_time, nc); DEV_ALLOC(P.class_top, nc);
            e->prof_cls_cap = std::max<int64_t>(nc, 1);
        }
        P.n_entries = ne; P.n_classes = nc;
        const unsigned threads = flat_threads(e);
        const dim3 tb(threads);
        // workgroups stride over the rows: at most 2048 of them clear and add up an LDS table
        const dim3 sweep(std::min(flat_grid(n_rows, threads), 2048u));
        HIPCHK(hipMemsetAsync(P.counters, 0, sizeof(unsigned long long) * kProfCounters, e->stream));
        HIPCHK(hipEventRecord(e->stage_ev[SE_PROF + 0], e->stream));
        hipLaunchKernelGGL(k_prof_clear, dim3(flat_grid(std::max<int64_t>({(int64_t)kProfCols * ne, n_rows, nc, 1}), threads)), tb, 0, e->stream, S, P);
        if (n_rows > 0) hipLaunchKernelGGL(k_prof_rows, sweep, tb, 0, e->stream, S, e->A, e->G, P);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(e->stage_ev[SE_PROF + 1], e->stream));
        if (nt > 0) hipLaunchKernelGGL(k_prof_trees, dim3(std::min(flat_grid(nt, threads), 2048u)), tb, 0, e->stream, S, e->A, e->G, P, nt);
        if (nc > 0) hipLaunchKernelGGL(k_prof_classes, dim3(flat_grid(nc, threads)), tb, 0, e->stream, e->G, P);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(e->stage_ev[SE_PROF + 2], e->stream));
        unsigned long long counters[kProfCounters];
        HIPCHK(hipMemcpyAsync(counters, P.counters, sizeof(counters), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        for (int k = 0; k < 6; k++) e->prof_summary[k] = (int64_t)counters[k];
    }
    if (summary != nullptr)
        for (int k = 0; k < 6; k++) summary[k] = e->prof_summary[k];
    if (out != nullptr) {
        int64_t* cols[kProfCols] = {out->rows, out->span_time, out->span_min, out->span_max, out->self_time, out->path_time, out->path_rows, out->path_trees,
                                    out->offset};
        for (int c = 0; c < kProfCols; c++)
            if (ne > 0) TWCHK(copy_out(e, cols[c], P.cells + (int64_t)c * ne, (size_t)ne));
        if (nc > 0) {
            TWCHK(copy_out(e, out->class_counted, P.class_counted, (size_t)nc));
            TWCHK(copy_out(e, out->class_latency, P.class_latency, (size_t)nc));
            TWCHK(copy_out(e, out->class_path_time, P.class_path_time, (size_t)nc));
            TWCHK(copy_out(e, out->class_top_entry, P.class_top, (size_t)nc));
        }
    }
    if (built) {
        HIPCHK(hipEventRecord(e->stage_ev[SE_PROF + 3], e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        for (int i = 0; i < 3; i++) TWCHK(stage_elapsed(e, SE_PROF, i, i + 1, &e->pf_ms[i]));
        e->prof_ready = true;
    } else if (out != nullptr) {
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return TW_OK;
}

/* ---- traces selected by a predicate: a flag bit every stage reads (tw_filt.h) --------------------------------------------- */
int tw_filter_traces(tw_engine* e, const tw_filter_query* q, const tw_filter_result* out, int64_t* summary) {
    if (e == nullptr || q == nullptr) return TW_ERR_ARG;
    TWCHK(need_forest(e, "tw_filter_traces"));
    if (!e->groups_set) return fail(e, TW_ERR_STATE, "tw_filter_traces before tw_set_row_groups (dropped with the row maps)");
    const int nc = q->n_clauses;
    if (nc < 0 || nc > TW_FILT_MAX_CLAUSES || (nc > 0 && q->clauses == nullptr)) return fail(e, TW_ERR_ARG, "tw_filter_traces: n_clauses outside [0, 16]");
    const int32_t G = e->A.n_groups;
    FiltQueryDev Q{};
    Q.need_flags = q->need_flags; Q.skip_flags = q->skip_flags; Q.n_clauses = nc;
    bool times = false, classes = false;
    for (int j = 0; j < nc; j++) {
        const tw_filter_clause& c = q->clauses[j];
        const std::string at = "tw_filter_traces: clause " + std::to_string(j) + ": ";
        if (c.term < 0 || c.term >= TW_FILT_MAX_TERMS) return fail(e, TW_ERR_ARG, at + "term outside [0, 8)");
        if (c.subject < FILT_LATENCY || c.subject > FILT_EDGE) return fail(e, TW_ERR_ARG, at + "subject outside [0, 5]");
        if (c.lo > c.hi) return fail(e, TW_ERR_ARG, at + "lo > hi");
        FiltClauseDev& d = Q.c[j];
        d.subject = c.subject; d.term = c.term; d.negate = c.negate != 0 ? 1 : 0; d.lo = c.lo; d.hi = c.hi;
        Q.term_used |= 1u << c.term;
        if (c.subject == FILT_CLASS) classes = true;
        if (c.subject != FILT_GROUP && c.subject != FILT_EDGE) continue;   // (group, caller, metric and reduce are read for these two only)
        const bool edge = c.subject == FILT_EDGE;
        if (c.metric < 0 || c.metric > (edge ? 1 : 4)) return fail(e, TW_ERR_ARG, at + (edge ? "metric outside [0, 1] of an EDGE clause" : "metric outside [0, 4]"));
        if (c.reduce < 0 || c.reduce > 2) return fail(e, TW_ERR_ARG, at + "reduce outside {0 sum, 1 min, 2 max}");
        if ((c.metric == 0 || c.metric == 4) && c.reduce != 0) return fail(e, TW_ERR_ARG, at + "a count (metric 0, 4) is summed: reduce must be 0");
        if (c.group < (edge ? 0 : -1) || c.group >= G) return fail(e, TW_ERR_ARG, at + (edge ? "group outside [0, n_groups)" : "group outside [-1, n_groups)"));
        if (edge && (c.caller < -1 || c.caller >= G)) return fail(e, TW_ERR_ARG, at + "caller outside [-1, n_groups)");
        d.group = c.group; d.caller = edge ? c.caller : 0; d.metric = c.metric; d.reduce = c.reduce;
        Q.row_mask |= 1u << j;
        if (edge) Q.cols |= FILT_COL_CALLER;
        Q.cols |= c.metric == 1 ? FILT_COL_SPAN : c.metric == 2 ? FILT_COL_SELF : c.metric == 3 ? FILT_COL_PATH : c.metric == 4 ? FILT_COL_FLAG : 0;
        if (c.metric >= 2) times = true;
    }
    if (times && !e->attributed)
        return fail(e, TW_ERR_STATE, "tw_filter_traces: a clause on self_time, path_time or the rows on the path needs a tw_attribute_traces call on the current forest");
    if (classes && !e->sig_ready)
        return fail(e, TW_ERR_STATE, "tw_filter_traces: a CLASS clause needs the result of a tw_trace_signatures call (tw_score_traces, new row groups and whatever "
                                     "drops the forest drop it)");
    HIPCHK(hipSetDevice(e->device));
    const StitchDev& S = e->S;
    FiltDev& F = e->FL;
    const int64_t nt = e->st_trees;
    if (F.counters == nullptr) DEV_ALLOC(F.counters, kFiltCounters);   // (all of them freed with the batch)
    if (F.tree_match == nullptr || nt > e->filt_trees_cap) {
        DEV_ALLOC(F.tree_match, nt); DEV_ALLOC(F.match_trees, nt); DEV_ALLOC(F.chunk_sum, nt / kSigScanItems + 2);
        e->filt_trees_cap = std::max<int64_t>(nt, 1);
    }
    if (F.clause_value == nullptr || nt * nc > e->filt_val_cap) {
        DEV_ALLOC(F.clause_value, nt * nc);
        e->filt_val_cap = std::max<int64_t>(nt * nc, 1);
    }
    F.row_group = e->A.row_group; F.self_time = e->A.self_time; F.path_time = e->A.path_time; F.row_flag = e->A.row_flag;
    F.tree_class = e->G.tree_class;
    unsigned long long counters[kFiltCounters] = {};
    counters[kFiltMinAt] = ~0ull;   // (the least key; the greatest starts at 0)
    HIPCHK(hipMemcpyAsync(F.counters, counters, sizeof(counters), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipEventRecord(e->stage_ev[SE_FILT + 0], e->stream));
    const WaveShape per_tree = wave_shape(e, nt, kFiltTrees, kFiltWaves);
    if (nt > 0) hipLaunchKernelGGL(k_filt_trees, per_tree.grid, per_tree.block, 0, e->stream, S, F, Q, nt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->stage_ev[SE_FILT + 1], e->stream));
    const unsigned threads = flat_threads(e);
    const dim3 tb(threads);
    const int64_t n_chunks = (nt + (int64_t)threads * kSigScanItems - 1) / ((int64_t)threads * kSigScanItems);
    if (nt > 0) {   // count, scan, list
        hipLaunchKernelGGL(k_sig_scan_sums<FiltScan>, dim3((unsigned)n_chunks), tb, 0, e->stream, FiltScan{F}, nt);
        hipLaunchKernelGGL(k_sig_scan_chunks<FiltScan>, dim3(1), tb, 0, e->stream, FiltScan{F}, n_chunks);
        hipLaunchKernelGGL(k_sig_scan_write<FiltScan>, dim3((unsigned)n_chunks), tb, 0, e->stream, FiltScan{F}, nt);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->stage_ev[SE_FILT + 2], e->stream));
    HIPCHK(hipMemcpyAsync(counters, F.counters, sizeof(counters), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    // the bit is rewritten: what was selected by it goes (read first, dropped afterwards)
    if (e->attributed && ((e->attr_need | e->attr_skip) & TW_TREE_MATCH) != 0) drop_attribution(e);
    if (e->sig_ready && ((e->sig_q.need_flags | e->sig_q.skip_flags) & TW_TREE_MATCH) != 0) drop_sig(e);
    const int64_t matched = (int64_t)counters[1];
    if (summary != nullptr) {
        summary[0] = (int64_t)counters[0]; summary[1] = matched; summary[2] = (int64_t)counters[2];
        summary[3] = matched > 0 ? (int64_t)(counters[kFiltMinAt] ^ (1ull << 63)) : INT64_MAX;
        summary[4] = matched > 0 ? (int64_t)(counters[kFiltMaxAt] ^ (1ull << 63)) : INT64_MIN;
        summary[5] = (int64_t)counters[5];
    }
    if (out != nullptr) {
        TWCHK(copy_out(e, out->tree_match, F.tree_match, (size_t)nt));
        TWCHK(copy_out(e, out->match_trees, F.match_trees, (size_t)matched));
        TWCHK(copy_out(e, out->clause_value, F.clause_value, (size_t)(nt * nc)));
        if (out->clause_trees != nullptr)
            for (int j = 0; j < nc; j++) out->clause_trees[j] = (int64_t)counters[kFiltClauseAt + j];
        if (out->term_trees != nullptr)
            for (int k = 0; k < TW_FILT_MAX_TERMS; k++) out->term_trees[k] = (int64_t)counters[kFiltTermAt + k];
    }
    HIPCHK(hipEventRecord(e->stage_ev[SE_FILT + 3], e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int i = 0; i < 3; i++) TWCHK(stage_elapsed(e, SE_FILT, i, i + 1, &e->fl_ms[i]));
    return TW_OK;
}

/* ---- reconstructed traces handed out as trees: exemplars, pre-order rows (tw_extr.h) ---------------------------------------- */
int tw_extract_traces(tw_engine* e, const tw_extract_query* q, int64_t* summary) {
    if (e == nullptr || q == nullptr) return TW_ERR_ARG;
    TWCHK(need_forest(e, "tw_extract_traces"));
    const int64_t nt = e->st_trees;
    if (q->mode < 0 || q->mode > 2) return fail(e, TW_ERR_ARG, "tw_extract_traces: mode outside {0 TOP, 1 QUANTILES, 2 LIST}");
    ExtrPick pick{};
    if (q->mode == 0) {
        if (q->order < 0 || q->order > 2) return fail(e, TW_ERR_ARG, "tw_extract_traces: order outside {0 by tree, 1 slowest first, 2 fastest first}");
        if (q->limit < 0) return fail(e, TW_ERR_ARG, "tw_extract_traces: limit is negative (0 takes every eligible tree)");
    } else if (q->mode == 1) {
        if (q->n_probs < 0 || q->n_probs > TW_EXTR_MAX_PROBS || (q->n_probs > 0 && q->probs == nullptr))
            return fail(e, TW_ERR_ARG, "tw_extract_traces: n_probs outside [0, 32]");
        for (int j = 0; j < q->n_probs; j++)
            if (!(q->probs[j] >= 0.0 && q->probs[j] <= 1.0)) return fail(e, TW_ERR_ARG, "tw_extract_traces: a prob outside [0, 1]");
    } else {
        if (q->n_list < 0 || q->n_list > TW_EXTR_MAX_LIST || (q->n_list > 0 && q->list == nullptr))
            return fail(e, TW_ERR_ARG, "tw_extract_traces: n_list outside [0, 2^20]");
        for (int j = 0; j < q->n_list; j++)
            if (q->list[j] < 0 || (int64_t)q->list[j] >= nt) return fail(e, TW_ERR_ARG, "tw_extract_traces: a listed tree outside [0, n_trees)");
    }
    HIPCHK(hipSetDevice(e->device));
    drop_extr(e);   // (the result's buffers are rewritten from here on)
    const StitchDev& S = e->S;
    ExtrDev& X = e->X;
    const bool by_latency = q->mode == 1 || (q->mode == 0 && q->order != 0);
    const int64_t sel_cap = std::max<int64_t>(std::max<int64_t>(nt, q->mode == 2 ? q->n_list : 0), TW_EXTR_MAX_PROBS);
    if (X.counters == nullptr) DEV_ALLOC(X.counters, kExtrCounters);   // (all of them freed with the batch)
    if (X.sel_tree == nullptr || sel_cap > e->extr_sel_cap) {
        DEV_ALLOC(X.sel_tree, sel_cap); DEV_ALLOC(X.sel_root, sel_cap); DEV_ALLOC(X.sel_latency, sel_cap); DEV_ALLOC(X.sel_start, sel_cap);
        DEV_ALLOC(X.sel_flags, sel_cap); DEV_ALLOC(X.out_off, sel_cap + 1); DEV_ALLOC(X.chunk_sum, sel_cap / kSigScanItems + 2);
        e->extr_sel_cap = sel_cap;
    }
    if (by_latency && (X.key_a == nullptr || nt > e->extr_sort_cap)) {
        DEV_ALLOC(X.key_a, nt); DEV_ALLOC(X.key_b, nt); DEV_ALLOC(X.val_a, nt); DEV_ALLOC(X.val_b, nt);
        e->extr_sort_cap = std::max<int64_t>(nt, 1);
    }
    X.row_group = e->groups_set ? e->A.row_group : nullptr;
    const bool times = e->attributed;
    X.self_time = times ? e->A.self_time : nullptr;
    X.path_time = times ? e->A.path_time : nullptr;
    const unsigned threads = flat_threads(e);
    const dim3 tb(threads);
    auto scan_chunks = [&](int64_t n) { return (n + (int64_t)threads * kSigScanItems - 1) / ((int64_t)threads * kSigScanItems); };
    unsigned long long counters[kExtrCounters] = {};
    HIPCHK(hipMemsetAsync(X.counters, 0, sizeof(counters), e->stream));
    HIPCHK(hipEventRecord(e->stage_ev[SE_EXTR + 0], e->stream));
    // 1. the selected trees into sel_tree
    int64_t n_elig = nt, n_sel = 0;
    if (q->mode == 2) {
        n_sel = q->n_list;
        if (n_sel > 0) HIPCHK(hipMemcpyAsync(X.sel_tree, q->list, sizeof(int32_t) * (size_t)n_sel, hipMemcpyHostToDevice, e->stream));
    } else if (!by_latency) {
        const ExtrSelScan V{S, X, q->need_flags, q->skip_flags, q->limit > 0 ? q->limit : nt};
        const int64_t n_chunks = scan_chunks(nt);
        if (nt > 0) {
            hipLaunchKernelGGL(k_sig_scan_sums<ExtrSelScan>, dim3((unsigned)n_chunks), tb, 0, e->stream, V, nt);
            hipLaunchKernelGGL(k_sig_scan_chunks<ExtrSelScan>, dim3(1), tb, 0, e->stream, V, n_chunks);
            hipLaunchKernelGGL(k_sig_scan_write<ExtrSelScan>, dim3((unsigned)n_chunks), tb, 0, e->stream, V, nt);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(counters, X.counters, sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        n_elig = (int64_t)counters[0];
        n_sel = q->limit > 0 ? std::min<int64_t>(q->limit, n_elig) : n_elig;
    } else {
        AttrDev V{};   // the view k_attr_flags writes through: keys, values and its counters
        V.key_a = X.key_a; V.key_b = X.key_b; V.val_a = X.val_a; V.val_b = X.val_b; V.counters = X.counters + kExtrAttrAt;
        const AttrQueryDev Q{0, 0, 0, q->need_flags, q->skip_flags};
        if (nt > 0) TWCHK(trees_by_latency(e, V, Q, nt));
        HIPCHK(hipMemcpyAsync(counters, V.counters, sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        n_elig = (int64_t)counters[0];
        if (q->mode == 1) {
            n_sel = n_elig > 0 ? q->n_probs : 0;
            pick.n = (int32_t)n_sel;
            for (int j = 0; j < pick.n; j++) pick.at[j] = std::min<int64_t>(n_elig - 1, (int64_t)(q->probs[j] * (double)n_elig));
            if (n_sel > 0) hipLaunchKernelGGL(k_extr_pick, dim3(1), tb, 0, e->stream, X, pick);
        } else {
            n_sel = q->limit > 0 ? std::min<int64_t>(q->limit, n_elig) : n_elig;
            if (n_sel > 0 && q->order == 2) HIPCHK(hipMemcpyAsync(X.sel_tree, X.val_b, sizeof(int32_t) * (size_t)n_sel, hipMemcpyDeviceToDevice, e->stream));
            if (n_sel > 0 && q->order == 1) hipLaunchKernelGGL(k_extr_slowest, dim3(flat_grid(n_sel, threads)), tb, 0, e->stream, X, n_elig, n_sel);
        }
        HIPCHK(hipGetLastError());
    }
    // 2. the per-tree columns, the sizes, out_off
    if (n_sel > 0) {
        const int64_t n_chunks = scan_chunks(n_sel);
        const ExtrOffScan V{S, X};
        hipLaunchKernelGGL(k_extr_sizes, dim3(flat_grid(n_sel, threads)), tb, 0, e->stream, S, X, n_sel);
        hipLaunchKernelGGL(k_sig_scan_sums<ExtrOffScan>, dim3((unsigned)n_chunks), tb, 0, e->stream, V, n_sel);
        hipLaunchKernelGGL(k_sig_scan_chunks<ExtrOffScan>, dim3(1), tb, 0, e->stream, V, n_chunks);
        hipLaunchKernelGGL(k_sig_scan_write<ExtrOffScan>, dim3((unsigned)n_chunks), tb, 0, e->stream, V, n_sel);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(counters, X.counters, sizeof(unsigned long long) * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int64_t n_out = n_sel > 0 ? (int64_t)counters[1] : 0, big_rows = (int64_t)counters[4];
    HIPCHK(hipMemcpyAsync(X.out_off + n_sel, &n_out, sizeof(int64_t), hipMemcpyHostToDevice, e->stream));   // the end of the last tree
    HIPCHK(hipEventRecord(e->stage_ev[SE_EXTR + 1], e->stream));
    // 3. the trees
    if (X.row == nullptr || n_out > e->extr_rows_cap) {
        DEV_ALLOC(X.row, n_out); DEV_ALLOC(X.parent, n_out); DEV_ALLOC(X.depth, n_out); DEV_ALLOC(X.subtree, n_out); DEV_ALLOC(X.group, n_out);
        DEV_ALLOC(X.kind, n_out); DEV_ALLOC(X.start, n_out); DEV_ALLOC(X.end, n_out); DEV_ALLOC(X.self, n_out); DEV_ALLOC(X.path, n_out);
        e->extr_rows_cap = std::max<int64_t>(n_out, 1);
    }
    if (big_rows > X.big_cap) {   // tables of the trees that outgrow a wavefront's LDS
        DEV_ALLOC(X.g_row, big_rows); DEV_ALLOC(X.g_lnk, big_rows); DEV_ALLOC(X.g_par, big_rows); DEV_ALLOC(X.g_dep, big_rows);
        DEV_ALLOC(X.g_sub, big_rows); DEV_ALLOC(X.g_pre, big_rows);
        X.big_cap = big_rows;
    }
    if (big_rows > 0 && (X.pos == nullptr || S.n_rows > e->extr_pos_cap)) {
        DEV_ALLOC(X.pos, S.n_rows);
        e->extr_pos_cap = S.n_rows;
    }
    if (n_sel > 0) {
        const WaveShape per_tree = wave_shape(e, n_sel, kExtrTrees, kExtrWaves);
        hipLaunchKernelGGL(k_extr_trees, per_tree.grid, per_tree.block, 0, e->stream, S, X, n_sel);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(e->stage_ev[SE_EXTR + 2], e->stream));
    unsigned long long err = 0;
    HIPCHK(hipMemcpyAsync(&err, X.counters + 6, sizeof(err), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (err == 2) return fail(e, TW_ERR_DEVICE, "tw_extract_traces: the tables of the large trees are smaller than the trees");
    if (err != 0) return fail(e, TW_ERR_ARG, "tw_extract_traces: a row is linked to a row outside its tree: not the forest tw_stitch_traces left behind");
    for (int i = 0; i < 2; i++) TWCHK(stage_elapsed(e, SE_EXTR, i, i + 1, &e->ex_ms[i]));
    if (summary != nullptr) {
        summary[0] = n_elig; summary[1] = n_sel; summary[2] = n_out; summary[3] = n_sel > 0 ? (int64_t)counters[2] : 0;
        summary[4] = (int64_t)counters[3]; summary[5] = times ? 1 : 0;
    }
    e->extr_sel = n_sel; e->extr_rows = n_out; e->extr_times = times;
    e->extr_ready = true;
    return TW_OK;
}

int tw_get_extracted(tw_engine* e, const tw_extracted* out) {
    if (e == nullptr || out == nullptr) return TW_ERR_ARG;
    if (!e->extr_ready) return fail(e, TW_ERR_STATE, "tw_get_extracted needs the result of a tw_extract_traces call (whatever drops the forest drops it)");
    if (!e->extr_times && (out->self_time != nullptr || out->path_time != nullptr))
        return fail(e, TW_ERR_STATE, "tw_get_extracted: the result holds no self / path times (no attribution was resident when it was made)");
    HIPCHK(hipSetDevice(e->device));
    const ExtrDev& X = e->X;
    const size_t ns = (size_t)e->extr_sel, nr = (size_t)e->extr_rows;
    HIPCHK(hipEventRecord(e->stage_ev[SE_EXTR + 3], e->stream));
    TWCHK(copy_out(e, out->sel_tree, X.sel_tree, ns));
    TWCHK(copy_out(e, out->sel_root, X.sel_root, ns));
    TWCHK(copy_out(e, out->sel_latency, X.sel_latency, ns));
    TWCHK(copy_out(e, out->sel_start, X.sel_start, ns));
    TWCHK(copy_out(e, out->sel_flags, X.sel_flags, ns));
    TWCHK(copy_out(e, out->out_off, X.out_off, ns + 1));
    TWCHK(copy_out(e, out->row, X.row, nr));
    TWCHK(copy_out(e, out->parent, X.parent, nr));
    TWCHK(copy_out(e, out->depth, X.depth, nr));
    TWCHK(copy_out(e, out->subtree, X.subtree, nr));
    TWCHK(copy_out(e, out->kind, X.kind, nr));
    TWCHK(copy_out(e, out->group, X.group, nr));
    TWCHK(copy_out(e, out->start, X.start, nr));
    TWCHK(copy_out(e, out->end, X.end, nr));
    TWCHK(copy_out(e, out->self_time, X.self, nr));
    TWCHK(copy_out(e, out->path_time, X.path, nr));
    HIPCHK(hipEventRecord(e->stage_ev[SE_EXTR + 4], e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return stage_elapsed(e, SE_EXTR, 3, 4, &e->ex_ms[2]);
}

/* ---- the classes of batch after batch: a catalogue on the device (tw_chist.h) -------------------------------------------- */
namespace {

// Buffers of the catalogue's own (not a load's).  A group of arrays grows together: every new array first, then the copies, then the
// old ones are freed, so that a failure leaves the catalogue intact.
struct ChistNew {
    std::vector<void*> got;
    ~ChistNew() { for (void* q : got) (void)hipFree(q); }   // (whatever was not adopted)
};
void* chist_new(tw_engine* e, ChistNew& N, int64_t bytes) {
    void* q = nullptr;
    if (hipMalloc(&q, (size_t)std::max<int64_t>(bytes, 1)) != hipSuccess) {
        (void)hipGetLastError();
        fail(e, TW_ERR_DEVICE, "tw_class_history: no device memory for " + std::to_string(bytes) + " bytes (the catalogue is as it was)");
        return nullptr;
    }
    N.got.push_back(q);
    return q;
}
#define CHIST_NEW(ptr, type, count)                                                    \
    do {                                                                               \
        (ptr) = (type*)chist_new(e, N, (int64_t)sizeof(type) * (int64_t)(count));      \
        if ((ptr) == nullptr) return TW_ERR_DEVICE;                                    \
    } while (0)

// Room for `classes` classes and `entries` entries: the store's arrays at least double.
int chist_reserve(tw_engine* e, int64_t classes, int64_t entries) {
    ChistDev& H = e->CH;
    if (H.off == nullptr || classes > H.cls_cap) {
        const int64_t cap = std::max<int64_t>(std::max<int64_t>(classes, 2 * H.cls_cap), kChistSlots / 2);
        ChistNew N;
        int64_t *off, *cls; unsigned long long *hash, *stamp;
        CHIST_NEW(off, int64_t, cap + 1); CHIST_NEW(hash, unsigned long long, cap); CHIST_NEW(stamp, unsigned long long, cap);
        CHIST_NEW(cls, int64_t, (int64_t)kChistClassCols * cap);
        HIPCHK(hipMemsetAsync(off, 0, sizeof(int64_t), e->stream));
        if (H.off != nullptr) {
            HIPCHK(hipMemcpyAsync(off, H.off, sizeof(int64_t) * (size_t)(H.C + 1), hipMemcpyDeviceToDevice, e->stream));
            HIPCHK(hipMemcpyAsync(hash, H.hash, sizeof(unsigned long long) * (size_t)H.C, hipMemcpyDeviceToDevice, e->stream));
            HIPCHK(hipMemcpyAsync(stamp, H.stamp, sizeof(unsigned long long) * (size_t)H.C, hipMemcpyDeviceToDevice, e->stream));
            for (int c = 0; c < kChistClassCols; c++)
                HIPCHK(hipMemcpyAsync(cls + (int64_t)c * cap, H.cls + (int64_t)c * H.cls_cap, sizeof(int64_t) * (size_t)H.C, hipMemcpyDeviceToDevice, e->stream));
        }
        HIPCHK(hipStreamSynchronize(e->stream));
        N.got = {H.off, H.hash, H.stamp, H.cls};   // the old ones go
        H.off = off; H.hash = hash; H.stamp = stamp; H.cls = cls; H.cls_cap = cap;
    }
    if (H.entries == nullptr || entries > H.ent_cap) {
        const int64_t cap = std::max<int64_t>(std::max<int64_t>(entries, 2 * H.ent_cap), kChistSlots);
        ChistNew N;
        int32_t* ent; int64_t* cell;
        CHIST_NEW(ent, int32_t, 4 * cap); CHIST_NEW(cell, int64_t, (int64_t)kProfCols * cap);
        if (H.entries != nullptr) {
            HIPCHK(hipMemcpyAsync(ent, H.entries, sizeof(int32_t) * 4 * (size_t)H.E, hipMemcpyDeviceToDevice, e->stream));
            for (int c = 0; c < kProfCols; c++)
                HIPCHK(hipMemcpyAsync(cell + (int64_t)c * cap, H.cell + (int64_t)c * H.ent_cap, sizeof(int64_t) * (size_t)H.E, hipMemcpyDeviceToDevice, e->stream));
        }
        HIPCHK(hipStreamSynchronize(e->stream));
        N.got = {H.entries, H.cell};
        H.entries = ent; H.cell = cell; H.ent_cap = cap;
    }
    return TW_OK;
}

// the table emptied and refilled from the classes held (a grown table; a refused merge that had claimed slots)
int chist_rehash(tw_engine* e) {
    ChistDev& H = e->CH;
    HIPCHK(hipMemsetAsync(H.table, 0, sizeof(unsigned long long) * (size_t)H.slots, e->stream));
    const unsigned threads = flat_threads(e);
    if (H.C > 0) hipLaunchKernelGGL(k_chist_insert, dim3(flat_grid(H.C, threads)), dim3(threads), 0, e->stream, H, (int64_t)0, H.C, 0);
    HIPCHK(hipGetLastError());
    return TW_OK;
}

// A table of at least two slots per class for `classes` classes: it at least doubles and is refilled from the classes held.
int chist_table(tw_engine* e, int64_t classes) {
    ChistDev& H = e->CH;
    int64_t want = kChistSlots;
    while (want < 2 * classes) want *= 2;
    if (H.table != nullptr && want <= H.slots) return TW_OK;
    want = std::max<int64_t>(want, 2 * H.slots);
    ChistNew N;
    unsigned long long* table;
    CHIST_NEW(table, unsigned long long, want);
    N.got = {H.table};
    H.table = table; H.slots = want;
    TWCHK(chist_rehash(e));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TW_OK;
}

int chist_scratch(tw_engine* e, int64_t classes) {
    ChistDev& H = e->CH;
    ChistNew N;
    if (H.counters == nullptr) {
        CHIST_NEW(H.counters, unsigned long long, kChistCounters);
        N.got.clear();
    }
    if (H.src_hash == nullptr || classes > e->ch_src_cap) {
        const int64_t cap = std::max<int64_t>(classes, 2 * e->ch_src_cap);
        unsigned long long *sh, *cs; int32_t *si, *ns;
        CHIST_NEW(sh, unsigned long long, cap); CHIST_NEW(si, int32_t, cap); CHIST_NEW(ns, int32_t, cap); CHIST_NEW(cs, unsigned long long, cap / kSigScanItems + 2);
        N.got = {H.src_hash, H.src_id, H.new_src, H.chunk_sum};
        H.src_hash = sh; H.src_id = si; H.new_src = ns; H.chunk_sum = cs; e->ch_src_cap = cap;
    }
    return TW_OK;
}

int chist_fits(tw_engine* e, const std::string& fn, int32_t mode, int32_t n_groups) {
    if (mode != 0 && mode != 1) return fail(e, TW_ERR_ARG, fn + ": mode outside {0 levels, 1 edges}");
    if (n_groups < 1) return fail(e, TW_ERR_ARG, fn + ": n_groups must be positive");
    if ((int64_t)n_groups > ((int64_t)1 << kSigGroupBits)) return fail(e, TW_ERR_UNSUPPORTED, fn + ": more than 2^20 groups");
    if (e->ch_G != 0 && (mode != e->ch_mode || n_groups != e->ch_G))
        return fail(e, TW_ERR_ARG, fn + ": the catalogue holds classes of mode " + std::to_string(e->ch_mode) + " over " + std::to_string(e->ch_G) + " groups, the source is of mode " +
                                       std::to_string(mode) + " over " + std::to_string(n_groups) + " (tw_class_history_reset opens it again)");
    return TW_OK;
}

// Hash, lookup and the scan's sums over the misses; new_classes / new_entries: what the catalogue does not hold.  Changes nothing
// that is returned (mark: the hits are marked with the call's serial number, and two source classes that hit one class are refused).
int chist_find(tw_engine* e, const std::string& fn, const ChistSrc& S, bool mark, int64_t& new_classes, int64_t& new_entries) {
    ChistDev& H = e->CH;
    const unsigned threads = flat_threads(e);
    const int64_t nc = S.n_classes;
    H.serial++;
    H.hash_bits = e->K.sig_hash_bits;
    HIPCHK(hipMemsetAsync(H.counters, 0, sizeof(unsigned long long) * kChistCounters, e->stream));
    unsigned long long counters[kChistCounters] = {0, 0, 0, 0};
    if (nc > 0) {
        const WaveShape per_class = wave_shape(e, nc, kChistPack, kChistWaves);
        hipLaunchKernelGGL(k_chist_lookup, per_class.grid, per_class.block, 0, e->stream, S, H, mark ? 1 : 0);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(e->stage_ev[SE_CHIST + 1], e->stream));
    if (nc > 0) {
        const int64_t n_chunks = (nc + (int64_t)threads * kSigScanItems - 1) / ((int64_t)threads * kSigScanItems);
        const ChistScan V{S, H};
        hipLaunchKernelGGL(k_sig_scan_sums<ChistScan>, dim3((unsigned)n_chunks), dim3(threads), 0, e->stream, V, nc);
        hipLaunchKernelGGL(k_sig_scan_chunks<ChistScan>, dim3(1), dim3(threads), 0, e->stream, V, n_chunks);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(counters, H.counters, sizeof(counters), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (counters[2] != 0) return fail(e, TW_ERR_ARG, fn + ": two classes of the source have equal signatures (the catalogue is as it was)");
    new_classes = (int64_t)(counters[0] >> 32);
    new_entries = (int64_t)(counters[0] & 0xffffffffull);
    return TW_OK;
}

void chist_summary(const tw_engine* e, int64_t new_classes, int64_t new_entries, int64_t held_classes, int64_t held_entries, int64_t src_classes, int64_t* summary) {
    if (summary == nullptr) return;
    summary[0] = new_classes; summary[1] = held_classes; summary[2] = new_entries; summary[3] = held_entries; summary[4] = e->ch_pushes; summary[5] = src_classes;
}

// A push or a merge of the source S (on the device).  Events SE_CHIST + 0 (recorded by the caller) .. + 3.
int chist_absorb(tw_engine* e, const std::string& fn, const ChistSrc& S, int what, bool merge, int32_t* class_map, int64_t* summary) {
    ChistDev& H = e->CH;
    const unsigned threads = flat_threads(e);
    const dim3 tb(threads);
    const int64_t nc = S.n_classes, ne = S.n_entries;
    int64_t new_classes = 0, new_entries = 0;
    TWCHK(chist_find(e, fn, S, true, new_classes, new_entries));
    if (H.C + new_classes > (int64_t)INT32_MAX || H.E + new_entries > (int64_t)INT32_MAX)
        return fail(e, TW_ERR_UNSUPPORTED, fn + ": more than 2^31 - 1 classes or entries in the catalogue (it is as it was)");
    TWCHK(chist_reserve(e, H.C + new_classes, H.E + new_entries));
    TWCHK(chist_table(e, H.C + new_classes));
    if (new_classes > 0) {
        const int64_t n_chunks = (nc + (int64_t)threads * kSigScanItems - 1) / ((int64_t)threads * kSigScanItems);
        const ChistScan V{S, H};
        hipLaunchKernelGGL(k_sig_scan_write<ChistScan>, dim3((unsigned)n_chunks), tb, 0, e->stream, V, nc);
        hipLaunchKernelGGL(k_chist_append, dim3(std::min(flat_grid(std::max(new_classes, new_entries), threads), 1u << 20)), tb, 0, e->stream, S, H, new_classes, new_entries);
        hipLaunchKernelGGL(k_chist_insert, dim3(flat_grid(new_classes, threads)), tb, 0, e->stream, H, H.C, H.C + new_classes, merge ? 1 : 0);
        HIPCHK(hipGetLastError());
        if (merge) {   // (the classes of a signature result differ by construction)
            unsigned long long counters[kChistCounters];
            HIPCHK(hipMemcpyAsync(counters, H.counters, sizeof(counters), hipMemcpyDeviceToHost, e->stream));
            HIPCHK(hipStreamSynchronize(e->stream));
            if (counters[2] != 0) {   // the new classes have claimed slots: the table again from the classes held
                TWCHK(chist_rehash(e));
                HIPCHK(hipStreamSynchronize(e->stream));
                return fail(e, TW_ERR_ARG, fn + ": two classes of the source have equal signatures (the catalogue is as it was)");
            }
        }
    }
    HIPCHK(hipEventRecord(e->stage_ev[SE_CHIST + 2], e->stream));
    const int64_t n_work = std::max<int64_t>(nc, (what & 2) != 0 ? ne : 0);
    if (n_work > 0) {
        hipLaunchKernelGGL(k_chist_accumulate, dim3(std::min(flat_grid(n_work, threads), 1u << 20)), tb, 0, e->stream, S, H, what);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(e->stage_ev[SE_CHIST + 3], e->stream));
    if (class_map != nullptr && nc > 0) HIPCHK(hipMemcpyAsync(class_map, H.src_id, sizeof(int32_t) * (size_t)nc, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int i = 0; i < 3; i++) TWCHK(stage_elapsed(e, SE_CHIST, i, i + 1, &e->ch_ms[i]));
    H.C += new_classes; H.E += new_entries;
    e->ch_mode = S.mode; e->ch_G = S.n_groups; e->ch_pushes++;
    chist_summary(e, new_classes, new_entries, H.C, H.E, nc, summary);
    return TW_OK;
}

// the resident signature result (and, with what & 2, the resident class profile) as a source
int chist_resident(tw_engine* e, const std::string& fn, int what, ChistSrc& S) {
    if (!e->sig_ready)
        return fail(e, TW_ERR_STATE, fn + " needs the result of a tw_trace_signatures call (tw_score_traces, new row groups and whatever drops the forest drop it)");
    if ((what & 2) != 0 && !e->prof_ready)
        return fail(e, TW_ERR_STATE, fn + ": what & 2 needs the result of a tw_class_profiles call on the resident signature result and attribution");
    S = ChistSrc{};
    S.n_classes = e->sig_summary[1]; S.n_entries = e->sig_summary[3];
    S.off = e->G.class_off; S.entries = e->G.class_entries;
    if ((what & 1) != 0) { S.cls[0] = e->G.class_trees; S.cls[1] = e->G.class_sum; S.cls[2] = e->G.class_min; S.cls[3] = e->G.class_max; }
    if ((what & 2) != 0) {
        S.cls[4] = e->F.class_counted; S.cls[5] = e->F.class_latency;
        for (int c = 0; c < kProfCols; c++) S.cell[c] = (const int64_t*)e->F.cells + (int64_t)c * S.n_entries;
    }
    S.mode = e->sig_q.mode; S.n_groups = e->A.n_groups;
    return TW_OK;
}

}  // namespace

int tw_class_history_reset(tw_engine* e) {
    if (e == nullptr) return TW_ERR_ARG;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    chist_free(e);
    return TW_OK;
}

int tw_class_history_push(tw_engine* e, int32_t what, int64_t epoch, int32_t* class_map, int64_t* summary) {
    if (e == nullptr) return TW_ERR_ARG;
    if (what < 1 || what > 3) return fail(e, TW_ERR_ARG, "tw_class_history_push: what outside {1 signatures, 2 profile, 3 both}");
    ChistSrc S;
    TWCHK(chist_resident(e, "tw_class_history_push", what, S));
    S.epoch = epoch;
    TWCHK(chist_fits(e, "tw_class_history_push", S.mode, S.n_groups));
    HIPCHK(hipSetDevice(e->device));
    TWCHK(chist_scratch(e, S.n_classes));
    HIPCHK(hipEventRecord(e->stage_ev[SE_CHIST + 0], e->stream));
    return chist_absorb(e, "tw_class_history_push", S, what, false, class_map, summary);
}

int tw_class_history_match(tw_engine* e, int32_t* class_map, int64_t* summary) {
    if (e == nullptr) return TW_ERR_ARG;
    ChistSrc S;
    TWCHK(chist_resident(e, "tw_class_history_match", 1, S));
    HIPCHK(hipSetDevice(e->device));
    if (e->ch_G != 0 && (S.mode != e->ch_mode || S.n_groups != e->ch_G)) {   // classes of another mode or other groups: none is held
        for (int64_t c = 0; class_map != nullptr && c < S.n_classes; c++) class_map[c] = -1;
        chist_summary(e, S.n_classes, S.n_entries, e->CH.C, e->CH.E, S.n_classes, summary);
        return TW_OK;
    }
    TWCHK(chist_scratch(e, S.n_classes));
    HIPCHK(hipEventRecord(e->stage_ev[SE_CHIST + 0], e->stream));
    int64_t new_classes = 0, new_entries = 0;
    TWCHK(chist_find(e, "tw_class_history_match", S, false, new_classes, new_entries));
    if (class_map != nullptr && S.n_classes > 0) HIPCHK(hipMemcpyAsync(class_map, e->CH.src_id, sizeof(int32_t) * (size_t)S.n_classes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    chist_summary(e, new_classes, new_entries, e->CH.C, e->CH.E, S.n_classes, summary);
    return TW_OK;
}

int tw_class_history_merge(tw_engine* e, const tw_class_catalogue* src, int64_t epoch, int32_t* class_map, int64_t* summary) {
    if (e == nullptr || src == nullptr) return TW_ERR_ARG;
    const std::string fn = "tw_class_history_merge";
    const int64_t nc = src->n_classes, ne = src->n_entries;
    if (nc < 0 || ne < 0 || src->class_off == nullptr) return fail(e, TW_ERR_ARG, fn + ": n_classes and n_entries must not be negative, class_off given");
    if (nc > (int64_t)INT32_MAX || ne > (int64_t)INT32_MAX) return fail(e, TW_ERR_UNSUPPORTED, fn + ": more than 2^31 - 1 classes or entries in the source");
    TWCHK(chist_fits(e, fn, src->mode, src->n_groups));
    if (src->class_off[0] != 0) return fail(e, TW_ERR_ARG, fn + ": class_off must start at 0");
    for (int64_t c = 0; c < nc; c++)
        if (src->class_off[c + 1] < src->class_off[c]) return fail(e, TW_ERR_ARG, fn + ": class_off must not decrease");
    if (src->class_off[nc] != ne) return fail(e, TW_ERR_ARG, fn + ": class_off must end at n_entries");
    if (ne > 0 && src->class_entries == nullptr) return fail(e, TW_ERR_ARG, fn + ": no class_entries for " + std::to_string(ne) + " entries");
    HIPCHK(hipSetDevice(e->device));
    TWCHK(chist_scratch(e, nc));
    // the source in one upload buffer: the offsets, the entries, then the figures that are given
    const int64_t* cls[kChistClassCols] = {src->trees, src->latency_sum, src->latency_min, src->latency_max, src->counted, src->latency,
                                           src->first_epoch, src->last_epoch, src->seen};
    const int64_t* cell[kProfCols] = {src->rows, src->span_time, src->span_min, src->span_max, src->self_time, src->path_time, src->path_rows, src->path_trees,
                                      src->offset};
    const auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
    size_t bytes = pad(sizeof(int64_t) * ((size_t)nc + 1)) + pad(sizeof(int32_t) * 4 * (size_t)ne);
    for (const int64_t* p : cls) bytes += p != nullptr ? pad(sizeof(int64_t) * (size_t)nc) : 0;
    for (const int64_t* p : cell) bytes += p != nullptr ? pad(sizeof(int64_t) * (size_t)ne) : 0;
    if (e->ch_up == nullptr || bytes > e->ch_up_bytes) {
        ChistNew N;
        void* up = chist_new(e, N, (int64_t)bytes);
        if (up == nullptr) return TW_ERR_DEVICE;
        N.got = {e->ch_up};
        e->ch_up = up; e->ch_up_bytes = bytes;
    }
    char* at = (char*)e->ch_up;
    const auto upload = [&](const void* host, size_t b) -> const void* {
        const void* dev = at;
        if (b > 0 && hipMemcpyAsync(at, host, b, hipMemcpyHostToDevice, e->stream) != hipSuccess) return nullptr;
        at += pad(b);
        return dev;
    };
    ChistSrc S{};
    S.n_classes = nc; S.n_entries = ne; S.epoch = epoch; S.mode = src->mode; S.n_groups = src->n_groups;
    S.off = (const int64_t*)upload(src->class_off, sizeof(int64_t) * ((size_t)nc + 1));
    S.entries = (const int32_t*)upload(src->class_entries, sizeof(int32_t) * 4 * (size_t)ne);
    bool sent = S.off != nullptr && S.entries != nullptr;
    for (int c = 0; c < kChistClassCols; c++)
        if (cls[c] != nullptr) { S.cls[c] = (const int64_t*)upload(cls[c], sizeof(int64_t) * (size_t)nc); sent = sent && S.cls[c] != nullptr; }
    for (int c = 0; c < kProfCols; c++)
        if (cell[c] != nullptr) { S.cell[c] = (const int64_t*)upload(cell[c], sizeof(int64_t) * (size_t)ne); sent = sent && S.cell[c] != nullptr; }
    if (!sent) { (void)hipGetLastError(); return fail(e, TW_ERR_DEVICE, fn + ": the upload of the source failed (the catalogue is as it was)"); }
    // the source's entries, checked before anything is changed
    HIPCHK(hipMemsetAsync(e->CH.counters, 0, sizeof(unsigned long long) * kChistCounters, e->stream));
    HIPCHK(hipEventRecord(e->stage_ev[SE_CHIST + 0], e->stream));
    if (ne > 0) {
        const unsigned threads = flat_threads(e);
        hipLaunchKernelGGL(k_chist_check, dim3(flat_grid(ne, threads)), dim3(threads), 0, e->stream, S, e->CH.counters);
        HIPCHK(hipGetLastError());
    }
    unsigned long long counters[kChistCounters];
    HIPCHK(hipMemcpyAsync(counters, e->CH.counters, sizeof(counters), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (counters[1] != 0)
        return fail(e, TW_ERR_ARG, fn + ": an entry of the source is out of range (level, cg, g, count) or a class' entries do not ascend strictly by (level, cg, g)");
    return chist_absorb(e, fn, S, 3, true, class_map, summary);
}

int tw_class_history_info(tw_engine* e, int64_t* out6) {
    if (e == nullptr || out6 == nullptr) return TW_ERR_ARG;
    const bool held = e->ch_G != 0;
    out6[0] = held ? e->CH.C : 0; out6[1] = held ? e->CH.E : 0; out6[2] = e->ch_pushes; out6[3] = held ? e->ch_mode : 0; out6[4] = e->ch_G;
    out6[5] = held ? e->CH.slots : 0;
    return TW_OK;
}

int tw_class_history_get(tw_engine* e, const tw_class_catalogue* out, int64_t* summary) {
    if (e == nullptr) return TW_ERR_ARG;
    if (e->ch_G == 0) return fail(e, TW_ERR_STATE, "tw_class_history_get on an empty catalogue (tw_class_history_push or tw_class_history_merge first; tw_class_history_reset empties it)");
    if (summary != nullptr) TWCHK(tw_class_history_info(e, summary));
    if (out == nullptr) return TW_OK;
    HIPCHK(hipSetDevice(e->device));
    const ChistDev& H = e->CH;
    const size_t nc = (size_t)H.C, ne = (size_t)H.E;
    int64_t* cls[kChistClassCols] = {out->trees, out->latency_sum, out->latency_min, out->latency_max, out->counted, out->latency, out->first_epoch, out->last_epoch,
                                     out->seen};
    int64_t* cell[kProfCols] = {out->rows, out->span_time, out->span_min, out->span_max, out->self_time, out->path_time, out->path_rows, out->path_trees, out->offset};
    TWCHK(copy_out(e, out->class_off, H.off, nc + 1));
    if (ne > 0) TWCHK(copy_out(e, out->class_entries, H.entries, 4 * ne));
    for (int c = 0; c < kChistClassCols && nc > 0; c++) TWCHK(copy_out(e, cls[c], H.cls + (int64_t)c * H.cls_cap, nc));
    for (int c = 0; c < kProfCols && ne > 0; c++) TWCHK(copy_out(e, cell[c], H.cell + (int64_t)c * H.ent_cap, ne));
    if (nc > 0 && (out->class_path_time != nullptr || out->class_top_entry != nullptr)) {
        ChistNew N;   // (freed when the call returns)
        int64_t* derived;
        CHIST_NEW(derived, int64_t, 2 * (int64_t)nc);
        const unsigned threads = flat_threads(e);
        hipLaunchKernelGGL(k_chist_derive, dim3(flat_grid((int64_t)nc, threads)), dim3(threads), 0, e->stream, H, derived, derived + nc);
        HIPCHK(hipGetLastError());
        TWCHK(copy_out(e, out->class_path_time, derived, nc));
        TWCHK(copy_out(e, out->class_top_entry, derived + nc, nc));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return TW_OK;
}

int tw_build_distributions(tw_engine* e, int64_t n, const int64_t* start, const int64_t* dur, const uint8_t* ep, int64_t large_delay,
                           int32_t E, int32_t* key_out, int64_t* sample_out) {
    if (e == nullptr || n <= 0 || !start || !dur || !ep || !key_out || !sample_out || E < 1 || E > TW_MAX_EP) return TW_ERR_ARG;
    HIPCHK(hipSetDevice(e->device));
    int64_t *d_s = nullptr, *d_d = nullptr, *d_v = nullptr;
    uint8_t* d_e = nullptr;
    int32_t* d_k = nullptr;
    hipError_t s = hipMalloc((void**)&d_s, sizeof(int64_t) * (size_t)n);
    if (s == hipSuccess) s = hipMalloc((void**)&d_d, sizeof(int64_t) * (size_t)n);
    if (s == hipSuccess) s = hipMalloc((void**)&d_v, sizeof(int64_t) * (size_t)n);
    if (s == hipSuccess) s = hipMalloc((void**)&d_e, (size_t)n);
    if (s == hipSuccess) s = hipMalloc((void**)&d_k, sizeof(int32_t) * (size_t)n);
    if (s == hipSuccess) s = hipMemcpyAsync(d_s, start, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, e->stream);
    if (s == hipSuccess) s = hipMemcpyAsync(d_d, dur, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, e->stream);
    if (s == hipSuccess) s = hipMemcpyAsync(d_e, ep, (size_t)n, hipMemcpyHostToDevice, e->stream);
    if (s == hipSuccess) {
        const unsigned threads = flat_threads(e);
        hipLaunchKernelGGL(k_build_distributions, dim3(flat_grid(n, threads)), dim3(threads), 0, e->stream,
                           (const int64_t*)d_s, (const int64_t*)d_d, (const uint8_t*)d_e, n, large_delay, (int)E, d_k, d_v);
        s = hipGetLastError();
    }
    if (s == hipSuccess) s = hipMemcpyAsync(key_out, d_k, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, e->stream);
    if (s == hipSuccess) s = hipMemcpyAsync(sample_out, d_v, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, e->stream);
    if (s == hipSuccess) s = hipStreamSynchronize(e->stream);
    (void)hipFree(d_s); (void)hipFree(d_d); (void)hipFree(d_v); (void)hipFree(d_e); (void)hipFree(d_k);
    if (s != hipSuccess) return fail(e, TW_ERR_DEVICE, std::string("tw_build_distributions: ") + hipGetErrorString(s));
    return TW_OK;
}

int tw_measure_hbm_copy(tw_engine* e, int64_t bytes, int32_t iters, double* gbps) {
    if (e == nullptr || gbps == nullptr || bytes < (1 << 20) || iters < 1) return TW_ERR_ARG;
    HIPCHK(hipSetDevice(e->device));
    void *a = nullptr, *b = nullptr;
    const size_t n16 = (size_t)bytes / 16;
    hipError_t s = hipMalloc(&a, n16 * 16);
    if (s == hipSuccess) s = hipMalloc(&b, n16 * 16);
    if (s == hipSuccess) s = hipMemsetAsync(a, 1, n16 * 16, e->stream);
    *gbps = 0.0;
    // One 16-byte load and store per thread, one workgroup per 4 KB (consecutive workgroups walk consecutive DRAM pages): 6.2 TB/s
    // on MI355X, the guide's float4-copy figure.  The grid-stride form of the same copy (2048 persistent workgroups, four loads in
    // flight) reaches 4.4-4.7 TB/s -- what round 3 quoted as the ceiling; it is timed too, the better one is reported.
    for (int variant = 0; variant < 2 && s == hipSuccess; variant++) {
        const unsigned grid = variant == 0 ? (unsigned)((n16 + 255) / 256) : 2048u;
        auto launch = [&]() {
            if (variant == 0) hipLaunchKernelGGL((k_copy16<1, false>), dim3(grid), dim3(256), 0, e->stream, (const uint4*)a, (uint4*)b, (int64_t)n16);
            else hipLaunchKernelGGL((k_copy16<4, false>), dim3(grid), dim3(256), 0, e->stream, (const uint4*)a, (uint4*)b, (int64_t)n16);
        };
        launch();  // warm-up
        s = hipEventRecord(e->ev[EV_BEGIN], e->stream);
        for (int k = 0; k < iters; k++) launch();
        if (s == hipSuccess) s = hipEventRecord(e->ev[EV_END], e->stream);
        if (s == hipSuccess) s = hipStreamSynchronize(e->stream);
        float ms = 0.f;
        if (s == hipSuccess) s = hipEventElapsedTime(&ms, e->ev[EV_BEGIN], e->ev[EV_END]);
        if (s == hipSuccess) {
            const double r = 2.0 * (double)(n16 * 16) * iters / ((double)ms * 1e-3) / 1e9;
            if (r > *gbps) *gbps = r;
        }
    }
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
    if (s != hipSuccess) return fail(e, TW_ERR_DEVICE, std::string("tw_measure_hbm_copy: ") + hipGetErrorString(s));
    return TW_OK;
}

int tw_host_alloc(int64_t bytes, void** out) {
    if (out == nullptr || bytes < 0) return TW_ERR_ARG;
    *out = nullptr;
    return hipHostMalloc(out, (size_t)std::max<int64_t>(bytes, 8), hipHostMallocDefault) == hipSuccess ? TW_OK : TW_ERR_DEVICE;
}

void tw_host_free(void* p) {
    if (p != nullptr) (void)hipHostFree(p);
}

/* Debug aid, not part of the public header: sizes of the work lists of the last pass --
 * out[0] = windows listed for k_select_heavy, out[1 + E] = spans listed for k_enumerate_heavy<E> (E <= kMaxEp),
 * out[2 + kMaxEp] = spans enumerated in parts, out[3 + kMaxEp] = of those, enumerated once more as a whole (out: 4 + kMaxEp ints). */
namespace {

struct BaseScratch {   // device scratch of one baseline call
    std::vector<void*> ptrs;
    ~BaseScratch() { for (void* p : ptrs) (void)hipFree(p); }
    void* raw(int64_t count, size_t elem, int fill) {
        void* p = nullptr;
        const size_t bytes = elem * (size_t)std::max<int64_t>(count, 1);
        if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        (void)hipMemset(p, fill, bytes);
        return p;
    }
};

int base_check(tw_engine* e, const char* who) {
    if (e->state < ST_LOADED) return fail(e, TW_ERR_STATE, std::string(who) + " before tw_load_batch");
    if (e->skip_mode) return fail(e, TW_ERR_UNSUPPORTED, std::string(who) + ": the lists of a skip-mode batch are not sorted; the host baselines serve it (traceweaver_amd/baselines.py)");
    return TW_OK;
}

}  // namespace

int tw_run_baseline(tw_engine* e, int kind, int32_t* parent_out) {
    if (e == nullptr || parent_out == nullptr) return TW_ERR_ARG;
    if (kind != TW_BASELINE_FCFS && kind != TW_BASELINE_VPATH) return fail(e, TW_ERR_ARG, "tw_run_baseline: kind is TW_BASELINE_FCFS or TW_BASELINE_VPATH (WAP5: tw_wap5_delays / tw_wap5_parents)");
    int rc = base_check(e, "tw_run_baseline");
    if (rc != TW_OK) return rc;
    if (kind == TW_BASELINE_VPATH && e->truth == nullptr) return fail(e, TW_ERR_STATE, "vPath follows a returning call to its request (vpath.py:42-46,81-84): tw_set_truth first");
    HIPCHK(hipSetDevice(e->device));
    const Dev& P = e->P;
    const dim3 tiles(P.n_tiles), tb(e->K.tile);
    BaseScratch S;
    BaseDev B{};
    B.truth = e->truth;
    B.parent = (int32_t*)S.raw(e->n_ie, sizeof(int32_t), 0);
    if (B.parent == nullptr) return fail(e, TW_ERR_DEVICE, "tw_run_baseline: out of device memory");
    if (kind == TW_BASELINE_FCFS) {
        hipLaunchKernelGGL(k_base_fcfs, tiles, tb, 0, e->stream, P, B);
    } else {
        B.count = (int32_t*)S.raw(e->n_ie, sizeof(int32_t), 0);
        B.unit_maxdur = (int64_t*)S.raw(P.n_units, sizeof(int64_t), 0);
        B.owner = (int32_t*)S.raw(P.n_out_total, sizeof(int32_t), 0x7f);
        int32_t *d_in = (int32_t*)S.raw(P.n_in_total, sizeof(int32_t), 0), *d_out = (int32_t*)S.raw(P.n_out_total, sizeof(int32_t), 0);
        int32_t *inv_in = (int32_t*)S.raw(P.n_in_total, sizeof(int32_t), 0), *inv_out = (int32_t*)S.raw(P.n_out_total, sizeof(int32_t), 0);
        if (B.count == nullptr || B.unit_maxdur == nullptr || B.owner == nullptr || d_in == nullptr || d_out == nullptr || inv_in == nullptr || inv_out == nullptr)
            return fail(e, TW_ERR_DEVICE, "tw_run_baseline: out of device memory");
        B.in_rank_inv = inv_in; B.out_rank_inv = inv_out;
        HIPCHK(hipDeviceSynchronize());   // (the fills above ran on the null stream)
        hipLaunchKernelGGL(k_rank_ends, tiles, tb, 0, e->stream, P, all_tiles_host(e), d_in, d_out);
        hipLaunchKernelGGL(k_place_ends, tiles, tb, 0, e->stream, P, all_tiles_host(e), (const int32_t*)d_in, (const int32_t*)d_out);
        hipLaunchKernelGGL(k_base_rank_inverse, tiles, tb, 0, e->stream, P, (const int32_t*)d_in, (const int32_t*)d_out, inv_in, inv_out);
        hipLaunchKernelGGL(k_base_prepare, tiles, tb, 0, e->stream, P, B);
        hipLaunchKernelGGL(k_base_vpath, tiles, tb, 0, e->stream, P, B);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(parent_out, B.parent, sizeof(int32_t) * e->n_ie, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TW_OK;
}

int tw_wap5_delays(tw_engine* e, int64_t* delay_sum, int32_t* delay_cnt, int64_t* unit_maxdur) {
    if (e == nullptr || delay_sum == nullptr || delay_cnt == nullptr) return TW_ERR_ARG;
    int rc = base_check(e, "tw_wap5_delays");
    if (rc != TW_OK) return rc;
    HIPCHK(hipSetDevice(e->device));
    const Dev& P = e->P;
    const dim3 tiles(P.n_tiles), tb(e->K.tile);
    BaseScratch S;
    BaseDev B{};
    B.parent = (int32_t*)S.raw(e->n_ie, sizeof(int32_t), 0); B.count = (int32_t*)S.raw(e->n_ie, sizeof(int32_t), 0);
    B.unit_maxdur = (int64_t*)S.raw(P.n_units, sizeof(int64_t), 0);
    B.delay_sum = (long long*)S.raw((int64_t)P.n_units * kMaxEp, sizeof(long long), 0); B.delay_cnt = (int32_t*)S.raw((int64_t)P.n_units * kMaxEp, sizeof(int32_t), 0);
    if (B.parent == nullptr || B.count == nullptr || B.unit_maxdur == nullptr || B.delay_sum == nullptr || B.delay_cnt == nullptr)
        return fail(e, TW_ERR_DEVICE, "tw_wap5_delays: out of device memory");
    HIPCHK(hipDeviceSynchronize());
    hipLaunchKernelGGL(k_base_prepare, tiles, tb, 0, e->stream, P, B);
    hipLaunchKernelGGL(k_wap5_delays, tiles, tb, 0, e->stream, P, B);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(delay_sum, B.delay_sum, sizeof(int64_t) * P.n_units * kMaxEp, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(delay_cnt, B.delay_cnt, sizeof(int32_t) * P.n_units * kMaxEp, hipMemcpyDeviceToHost, e->stream));
    if (unit_maxdur != nullptr) HIPCHK(hipMemcpyAsync(unit_maxdur, B.unit_maxdur, sizeof(int64_t) * P.n_units, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TW_OK;
}

int tw_wap5_parents(tw_engine* e, const double* mean, int32_t* parent_out, int32_t* call_request) {
    if (e == nullptr || mean == nullptr || parent_out == nullptr) return TW_ERR_ARG;
    int rc = base_check(e, "tw_wap5_parents");
    if (rc != TW_OK) return rc;
    HIPCHK(hipSetDevice(e->device));
    const Dev& P = e->P;
    const dim3 tiles(P.n_tiles), tb(e->K.tile);
    BaseScratch S;
    BaseDev B{};
    B.parent = (int32_t*)S.raw(e->n_ie, sizeof(int32_t), 0xff); B.count = (int32_t*)S.raw(e->n_ie, sizeof(int32_t), 0);
    double* mean_d = (double*)S.raw((int64_t)P.n_units * kMaxEp, sizeof(double), 0);
    B.call_request = (int32_t*)S.raw(P.n_out_total, sizeof(int32_t), 0xff);
    if (B.parent == nullptr || B.count == nullptr || mean_d == nullptr || B.call_request == nullptr) return fail(e, TW_ERR_DEVICE, "tw_wap5_parents: out of device memory");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyAsync(mean_d, mean, sizeof(double) * P.n_units * kMaxEp, hipMemcpyHostToDevice, e->stream));
    B.mean = mean_d;
    hipLaunchKernelGGL(k_wap5_parents, tiles, tb, 0, e->stream, P, B);
    hipLaunchKernelGGL(k_wap5_finish, tiles, tb, 0, e->stream, P, B);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(parent_out, B.parent, sizeof(int32_t) * e->n_ie, hipMemcpyDeviceToHost, e->stream));
    if (call_request != nullptr) HIPCHK(hipMemcpyAsync(call_request, B.call_request, sizeof(int32_t) * (size_t)P.n_out_total, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return TW_OK;
}

/* Debug aid, not part of the public header: the model-selection fits of the last refit, [n_slots][5][16] = BIC (inf = raised),
 * weights[5], means[5], precision_cholesky[5]. */
extern "C" int tw_debug_fit_models(tw_engine* e, double* out) {
    if (e == nullptr || out == nullptr) return TW_ERR_ARG;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(out, e->fit_models, sizeof(double) * e->n_slots * kMaxComp * kModelStride, hipMemcpyDeviceToHost, e->stream));

    HIPCHK(hipStreamSynchronize(e->stream));
    return TW_OK;
}

int tw_debug_worklists(tw_engine* e, int32_t* out) {
    if (e == nullptr || out == nullptr || e->state < ST_PASS1) return TW_ERR_ARG;
    static int32_t sel_all[4 * kSelSeg * kCtrStride];
    HIPCHK(hipMemcpyAsync(sel_all, e->P.heavy_count, sizeof(sel_all), hipMemcpyDeviceToHost, e->stream));
    int32_t both[2 * (kMaxEp + 1)];
    HIPCHK(hipMemcpyAsync(both, e->P.heavy_in_count, sizeof(both), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    out[0] = 0;
    for (int k = 0; k < 4 * kSelSeg; k++) out[0] += sel_all[k * kCtrStride];
    for (int k = 0; k <= kMaxEp; k++) out[1 + k] = both[k] + both[kMaxEp + 1 + k];
    if (e->K.debug_lists != 0)   // (the first enumeration's lists, as its chain left them: narrow + wide + long enumerations)
        for (int k = 1; k <= kMaxEp; k++) out[1 + k] = e->first_lists[0][k] + e->first_lists[1][k] + e->first_lists[2][k];
    int32_t split[kMaxEp + 1];   // [0] spans listed again after the merge, [E >= 2] split spans of the class
    HIPCHK(hipMemcpy(split, e->P.split_count, sizeof(split), hipMemcpyDeviceToHost));
    out[2 + kMaxEp] = 0; out[3 + kMaxEp] = split[0];
    for (int k = 2; k <= kMaxEp; k++) out[2 + kMaxEp] += split[k];
    // [12] items k_enumerate_lean handed to k_enumerate_heavy, [13] spans refused list parts / parts (budget or arena), [14] list parts
    int32_t more[3][kMaxEp + 1];
    HIPCHK(hipMemcpy(more[0], e->P.fb_total, sizeof(more[0]), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(more[1], e->P.defer_refused, sizeof(more[1]), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(more[2], e->P.defer_count, sizeof(more[2]), hipMemcpyDeviceToHost));
    for (int q = 0; q < 3; q++) { out[4 + kMaxEp + q] = 0; for (int k = 0; k <= kMaxEp; k++) out[4 + kMaxEp + q] += more[q][k]; }
    return TW_OK;
}

int tw_assign_service(tw_engine* e, int32_t n_in, const int64_t* in_start, const int64_t* in_end, int32_t E,
                      const int64_t* out_off, const int64_t* out_start, const int64_t* out_end, const uint8_t* dag,
                      const int32_t* key_rank, const int32_t* mix_n, const double* mix_p, const tw_results* r) {
    if (e == nullptr) return TW_ERR_ARG;
    const int64_t in_off[2] = {0, n_in};
    tw_batch b;
    b.n_units = 1; b.unit_in_off = in_off; b.unit_E = &E; b.ep_off = out_off; b.dag = dag; b.key_rank = key_rank;
    b.in_start = in_start; b.in_end = in_end; b.out_start = out_start; b.out_end = out_end;
    b.batch_size = 100; b.batch_size_mis = 30; b.topk = TW_TOPK; b.unit_time_scale = nullptr; b.skip = nullptr; b.unit_part = nullptr;
    int rc = tw_load_batch(e, &b, 0);
    if (rc == TW_OK) rc = tw_run_pass1(e);
    if (rc == TW_OK && mix_n != nullptr) {
        rc = tw_set_mixtures(e, mix_n, mix_p);
        if (rc == TW_OK) rc = tw_run_pass2(e);
    }
    if (rc == TW_OK && r != nullptr) rc = tw_get_results(e, mix_n != nullptr ? 2 : 1, r);
    return rc;
}

}  // extern "C"

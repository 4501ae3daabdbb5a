// tw_filt.h -- traces selected by a predicate on the device: a filter every trace stage reads (tw_filter_traces).
//
// Extends: the one hard-coded query of the reference (src/query_engine/delay_culprit.py:19-28 -- whole traces, the slowest X %, started
// after Y) to a predicate in disjunctive normal form over the stitched trees: up to 16 clauses in up to 8 terms, each clause a range
// test on a figure of the tree -- its latency, rows, start or class, or a sum / minimum / maximum over its rows of one group or over
// its signature items of one caller -> callee edge.  The result is bit TW_TREE_MATCH of the device forest's tree_flags, which every
// later stage selects by through need_flags, as it does by TW_TREE_CONFIDENT.  include/traceweaver_amd.h has the definitions.
//
//   k_filt_trees      one wavefront per kFiltTrees consecutive trees of the CSR grouping (as k_dist_cohort): one 64-bit cell per (tree
//                     slot, clause) in LDS -- a sum in two's complement, a minimum / maximum as a sign-flipped unsigned key -- and one
//                     mask per tree slot of the clauses that met a row.  A lane's positions ascend, so it keeps its sums, minima and
//                     maxima in registers while its tree does not change and folds them into the cells (64-bit LDS atomic add / min /
//                     max) when the tree changes and at the end.  A tree of more than kFiltCap rows is taken by the wavefront alone and
//                     reduced by shuffles.  Then one lane per (tree, clause) decides the clause and writes clause_value, one lane per
//                     tree decides the terms and the match and rewrites bit 4 of tree_flags[t] (the wavefront owns its trees: no race).
//                     clause_trees, term_trees and the summary: __ballot / __popcll and shuffle reductions into a table of the
//                     wavefront, added to global memory once per wavefront and non-zero cell.
//   count, scan, list the ascending list of the matched trees: the three scan kernels of tw_sig.h (k_sig_scan_sums / _chunks / _write)
//                     over the view FiltScan -- block counts, their exclusive scan, the write.  No cursor: where a tree lies in the
//                     list does not depend on scheduling.
//
// Every output is a pure function of the inputs: no floating point; the atomics are integer adds, minima, maxima and ors of which
// only the result is read.
#pragma once
#include "tw_prof.h"

namespace tw {

#ifdef TW_TILE_SMALL   // the tiny values of the tests' host build: the packed route and the single-tree route both occur
constexpr int kFiltTrees = 4;
constexpr int kFiltCap = 12;
#else
constexpr int kFiltTrees = 16;       // consecutive trees a wavefront takes together
constexpr int kFiltCap = 256;        // rows of a tree beyond which the wavefront takes it alone (64 lanes on one cell cost more than six shuffle rounds)
#endif
constexpr int kFiltWaves = 4;
constexpr int kFiltMaxClauses = 16, kFiltMaxTerms = 8;
constexpr uint32_t kFiltBit = 16;    // TW_TREE_MATCH
// counters: [0] eligible, [1] matched, [2] latency sum, [3] least / [4] greatest latency key of the matched trees, [5] their rows,
// [6] the total of the list's scan, [8 .. 24) clause_trees, [24 .. 32) term_trees
constexpr int kFiltCounters = 32, kFiltClauseAt = 8, kFiltTermAt = 24, kFiltMinAt = 3, kFiltMaxAt = 4;
enum { FILT_LATENCY = 0, FILT_ROWS = 1, FILT_START = 2, FILT_CLASS = 3, FILT_GROUP = 4, FILT_EDGE = 5 };
enum { FILT_COL_SPAN = 1, FILT_COL_SELF = 2, FILT_COL_PATH = 4, FILT_COL_FLAG = 8, FILT_COL_CALLER = 16 };

struct FiltClauseDev {
    int32_t subject, group, caller, metric, reduce, negate, term, pad;
    int64_t lo, hi;
};
struct FiltQueryDev {
    uint32_t need_flags, skip_flags;
    int32_t n_clauses;
    uint32_t row_mask;               // the clauses over rows (GROUP, EDGE)
    uint32_t term_used;              // the terms with a clause
    uint32_t cols;                   // what the row clauses read (FILT_COL_*)
    FiltClauseDev c[kFiltMaxClauses];
};
struct FiltDev {
    const int32_t* row_group;
    const int64_t *self_time, *path_time;   // of the resident attribution (read only with FILT_COL_SELF / _PATH / _FLAG)
    const uint8_t* row_flag;
    const int32_t* tree_class;              // of the resident signature result (read only by a CLASS clause)
    uint8_t* tree_match;
    int32_t* match_trees;
    int64_t* clause_value;                  // [n_trees][n_clauses]
    unsigned long long *chunk_sum, *counters;
};

// A cell holds a sum in two's complement or a minimum / maximum as dist_key: identity and fold.
__device__ __forceinline__ unsigned long long filt_identity(int reduce) { return reduce == 1 ? ~0ull : 0ull; }
__device__ __forceinline__ unsigned long long filt_fold(int reduce, unsigned long long a, unsigned long long b) {
    return reduce == 0 ? a + b : reduce == 1 ? dist_umin(a, b) : dist_umax(a, b);
}

struct FiltRow {
    int32_t g, cg;
    bool server;
    int64_t d, st, pt, on;
};

__device__ __forceinline__ FiltRow filt_row(const StitchDev& S, const FiltDev& F, uint32_t cols, int32_t r) {
    FiltRow w{};
    w.g = F.row_group[r];
    w.cg = -2;   // (no clause names it)
    if (cols & FILT_COL_CALLER) {
        w.server = S.row_kind[r] == 1;
        if (w.server && w.g >= 0) w.cg = sig_caller_group(S, F.row_group, r);
    }
    if (cols & FILT_COL_SPAN) {
        const int64_t s = S.row_start[r];
        w.d = stitch_max(S.row_end[r], s) - s;
    }
    if (cols & FILT_COL_SELF) w.st = F.self_time[r];
    if (cols & FILT_COL_PATH) w.pt = F.path_time[r];
    if (cols & FILT_COL_FLAG) w.on = F.row_flag[r] & 1;
    return w;
}

// does row w count for clause c, and with which value (as the clause's cell holds it)?
__device__ __forceinline__ bool filt_row_value(const FiltClauseDev& c, const FiltRow& w, unsigned long long& v) {
    const bool hit = c.subject == FILT_GROUP ? (c.group < 0 ? w.g >= 0 : w.g == c.group) : (w.server && w.g == c.group && w.cg == c.caller);
    if (!hit) return false;
    const int64_t x = c.metric == 0 ? 1 : c.metric == 1 ? w.d : c.metric == 2 ? w.st : c.metric == 3 ? w.pt : w.on;
    v = c.reduce == 0 ? (unsigned long long)x : dist_key(x);
    return true;
}

// One row into the lane's registers: acc[j] and bit j of seen for every row clause j the row counts for.
__device__ __forceinline__ void filt_take(const FiltQueryDev& Q, const FiltRow& w, unsigned long long (&acc)[kFiltMaxClauses], uint32_t& seen) {
#pragma unroll
    for (int j = 0; j < kFiltMaxClauses; j++)
        if ((Q.row_mask >> j) & 1u) {
            unsigned long long v;
            if (filt_row_value(Q.c[j], w, v)) {
                acc[j] = filt_fold(Q.c[j].reduce, acc[j], v);
                seen |= 1u << j;
            }
        }
}

// The lane's registers into the cells of tree slot `slot`, and back to the identities.
__device__ __forceinline__ void filt_flush(const FiltQueryDev& Q, unsigned long long* cell, uint32_t* slot_seen, int slot,
                                           unsigned long long (&acc)[kFiltMaxClauses], uint32_t& seen) {
    if (seen == 0) return;
#pragma unroll
    for (int j = 0; j < kFiltMaxClauses; j++)
        if ((seen >> j) & 1u) {
            unsigned long long* x = cell + slot * kFiltMaxClauses + j;
            const int reduce = Q.c[j].reduce;
            if (reduce == 0) { if (acc[j] != 0) atomicAdd(x, acc[j]); }
            else if (reduce == 1) atomicMin(x, acc[j]);
            else atomicMax(x, acc[j]);
            acc[j] = filt_identity(reduce);
        }
    atomicOr(&slot_seen[slot], seen);
    seen = 0;
}

__global__ void __launch_bounds__(64 * kFiltWaves) k_filt_trees(StitchDev S, FiltDev F, FiltQueryDev Q, int64_t n_trees) {
    __shared__ unsigned long long s_cell[kFiltWaves][kFiltTrees * kFiltMaxClauses];
    __shared__ unsigned long long s_cnt[kFiltWaves][kFiltCounters];
    __shared__ int64_t s_off[kFiltWaves][kFiltTrees + 1];
    __shared__ uint32_t s_seen[kFiltWaves][kFiltTrees];
    __shared__ uint8_t s_hold[kFiltWaves][kFiltTrees * kFiltMaxClauses];
    __shared__ FiltClauseDev s_clause[kFiltMaxClauses];   // for the lanes that each decide another clause
    const int nl = (int)stitch_min(blockDim.x, 64), lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const int wpb = (int)stitch_max(blockDim.x / 64, 1);
    const int nc = Q.n_clauses;
    unsigned long long* cell = s_cell[wave];
    unsigned long long* cnt = s_cnt[wave];
    int64_t* off = s_off[wave];
    uint32_t* slot_seen = s_seen[wave];
    uint8_t* hold = s_hold[wave];
    for (int j = threadIdx.x; j < kFiltMaxClauses; j += blockDim.x) s_clause[j] = Q.c[j];   // (beyond nc: zeros)
    for (int q = lane; q < kFiltCounters; q += nl) cnt[q] = q == kFiltMinAt ? ~0ull : 0ull;
    __syncthreads();
    unsigned long long acc[kFiltMaxClauses];
#pragma unroll
    for (int j = 0; j < kFiltMaxClauses; j++) acc[j] = filt_identity(Q.c[j].reduce);
    uint32_t seen = 0;
    const int64_t n_chunks = (n_trees + kFiltTrees - 1) / kFiltTrees;
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < n_chunks; c += (int64_t)gridDim.x * wpb) {
        const int64_t c0 = c * kFiltTrees;
        const int nt = (int)stitch_min((int64_t)kFiltTrees, n_trees - c0);
        for (int t = lane; t <= nt; t += nl) {
            off[t] = S.tree_off[c0 + t];
            if (t < nt) slot_seen[t] = 0;
        }
        for (int q = lane; q < nt * kFiltMaxClauses; q += nl) cell[q] = filt_identity(s_clause[q % kFiltMaxClauses].reduce);   // (beyond nc: never read)
        stitch_wave_sync();
        // 1. the rows: runs of trees of at most kFiltCap rows together, a larger tree alone
        for (int t0 = 0; Q.row_mask != 0 && t0 < nt;) {
            if (off[t0 + 1] - off[t0] > kFiltCap) {
                for (int64_t k = off[t0] + lane; k < off[t0 + 1]; k += nl) filt_take(Q, filt_row(S, F, Q.cols, S.tree_rows[k]), acc, seen);
                uint32_t any = 0;
#pragma unroll
                for (int j = 0; j < kFiltMaxClauses; j++)
                    if ((Q.row_mask >> j) & 1u) {
                        const int reduce = Q.c[j].reduce;
                        unsigned long long x = acc[j];
                        for (int o = 32; o >= 1; o >>= 1)
                            if (o < nl) x = filt_fold(reduce, x, (unsigned long long)__shfl_xor((long long)x, o));
                        if (__ballot((seen >> j) & 1u) != 0) any |= 1u << j;
                        if (lane == 0) cell[t0 * kFiltMaxClauses + j] = x;
                        acc[j] = filt_identity(reduce);
                    }
                if (lane == 0) slot_seen[t0] = any;
                seen = 0;
                t0++;
                continue;
            }
            int t1 = t0 + 1;
            while (t1 < nt && off[t1 + 1] - off[t1] <= kFiltCap) t1++;
            int t = t0;   // a lane's positions ascend, so its tree only moves forward
            for (int64_t k = off[t0] + lane; k < off[t1]; k += nl) {
                int tn = t;
                while (tn + 1 < t1 && off[tn + 1] <= k) tn++;
                if (tn != t) { filt_flush(Q, cell, slot_seen, t, acc, seen); t = tn; }
                filt_take(Q, filt_row(S, F, Q.cols, S.tree_rows[k]), acc, seen);
            }
            filt_flush(Q, cell, slot_seen, t, acc, seen);
            t0 = t1;
        }
        stitch_wave_sync();
        // 2. one lane per (tree, clause): the value and whether the clause holds
        for (int q = lane; q < nt * nc; q += nl) {
            const int tl = q / nc, j = q - tl * nc;
            const int64_t t = c0 + tl;
            const FiltClauseDev cl = s_clause[j];
            bool has = true;
            int64_t v = 0;
            if (cl.subject == FILT_LATENCY) v = S.tree_latency[t];
            else if (cl.subject == FILT_ROWS) v = off[tl + 1] - off[tl];
            else if (cl.subject == FILT_START) v = S.row_start[S.tree_root[t]];
            else if (cl.subject == FILT_CLASS) v = F.tree_class[t];
            else {
                const unsigned long long x = cell[tl * kFiltMaxClauses + j];
                if (cl.reduce == 0) v = (int64_t)x;
                else { has = ((slot_seen[tl] >> j) & 1u) != 0; v = (int64_t)(x ^ (1ull << 63)); }
            }
            F.clause_value[t * nc + j] = has ? v : INT64_MIN;
            hold[tl * kFiltMaxClauses + j] = (has && ((cl.lo <= v && v <= cl.hi) != (cl.negate != 0))) ? 1 : 0;
        }
        stitch_wave_sync();
        // 3. one lane per tree: the terms, the match, the bit; the counts by ballot (the control flow is the same in every lane)
        for (int tb = 0; tb < nt; tb += nl) {
            const int tl = tb + lane;
            const int64_t t = c0 + tl;
            bool elig = false, match = false;
            uint32_t held = 0, bad = 0;
            int64_t lat = 0, rows = 0;
            if (tl < nt) {
                const uint32_t f = S.tree_flags[t];
                elig = (f & Q.need_flags) == Q.need_flags && (f & Q.skip_flags) == 0;
                for (int j = 0; j < nc; j++) {
                    if (hold[tl * kFiltMaxClauses + j] != 0) held |= 1u << j;
                    else bad |= 1u << s_clause[j].term;
                }
                match = elig && (nc == 0 || (Q.term_used & ~bad) != 0);
                S.tree_flags[t] = (uint8_t)((f & ~kFiltBit) | (match ? kFiltBit : 0u));
                F.tree_match[t] = match ? 1 : 0;
                if (match) { lat = S.tree_latency[t]; rows = off[tl + 1] - off[tl]; }
            }
            const unsigned long long be = __ballot(elig), bm = __ballot(match);
            if (be == 0) continue;
            for (int j = 0; j < nc; j++) {
                const unsigned long long b = __ballot(elig && ((held >> j) & 1u));
                if (lane == 0 && b != 0) cnt[kFiltClauseAt + j] += (unsigned long long)__popcll(b);
            }
            for (int k = 0; k < kFiltMaxTerms; k++) {
                if (((Q.term_used >> k) & 1u) == 0) continue;
                const unsigned long long b = __ballot(elig && ((bad >> k) & 1u) == 0);
                if (lane == 0 && b != 0) cnt[kFiltTermAt + k] += (unsigned long long)__popcll(b);
            }
            if (lane == 0) cnt[0] += (unsigned long long)__popcll(be);
            if (bm == 0) continue;
            unsigned long long sl = (unsigned long long)lat, sr = (unsigned long long)rows;
            unsigned long long lo = match ? dist_key(lat) : ~0ull, hi = match ? dist_key(lat) : 0ull;
            sl = dist_wave_sum(sl, nl);
            sr = dist_wave_sum(sr, nl);
            for (int o = 32; o >= 1; o >>= 1)
                if (o < nl) {
                    lo = dist_umin(lo, (unsigned long long)__shfl_xor((long long)lo, o));
                    hi = dist_umax(hi, (unsigned long long)__shfl_xor((long long)hi, o));
                }
            if (lane == 0) {
                cnt[1] += (unsigned long long)__popcll(bm);
                cnt[2] += sl;
                cnt[kFiltMinAt] = dist_umin(cnt[kFiltMinAt], lo);
                cnt[kFiltMaxAt] = dist_umax(cnt[kFiltMaxAt], hi);
                cnt[5] += sr;
            }
        }
        stitch_wave_sync();   // ... before the next trees overwrite the slots
    }
    // the wavefront's table onto the global counters: one atomic per non-zero cell
    stitch_wave_sync();
    const bool matched = cnt[1] != 0;
    for (int q = lane; q < kFiltCounters; q += nl) {
        const unsigned long long x = cnt[q];
        if (q == kFiltMinAt) { if (matched) atomicMin(&F.counters[q], x); }
        else if (q == kFiltMaxAt) { if (matched) atomicMax(&F.counters[q], x); }
        else if (x != 0) atomicAdd(&F.counters[q], x);
    }
}

// The list of the matched trees by the scan kernels of tw_sig.h: item t counts 1 when it matched, and lies at the number of matched
// trees before it.
struct FiltScan {
    FiltDev F;
    __device__ __forceinline__ unsigned long long packed(int64_t t) const { return F.tree_match[t] != 0 ? 1ull : 0ull; }
    __device__ __forceinline__ unsigned long long* chunks() const { return F.chunk_sum; }
    __device__ __forceinline__ void total(unsigned long long run) const { F.counters[6] = run; }
    __device__ __forceinline__ void emit(int64_t t, unsigned long long run) const { F.match_trees[run] = (int32_t)t; }
};
}  // namespace tw

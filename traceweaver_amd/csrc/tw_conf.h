// tw_conf.h -- how far the reconstructed traces can be trusted (tw_get_decisions / tw_score_traces).
//
// Replaces: the reference's one figure of trust, not_best_count / num_spans per service -- the requests whose selected tuple is
// not their own best-scoring one (traceweaver_v3.py:1201-1207), written to confidence_scores_*.pickle (executor.py:1203-1205,
// 1241) and plotted as 1 - not_best / n against accuracy (utils/plot_accuracy_vs_confidence_multiple_cgs.py:76-84).  The
// facts behind that scalar are resident after every pass (chosen, rep, the two candidate lists); here they leave the device per
// request, are reduced over the trees the last tw_stitch_traces left behind, and are counted against ground truth.
//
//   k_conf_requests  one lane per request: rank = chosen, list_n and the decision margin (one binary64 subtraction of two
//                    scores of the list `chosen` indexes, read through cand_score; lanes of a tile read neighbouring words)
//   k_conf_scatter   row_request[in_row[g]] = g (the rows are distinct, tw_set_span_rows checks it: plain stores)
//   k_conf_trees     one wavefront per kConfTrees consecutive trees of the CSR grouping: lanes stride over the trees' rows;
//                    counts by integer adds in LDS, min_margin as an atomicMin on an order-preserving 64-bit key of the double,
//                    then -- a second sweep over the same rows -- weakest_row as an atomicMin among the rows whose key is
//                    the tree's minimum; writes the per-tree figures and rewrites bit 3 (TW_TREE_CONFIDENT) of tree_flags
//   k_conf_calib     one lane per tree: the calibration table and the summary, added up in LDS per workgroup first, then one
//                    64-bit integer atomicAdd per workgroup and nonzero cell
//
// Every output is a pure function of the inputs: the one floating-point operation is the subtraction that defines a margin;
// minima are taken on integer keys; the atomic adds are integer adds whose sum alone is read.
#pragma once
#include "tw_kernels.h"
#include "tw_stitch.h"

namespace tw {

constexpr int kConfTrees = 16;       // consecutive trees a wavefront takes together (one LDS slot each)
constexpr int kConfWaves = 4;        // wavefronts per workgroup of k_conf_trees
constexpr int kConfMaxEdges = 15;    // bucket edges of the calibration table: at most kConfMaxEdges + 2 buckets
constexpr int kConfCalibCols = 3;    // trees, exact trees, decisions
constexpr int kConfCells = (kConfMaxEdges + 2) * kConfCalibCols + 5;   // ... and summary5 behind the table
constexpr unsigned long long kConfNan = 0x7ff8000000000000ull;         // the one NaN a margin is stored as
constexpr unsigned long long kConfKeyInf = 0xfff0000000000000ull;      // conf_key(+inf): the largest key of a number

struct ConfDev {
    // per request
    int32_t *rank, *list_n;
    double* margin;
    // per row
    int32_t* row_request;            // request whose incoming span the row is, -1 = none
    // per tree
    int32_t *decisions, *not_best, *unassigned, *weakest_row;
    double* min_margin;
    uint8_t* confident;
    unsigned long long* cells;       // [kConfCells] calib[bucket][col], then summary5
};

struct ConfQueryDev {
    double threshold;
    int32_t n_edges;
    double edges[kConfMaxEdges];
};

// binary64 -> uint64, ascending in the order -inf < ... < -0 < +0 < ... < +inf (NaN never gets a key)
__device__ __forceinline__ unsigned long long conf_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double conf_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

__global__ void __launch_bounds__(kTile) k_conf_requests(Dev P, ConfDev C) {
    const TileDev Tl = P.tiles[blockIdx.x];
    const UnitDev& U = P.units[Tl.unit];
    const int i = Tl.first + threadIdx.x;
    if (i >= U.n_in) return;
    const int64_t g = U.in_off + i;
    const int c = P.chosen[g], n = cand_n(P, U, i);
    double m = __longlong_as_double((long long)kConfNan);
    if (c == 0) m = n > 1 ? cand_score(P, U, i, 0) - cand_score(P, U, i, 1) : __longlong_as_double(0x7ff0000000000000ll);
    else if (c > 0 && c < kTopK) m = cand_score(P, U, i, c) - cand_score(P, U, i, 0);
    if (m != m) m = __longlong_as_double((long long)kConfNan);   // (inf - inf: the sign of the NaN differs between machines)
    C.rank[g] = c;
    C.list_n[g] = n;
    C.margin[g] = m;
}

__global__ void __launch_bounds__(256) k_conf_scatter(StitchDev S, ConfDev C, int64_t n_in) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n_in) C.row_request[S.in_row[g]] = (int32_t)g;
}

__global__ void __launch_bounds__(64 * kConfWaves) k_conf_trees(StitchDev S, ConfDev C, ConfQueryDev Q, int64_t n_trees) {
    __shared__ unsigned long long s_key[kConfWaves][kConfTrees];
    __shared__ int64_t s_off[kConfWaves][kConfTrees + 1];
    __shared__ int32_t s_row[kConfWaves][kConfTrees];
    __shared__ int32_t s_cnt[kConfWaves][3][kConfTrees];
    const int nl = (int)stitch_min(blockDim.x, 64), lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const int wpb = (int)stitch_max(blockDim.x / 64, 1);
    unsigned long long* key = s_key[wave];
    int64_t* off = s_off[wave];
    int32_t* row = s_row[wave];
    int32_t *cnt_d = s_cnt[wave][0], *cnt_nb = s_cnt[wave][1], *cnt_una = s_cnt[wave][2];
    const int64_t n_chunks = (n_trees + kConfTrees - 1) / kConfTrees;
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < n_chunks; c += (int64_t)gridDim.x * wpb) {
        const int64_t c0 = c * kConfTrees;
        const int nt = (int)stitch_min((int64_t)kConfTrees, n_trees - c0);
        for (int t = lane; t <= nt; t += nl) {
            off[t] = S.tree_off[c0 + t];
            if (t < nt) { key[t] = ~0ull; row[t] = INT32_MAX; cnt_d[t] = 0; cnt_nb[t] = 0; cnt_una[t] = 0; }
        }
        stitch_wave_sync();
        const int64_t a = off[0], m = off[nt] - a;
        // 1. counts and the smallest key; a lane's positions ascend, so its tree only moves forward
        int t = 0;
        for (int64_t k = lane; k < m; k += nl) {
            while (t + 1 < nt && off[t + 1] <= a + k) t++;
            const int32_t g = C.row_request[S.tree_rows[a + k]];
            if (g < 0) continue;
            const int32_t rk = C.rank[g];
            const double mg = C.margin[g];
            atomicAdd(&cnt_d[t], 1);
            if (rk != 0) atomicAdd(&cnt_nb[t], 1);
            if (rk < 0) atomicAdd(&cnt_una[t], 1);
            if (mg == mg) atomicMin(&key[t], conf_key(mg));
        }
        stitch_wave_sync();
        // 2. the smallest row among those that attain it
        t = 0;
        for (int64_t k = lane; k < m; k += nl) {
            while (t + 1 < nt && off[t + 1] <= a + k) t++;
            const int32_t r = S.tree_rows[a + k];
            const int32_t g = C.row_request[r];
            if (g < 0) continue;
            const double mg = C.margin[g];
            if (mg == mg && conf_key(mg) == key[t]) atomicMin(&row[t], r);
        }
        stitch_wave_sync();
        for (int q = lane; q < nt; q += nl) {
            const int64_t tr = c0 + q;
            const bool any = key[q] != ~0ull;
            const double mm = conf_unkey(any ? key[q] : kConfKeyInf);
            const bool conf = cnt_d[q] > 0 && cnt_nb[q] == 0 && mm >= Q.threshold;
            C.decisions[tr] = cnt_d[q];
            C.not_best[tr] = cnt_nb[q];
            C.unassigned[tr] = cnt_una[q];
            C.min_margin[tr] = mm;
            C.weakest_row[tr] = any ? row[q] : -1;
            C.confident[tr] = conf ? 1 : 0;
            S.tree_flags[tr] = (uint8_t)((S.tree_flags[tr] & ~TW_TREE_CONFIDENT) | (conf ? TW_TREE_CONFIDENT : 0));
        }
        stitch_wave_sync();   // ... before the next trees overwrite the slots
    }
}

__global__ void __launch_bounds__(256) k_conf_calib(StitchDev S, ConfDev C, ConfQueryDev Q, int64_t n_trees) {
    __shared__ unsigned long long acc[kConfCells];
    for (int q = threadIdx.x; q < kConfCells; q += blockDim.x) acc[q] = 0;
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int nl = (int)stitch_min(blockDim.x, 64);
    int32_t d = 0, nb = 0, una = 0;
    bool conf = false;
    if (t < n_trees) {
        d = C.decisions[t]; nb = C.not_best[t]; una = C.unassigned[t];
        conf = C.confident[t] != 0;
        const uint32_t f = S.tree_flags[t];
        if ((f & 1u) != 0 && d > 0) {
            int b = 0;
            if (nb == 0) {
                const double mm = C.min_margin[t];
                b = 1;
                for (int j = 0; j < Q.n_edges; j++) b += mm >= Q.edges[j] ? 1 : 0;
            }
            atomicAdd(&acc[b * kConfCalibCols + 0], 1ull);
            if (f & 4u) atomicAdd(&acc[b * kConfCalibCols + 1], 1ull);
            atomicAdd(&acc[b * kConfCalibCols + 2], (unsigned long long)d);
        }
    }
    // summary5: one add per wavefront and cell
    unsigned long long sums[3] = {(unsigned long long)d, (unsigned long long)nb, (unsigned long long)una};
    for (int off = 32; off >= 1; off >>= 1)
        if (off < nl)
            for (int k = 0; k < 3; k++) sums[k] += (unsigned long long)__shfl_xor((long long)sums[k], off);
    const unsigned long long scored = __ballot(d > 0), sure = __ballot(conf);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* sm = acc + (kConfMaxEdges + 2) * kConfCalibCols;
        if (scored) atomicAdd(&sm[0], (unsigned long long)__popcll(scored));
        if (sure) atomicAdd(&sm[1], (unsigned long long)__popcll(sure));
        for (int k = 0; k < 3; k++)
            if (sums[k]) atomicAdd(&sm[2 + k], sums[k]);
    }
    __syncthreads();
    for (int q = threadIdx.x; q < kConfCells; q += blockDim.x)
        if (acc[q] != 0) atomicAdd(&C.cells[q], acc[q]);
}

}  // namespace tw

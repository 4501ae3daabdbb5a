// tw_extr.h -- reconstructed traces handed out as trees: exemplars, pre-order rows (tw_extract_traces / tw_get_extracted).
//
// Extends: the aggregate answers of the trace stages (culprits, distributions, classes, a match bit) by the traces themselves.  The
// reference walks every trace on the host (src/query_engine/delay_culprit.py:30-97) and never hands one out; here a query selects
// trees of the stitched forest -- the first `limit` in id, slowest-first or fastest-first order, the trees at given quantiles of the
// latency, or a list -- and the result is a packed sub-forest: every selected tree in pre-order with local parent indices, which a
// renderer or a writer needs nothing else for.  include/traceweaver_amd.h has the definitions.
//
//   selection         order 0 and the eligible count: the three scan kernels of tw_sig.h over the view ExtrSelScan (no cursor).  The
//                     latency orders: the (latency, tree) sort of the attribution's selection (k_attr_flags + radix sort, the engine's
//                     trees_by_latency); k_extr_slowest reads it from the end and turns every run of equal latencies round again, so
//                     that ties ascend in tree; k_extr_pick reads the few entries a quantile query names.
//   k_extr_sizes      per selected tree the sel_* columns; the largest tree, the trees and rows of the single-tree route
//   (scan)            out_off: the scan kernels over the view ExtrOffScan
//   k_extr_trees      one wavefront per kExtrTrees consecutive selected trees: runs of trees whose rows fit kExtrCap are staged in LDS
//                     from tree_rows (ordered by (start, row) inside a tree, so siblings already stand in their order): parent slot by
//                     search in the tree's slice, subtree sizes added up the levels (deepest first, LDS integer adds), pre-order index
//                     down the levels (pre[c] = pre[p] + 1 + the subtrees of the siblings staged before c), the inverse permutation,
//                     then one coalesced write per output column.  A tree of more than kExtrCap rows is taken by the wavefront alone
//                     on tables in global memory (the same code, an agent-scope fence between its phases); there the parent's slot
//                     comes from a row-indexed table instead of a search.  Cost of that route: rows x (preceding rows) / 64 for the
//                     sibling sums plus depth x rows / 64 for the two sweeps over the levels.
//
// Every output is a pure function of the inputs: integers only; the atomics are integer adds of which only the sum is read and a
// cursor that hands out scratch space (where a large tree's tables lie, never what they hold).
#pragma once
#include "tw_filt.h"

namespace tw {

#ifdef TW_TILE_SMALL   // the tiny values of the tests' host build: the packed route and the single-tree route both occur
constexpr int kExtrTrees = 4;
constexpr int kExtrCap = 12;
#else
constexpr int kExtrTrees = 16;       // consecutive selected trees a wavefront takes together
constexpr int kExtrCap = 256;        // rows a wavefront stages in LDS (28 B each: 28 KiB per workgroup of four)
#endif
constexpr int kExtrWaves = 4;
constexpr int kExtrMaxProbs = 32;
// counters: [0] eligible trees, [1] rows of the selected trees, [2] rows of the largest, [3] trees / [4] rows of the single-tree
// route, [5] scratch cursor, [6] error, [8 .. 12) the counters of k_attr_flags
constexpr int kExtrCounters = 16, kExtrAttrAt = 8;

struct ExtrDev {
    // selection
    unsigned long long *key_a, *key_b;      // the sort of trees_by_latency
    int32_t *val_a, *val_b;
    unsigned long long *chunk_sum, *counters;
    // tables of the trees beyond kExtrCap (big_cap rows, handed out by counters[5]) and the slot of a row in them
    int64_t big_cap;
    int32_t *g_row, *g_lnk, *g_par, *g_dep, *g_sub, *g_pre;
    int32_t* pos;                           // [n_rows]
    // what is resident besides the forest (null: not resident)
    const int32_t* row_group;
    const int64_t *self_time, *path_time;
    // the result
    int32_t *sel_tree, *sel_root;
    int64_t *sel_latency, *sel_start;
    uint8_t* sel_flags;
    int64_t* out_off;
    int32_t *row, *parent, *depth, *subtree, *group;
    uint8_t* kind;
    int64_t *start, *end, *self, *path;
};

// order 0: the eligible trees in ascending order, the first `cap` of them into sel_tree
struct ExtrSelScan {
    StitchDev S;
    ExtrDev X;
    uint32_t need_flags, skip_flags;
    int64_t cap;
    __device__ __forceinline__ unsigned long long packed(int64_t t) const {
        const uint32_t f = S.tree_flags[t];
        return ((f & need_flags) == need_flags && (f & skip_flags) == 0) ? 1ull : 0ull;
    }
    __device__ __forceinline__ unsigned long long* chunks() const { return X.chunk_sum; }
    __device__ __forceinline__ void total(unsigned long long run) const { X.counters[0] = run; }
    __device__ __forceinline__ void emit(int64_t t, unsigned long long run) const {
        if ((int64_t)run < cap) X.sel_tree[run] = (int32_t)t;
    }
};

// out_off: output tree j begins at the rows of the selected trees before it (every tree has a row: no item counts 0)
struct ExtrOffScan {
    StitchDev S;
    ExtrDev X;
    __device__ __forceinline__ unsigned long long packed(int64_t j) const {
        const int32_t t = X.sel_tree[j];
        return (unsigned long long)(S.tree_off[t + 1] - S.tree_off[t]);
    }
    __device__ __forceinline__ unsigned long long* chunks() const { return X.chunk_sum; }
    __device__ __forceinline__ void total(unsigned long long run) const { X.counters[1] = run; }
    __device__ __forceinline__ void emit(int64_t j, unsigned long long run) const { X.out_off[j] = (int64_t)run; }
};

// Slowest first from the ascending order val_b[0 .. n): entry i is the one at p = n - 1 - i, except that a run of equal latencies
// [lo, hi] is read forwards again (key (latency descending, tree ascending)).
__global__ void __launch_bounds__(256) k_extr_slowest(ExtrDev X, int64_t n, int64_t n_sel) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_sel) return;
    const int64_t p = n - 1 - i;
    const unsigned long long key = X.key_b[p];
    int64_t a = 0, b = p;   // lo: the first position that holds key
    while (a < b) {
        const int64_t mid = a + (b - a) / 2;
        if (X.key_b[mid] < key) a = mid + 1; else b = mid;
    }
    const int64_t lo = a;
    a = p; b = n - 1;       // hi: the last one
    while (a < b) {
        const int64_t mid = a + (b - a + 1) / 2;
        if (X.key_b[mid] > key) b = mid - 1; else a = mid;
    }
    X.sel_tree[i] = X.val_b[lo + (a - p)];
}

struct ExtrPick {
    int32_t n;
    int64_t at[kExtrMaxProbs];
};
__global__ void __launch_bounds__(256) k_extr_pick(ExtrDev X, ExtrPick P) {
    for (int j = threadIdx.x; j < P.n; j += blockDim.x) X.sel_tree[j] = X.val_b[P.at[j]];
}

__global__ void __launch_bounds__(256) k_extr_sizes(StitchDev S, ExtrDev X, int64_t n_sel) {
    const int nl = (int)stitch_min(blockDim.x, 64);
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long m = 0;
    if (j < n_sel) {
        const int32_t t = X.sel_tree[j];
        const int32_t R = S.tree_root[t];
        X.sel_root[j] = R;
        X.sel_latency[j] = S.tree_latency[t];
        X.sel_start[j] = S.row_start[R];
        X.sel_flags[j] = S.tree_flags[t];
        m = (unsigned long long)(S.tree_off[t + 1] - S.tree_off[t]);
    }
    const bool big = m > (unsigned long long)kExtrCap;
    const unsigned long long nb = (unsigned long long)__popcll(__ballot(big));
    unsigned long long mx = m, rows = dist_wave_sum(big ? m : 0ull, nl);
    for (int o = 32; o >= 1; o >>= 1)
        if (o < nl) mx = dist_umax(mx, (unsigned long long)__shfl_xor((long long)mx, o));
    if ((threadIdx.x & 63) == 0) {
        if (mx != 0) atomicMax(&X.counters[2], mx);
        if (nb != 0) { atomicAdd(&X.counters[3], nb); atomicAdd(&X.counters[4], rows); }
    }
}

// The tables of one wavefront, by staged position: the row, the row it links to (later: the staged position of a pre-order index),
// the parent's position, the depth, the subtree's rows, the pre-order index, the tree's slot (null for a single tree).
struct ExtrTab {
    int32_t *row, *lnk, *par, *dep, *sub, *pre, *tr;
};

// Selected trees t0 .. t1 - 1 of the wavefront's slots (off: where their rows begin in the output, src: in tree_rows) on the tables T.
template <bool kGlobal>
__device__ void extr_trees(const StitchDev& S, const ExtrDev& X, const ExtrTab& T, const int64_t* off, const int64_t* src, int t0, int t1, int lane,
                           int nl) {
    const int64_t a = off[t0];
    const int m = (int)(off[t1] - a);
    // 1. the rows in the order of tree_rows
    int maxd = 0;
    {
        int t = t0;   // a lane's positions ascend, so its tree only moves forward
        for (int k = lane; k < m; k += nl) {
            while (t + 1 < t1 && off[t + 1] - a <= k) t++;
            const int32_t r = S.tree_rows[src[t] + (k - (int)(off[t] - a))];
            const int32_t d = S.depth[r];
            T.row[k] = r;
            T.lnk[k] = S.link[r];
            T.dep[k] = d;
            T.sub[k] = 1;
            T.pre[k] = 0;
            if (T.tr != nullptr) T.tr[k] = t;
            if (kGlobal) X.pos[r] = k;
            maxd = d > maxd ? d : maxd;
        }
    }
    for (int o = 32; o >= 1; o >>= 1)
        if (o < nl) { const int other = __shfl_xor(maxd, o); maxd = other > maxd ? other : maxd; }
    maxd = maxd < m ? maxd : m;   // (a tree is deeper than it has rows only where the forest is not the stitch's)
    attr_sync<kGlobal>();
#define EXTR_RANGE(k, lo, hi)                                   \
    const int ts_ = T.tr != nullptr ? T.tr[k] : t0;             \
    const int lo = (int)(off[ts_] - a), hi = (int)(off[ts_ + 1] - a)
    // 2. position of the parent: by search in the tree's slice, or (a large tree) from the table the rows wrote their positions to
    for (int k = lane; k < m; k += nl) {
        EXTR_RANGE(k, lo, hi);
        const int32_t l = T.lnk[k];
        int p = -1;
        if (l >= 0) {
            if (kGlobal) {
                const int q = X.pos[l];
                if (q >= lo && q < hi && T.row[q] == l) p = q;
            } else {
                for (int j = lo; j < hi; j++)
                    if (T.row[j] == l) { p = j; break; }
            }
            if (p < 0) X.counters[6] = 1;   // a row linked to a row of another tree: not a forest the stitch left behind
        }
        T.par[k] = p;
    }
    attr_sync<kGlobal>();
    // 3. subtree sizes, the deepest level first: a row's own count is complete when its level is reached
    for (int d = maxd; d >= 1; d--) {
        for (int k = lane; k < m; k += nl)
            if (T.dep[k] == d && T.par[k] >= 0) atomicAdd(&T.sub[T.par[k]], T.sub[k]);
        attr_sync<kGlobal>();
    }
    // 4. pre-order index down the levels: the parent's, 1, and the subtrees of the siblings staged before the row
    for (int d = 1; d <= maxd; d++) {
        for (int k = lane; k < m; k += nl) {
            if (T.dep[k] != d) continue;
            const int p = T.par[k];
            if (p < 0) continue;
            int before = 0;
            EXTR_RANGE(k, lo, hi);
            (void)hi;
            for (int s = lo; s < k; s++)
                if (T.par[s] == p) before += T.sub[s];
            T.pre[k] = T.pre[p] + 1 + before;
        }
        attr_sync<kGlobal>();
    }
    // 5. the inverse permutation: which staged position a place of the output reads
    for (int k = lane; k < m; k += nl) T.lnk[k] = -1;
    attr_sync<kGlobal>();
    for (int k = lane; k < m; k += nl) {
        EXTR_RANGE(k, lo, hi);
        const int q = T.pre[k];
        if (q < 0 || q >= hi - lo) { X.counters[6] = 1; continue; }
        T.lnk[lo + q] = k;
    }
    attr_sync<kGlobal>();
    // 6. the columns, one after another: consecutive lanes write consecutive places
    for (int q = lane; q < m; q += nl) {
        const int k = T.lnk[q];
        if (k < 0) { X.counters[6] = 1; continue; }
        const int p = T.par[k];
        X.row[a + q] = T.row[k];
        X.parent[a + q] = p < 0 ? -1 : T.pre[p];
        X.depth[a + q] = T.dep[k];
        X.subtree[a + q] = T.sub[k];
    }
    for (int q = lane; q < m; q += nl) {
        const int k = T.lnk[q];
        if (k < 0) continue;
        const int32_t r = T.row[k];
        X.kind[a + q] = S.row_kind[r];
        X.group[a + q] = X.row_group != nullptr ? X.row_group[r] : -1;
        X.start[a + q] = S.row_start[r];
        X.end[a + q] = S.row_end[r];
        if (X.self_time != nullptr) {
            X.self[a + q] = X.self_time[r];
            X.path[a + q] = X.path_time[r];
        }
    }
    attr_sync<kGlobal>();   // ... before the next trees overwrite the tables
#undef EXTR_RANGE
}

__global__ void __launch_bounds__(64 * kExtrWaves) k_extr_trees(StitchDev S, ExtrDev X, int64_t n_sel) {
    __shared__ int32_t s_tab[kExtrWaves][7][kExtrCap];
    __shared__ int64_t s_off[kExtrWaves][kExtrTrees + 1];
    __shared__ int64_t s_src[kExtrWaves][kExtrTrees];
    const int nl = (int)stitch_min(blockDim.x, 64), lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const int wpb = (int)stitch_max(blockDim.x / 64, 1);
    int64_t* off = s_off[wave];
    int64_t* src = s_src[wave];
    ExtrTab L;
    L.row = s_tab[wave][0]; L.lnk = s_tab[wave][1]; L.par = s_tab[wave][2]; L.dep = s_tab[wave][3]; L.sub = s_tab[wave][4];
    L.pre = s_tab[wave][5]; L.tr = s_tab[wave][6];
    const int64_t n_chunks = (n_sel + kExtrTrees - 1) / kExtrTrees;
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < n_chunks; c += (int64_t)gridDim.x * wpb) {
        const int64_t j0 = c * kExtrTrees;
        const int nt = (int)stitch_min((int64_t)kExtrTrees, n_sel - j0);
        for (int t = lane; t <= nt; t += nl) {
            off[t] = X.out_off[j0 + t];
            if (t < nt) src[t] = S.tree_off[X.sel_tree[j0 + t]];
        }
        stitch_wave_sync();
        // runs of trees whose rows fit the tables together, a larger tree alone
        for (int t0 = 0; t0 < nt;) {
            const int64_t n = off[t0 + 1] - off[t0];
            if (n > kExtrCap) {
                unsigned long long at = 0;
                if (lane == 0) at = atomicAdd(&X.counters[5], (unsigned long long)n);
                at = (unsigned long long)__shfl((long long)at, 0);
                if ((int64_t)at + n > X.big_cap) {   // (the host sized the tables by counters[4])
                    X.counters[6] = 2;
                } else {
                    ExtrTab G;
                    G.row = X.g_row + at; G.lnk = X.g_lnk + at; G.par = X.g_par + at; G.dep = X.g_dep + at; G.sub = X.g_sub + at;
                    G.pre = X.g_pre + at; G.tr = nullptr;
                    extr_trees<true>(S, X, G, off, src, t0, t0 + 1, lane, nl);
                }
                t0++;
                continue;
            }
            int t1 = t0 + 1;
            while (t1 < nt && off[t1 + 1] - off[t0] <= kExtrCap) t1++;
            extr_trees<false>(S, X, L, off, src, t0, t1, lane, nl);
            t0 = t1;
        }
        stitch_wave_sync();   // ... before the next trees overwrite the slots
    }
}

}  // namespace tw

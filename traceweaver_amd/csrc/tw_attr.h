// tw_attr.h -- latency attribution on the stitched forest (tw_set_row_groups / tw_attribute_traces).
//
// Replaces: the consumer of reconstructed traces, src/query_engine/delay_culprit.py:19-28 (the question: of the end-to-end
// requests in the top X %ile latency bracket that started after time Y, which service performs worst and what is its mean
// service latency) and :30-97 (its walk over every trace on the host).  It works on what the last tw_stitch_traces left on
// the device: the link table (StitchDev::link), the row intervals, the CSR grouping and the per-tree figures.
//
// Definitions (integer microseconds throughout; a row with end < start counts as end = start):
//   self_time[p]  (end_p - start_p) less the measure of the union of p's children's intervals clipped to p's
//   path_time[p]  p's share of its tree's critical path: walk(p, lo, hi) sweeps a cursor from hi to the left; the child with the
//                 greatest ce = min(end_c, cursor) among those with cs = max(start_c, lo) < cursor and end_c > cs (ties: smaller
//                 cs, then smaller row) is walked with [cs, ce], the gap cursor - ce is p's own, the cursor moves to cs; what
//                 is left when no child qualifies, cursor - lo, is p's own too.  The root is walked with its own interval, so
//                 the path times of a tree sum to the root's duration.  Rows never walked have 0.
//
//   k_attr_flags   per tree: eligible by its flags?  sort key (latency, sign bit flipped; ~0 when not eligible), the count of
//                  eligible trees and the rows of the trees that outgrow a wavefront's LDS tables
//   (rocprim::radix_sort_pairs, stable: eligible trees in order of (latency, tree))
//   k_attr_mark    rank >= k and root start inside the window -> tree_selected
//   k_attr_tree    one wavefront per kAttrTrees consecutive trees whose rows fit its LDS tables (a larger tree alone; one of more
//                  than kAttrCap rows on tables in global memory -- the same code, an agent-scope fence between its phases):
//                    parent position of every row (search in the tree), rank sort by (parent, end descending, start, row): a
//                    row's children are a contiguous run, latest end first; self times, one lane per parent, one sweep over the
//                    run; the walk level by level -- every row that got a window in round i is walked in round i + 1, lanes
//                    spread over rows; per-tree group sums by comparison inside the tree (no atomics: the wavefront owns the tree)
//   k_attr_reduce  per row of a selected tree: the seven per-group totals, added up in LDS per workgroup first (n_groups <=
//                  kAttrGroupsLds), then one 64-bit integer atomicAdd per workgroup and nonzero cell
//
// Every output is a pure function of the inputs: no floating point; the atomics are integer adds whose sum alone is read, and a
// cursor that hands out scratch space (where a large tree's tables lie, never what they hold).
#pragma once
#include "tw_stitch.h"

namespace tw {

#ifdef TW_TILE_SMALL   // the tiny tables of the tests' host build: the packed, the single-tree and the global-memory route all occur
constexpr int kAttrCap = 12;
constexpr int kAttrTrees = 4;
constexpr int kAttrGroupsLds = 4;
#else
constexpr int kAttrCap = 256;        // rows a wavefront holds in LDS (56 B each, 56 KiB per workgroup of four: two workgroups per CU)
constexpr int kAttrTrees = 16;       // consecutive trees a wavefront takes together when their rows fit
constexpr int kAttrGroupsLds = 512;  // groups whose seven totals a workgroup of k_attr_reduce keeps in LDS (28 KiB)
#endif
constexpr int kAttrWaves = 4;
constexpr int kAttrCols = 7;         // path_time, path_rows, self_time, span_time, span_rows, trees, top_trees

struct AttrDev {
    int32_t n_groups;
    const int32_t* row_group;        // [n_rows] group of every row, -1 = not counted
    // per row
    int64_t *self_time, *path_time;
    int32_t* row_tree;               // tree number of the row
    uint8_t* row_flag;               // bit 0 on the critical path, bit 1 the first such row of its group in its tree
    // per tree
    int32_t *tree_top, *tree_path_rows;
    uint8_t* tree_sel;
    unsigned long long *key_a, *key_b;
    int32_t *val_a, *val_b;
    // per group
    unsigned long long* totals;      // [kAttrCols][n_groups]
    unsigned long long* counters;    // [0] eligible trees, [1] rows of trees beyond kAttrCap, [2] selected trees, [3] scratch cursor
    int32_t* err;
    // tables of the trees beyond kAttrCap (big_cap rows, handed out by counters[3])
    int64_t big_cap;
    int64_t *g_s, *g_e, *g_s2, *g_e2;
    int32_t *g_row, *g_par, *g_rank, *g_row2, *g_par2;
};

struct AttrQueryDev {
    int64_t start_min, start_max, k;
    uint32_t need_flags, skip_flags;
};

// The tables of one wavefront.  Before the sort: row, s, e, par, rank by position in tree_rows; after it row2, s2, e2, par2 by
// sorted position, and the first five hold what the walk needs (see the aliases in attr_trees).  tr: tree (less t0) of a
// position, null for a single tree.
struct AttrTab {
    int64_t *s, *e, *s2, *e2;
    int32_t *row, *par, *rank, *row2, *par2, *tr;
};

__global__ void __launch_bounds__(256) k_attr_flags(StitchDev S, AttrDev A, AttrQueryDev Q, int64_t n_trees) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool elig = false;
    int64_t big = 0;
    if (t < n_trees) {
        const uint32_t f = S.tree_flags[t];
        elig = (f & Q.need_flags) == Q.need_flags && (f & Q.skip_flags) == 0;
        A.key_a[t] = elig ? ((unsigned long long)S.tree_latency[t] ^ (1ull << 63)) : ~0ull;
        A.val_a[t] = (int32_t)t;
        const int64_t m = S.tree_off[t + 1] - S.tree_off[t];
        if (m > kAttrCap) big = m;
    }
    const unsigned long long any = __ballot(elig);
    if (any != 0 && (threadIdx.x & 63) == 0) atomicAdd(&A.counters[0], (unsigned long long)__popcll(any));
    if (big > 0) atomicAdd(&A.counters[1], (unsigned long long)big);
}

// q: position in the sorted order.  The eligible trees come first (the key of the others is the largest there is).
__global__ void __launch_bounds__(256) k_attr_mark(StitchDev S, AttrDev A, AttrQueryDev Q, int64_t n_trees, int64_t n_eligible) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool sel = false;
    if (q < n_trees) {
        const int32_t t = A.val_b[q];
        const int64_t start = S.row_start[S.tree_root[t]];
        sel = q < n_eligible && q >= Q.k && start >= Q.start_min && start < Q.start_max;
        A.tree_sel[t] = sel ? 1 : 0;
    }
    const unsigned long long any = __ballot(sel);
    if (any != 0 && (threadIdx.x & 63) == 0) atomicAdd(&A.counters[2], (unsigned long long)__popcll(any));
}

template <bool kGlobal>
__device__ __forceinline__ void attr_sync() {
    if (kGlobal) {   // the tables lie in global memory: what a lane stored must have reached L2 before another lane loads it
        __threadfence();
        __builtin_amdgcn_wave_barrier();
        __threadfence();
    } else {
        stitch_wave_sync();
    }
}

// Trees t0 .. t1 - 1, whose m rows start at tree_rows[a], on the tables T.
template <bool kGlobal>
__device__ void attr_trees(const StitchDev& S, const AttrDev& A, const AttrTab& T, int64_t t0, int64_t t1, int64_t a, int m, int lane, int nl) {
#define ATTR_RANGE(k, t, lo, hi)                                                     \
    const int64_t t = t0 + (T.tr != nullptr ? T.tr[k] : 0);                          \
    const int lo = (int)(S.tree_off[t] - a), hi = (int)(S.tree_off[t + 1] - a)
    // 1. the rows; rank holds the row linked to until the parent's position is known
    for (int k = lane; k < m; k += nl) {
        const int32_t r = S.tree_rows[a + k];
        const int64_t s = S.row_start[r];
        T.row[k] = r;
        T.s[k] = s;
        T.e[k] = stitch_max(S.row_end[r], s);
        T.rank[k] = S.link[r];
        if (T.tr != nullptr) {
            int64_t t = t0;
            while (t + 1 < t1 && S.tree_off[t + 1] <= a + k) t++;
            T.tr[k] = (int32_t)(t - t0);
        }
    }
    attr_sync<kGlobal>();
    // 2. position of the parent
    for (int k = lane; k < m; k += nl) {
        ATTR_RANGE(k, t, lo, hi);
        const int32_t l = T.rank[k];
        int p = -1;
        if (l >= 0) {
            for (int j = lo; j < hi; j++)
                if (T.row[j] == l) { p = j; break; }
            if (p < 0) *A.err = TW_ERR_ARG;   // a row linked to a row of another tree: not a forest the stitch left behind
        } else if (T.row[k] != S.tree_root[t]) {
            *A.err = TW_ERR_ARG;
        }
        T.par[k] = p;
    }
    attr_sync<kGlobal>();
    // 3. rank by (parent, end descending, start, row)
    for (int k = lane; k < m; k += nl) {
        ATTR_RANGE(k, t, lo, hi);
        const int pk = T.par[k];
        const int64_t ek = T.e[k], sk = T.s[k];
        const int32_t rk = T.row[k];
        int rank = lo;
        for (int j = lo; j < hi; j++) {
            const int pj = T.par[j];
            const int64_t ej = T.e[j], sj = T.s[j];
            const bool before = pj != pk ? pj < pk : ej != ek ? ej > ek : sj != sk ? sj < sk : T.row[j] < rk;
            rank += before ? 1 : 0;
        }
        T.rank[k] = rank;
    }
    attr_sync<kGlobal>();
    // 4. the sorted tables
    for (int k = lane; k < m; k += nl) {
        const int j = T.rank[k], p = T.par[k];
        T.row2[j] = T.row[k];
        T.s2[j] = T.s[k];
        T.e2[j] = T.e[k];
        T.par2[j] = p < 0 ? -1 : T.rank[p];
    }
    attr_sync<kGlobal>();
    // 5. the unsorted tables make room: first child, round of the walk, window (lo, then the row's path time; hi, then its
    // group's sum), group
    int32_t *cfirst = T.par, *lvl = T.rank, *grp = T.row;
    int64_t *wlo = T.s, *whi = T.e;
    for (int j = lane; j < m; j += nl) {
        ATTR_RANGE(j, t, lo, hi);
        (void)lo; (void)hi;
        const int32_t r = T.row2[j];
        const bool root = r == S.tree_root[t];
        cfirst[j] = -1;
        lvl[j] = root ? 0 : -1;
        grp[j] = A.row_group[r];
        wlo[j] = T.s2[j];
        whi[j] = T.e2[j];
        A.row_tree[r] = (int32_t)t;
    }
    attr_sync<kGlobal>();
    for (int j = lane; j < m; j += nl) {
        ATTR_RANGE(j, t, lo, hi);
        (void)hi;
        const int p = T.par2[j];
        if (p >= 0 && (j == lo || T.par2[j - 1] != p)) cfirst[p] = j;
    }
    attr_sync<kGlobal>();
    // 6. self time: the children come latest end first, so what a child adds to the union lies below the lowest start so far
    for (int p = lane; p < m; p += nl) {
        ATTR_RANGE(p, t, lo, hi);
        (void)lo;
        const int64_t ps = T.s2[p], pe = T.e2[p];
        int64_t covered = 0, lowest = pe;
        const int c0 = cfirst[p];
        if (c0 >= 0)
            for (int c = c0; c < hi && T.par2[c] == p; c++) {
                const int64_t cs = stitch_max(T.s2[c], ps), ce = stitch_min(T.e2[c], pe);
                if (ce <= cs) continue;
                const int64_t top = stitch_min(ce, lowest);
                if (top > cs) covered += top - cs;
                lowest = stitch_min(lowest, cs);
            }
        A.self_time[T.row2[p]] = (pe - ps) - covered;
    }
    // 7. the walk: a row that got its window in round it - 1 (the root: its own interval) is walked in round it
    for (int it = 0;; it++) {
        bool marked = false;
        for (int p = lane; p < m; p += nl) {
            if (lvl[p] != it) continue;
            ATTR_RANGE(p, t, lo, hi);
            (void)lo;
            const int64_t wl = wlo[p];
            int64_t cursor = whi[p], own = 0;
            const int c0 = cfirst[p];
            while (c0 >= 0) {
                int best = -1;
                int64_t bce = 0, bcs = 0;
                for (int c = c0; c < hi && T.par2[c] == p; c++) {
                    const int64_t ec = T.e2[c];
                    if (best >= 0 && stitch_min(ec, cursor) < bce) break;   // ends descend: no later child reaches bce
                    const int64_t cs = stitch_max(T.s2[c], wl);
                    if (cs >= cursor || ec <= cs) continue;
                    const int64_t ce = stitch_min(ec, cursor);
                    if (best < 0 || ce > bce || (ce == bce && (cs < bcs || (cs == bcs && T.row2[c] < T.row2[best])))) { best = c; bce = ce; bcs = cs; }
                }
                if (best < 0) break;
                own += cursor - bce;
                lvl[best] = it + 1;
                wlo[best] = bcs;
                whi[best] = bce;
                cursor = bcs;
                marked = true;
            }
            wlo[p] = own + (cursor - wl);
        }
        attr_sync<kGlobal>();
        if (__ballot(marked) == 0) break;
        if (it > m) { *A.err = TW_ERR_ARG; break; }   // (more rounds than rows: not a forest)
    }
    // 8. path times; whi makes room for the group sums
    for (int j = lane; j < m; j += nl) {
        const int64_t pt = lvl[j] >= 0 ? wlo[j] : 0;
        wlo[j] = pt;
        A.path_time[T.row2[j]] = pt;
    }
    attr_sync<kGlobal>();
    // 9. per counted row on the path: the path time of its group in its tree
    for (int j = lane; j < m; j += nl) {
        ATTR_RANGE(j, t, lo, hi);
        (void)t;
        const int32_t g = grp[j];
        const bool on = lvl[j] >= 0;
        bool first = on;
        int64_t sum = 0;
        if (on && g >= 0)
            for (int i = lo; i < hi; i++)
                if (lvl[i] >= 0 && grp[i] == g) { sum += wlo[i]; if (i < j) first = false; }
        whi[j] = sum;
        A.row_flag[T.row2[j]] = (uint8_t)((on ? 1 : 0) | (first && g >= 0 ? 2 : 0));
    }
    attr_sync<kGlobal>();
    // 10. per tree: rows on the path, the group with the largest sum (ties: the smallest id)
    for (int64_t t = t0 + lane; t < t1; t += nl) {
        const int lo = (int)(S.tree_off[t] - a), hi = (int)(S.tree_off[t + 1] - a);
        int32_t top = -1, rows = 0;
        int64_t best = 0;
        for (int j = lo; j < hi; j++) {
            if (lvl[j] < 0) continue;
            rows++;
            const int32_t g = grp[j];
            if (g >= 0 && (top < 0 || whi[j] > best || (whi[j] == best && g < top))) { top = g; best = whi[j]; }
        }
        A.tree_top[t] = top;
        A.tree_path_rows[t] = rows;
    }
    attr_sync<kGlobal>();   // ... before the next trees overwrite the tables
#undef ATTR_RANGE
}

__global__ void __launch_bounds__(64 * kAttrWaves) k_attr_tree(StitchDev S, AttrDev A, int64_t n_trees) {
    __shared__ int64_t s_i64[kAttrWaves][4][kAttrCap];
    __shared__ int32_t s_i32[kAttrWaves][6][kAttrCap];
    const int nl = (int)stitch_min(blockDim.x, 64), lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const int wpb = (int)stitch_max(blockDim.x / 64, 1);
    AttrTab L;
    L.s = s_i64[wave][0]; L.e = s_i64[wave][1]; L.s2 = s_i64[wave][2]; L.e2 = s_i64[wave][3];
    L.row = s_i32[wave][0]; L.par = s_i32[wave][1]; L.rank = s_i32[wave][2]; L.row2 = s_i32[wave][3]; L.par2 = s_i32[wave][4]; L.tr = s_i32[wave][5];
    const int64_t n_chunks = (n_trees + kAttrTrees - 1) / kAttrTrees;
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < n_chunks; c += (int64_t)gridDim.x * wpb) {
        const int64_t c0 = c * kAttrTrees, c1 = stitch_min(c0 + kAttrTrees, n_trees);
        const bool packed = S.tree_off[c1] - S.tree_off[c0] <= kAttrCap;
        for (int64_t t0 = c0; t0 < c1; t0 = packed ? c1 : t0 + 1) {
            const int64_t t1 = packed ? c1 : t0 + 1;
            const int64_t a = S.tree_off[t0], n = S.tree_off[t1] - a;
            if (n <= kAttrCap) {
                attr_trees<false>(S, A, L, t0, t1, a, (int)n, lane, nl);
            } else {
                unsigned long long at = 0;
                if (lane == 0) at = atomicAdd(&A.counters[3], (unsigned long long)n);
                at = (unsigned long long)__shfl((long long)at, 0);
                if ((int64_t)at + n > A.big_cap) { *A.err = TW_ERR_DEVICE; continue; }   // (the host sized the tables by counters[1])
                AttrTab G;
                G.s = A.g_s + at; G.e = A.g_e + at; G.s2 = A.g_s2 + at; G.e2 = A.g_e2 + at;
                G.row = A.g_row + at; G.par = A.g_par + at; G.rank = A.g_rank + at; G.row2 = A.g_row2 + at; G.par2 = A.g_par2 + at; G.tr = nullptr;
                attr_trees<true>(S, A, G, t0, t1, a, (int)n, lane, nl);
            }
        }
    }
}

// One thread per row: a selected tree's row adds to its group's totals; the tree's root adds the tree to its top group's.
__global__ void __launch_bounds__(256) k_attr_reduce(StitchDev S, AttrDev A) {
    __shared__ unsigned long long acc[kAttrCols * kAttrGroupsLds];
    const int G = A.n_groups;
    const bool lds = G <= kAttrGroupsLds;
    if (lds) {
        for (int q = threadIdx.x; q < kAttrCols * G; q += blockDim.x) acc[q] = 0;
        __syncthreads();
    }
    unsigned long long* dst = lds ? acc : A.totals;
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < S.n_rows) {
        const int32_t t = A.row_tree[r];
        if (A.tree_sel[t] != 0) {
            const int32_t g = A.row_group[r];
            if (g >= 0) {
                const uint8_t f = A.row_flag[r];
                const int64_t s = S.row_start[r], d = stitch_max(S.row_end[r], s) - s;
                if (f & 1) {
                    const int64_t pt = A.path_time[r];
                    if (pt != 0) atomicAdd(&dst[0 * G + g], (unsigned long long)pt);
                    atomicAdd(&dst[1 * G + g], 1ull);
                }
                const int64_t st = A.self_time[r];
                if (st != 0) atomicAdd(&dst[2 * G + g], (unsigned long long)st);
                if (d != 0) atomicAdd(&dst[3 * G + g], (unsigned long long)d);
                atomicAdd(&dst[4 * G + g], 1ull);
                if (f & 2) atomicAdd(&dst[5 * G + g], 1ull);
            }
            if (S.tree_root[t] == (int32_t)r) {
                const int32_t top = A.tree_top[t];
                if (top >= 0) atomicAdd(&dst[6 * G + top], 1ull);
            }
        }
    }
    if (lds) {
        __syncthreads();
        for (int q = threadIdx.x; q < kAttrCols * G; q += blockDim.x)
            if (acc[q] != 0) atomicAdd(&A.totals[q], acc[q]);
    }
}

}  // namespace tw

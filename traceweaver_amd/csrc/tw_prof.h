// tw_prof.h -- per-class latency profiles: the aggregate trace of every call-graph class (tw_class_profiles).
//
// Replaces: PreparePerCGData of the reference (alibaba-analysis/analysis.py:233-292), which takes the traces of one call graph at a
// time and collects per call the delays behind it.  tw_trace_signatures says what the traces look like, tw_attribute_traces where
// every row spends its time; this joins the two: per class and entry (level, caller, service) of its signature, over the selected
// trees of the class, how many rows, how long, how much of it on the critical path, and where in the trace the entry begins.  It
// works on what the two calls left on the device: the forest (CSR grouping, row intervals, tree latencies), tree_class, class_off
// and class_entries of the signature result, tree_sel, self_time, path_time and row_flag of the attribution.
// include/traceweaver_amd.h has the definitions.
//
//   k_prof_clear      the cells (0, and the identities of min / max), the per-class sums and the (tree, entry) marks
//   k_prof_rows       one lane per position of tree_rows (the coalesced sweep of k_sig_items; the row's columns are gathered): the
//                     row's item key again (sig_item_key), its tree's class and selection, the entry by binary search over the class'
//                     entries.  Consecutive trees mostly share a class, so the lanes of a wavefront meet on a few cells: one round per
//                     distinct entry among the live lanes (__shfl of the first live lane's entry, __ballot of the matches, __popcll for
//                     the counts, shuffle reductions for the sums, the minimum and the maximum), after which one lane adds once per
//                     cell and wavefront -- into an LDS table per workgroup while the entries fit it (kProfCells), which is cleared once
//                     and added to global memory once per workgroup and filled cell; beyond the table straight onto the global cells.
//                     path_trees: entry j of tree t owns the mark seen[tree_off[t] + j] (a tree has at least as many rows as its class
//                     has entries); a path row exchanges 1 into it and the lane that read 0 counts the tree -- which lane that is
//                     depends on scheduling, the count does not.
//   k_prof_trees      one lane per tree: counted (class >= 0 and selected)?  class_counted and class_latency with the same rounds per
//                     distinct class, through an LDS table while the classes fit it (kProfClassCells); the three tree counts of the
//                     summary, kept per wavefront and added once
//   k_prof_classes    one lane per class over its entries: class_path_time, class_top_entry; classes with a counted tree and entries
//                     with a row for the summary
//
// Every output is a pure function of the inputs: no floating point; the atomics are integer adds, minima, maxima and exchanges of
// which only the result described above is read.
#pragma once
#include "tw_sig.h"

// Entries whose nine cells a workgroup of k_prof_rows keeps in LDS (72 B each: 36 KiB, four workgroups per CU).  The tests' host
// build takes the tiny value, so that the LDS and the global route both occur there; traces.PROFILE_TABLE_CELLS mirrors the first.
#define TW_PROF_TABLE_CELLS 512
#define TW_PROF_TABLE_CELLS_SMALL 8

namespace tw {

#ifdef TW_TILE_SMALL
constexpr int kProfCells = TW_PROF_TABLE_CELLS_SMALL;
constexpr int kProfClassCells = 4;
#else
constexpr int kProfCells = TW_PROF_TABLE_CELLS;
constexpr int kProfClassCells = 256;   // classes whose counted trees and latency sum a workgroup of k_prof_trees keeps in LDS (4 KiB)
#endif
constexpr int kProfCols = 9;         // rows, span_time, span_min, span_max, self_time, path_time, path_rows, path_trees, offset
constexpr int kProfMin = 2, kProfMax = 3;
constexpr int kProfCounters = 6;     // summary6: counted trees, classes with one, counted item rows, entries with a row, classed trees
                                     // that are not selected, selected trees without a class

struct ProfDev {
    int64_t n_entries, n_classes;
    unsigned long long* cells;       // [kProfCols][n_entries] (sums in two's complement, min / max as signed values)
    uint32_t* seen;                  // [n_rows] marks of the (tree, entry) pairs with a row on the path
    int64_t *class_counted, *class_latency, *class_path_time, *class_top;   // [n_classes]
    unsigned long long* counters;    // [kProfCounters]
};

__device__ __forceinline__ unsigned long long prof_identity(int col) {
    return col == kProfMin ? (unsigned long long)INT64_MAX : col == kProfMax ? (unsigned long long)INT64_MIN : 0ull;
}

__global__ void __launch_bounds__(256) k_prof_clear(StitchDev S, ProfDev P) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < kProfCols * P.n_entries) P.cells[q] = prof_identity((int)(q / P.n_entries));
    if (q < S.n_rows) P.seen[q] = 0;
    if (q < P.n_classes) { P.class_counted[q] = 0; P.class_latency[q] = 0; }
}

// The least / the greatest v over the lanes of a wavefront, in every lane (nl: lanes of the wavefront, a power of two).
__device__ __forceinline__ long long prof_wave_min(long long v, int nl) {
    for (int off = 32; off >= 1; off >>= 1)
        if (off < nl) { const long long o = __shfl_xor(v, off); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ long long prof_wave_max(long long v, int nl) {
    for (int off = 32; off >= 1; off >>= 1)
        if (off < nl) { const long long o = __shfl_xor(v, off); v = o > v ? o : v; }
    return v;
}

// entry e (level, caller group, group, count) of class_entries as the key its items have
__device__ __forceinline__ unsigned long long prof_entry_key(const SigDev& G, int64_t e) {
    const int32_t* x = G.class_entries + 4 * e;
    return sig_pack(x[0], G.mode == 1 ? (unsigned long long)(x[1] + 1) : 1ull, x[2]);
}

// Workgroups stride over the positions, so that the LDS table is cleared and added to global memory once per workgroup.
__global__ void __launch_bounds__(256) k_prof_rows(StitchDev S, AttrDev A, SigDev G, ProfDev P) {
    __shared__ unsigned long long acc[kProfCols * kProfCells];
    const bool lds = P.n_entries <= kProfCells;
    const int64_t ne = P.n_entries;   // the stride between the columns, of the table as of the global cells
    if (lds) {
        for (int q = threadIdx.x; q < kProfCols * (int)ne; q += blockDim.x) acc[q] = prof_identity(q / (int)ne);
        __syncthreads();
    }
    unsigned long long* dst = lds ? acc : P.cells;
    const int nl = (int)stitch_min(blockDim.x, 64), lane = threadIdx.x % 64;
    unsigned long long w_rows = 0;   // the same in every lane of a wavefront
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < S.n_rows; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = base + threadIdx.x;
        bool has = false, on = false, first = false;
        int32_t i = -1;   // the global entry index (entries < 2^32 by the packed scan, <= rows < 2^31)
        int64_t d = 0, st = 0, pt = 0, off = 0;
        if (k < S.n_rows) {
            const int32_t r = S.tree_rows[k];
            const int32_t t = A.row_tree[r];
            const int32_t c = G.tree_class[t];
            if (c >= 0 && A.tree_sel[t] != 0) {
                int32_t level;
                bool deep;
                const unsigned long long key = sig_item_key(S, G, r, level, deep);
                if (key != kSigNone) {
                    const int64_t a = G.class_off[c], b = G.class_off[c + 1];
                    int64_t lo = a, hi = b;   // the first entry whose key is not below the row's
                    while (lo < hi) {
                        const int64_t mid = lo + (hi - lo) / 2;
                        if (prof_entry_key(G, mid) < key) lo = mid + 1;
                        else hi = mid;
                    }
                    const int64_t mark = S.tree_off[t] + (lo - a);
                    // (t's signature is its class': the entry exists, and a tree has no fewer rows than entries)
                    if (lo < b && prof_entry_key(G, lo) == key && mark < S.tree_off[t + 1]) {
                        has = true;
                        i = (int32_t)lo;
                        const int64_t s = S.row_start[r];
                        d = stitch_max(S.row_end[r], s) - s;
                        st = A.self_time[r];
                        off = s - S.row_start[S.tree_root[t]];
                        on = (A.row_flag[r] & 1) != 0;
                        if (on) {
                            pt = A.path_time[r];
                            first = atomicExch(&P.seen[mark], 1u) == 0u;
                        }
                    }
                }
            }
        }
        // one round per distinct entry among the lanes; the control flow is the same in every lane
        unsigned long long todo = __ballot(has);
        w_rows += (unsigned long long)__popcll(todo);
        while (todo != 0) {
            const int leader = __ffsll((long long)todo) - 1;
            const int32_t cell = __shfl(i, leader);
            const bool mine = has && i == cell;
            const unsigned long long m = __ballot(mine), m2 = __ballot(mine && on), m3 = __ballot(mine && first);
            todo &= ~m;
            unsigned long long sd = mine ? (unsigned long long)d : 0ull, ss = mine ? (unsigned long long)st : 0ull;
            unsigned long long sp = mine && on ? (unsigned long long)pt : 0ull, so = mine ? (unsigned long long)off : 0ull;
            long long mn = mine ? (long long)d : INT64_MAX, mx = mine ? (long long)d : INT64_MIN;
            if (__popcll(m) > 1) {   // (a lane alone on its entry holds the figures already)
                sd = dist_wave_sum(sd, nl);
                ss = dist_wave_sum(ss, nl);
                so = dist_wave_sum(so, nl);
                if (m2 != 0) sp = dist_wave_sum(sp, nl);
                mn = prof_wave_min(mn, nl);
                mx = prof_wave_max(mx, nl);
            }
            if (lane == leader) {
                unsigned long long* x = dst + cell;
                atomicAdd(&x[0 * ne], (unsigned long long)__popcll(m));
                if (sd != 0) atomicAdd(&x[1 * ne], sd);
                atomicMin((long long*)&x[kProfMin * ne], mn);
                atomicMax((long long*)&x[kProfMax * ne], mx);
                if (ss != 0) atomicAdd(&x[4 * ne], ss);
                if (sp != 0) atomicAdd(&x[5 * ne], sp);
                if (m2 != 0) atomicAdd(&x[6 * ne], (unsigned long long)__popcll(m2));
                if (m3 != 0) atomicAdd(&x[7 * ne], (unsigned long long)__popcll(m3));
                if (so != 0) atomicAdd(&x[8 * ne], so);
            }
        }
    }
    if (lane == 0 && w_rows != 0) atomicAdd(&P.counters[2], w_rows);
    if (lds) {
        __syncthreads();
        for (int q = threadIdx.x; q < (int)ne; q += blockDim.x) {
            if (acc[q] == 0) continue;   // no row of this workgroup at the entry: its other cells hold their identities
            for (int col = 0; col < kProfCols; col++) {
                const unsigned long long v = acc[col * ne + q];
                if (col == kProfMin) atomicMin((long long*)&P.cells[col * ne + q], (long long)v);
                else if (col == kProfMax) atomicMax((long long*)&P.cells[col * ne + q], (long long)v);
                else if (v != 0) atomicAdd(&P.cells[col * ne + q], v);
            }
        }
    }
}

// Workgroups stride over the trees: the three counts are kept per wavefront and added once at the end, the per-class sums go through
// an LDS table (cleared once, added to global memory once per workgroup and filled cell) while the classes fit it.
__global__ void __launch_bounds__(256) k_prof_trees(StitchDev S, AttrDev A, SigDev G, ProfDev P, int64_t n_trees) {
    __shared__ unsigned long long acc[2 * kProfClassCells];
    const int64_t nc = P.n_classes;
    const bool lds = nc <= kProfClassCells;
    if (lds) {
        for (int q = threadIdx.x; q < 2 * (int)nc; q += blockDim.x) acc[q] = 0;
        __syncthreads();
    }
    unsigned long long* cnt = lds ? acc : (unsigned long long*)P.class_counted;
    unsigned long long* sum = lds ? acc + nc : (unsigned long long*)P.class_latency;
    const int nl = (int)stitch_min(blockDim.x, 64), lane = threadIdx.x % 64;
    unsigned long long w_counted = 0, w_idle = 0, w_loose = 0;   // the same in every lane of a wavefront
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n_trees; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = base + threadIdx.x;
        bool counted = false, idle = false, loose = false;
        int32_t c = -1;
        int64_t lat = 0;
        if (t < n_trees) {
            c = G.tree_class[t];
            const bool sel = A.tree_sel[t] != 0;
            counted = c >= 0 && sel;
            idle = c >= 0 && !sel;
            loose = c < 0 && sel;
            if (counted) lat = S.tree_latency[t];
        }
        unsigned long long todo = __ballot(counted);   // one round per distinct class among the counted trees of the wavefront
        w_counted += (unsigned long long)__popcll(todo);
        w_idle += (unsigned long long)__popcll(__ballot(idle));
        w_loose += (unsigned long long)__popcll(__ballot(loose));
        while (todo != 0) {
            const int leader = __ffsll((long long)todo) - 1;
            const int32_t k = __shfl(c, leader);
            const bool mine = counted && c == k;
            const unsigned long long m = __ballot(mine);
            todo &= ~m;
            unsigned long long sl = mine ? (unsigned long long)lat : 0ull;
            if (__popcll(m) > 1) sl = dist_wave_sum(sl, nl);
            if (lane == leader) {
                atomicAdd(&cnt[k], (unsigned long long)__popcll(m));
                if (sl != 0) atomicAdd(&sum[k], sl);
            }
        }
    }
    if (lane == 0) {
        if (w_counted != 0) atomicAdd(&P.counters[0], w_counted);
        if (w_idle != 0) atomicAdd(&P.counters[4], w_idle);
        if (w_loose != 0) atomicAdd(&P.counters[5], w_loose);
    }
    if (lds) {
        __syncthreads();
        for (int q = threadIdx.x; q < (int)nc; q += blockDim.x) {
            if (acc[q] != 0) atomicAdd((unsigned long long*)&P.class_counted[q], acc[q]);
            if (acc[nc + q] != 0) atomicAdd((unsigned long long*)&P.class_latency[q], acc[nc + q]);
        }
    }
}

// (after k_prof_rows and k_prof_trees: the cells and class_counted are final)
__global__ void __launch_bounds__(256) k_prof_classes(SigDev G, ProfDev P) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int nl = (int)stitch_min(blockDim.x, 64), lane = threadIdx.x % 64;
    const int64_t ne = P.n_entries;
    bool live = false;
    unsigned long long filled = 0;
    if (c < P.n_classes) {
        int64_t sum = 0, top = -1, best = 0;
        for (int64_t i = G.class_off[c]; i < G.class_off[c + 1]; i++) {
            if (P.cells[i] != 0) filled++;
            const int64_t pt = (int64_t)P.cells[5 * ne + i];
            sum += pt;
            if (P.cells[6 * ne + i] != 0 && (top < 0 || pt > best)) { top = i; best = pt; }   // ties: the smallest index
        }
        P.class_path_time[c] = sum;
        P.class_top[c] = top;
        live = P.class_counted[c] > 0;
    }
    const unsigned long long b = __ballot(live);
    filled = dist_wave_sum(filled, nl);
    if (lane == 0) {
        if (b != 0) atomicAdd(&P.counters[1], (unsigned long long)__popcll(b));
        if (filled != 0) atomicAdd(&P.counters[3], filled);
    }
}

}  // namespace tw

// tw_dist.h -- per-service latency distributions and cohorts (tw_set_row_cohorts / tw_latency_distributions).
//
// Replaces: what the delay-culprit query writes, src/query_engine/delay_culprit.py:80-97 -- per service the list of the span
// latencies of the selected requests, for the true and for the predicted traces, compared afterwards as distributions.  It
// works on what the last tw_attribute_traces left on the device: tree_sel, self_time, path_time, row_flag, row_tree, the
// groups, and the forest of the stitch (tree_latency, the CSR grouping).  include/traceweaver_amd.h has the definitions
// (cohort of a tree, the four metrics, the segments c * (3 G + 1) + m * G + g).
//
//   k_dist_cohort     one wavefront per kDistTrees consecutive trees of the CSR grouping: the smallest label of a tree's rows as an
//                     atomicMin on an unsigned key (-1 is the largest value and never wins) in one LDS slot per tree
//   k_dist_items<0>   one lane per row (the tree's root row also stands for its tree: metric 3): counts and sums per segment.  The
//                     lanes of a wavefront that meet on one (cohort, group) are counted by __ballot / __popcll and their values added
//                     by a shuffle reduction, so that one lane adds once per wavefront and segment; into an LDS table per workgroup
//                     (n_seg <= kDistSegLds), which is added to global memory once per workgroup and nonzero cell, else straight onto
//                     the global cells.  Also the number of items and the least and the greatest value (the key width).
//   k_dist_items<1>   the same rows again, now that the key width is known: every item as a sort key, segment << vbits | (value - min)
//                     (or value - min and the segment as a pair, where the two do not fit 64 bits); positions from one atomicAdd
//                     per wavefront on a cursor, the lanes' offsets by ballot prefix
//   (rocprim::radix_sort_keys on the packed key; else two stable radix_sort_pairs passes, value first, then the segment bits)
//   k_dist_scan       seg_off = exclusive scan of the counts; the number of non-empty segments
//   k_dist_unpack     values[i] = (key & mask) + min
//   k_dist_quantiles  one lane per (segment, prob): a gather at min(n - 1, (int64)(prob * (double)n))
//   k_dist_hist       one lane per (segment, bin): two lower-bound searches in the segment's sorted values, the bin is their difference
//
// Why two sweeps over the rows instead of one that writes (segment, value) pairs and a kernel that packs them: the packed key needs
// the least value, which is known only after all rows have been seen; writing the pairs first costs 12 B written, 12 B read and 8 B
// written per item and buffers sized for three items per row, the second sweep reads a row's tree and its selection byte again (all
// that an unselected row costs) and writes 8 B per item into buffers of exactly n_items.
//
// Every output is a pure function of the inputs: no floating point but the one product of k_dist_quantiles (a single binary64
// multiplication); the atomics are integer adds and minima of which only the result is read, and a cursor that decides where an
// item lies before the sort, never what the output holds.
#pragma once
#include "tw_attr.h"

namespace tw {

#ifdef TW_TILE_SMALL   // the tiny table of the tests' host build: the LDS and the global route of k_dist_items both occur
constexpr int kDistSegLds = 16;
#else
constexpr int kDistSegLds = 2048;    // segments whose count and sum a workgroup of k_dist_items keeps in LDS (32 KiB: at least two workgroups per CU)
#endif
constexpr int kDistTrees = 16;       // consecutive trees a wavefront of k_dist_cohort takes together (one LDS slot each)
constexpr int kDistWaves = 4;
constexpr int kDistMaxQ = 32;
constexpr int kDistMaxEdges = 63;
constexpr int kDistCounters = 8;     // items, least key, greatest key, trees counted, trees left out, non-empty segments, cursor, error
constexpr int64_t kDistMaxSeg = (int64_t)1 << 24;

struct DistDev {
    int32_t n_cohorts;
    const int32_t* row_cohort;       // [n_rows], null = every tree has cohort 0
    int32_t* tree_cohort;            // [n_trees]
    int64_t n_seg;
    unsigned long long *seg_count, *seg_sum;   // [n_seg] (the sums in two's complement)
    int64_t* seg_off;                // [n_seg + 1]
    // items
    int64_t items_cap;
    unsigned long long *key_a, *key_b;
    uint32_t *seg_a, *seg_b;         // the segments of the items where segment and value do not fit one key
    int64_t* values;
    unsigned long long* counters;    // [kDistCounters]
    int64_t *quant, *hist;
};

struct DistKeyDev {                  // how k_dist_items<1> writes an item
    unsigned long long vmin;         // the least value (two's complement)
    int32_t vbits;                   // bits of greatest - least
    int32_t wide;                    // segment bits + vbits > 64: (value - min, segment) pairs
};

struct DistQueryDev {
    int32_t n_q, n_edges;
    double probs[kDistMaxQ];
    int64_t edges[kDistMaxEdges];
};

// int64 -> uint64, ascending in signed order
__device__ __forceinline__ unsigned long long dist_key(int64_t v) { return (unsigned long long)v ^ (1ull << 63); }
__device__ __forceinline__ unsigned long long dist_umin(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned long long dist_umax(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

__global__ void __launch_bounds__(64 * kDistWaves) k_dist_cohort(StitchDev S, DistDev D, int64_t n_trees) {
    __shared__ uint32_t s_key[kDistWaves][kDistTrees];
    __shared__ int64_t s_off[kDistWaves][kDistTrees + 1];
    const int nl = (int)stitch_min(blockDim.x, 64), lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const int wpb = (int)stitch_max(blockDim.x / 64, 1);
    uint32_t* key = s_key[wave];
    int64_t* off = s_off[wave];
    const int64_t n_chunks = (n_trees + kDistTrees - 1) / kDistTrees;
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < n_chunks; c += (int64_t)gridDim.x * wpb) {
        const int64_t c0 = c * kDistTrees;
        const int nt = (int)stitch_min((int64_t)kDistTrees, n_trees - c0);
        for (int t = lane; t <= nt; t += nl) {
            off[t] = S.tree_off[c0 + t];
            if (t < nt) key[t] = ~0u;
        }
        stitch_wave_sync();
        const int64_t a = off[0], m = off[nt] - a;
        int t = 0;   // a lane's positions ascend, so its tree only moves forward
        for (int64_t k = lane; k < m; k += nl) {
            while (t + 1 < nt && off[t + 1] <= a + k) t++;
            const uint32_t label = (uint32_t)D.row_cohort[S.tree_rows[a + k]];
            if (label != ~0u) atomicMin(&key[t], label);
        }
        stitch_wave_sync();
        for (int q = lane; q < nt; q += nl) D.tree_cohort[c0 + q] = (int32_t)key[q];
        stitch_wave_sync();   // ... before the next trees overwrite the slots
    }
}

// The sum of v over the lanes of a wavefront, in every lane (nl: lanes of the wavefront, a power of two).
__device__ __forceinline__ unsigned long long dist_wave_sum(unsigned long long v, int nl) {
    for (int off = 32; off >= 1; off >>= 1)
        if (off < nl) v += (unsigned long long)__shfl_xor((long long)v, off);
    return v;
}

__device__ __forceinline__ void dist_cell_add(unsigned long long* cnt, unsigned long long* sum, int64_t seg, unsigned long long n, unsigned long long s) {
    atomicAdd(&cnt[seg], n);
    if (s != 0) atomicAdd(&sum[seg], s);
}

// kWrite = false: counts, sums, the number of items, the least and the greatest value.  kWrite = true: the items as sort keys.
// Workgroups stride over the rows, so that the LDS table is cleared and added to global memory once per workgroup, not per 256 rows.
template <bool kWrite>
__global__ void __launch_bounds__(256) k_dist_items(StitchDev S, AttrDev A, DistDev D, DistKeyDev K) {
    __shared__ unsigned long long acc[kWrite ? 1 : 2 * kDistSegLds];
    const int G = A.n_groups;
    const int64_t per = 3 * (int64_t)G + 1;
    const bool lds = !kWrite && D.n_seg <= kDistSegLds;
    if (lds) {
        for (int q = threadIdx.x; q < 2 * (int)D.n_seg; q += blockDim.x) acc[q] = 0;
        __syncthreads();
    }
    unsigned long long* cnt = lds ? acc : D.seg_count;
    unsigned long long* sum = lds ? acc + D.n_seg : D.seg_sum;
    const int nl = (int)stitch_min(blockDim.x, 64), lane = threadIdx.x % 64;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));   // the lanes before this one
    unsigned long long w_items = 0, w_counted = 0, w_left = 0;   // the same in every lane of a wavefront
    unsigned long long lo = ~0ull, hi = 0;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < S.n_rows; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = base + threadIdx.x;
        bool has = false, on = false, root = false, left = false;
        int32_t c = -1, g = -1;
        int64_t d = 0, st = 0, pt = 0, lat = 0;
        if (r < S.n_rows) {
            const int32_t t = A.row_tree[r];
            if (A.tree_sel[t] != 0) {
                const bool is_root = S.tree_root[t] == (int32_t)r;
                c = D.row_cohort != nullptr ? D.tree_cohort[t] : 0;
                if (c >= 0) {
                    g = A.row_group[r];
                    if (g >= 0) {
                        has = true;
                        const int64_t s = S.row_start[r];
                        d = stitch_max(S.row_end[r], s) - s;
                        st = A.self_time[r];
                        on = (A.row_flag[r] & 1) != 0;
                        if (on) pt = A.path_time[r];
                    }
                    root = is_root;
                    if (root) lat = S.tree_latency[t];
                } else {
                    left = is_root;
                }
            }
        }
        const unsigned long long b0 = __ballot(has), b2 = __ballot(has && on), b3 = __ballot(root);
        const unsigned long long n0 = (unsigned long long)__popcll(b0), n2 = (unsigned long long)__popcll(b2), n3 = (unsigned long long)__popcll(b3);
        const unsigned long long total = 2 * n0 + n2 + n3;
        if (!kWrite) {
            w_items += total;
            w_counted += n3;
            w_left += (unsigned long long)__popcll(__ballot(left));
            if (has) {
                lo = dist_umin(lo, dist_umin(dist_key(d), dist_key(st)));
                hi = dist_umax(hi, dist_umax(dist_key(d), dist_key(st)));
                if (on) { lo = dist_umin(lo, dist_key(pt)); hi = dist_umax(hi, dist_key(pt)); }
            }
            if (root) { lo = dist_umin(lo, dist_key(lat)); hi = dist_umax(hi, dist_key(lat)); }
            // metrics 0 .. 2: one round per distinct (cohort, group) among the lanes; the control flow is the same in every lane
            const int32_t cg = c * G + g;
            unsigned long long todo = b0;
            while (todo != 0) {
                const int leader = __ffsll((long long)todo) - 1;
                const int32_t k = __shfl(cg, leader);
                const bool mine = has && cg == k;
                const unsigned long long m = __ballot(mine), m2 = __ballot(mine && on);
                todo &= ~m;
                unsigned long long sd = mine ? (unsigned long long)d : 0ull, ss = mine ? (unsigned long long)st : 0ull;
                unsigned long long sp = mine && on ? (unsigned long long)pt : 0ull;
                if (__popcll(m) > 1) {   // (a lane alone in its segment holds the sums already)
                    sd = dist_wave_sum(sd, nl);
                    ss = dist_wave_sum(ss, nl);
                    if (m2 != 0) sp = dist_wave_sum(sp, nl);
                }
                if (lane == leader) {
                    const int64_t seg = (int64_t)c * per + g;
                    dist_cell_add(cnt, sum, seg, (unsigned long long)__popcll(m), sd);
                    dist_cell_add(cnt, sum, seg + G, (unsigned long long)__popcll(m), ss);
                }
                if (m2 != 0 && lane == __ffsll((long long)m2) - 1) dist_cell_add(cnt, sum, (int64_t)c * per + 2 * G + g, (unsigned long long)__popcll(m2), sp);
            }
            // metric 3: one round per distinct cohort among the root rows
            todo = b3;
            while (todo != 0) {
                const int leader = __ffsll((long long)todo) - 1;
                const int32_t k = __shfl(c, leader);
                const bool mine = root && c == k;
                const unsigned long long m = __ballot(mine);
                todo &= ~m;
                unsigned long long sl = mine ? (unsigned long long)lat : 0ull;
                if (__popcll(m) > 1) sl = dist_wave_sum(sl, nl);
                if (lane == leader) dist_cell_add(cnt, sum, (int64_t)c * per + 3 * G, (unsigned long long)__popcll(m), sl);
            }
        } else if (total != 0) {
            unsigned long long at = 0;
            if (lane == 0) at = atomicAdd(&D.counters[6], total);
            at = (unsigned long long)__shfl((long long)at, 0);
            const int64_t seg = (int64_t)c * per + g;
            const int64_t p0 = (int64_t)at + __popcll(b0 & below), p2 = (int64_t)(at + 2 * n0) + __popcll(b2 & below);
            const int64_t p3 = (int64_t)(at + 2 * n0 + n2) + __popcll(b3 & below);
#define DIST_PUT(pos, sg, v)                                                                                          \
    do {                                                                                                              \
        const int64_t q_ = (pos);                                                                                     \
        const unsigned long long x_ = (unsigned long long)(v) - K.vmin;                                               \
        if (q_ >= D.items_cap) D.counters[7] = 1;   /* (the host sized the buffers by the count of the first sweep) */ \
        else if (K.wide) { D.key_a[q_] = x_; D.seg_a[q_] = (uint32_t)(sg); }                                          \
        else D.key_a[q_] = ((unsigned long long)(sg) << K.vbits) | x_;                                                \
    } while (0)
            if (has) {
                DIST_PUT(p0, seg, d);
                DIST_PUT(p0 + (int64_t)n0, seg + G, st);
                if (on) DIST_PUT(p2, seg + 2 * G, pt);
            }
            if (root) DIST_PUT(p3, (int64_t)c * per + 3 * G, lat);
#undef DIST_PUT
        }
    }
    if (!kWrite) {
        for (int off = 32; off >= 1; off >>= 1)
            if (off < nl) {
                lo = dist_umin(lo, (unsigned long long)__shfl_xor((long long)lo, off));
                hi = dist_umax(hi, (unsigned long long)__shfl_xor((long long)hi, off));
            }
        if (lane == 0) {
            if (w_items != 0) { atomicAdd(&D.counters[0], w_items); atomicMin(&D.counters[1], lo); atomicMax(&D.counters[2], hi); }
            if (w_counted != 0) atomicAdd(&D.counters[3], w_counted);
            if (w_left != 0) atomicAdd(&D.counters[4], w_left);
        }
        if (lds) {
            __syncthreads();
            for (int q = threadIdx.x; q < (int)D.n_seg; q += blockDim.x) {
                if (acc[q] != 0) atomicAdd(&D.seg_count[q], acc[q]);
                if (acc[D.n_seg + q] != 0) atomicAdd(&D.seg_sum[q], acc[D.n_seg + q]);
            }
        }
    }
}

// One workgroup: every thread a contiguous run of segments.
__global__ void __launch_bounds__(256) k_dist_scan(DistDev D) {
    __shared__ unsigned long long sh[256];
    const int64_t per = (D.n_seg + blockDim.x - 1) / blockDim.x;
    const int64_t lo = stitch_min((int64_t)threadIdx.x * per, D.n_seg), hi = stitch_min(lo + per, D.n_seg);
    unsigned long long s = 0, filled = 0;
    for (int64_t q = lo; q < hi; q++) { s += D.seg_count[q]; filled += D.seg_count[q] != 0 ? 1 : 0; }
    sh[threadIdx.x] = s;
    __syncthreads();
    unsigned long long run = 0;
    for (unsigned k = 0; k < threadIdx.x; k++) run += sh[k];
    for (int64_t q = lo; q < hi; q++) { D.seg_off[q] = (int64_t)run; run += D.seg_count[q]; }
    if (threadIdx.x == blockDim.x - 1) D.seg_off[D.n_seg] = (int64_t)run;
    if (filled != 0) atomicAdd(&D.counters[5], filled);
}

__global__ void __launch_bounds__(256) k_dist_unpack(DistDev D, DistKeyDev K, const unsigned long long* sorted, int64_t n_items) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_items) return;
    const unsigned long long mask = K.wide || K.vbits >= 64 ? ~0ull : ((1ull << K.vbits) - 1ull);
    D.values[q] = (int64_t)((sorted[q] & mask) + K.vmin);
}

__global__ void __launch_bounds__(256) k_dist_quantiles(DistDev D, DistQueryDev Q) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= D.n_seg * Q.n_q) return;
    const int64_t seg = q / Q.n_q;
    const int j = (int)(q - seg * Q.n_q);
    const int64_t n = (int64_t)D.seg_count[seg];
    int64_t v = INT64_MIN;
    if (n > 0) v = D.values[D.seg_off[seg] + stitch_min(n - 1, (int64_t)(Q.probs[j] * (double)n))];
    D.quant[q] = v;
}

// first position in [a, b) whose value is not below x
__device__ __forceinline__ int64_t dist_lower_bound(const int64_t* v, int64_t a, int64_t b, int64_t x) {
    while (a < b) {
        const int64_t mid = a + (b - a) / 2;
        if (v[mid] < x) a = mid + 1;
        else b = mid;
    }
    return a;
}

__global__ void __launch_bounds__(256) k_dist_hist(DistDev D, DistQueryDev Q) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int bins = Q.n_edges + 1;
    if (q >= D.n_seg * bins) return;
    const int64_t seg = q / bins;
    const int b = (int)(q - seg * bins);
    const int64_t a = D.seg_off[seg], z = a + (int64_t)D.seg_count[seg];
    const int64_t from = b > 0 ? dist_lower_bound(D.values, a, z, Q.edges[b - 1]) : a;
    const int64_t to = b < Q.n_edges ? dist_lower_bound(D.values, from, z, Q.edges[b]) : z;
    D.hist[q] = to - from;
}

}  // namespace tw

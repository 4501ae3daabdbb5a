// tw_hist.h -- the latency distributions of batch after batch kept on the device (tw_history_push / tw_history_merge and the queries
// tw_history_distributions / tw_history_compare).
//
// Replaces: the pickles of latency lists the delay-culprit query writes per run and reads side by side,
// src/query_engine/delay_culprit.py:32-97 -- one run against another, not two cohorts of one run.  The history holds what
// tw_latency_distributions leaves of a batch (DistDev: every segment's values ascending, counts, sums) for C_h cohorts of its own;
// a push merges a batch's segments into the cohorts a map names.  include/traceweaver_amd.h has the definitions.
//
//   k_hist_source  (tw_history_merge only) one lane per item of the uploaded source: its segment by a search of the offsets, the
//                  test values[i - 1] <= values[i] inside a segment (the error flag), and the segment's sum by the add of
//                  k_dist_items (the lanes of a wavefront that meet on one segment add once); one lane per segment for the counts
//   k_hist_plan    one workgroup, every thread a contiguous run of history segments (the manner of k_dist_scan): new count = old +
//                  mapped source, new sum likewise, the offsets and the tile table (a segment of n items owns ceil(n / kHistTile)
//                  tiles, an empty one none) as two exclusive scans; items added, items held, tiles
//   k_hist_merge   one workgroup per tile (merge path).  The tile's segment by a search of the tile table (the idiom of cmp_row_of);
//                  the splits of the tile's first and last diagonal by two binary searches over the two runs in global memory (two
//                  threads), items of the history before equal items of the source; the <= kHistTile items the tile consumes of either
//                  run staged in LDS, coalesced; every thread then finds the split of its own diagonal on the LDS copies and merges
//                  its ceil(kHistTile / blockDim) items into a second LDS array, which leaves coalesced.  A tile of a segment with
//                  one run empty is a copy and skips the LDS.
//
// The store is rewritten by every push (16 B per item held afterwards: 8 read, 8 written); what a push does not touch is copied by
// the same kernel, so that the other value buffer holds the whole history and the two are swapped when nothing has failed.
//
// Every output is a function of the inputs alone: integers throughout, the sums wrap as those of DistDev do, the only atomics are
// the integer adds of k_hist_source and its error flag.
#pragma once
#include "tw_cmp.h"

namespace tw {

#ifdef TW_TILE_SMALL   // the tiny tile of the tests' host build: a few dozen rows cross tile boundaries
constexpr int kHistTile = 8;
#else
constexpr int kHistTile = 2048;      // items of the result per workgroup: 16 KiB staged + 16 KiB merged, five workgroups per CU's 160 KiB
#endif
constexpr int kHistThreads = 256;
constexpr int kHistCounters = 4;     // items added, items held afterwards, tiles, error (an unsorted source segment)

struct HistDev {
    int64_t per;                     // 3 G + 1
    int64_t n_seg, n_old;            // segments afterwards (C_h' * per) and before (C_h * per <= n_seg)
    // the history as it is
    const int64_t* old_off;          // [n_old + 1]
    const unsigned long long *old_count, *old_sum;   // [n_old]
    const int64_t* old_values;
    // the source: the resident distribution items (push) or the uploaded arrays (merge)
    const int32_t* inv;              // [n_seg / per]: the source cohort that goes to history cohort h, -1 = none
    const int64_t* src_off;          // [n_src_seg + 1]
    const unsigned long long *src_count, *src_sum;   // [n_src_seg]
    const int64_t* src_values;
    // the history afterwards
    int64_t* new_off;                // [n_seg + 1]
    unsigned long long *new_count, *new_sum;         // [n_seg]
    int64_t* new_values;
    int64_t* tile_off;               // [n_seg + 1]: segment s owns tiles tile_off[s] .. tile_off[s + 1]
    unsigned long long* counters;    // [kHistCounters]
};

struct HistSrcDev {                  // the uploaded source of tw_history_merge
    int64_t n_seg, n_items;
    const int64_t *off, *values;
    unsigned long long *count, *sum; // [n_seg], the sums cleared by the host
    unsigned long long* counters;
};

__global__ void __launch_bounds__(256) k_hist_source(HistSrcDev S) {
    const int nl = (int)stitch_min(blockDim.x, 64), lane = threadIdx.x % 64;
    const int64_t n_work = stitch_max(S.n_items, S.n_seg);
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n_work; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + threadIdx.x;
        if (i < S.n_seg) S.count[i] = (unsigned long long)(S.off[i + 1] - S.off[i]);
        const bool has = i < S.n_items;
        int64_t seg = -1;
        unsigned long long v = 0;
        if (has) {
            seg = cmp_upper_bound(S.off, 0, S.n_seg + 1, i) - 1;   // (the last segment whose offset is not above i: empty ones are stepped over)
            const int64_t x = S.values[i];
            v = (unsigned long long)x;
            if (i > S.off[seg] && S.values[i - 1] > x) S.counters[3] = 1;
        }
        // one round per distinct segment among the lanes; the control flow is the same in every lane
        unsigned long long todo = __ballot(has);
        while (todo != 0) {
            const int leader = __ffsll((long long)todo) - 1;
            const int64_t k = __shfl((long long)seg, leader);
            const bool mine = has && seg == k;
            const unsigned long long m = __ballot(mine);
            todo &= ~m;
            unsigned long long s = mine ? v : 0ull;
            if (__popcll(m) > 1) s = dist_wave_sum(s, nl);
            if (lane == leader && s != 0) atomicAdd(&S.sum[k], s);
        }
    }
}

struct HistRun {                     // the two runs of a history segment
    int64_t a0, na, b0, nb;
    unsigned long long sa, sb;       // their sums
};
__device__ __forceinline__ HistRun hist_run(const HistDev& H, int64_t seg) {
    HistRun R{0, 0, 0, 0, 0, 0};
    if (seg < H.n_old) { R.a0 = H.old_off[seg]; R.na = (int64_t)H.old_count[seg]; R.sa = H.old_sum[seg]; }
    const int64_t h = seg / H.per;
    const int32_t c = H.inv[h];
    if (c >= 0) {
        const int64_t s = (int64_t)c * H.per + (seg - h * H.per);
        R.b0 = H.src_off[s]; R.nb = (int64_t)H.src_count[s]; R.sb = H.src_sum[s];
    }
    return R;
}

// One workgroup: every thread a contiguous run of segments.
__global__ void __launch_bounds__(256) k_hist_plan(HistDev H) {
    __shared__ unsigned long long sh_n[256], sh_t[256], sh_b[256];
    const int64_t per = (H.n_seg + blockDim.x - 1) / blockDim.x;
    const int64_t lo = stitch_min((int64_t)threadIdx.x * per, H.n_seg), hi = stitch_min(lo + per, H.n_seg);
    unsigned long long n = 0, t = 0, b = 0;
    for (int64_t q = lo; q < hi; q++) {
        const HistRun R = hist_run(H, q);
        const unsigned long long c = (unsigned long long)(R.na + R.nb);
        H.new_count[q] = c;
        H.new_sum[q] = R.sa + R.sb;
        n += c; t += (c + kHistTile - 1) / kHistTile; b += (unsigned long long)R.nb;
    }
    sh_n[threadIdx.x] = n; sh_t[threadIdx.x] = t; sh_b[threadIdx.x] = b;
    __syncthreads();
    unsigned long long run = 0, tiles = 0;
    for (unsigned k = 0; k < threadIdx.x; k++) { run += sh_n[k]; tiles += sh_t[k]; }
    for (int64_t q = lo; q < hi; q++) {
        H.new_off[q] = (int64_t)run; H.tile_off[q] = (int64_t)tiles;
        run += H.new_count[q]; tiles += (H.new_count[q] + kHistTile - 1) / kHistTile;
    }
    if (threadIdx.x == blockDim.x - 1) {
        unsigned long long added = 0;
        for (unsigned k = 0; k < blockDim.x; k++) added += sh_b[k];
        H.new_off[H.n_seg] = (int64_t)run; H.tile_off[H.n_seg] = (int64_t)tiles;
        H.counters[0] = added; H.counters[1] = run; H.counters[2] = tiles;
    }
}

// Merge path: how many of the first d items of the merged run come from a[0 .. na) -- an item of a lies before an equal item of b.
// (d <= na + nb; the search reads a and b inside their runs only.)
__device__ __forceinline__ int64_t hist_split(const int64_t* a, int64_t na, const int64_t* b, int64_t nb, int64_t d) {
    int64_t lo = stitch_max((int64_t)0, d - nb), hi = stitch_min(d, na);
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= b[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kHistThreads) k_hist_merge(HistDev H, int64_t n_tiles) {
    __shared__ int64_t s_in[kHistTile], s_out[kHistTile];
    __shared__ int64_t s_cut[2];
    const int bd = (int)blockDim.x, tid = (int)threadIdx.x;
    const int ipt = (kHistTile + bd - 1) / bd;   // items of the result per thread
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t seg = cmp_upper_bound(H.tile_off, 0, H.n_seg + 1, t) - 1;   // (segments without tiles are stepped over)
        const HistRun R = hist_run(H, seg);
        const int64_t n = R.na + R.nb;
        const int64_t d0 = (t - H.tile_off[seg]) * kHistTile, d1 = stitch_min(d0 + kHistTile, n);
        int64_t* dst = H.new_values + H.new_off[seg] + d0;
        const int len = (int)(d1 - d0);
        if (R.na == 0 || R.nb == 0) {   // the degenerate merge: a copy (the same branch in the whole workgroup)
            const int64_t* src = R.nb == 0 ? H.old_values + R.a0 + d0 : H.src_values + R.b0 + d0;
            for (int x = tid; x < len; x += bd) dst[x] = src[x];
            continue;
        }
        const int64_t* a = H.old_values + R.a0;
        const int64_t* b = H.src_values + R.b0;
        for (int k = tid; k < 2; k += bd) s_cut[k] = hist_split(a, R.na, b, R.nb, k == 0 ? d0 : d1);
        __syncthreads();
        const int64_t i0 = s_cut[0], j0 = d0 - i0;
        const int ca = (int)(s_cut[1] - i0), cb = len - ca;   // what the tile consumes of either run: ca + cb = len <= kHistTile
        for (int x = tid; x < len; x += bd) s_in[x] = x < ca ? a[i0 + x] : b[j0 + (x - ca)];
        __syncthreads();
        const int64_t *la = s_in, *lb = s_in + ca;
        const int e0 = (int)stitch_min((int64_t)tid * ipt, (int64_t)len), e1 = (int)stitch_min((int64_t)e0 + ipt, (int64_t)len);
        if (e0 < e1) {
            int i = (int)hist_split(la, ca, lb, cb, e0), j = e0 - i;
            for (int k = e0; k < e1; k++) {
                const bool from_a = j >= cb || (i < ca && la[i] <= lb[j]);
                s_out[k] = from_a ? la[i++] : lb[j++];
            }
        }
        __syncthreads();
        for (int x = tid; x < len; x += bd) dst[x] = s_out[x];
        __syncthreads();   // ... before the next tile overwrites the LDS arrays
    }
}

}  // namespace tw

// tw_sig.h -- reconstructed traces grouped by call-graph signature (tw_trace_signatures).
//
// Replaces: AssignCGSignature and FindUniqueCGs of the reference (alibaba-analysis/analysis.py:99-126, 214-221) -- per trace the
// services seen at every depth, and the traces grouped by that.  It works on what the last tw_stitch_traces left on the device
// (link, depth, the CSR grouping, the per-tree figures) and on the row groups of tw_set_row_groups.  include/traceweaver_amd.h has
// the definitions (level, items, the two key modes, signature, classes, the reference set).
//
//   k_sig_items       one lane per position of tree_rows (a coalesced sweep; the row's columns are gathered): the level of the row and
//                     its packed key level << 41 | (caller group + 1, or 1 in mode 0) << 20 | group -- 16 + 21 + 20 bits -- at the
//                     row's own position, so that a tree's keys lie in the tree's segment of the CSR grouping; ~0 for a row that is
//                     no item, which sorts behind every key
//   k_sig_trees       per tree: eligible by its flags?  The trees of more than kSigCap rows are listed for the segmented sort
//   (rocprim::segmented_radix_sort_keys on the listed trees alone)
//   k_sig_sign        one wavefront per kSigTrees consecutive trees whose rows fit its LDS table (a larger tree alone): rank sort in
//                     LDS; then per tree the run lengths of the sorted keys -- heads and tails of the runs by ballot, an entry's
//                     number by the popcount of the lanes before it -- written over the tree's own segment (entry keys over the
//                     item keys, counts beside them), and the hash: the sum over the entries of mix(key, count, number), the
//                     number of entries folded in.  A listed tree: the same on the keys rocprim sorted in global memory.
//   (rocprim::radix_sort_pairs of (hash, tree): stable, the trees go in in ascending order)
//   k_sig_rep         per tree: the head of its run of equal hashes by binary search, then the first eligible tree of the run whose
//                     entries equal its own, entry by entry -- the hash orders and buckets, it never decides equality
//   k_sig_scan_*      exclusive scan of (1, entries) over the trees with rep[t] == t: class numbers in ascending order of the rep,
//                     class_off
//   k_sig_classes     per eligible tree: its class, the class' trees and latency sum / min / max by integer atomics; the rep writes
//                     the class' entries
//   k_sig_compare     per eligible tree: the reference set's signature under the same root row, compared entry by entry
//   k_sig_keep        the reference set: per root row of an eligible tree where its entries lie in the copies of the entry arrays
//
// Every output is a pure function of the inputs: no floating point; the atomics are integer adds, minima and maxima of which only
// the result is read, a cursor that orders the list of the large trees (which of them rocprim sorts first), and stores of the
// constant 1.
#pragma once
#include "tw_dist.h"

namespace tw {

#ifdef TW_TILE_SMALL   // the tiny table of the tests' host build: the packed, the single-tree and the rocprim route all occur
constexpr int kSigCap = 12;
constexpr int kSigTrees = 4;
constexpr int kSigLevelBits = 6;     // (the refusal of a level beyond the key is reached with a chain of 65 rows, not of 65537)
#else
constexpr int kSigCap = 512;         // rows a wavefront sorts in LDS (two tables of 8 B each: 32 KiB per workgroup of four)
constexpr int kSigTrees = 16;        // consecutive trees a wavefront takes together when their rows fit
constexpr int kSigLevelBits = 16;
#endif
constexpr int kSigWaves = 4;
constexpr int kSigScanItems = 8;     // trees per thread of the scan kernels
constexpr int kSigCallerBits = 21, kSigGroupBits = 20;
constexpr int kSigCounters = 8;      // eligible trees, their items, listed trees, level overflow, compared trees, same trees, classes << 32 | entries
constexpr unsigned long long kSigNone = ~0ull;

struct SigDev {
    int32_t mode, hash_bits;
    uint32_t need_flags, skip_flags;
    const int32_t* row_group;
    // per row / position of tree_rows
    int32_t* row_level;
    unsigned long long *key_a, *key_b;   // item keys, then (in place) entry keys of the tree at its tree_off; the listed trees' sorted keys
    int32_t* ent_cnt;                    // entry counts, beside the entry keys
    uint32_t *big_begin, *big_end;       // segments of the listed trees
    // per tree
    unsigned long long *hkey_a, *hkey_b;
    int32_t *val_a, *val_b, *tree_ent, *rep, *tree_class;
    int64_t* tree_items;
    uint8_t *elig, *tree_same;
    unsigned long long* chunk_sum;
    // per class (capacity: trees)
    int32_t* class_rep;
    int64_t *class_trees, *class_sum, *class_min, *class_max, *class_off;
    int32_t* class_entries;              // [4 * entries of all classes]
    unsigned long long* counters;        // [kSigCounters]
    // reference set, keyed by root row
    unsigned long long* ref_key;
    int32_t *ref_cnt, *ref_n;            // ref_n[row]: entries of the tree rooted there, -1 = the set holds none
    int64_t* ref_pos;
};

__device__ __forceinline__ unsigned long long sig_mix(unsigned long long x) {   // the finaliser of splitmix64
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ bool sig_eligible(const SigDev& D, uint32_t f) { return (f & D.need_flags) == D.need_flags && (f & D.skip_flags) == 0; }

// The packed key of a (level, caller group + 1 -- 1 in mode 0 --, group) triple.
__device__ __forceinline__ unsigned long long sig_pack(int32_t level, unsigned long long c, int32_t g) {
    return ((unsigned long long)level << (kSigCallerBits + kSigGroupBits)) | (c << kSigGroupBits) | (unsigned long long)g;
}

// The caller group of server row r (mode 1; the EDGE clauses of tw_filt.h): the group of its nearest server ancestor, -1 without one.
__device__ __forceinline__ int32_t sig_caller_group(const StitchDev& S, const int32_t* row_group, int32_t r) {
    int32_t p = S.link[r];   // (the stitch refuses cycles; two hops in a valid table)
    while (p >= 0 && S.row_kind[p] != 1) p = S.link[p];
    return p >= 0 ? row_group[p] : -1;
}

// Level and item key of row r (k_sig_items; k_prof_rows of tw_prof.h computes a row's key again with it): kSigNone for a row that is
// no item; `deep` is set for a server row whose level does not fit the key.
__device__ __forceinline__ unsigned long long sig_item_key(const StitchDev& S, const SigDev& D, int32_t r, int32_t& level, bool& deep) {
    unsigned long long key = kSigNone;
    level = -1;
    deep = false;
    if (S.row_kind[r] == 1) {
        level = S.depth[r] >> 1;   // server rows hang under client rows and client rows under server rows: every other ancestor is one
        const int32_t g = D.row_group[r];
        if (level >= (1 << kSigLevelBits)) {
            deep = true;
        } else if (g >= 0) {
            const unsigned long long c = D.mode == 1 ? (unsigned long long)(sig_caller_group(S, D.row_group, r) + 1) : 1ull;
            key = sig_pack(level, c, g);
        }
    }
    return key;
}

__global__ void __launch_bounds__(256) k_sig_items(StitchDev S, SigDev D) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= S.n_rows) return;
    const int32_t r = S.tree_rows[k];
    int32_t level;
    bool deep;
    const unsigned long long key = sig_item_key(S, D, r, level, deep);
    if (deep) D.counters[3] = 1;
    D.row_level[r] = level;
    D.key_a[k] = key;
}

__global__ void __launch_bounds__(256) k_sig_trees(StitchDev S, SigDev D, int64_t n_trees) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool elig = false;
    if (t < n_trees) {
        elig = sig_eligible(D, S.tree_flags[t]);
        D.elig[t] = elig ? 1 : 0;
        const int64_t a = S.tree_off[t], b = S.tree_off[t + 1];
        if (b - a > kSigCap) {
            const unsigned long long at = atomicAdd(&D.counters[2], 1ull);
            D.big_begin[at] = (uint32_t)a;
            D.big_end[at] = (uint32_t)b;
        }
    }
    const unsigned long long any = __ballot(elig);
    if (any != 0 && (threadIdx.x & 63) == 0) atomicAdd(&D.counters[0], (unsigned long long)__popcll(any));
}

// The run lengths and the hash of one tree's sorted keys srt[0 .. n) (the keys that are no item last), by one wavefront: entry i =
// (ent_key[i], ent_cnt[i]).  `first` holds the runs' first positions between the two sweeps (it may be ent_cnt itself).  The three
// results are the same in every lane.
template <bool kGlobal>
__device__ __forceinline__ void sig_runs(const unsigned long long* srt, int32_t* first, unsigned long long* ent_key, int32_t* ent_cnt, int64_t n,
                                         int lane, int nl, int64_t& items, int32_t& entries, unsigned long long& hash) {
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));   // the lanes before this one
    int64_t n_items = 0;
    int32_t base = 0;
    for (int64_t k0 = 0; k0 < n; k0 += nl) {
        const int64_t k = k0 + lane;
        const unsigned long long key = k < n ? srt[k] : kSigNone;
        const bool item = key != kSigNone;
        const bool head = item && (k == 0 || srt[k - 1] != key);
        const unsigned long long hb = __ballot(head);
        n_items += __popcll(__ballot(item));
        if (head) {
            const int32_t i = base + __popcll(hb & below);
            ent_key[i] = key;
            first[i] = (int32_t)k;
        }
        base += __popcll(hb);
    }
    attr_sync<kGlobal>();
    unsigned long long h = 0;
    base = 0;
    for (int64_t k0 = 0; k0 < n; k0 += nl) {
        const int64_t k = k0 + lane;
        const unsigned long long key = k < n ? srt[k] : kSigNone;
        const bool tail = key != kSigNone && (k + 1 == n || srt[k + 1] != key);
        const unsigned long long tb = __ballot(tail);
        if (tail) {
            const int32_t i = base + __popcll(tb & below);
            const int32_t len = (int32_t)(k + 1) - first[i];
            ent_cnt[i] = len;
            h += sig_mix(key ^ sig_mix(((unsigned long long)(uint32_t)i << 32) | (unsigned long long)(uint32_t)len));
        }
        base += __popcll(tb);
    }
    h = dist_wave_sum(h, nl);
    items = n_items;
    entries = base;
    hash = sig_mix(h + 0x9e3779b97f4a7c15ull * (unsigned long long)(uint32_t)base);
    attr_sync<kGlobal>();   // ... before the next tree reuses `first`
}

__global__ void __launch_bounds__(64 * kSigWaves) k_sig_sign(StitchDev S, SigDev D, int64_t n_trees) {
    __shared__ unsigned long long s_raw[kSigWaves][kSigCap];
    __shared__ unsigned long long s_srt[kSigWaves][kSigCap];
    const int nl = (int)stitch_min(blockDim.x, 64), lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const int wpb = (int)stitch_max(blockDim.x / 64, 1);
    unsigned long long* raw = s_raw[wave];
    unsigned long long* srt = s_srt[wave];
    const unsigned long long mask = D.hash_bits >= 64 ? ~0ull : ((1ull << D.hash_bits) - 1ull);
    const int64_t n_chunks = (n_trees + kSigTrees - 1) / kSigTrees;
    unsigned long long w_items = 0;   // the same in every lane
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < n_chunks; c += (int64_t)gridDim.x * wpb) {
        const int64_t c0 = c * kSigTrees, c1 = stitch_min(c0 + kSigTrees, n_trees);
        const bool packed = S.tree_off[c1] - S.tree_off[c0] <= kSigCap;
        // the chunk's trees together when their rows fit, else tree by tree
        for (int64_t t0 = c0; t0 < c1; t0 = packed ? c1 : t0 + 1) {
            const int64_t t1 = packed ? c1 : t0 + 1;
            const int64_t a = S.tree_off[t0], m64 = S.tree_off[t1] - a;
            if (m64 <= kSigCap) {
                const int m = (int)m64;
                for (int k = lane; k < m; k += nl) raw[k] = D.key_a[a + k];
                stitch_wave_sync();
                for (int k = lane; k < m; k += nl) {
                    int64_t t = t0;
                    while (t + 1 < t1 && S.tree_off[t + 1] <= a + k) t++;
                    const int lo = (int)(S.tree_off[t] - a), hi = (int)(S.tree_off[t + 1] - a);
                    const unsigned long long kk = raw[k];
                    int rank = 0;
                    for (int j = lo; j < hi; j++) rank += (raw[j] < kk || (raw[j] == kk && j < k)) ? 1 : 0;
                    srt[lo + rank] = kk;
                }
                stitch_wave_sync();   // every key is sorted and read: the first table now holds the runs' first positions
                for (int64_t t = t0; t < t1; t++) {
                    const int lo = (int)(S.tree_off[t] - a), hi = (int)(S.tree_off[t + 1] - a);
                    int64_t items; int32_t entries; unsigned long long hash;
                    sig_runs<false>(srt + lo, (int32_t*)raw, D.key_a + a + lo, D.ent_cnt + a + lo, (int64_t)(hi - lo), lane, nl, items, entries, hash);
                    const bool elig = D.elig[t] != 0;
                    if (lane == 0) {
                        D.hkey_a[t] = elig ? (hash & mask) : kSigNone;
                        D.val_a[t] = (int32_t)t;
                        D.tree_ent[t] = entries;
                        D.tree_items[t] = items;
                    }
                    if (elig) w_items += (unsigned long long)items;
                }
            } else {
                // a listed tree: rocprim sorted its keys into key_b; the entries go over the item keys, the counts hold the first positions
                int64_t items; int32_t entries; unsigned long long hash;
                sig_runs<true>(D.key_b + a, D.ent_cnt + a, D.key_a + a, D.ent_cnt + a, m64, lane, nl, items, entries, hash);
                const bool elig = D.elig[t0] != 0;
                if (lane == 0) {
                    D.hkey_a[t0] = elig ? (hash & mask) : kSigNone;
                    D.val_a[t0] = (int32_t)t0;
                    D.tree_ent[t0] = entries;
                    D.tree_items[t0] = items;
                }
                if (elig) w_items += (unsigned long long)items;
            }
        }
    }
    if (lane == 0 && w_items != 0) atomicAdd(&D.counters[1], w_items);
}

// do the trees u and t have the same entries?  (keys and counts of tree x at x's tree_off)
__device__ __forceinline__ bool sig_equal(const unsigned long long* ka, const int32_t* ca, int64_t a, const unsigned long long* kb, const int32_t* cb,
                                          int64_t b, int32_t n) {
    for (int32_t i = 0; i < n; i++)
        if (ka[a + i] != kb[b + i] || ca[a + i] != cb[b + i]) return false;
    return true;
}

// q: position in the order of (hash, tree).  The trees of one run of equal hashes ascend, so the first equal one is the smallest.
__global__ void __launch_bounds__(256) k_sig_rep(StitchDev S, SigDev D, int64_t n_trees) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_trees) return;
    const int32_t t = D.val_b[q];
    if (D.elig[t] == 0) { D.rep[t] = -1; return; }
    const unsigned long long key = D.hkey_b[q];
    int64_t lo = 0, hi = q;   // the head of the run: the first position whose hash is not below this one
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (D.hkey_b[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    const int32_t n = D.tree_ent[t];
    const int64_t a = S.tree_off[t];
    int32_t rep = t;
    for (int64_t j = lo; j < q; j++) {
        const int32_t u = D.val_b[j];
        if (D.elig[u] == 0 || D.tree_ent[u] != n) continue;
        if (sig_equal(D.key_a, D.ent_cnt, a, D.key_a, D.ent_cnt, S.tree_off[u], n)) { rep = u; break; }
    }
    D.rep[t] = rep;
}

// Exclusive scan of (1, entries) over the reps in tree order, packed as classes << 32 | entries, in the manner of k_stitch_scan_*.
// The three kernels take the view V they scan over (tw_chist.h scans the classes a catalogue does not hold with them): V.packed(t)
// is item t's value, 0 = not counted; V.chunks() the per-workgroup sums [chunks + 1]; V.total(run) gets the sum over all items;
// V.emit(t, run) the sum over the items before a counted item t.
__device__ __forceinline__ unsigned long long sig_packed(const SigDev& D, int64_t t) {
    return D.rep[t] == (int32_t)t ? ((1ull << 32) | (unsigned long long)(uint32_t)D.tree_ent[t]) : 0ull;
}
struct SigScan {
    SigDev D;
    __device__ __forceinline__ unsigned long long packed(int64_t t) const { return sig_packed(D, t); }
    __device__ __forceinline__ unsigned long long* chunks() const { return D.chunk_sum; }
    __device__ __forceinline__ void total(unsigned long long run) const {
        D.counters[6] = run;
        D.class_off[run >> 32] = (int64_t)(run & 0xffffffffull);   // the end of the last class' entries
    }
    __device__ __forceinline__ void emit(int64_t t, unsigned long long run) const {
        const int64_t c = (int64_t)(run >> 32);
        D.tree_class[t] = (int32_t)c;
        D.class_rep[c] = (int32_t)t;
        D.class_off[c] = (int64_t)(run & 0xffffffffull);
        D.class_trees[c] = 0;
        D.class_sum[c] = 0;
        D.class_min[c] = INT64_MAX;
        D.class_max[c] = INT64_MIN;
    }
};
template <class V>
__device__ __forceinline__ unsigned long long sig_thread_sum(const V& v, int64_t first, int64_t n) {
    unsigned long long sum = 0;
    for (int k = 0; k < kSigScanItems; k++)
        if (first + k < n) sum += v.packed(first + k);
    return sum;
}

template <class V>
__global__ void __launch_bounds__(256) k_sig_scan_sums(V v, int64_t n) {
    __shared__ unsigned long long sh[256];
    const int64_t first = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * kSigScanItems;
    sh[threadIdx.x] = sig_thread_sum(v, first, n);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (int t = 0; t < (int)blockDim.x; t++) total += sh[t];
        v.chunks()[blockIdx.x] = total;
    }
}

template <class V>
__global__ void __launch_bounds__(256) k_sig_scan_chunks(V v, int64_t n_chunks) {
    __shared__ unsigned long long sh[256];
    unsigned long long* chunk_sum = v.chunks();
    const int64_t per = (n_chunks + blockDim.x - 1) / blockDim.x;
    const int64_t lo = stitch_min((int64_t)threadIdx.x * per, n_chunks), hi = stitch_min(lo + per, n_chunks);
    unsigned long long sum = 0;
    for (int64_t c = lo; c < hi; c++) sum += chunk_sum[c];
    sh[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < (int)blockDim.x; t++) { const unsigned long long x = sh[t]; sh[t] = run; run += x; }
        v.total(run);
    }
    __syncthreads();
    unsigned long long run = sh[threadIdx.x];
    for (int64_t c = lo; c < hi; c++) { const unsigned long long x = chunk_sum[c]; chunk_sum[c] = run; run += x; }
}

template <class V>
__global__ void __launch_bounds__(256) k_sig_scan_write(V v, int64_t n) {
    __shared__ unsigned long long sh[256];
    const int64_t first = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * kSigScanItems;
    sh[threadIdx.x] = sig_thread_sum(v, first, n);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < (int)blockDim.x; t++) { const unsigned long long x = sh[t]; sh[t] = run; run += x; }
    }
    __syncthreads();
    unsigned long long run = v.chunks()[blockIdx.x] + sh[threadIdx.x];
    for (int k = 0; k < kSigScanItems; k++) {
        const int64_t t = first + k;
        if (t >= n) break;
        const unsigned long long x = v.packed(t);
        if (x != 0) {
            v.emit(t, run);
            run += x;
        }
    }
}

__global__ void __launch_bounds__(256) k_sig_classes(StitchDev S, SigDev D, int64_t n_trees) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_trees) return;
    const int32_t rep = D.rep[t];
    if (rep < 0) { D.tree_class[t] = -1; return; }
    const int32_t c = D.tree_class[rep];   // (of a rep: written by k_sig_scan_write)
    const int64_t lat = S.tree_latency[t];
    atomicAdd((unsigned long long*)&D.class_trees[c], 1ull);
    atomicAdd((unsigned long long*)&D.class_sum[c], (unsigned long long)lat);
    atomicMin((long long*)&D.class_min[c], (long long)lat);
    atomicMax((long long*)&D.class_max[c], (long long)lat);
    if (rep != (int32_t)t) { D.tree_class[t] = c; return; }
    const int64_t a = S.tree_off[t], at = D.class_off[c];
    const int32_t n = D.tree_ent[t];
    for (int32_t i = 0; i < n; i++) {
        const unsigned long long key = D.key_a[a + i];
        int32_t* out = D.class_entries + 4 * (at + i);
        out[0] = (int32_t)(key >> (kSigCallerBits + kSigGroupBits));
        out[1] = D.mode == 1 ? (int32_t)((key >> kSigGroupBits) & ((1ull << kSigCallerBits) - 1ull)) - 1 : 0;
        out[2] = (int32_t)(key & ((1ull << kSigGroupBits) - 1ull));
        out[3] = D.ent_cnt[a + i];
    }
}

__global__ void __launch_bounds__(256) k_sig_compare(StitchDev S, SigDev D, int64_t n_trees) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool found = false, same = false;
    if (t < n_trees) {
        if (D.elig[t] != 0) {
            const int32_t R = S.tree_root[t];
            const int32_t n = D.ref_n[R];
            if (n >= 0) {
                found = true;
                same = n == D.tree_ent[t] && sig_equal(D.key_a, D.ent_cnt, S.tree_off[t], D.ref_key, D.ref_cnt, D.ref_pos[R], n);
            }
        }
        D.tree_same[t] = found ? (same ? 1 : 0) : 255;
    }
    const unsigned long long f = __ballot(found), s = __ballot(same);
    if ((threadIdx.x & 63) == 0) {
        if (f != 0) atomicAdd(&D.counters[4], (unsigned long long)__popcll(f));
        if (s != 0) atomicAdd(&D.counters[5], (unsigned long long)__popcll(s));
    }
}

// (ref_n cleared to -1 and the entry arrays copied by the host)
__global__ void __launch_bounds__(256) k_sig_keep(StitchDev S, SigDev D, int64_t n_trees) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_trees || D.elig[t] == 0) return;
    const int32_t R = S.tree_root[t];
    D.ref_n[R] = D.tree_ent[t];
    D.ref_pos[R] = S.tree_off[t];
}

}  // namespace tw

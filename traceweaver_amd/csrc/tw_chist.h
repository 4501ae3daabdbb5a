// tw_chist.h -- the call-graph classes of batch after batch kept in a catalogue on the device (tw_class_history_*).
//
// Replaces: FindUniqueCGs / PreparePerCGData of the reference run over a whole directory of traces (alibaba-analysis/analysis.py:
// 214-221, 233-292): classes whose numbers hold across batches, with per-class and per-entry figures that add up across them.  The
// catalogue holds what tw_trace_signatures and tw_class_profiles leave of a batch (class_off / class_entries, the per-class figures,
// the nine cells per entry) for C classes of its own; a push finds every class of the batch in it or appends it, then adds the
// batch's figures.  include/traceweaver_amd.h has the definitions.
//
//   k_chist_check       (tw_class_history_merge only) one lane per entry of the uploaded source: its class by a search of the
//                       offsets, the ranges of level, cg, g and count, and (level, cg, g) strictly above the entry before it in the class
//   k_chist_lookup      one wavefront per kChistPack consecutive source classes.  Hash: the lanes stride over the chunk's entries, which
//                       lie behind one another (a long class is walked by all 64 lanes, short ones share a sweep); one round per
//                       distinct class among the lanes sums mix(key, count, position) -- the sum of k_sig_sign, so that the hash needs
//                       the entries alone --, the number of entries is folded in.  Lookup: the wavefront probes the table class by
//                       class in lock step; where a slot's hash bits match, the lanes compare the entries sixteen bytes each, coalesced
//                       on both sides, and a ballot decides.  The hash buckets, it never decides equality.  A hit marks the class with
//                       the call's serial number: a second source class that hits the same one finds the mark (a duplicate).
//   k_sig_scan_*        (tw_sig.h, over ChistScan) exclusive scan of (1, entries) over the misses in source order: the new ids
//                       C + k and the offsets of their entries behind the store's
//   k_chist_append      one lane per new entry (copy, the identities of its nine cells) and per new class (the identities of its figures)
//   k_chist_insert      one lane per class: claims a slot of the table by a 64-bit compare-and-swap on (hash bits << 32 | id + 1);
//                       with `check` a slot taken by another new class with the same hash bits is compared entry by entry (two equal
//                       classes in one source).  Over [0, C) without `check` it is the rehash of a grown table.
//   k_chist_accumulate  one lane per source entry (nine cells, the source side coalesced) and per source class.  Source -> catalogue is
//                       injective within a call: plain loads and stores.
//   k_chist_derive      (tw_class_history_get) one lane per class over its entries: class_path_time, class_top_entry, as k_prof_classes
//
// Every output is a function of the inputs and of the order of the calls alone: integers throughout; where the table put a class
// depends on scheduling and is never returned; the only other atomics are the exchange of the marks and stores of the constant 1.
#pragma once
#include "tw_prof.h"

namespace tw {

#ifdef TW_TILE_SMALL   // the tiny table of the tests' host build: a few dozen classes refill it several times
constexpr int kChistSlots = 8;
constexpr int kChistPack = 4;
#else
constexpr int kChistSlots = 1024;    // the table's first capacity; it doubles (at least) whenever it would hold fewer than two slots per class
constexpr int kChistPack = 16;       // consecutive source classes a wavefront takes together
#endif
constexpr int kChistWaves = 4;
constexpr int kChistLevels = 1 << 16;
constexpr int kChistClassCols = 9;   // trees, latency_sum, latency_min, latency_max, counted, latency, first_epoch, last_epoch, seen
constexpr int kChistCounters = 4;    // new classes << 32 | new entries; a source error; a duplicate class in the source

struct ChistSrc {                    // the source of a call: the resident signature result and class profile, or the uploaded arrays
    int64_t n_classes, n_entries;
    const int64_t* off;              // [n_classes + 1]
    const int32_t* entries;          // [4 * n_entries]
    const int64_t* cls[kChistClassCols];   // per class, NULL = nothing to add (the epochs: `epoch`, seen: 1)
    const int64_t* cell[kProfCols];        // per entry, NULL = nothing to add
    int64_t epoch;
    int32_t mode, n_groups;
};

struct ChistDev {
    int64_t C, E;                    // classes and entries held before the call
    int64_t slots;                   // the table's capacity, a power of two (0: no table yet)
    unsigned long long* table;       // hash bits << 32 | id + 1, 0 = free
    int64_t* off;                    // [cls_cap + 1]
    int32_t* entries;                // [4 * ent_cap]
    unsigned long long *hash, *stamp;   // [cls_cap] the class' hash (for a rehash); the serial number of the last call that hit it
    int64_t* cls; int64_t cls_cap;   // [kChistClassCols][cls_cap]
    int64_t* cell; int64_t ent_cap;  // [kProfCols][ent_cap]
    // scratch of a call, per source class
    unsigned long long* src_hash;
    int32_t *src_id, *new_src;       // the catalogue id (-1 = not held); the source class of new class k
    unsigned long long* chunk_sum;
    unsigned long long* counters;    // [kChistCounters]
    unsigned long long serial;
    int32_t hash_bits;
};

__device__ __forceinline__ bool chist_same(const uint4& x, const uint4& y) { return x.x == y.x && x.y == y.y && x.z == y.z && x.w == y.w; }

__global__ void __launch_bounds__(256) k_chist_check(ChistSrc S, unsigned long long* counters) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S.n_entries) return;
    const int32_t* x = S.entries + 4 * i;
    bool bad = x[0] < 0 || x[0] >= kChistLevels || x[2] < 0 || x[2] >= S.n_groups || x[3] < 1;
    bad = bad || (S.mode == 1 ? (x[1] < -1 || x[1] >= S.n_groups) : x[1] != 0);
    const int64_t c = cmp_upper_bound(S.off, 0, S.n_classes + 1, i) - 1;   // (empty classes are stepped over)
    if (i > S.off[c]) {
        const int32_t* w = x - 4;
        const bool above = w[0] != x[0] ? w[0] < x[0] : w[1] != x[1] ? w[1] < x[1] : w[2] < x[2];
        bad = bad || !above;
    }
    if (bad) counters[1] = 1;
}

__global__ void __launch_bounds__(64 * kChistWaves) k_chist_lookup(ChistSrc S, ChistDev H, int mark) {
    __shared__ unsigned long long s_acc[kChistWaves][kChistPack];
    const int nl = (int)stitch_min(blockDim.x, 64), lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const int wpb = (int)stitch_max(blockDim.x / 64, 1);
    unsigned long long* acc = s_acc[wave];
    const unsigned long long mask = H.hash_bits >= 64 ? ~0ull : ((1ull << H.hash_bits) - 1ull);
    const uint4* src = (const uint4*)S.entries;
    const uint4* held = (const uint4*)H.entries;
    const int64_t n_chunks = (S.n_classes + kChistPack - 1) / kChistPack;
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < n_chunks; c += (int64_t)gridDim.x * wpb) {
        const int64_t c0 = c * kChistPack, c1 = stitch_min(c0 + kChistPack, S.n_classes);
        const int64_t a = S.off[c0], total = S.off[c1] - a;
        for (int k = lane; k < kChistPack; k += nl) acc[k] = 0;
        stitch_wave_sync();
        for (int64_t k0 = 0; k0 < total; k0 += nl) {
            const int64_t k = k0 + lane;
            const bool has = k < total;
            int64_t t = c0;
            unsigned long long term = 0;
            if (has) {
                while (t + 1 < c1 && S.off[t + 1] <= a + k) t++;
                const uint4 x = src[a + k];
                const unsigned long long key = sig_pack((int32_t)x.x, (unsigned long long)(x.y + 1u), (int32_t)x.z);
                term = sig_mix(key ^ sig_mix(((unsigned long long)(uint32_t)(a + k - S.off[t]) << 32) | (unsigned long long)x.w));
            }
            // one round per distinct class among the lanes; the control flow is the same in every lane
            unsigned long long todo = __ballot(has);
            while (todo != 0) {
                const int leader = __ffsll((long long)todo) - 1;
                const int64_t kk = __shfl((long long)t, leader);
                const bool mine = has && t == kk;
                todo &= ~__ballot(mine);
                const unsigned long long s = dist_wave_sum(mine ? term : 0ull, nl);
                if (lane == 0) acc[kk - c0] += s;
            }
        }
        stitch_wave_sync();
        for (int64_t t = c0; t < c1; t++) {   // the probes: every lane walks the same slots
            const int64_t at = S.off[t], n = S.off[t + 1] - at;
            const unsigned long long h = sig_mix(acc[t - c0] + 0x9e3779b97f4a7c15ull * (unsigned long long)(uint32_t)n) & mask;
            int32_t id = -1;
            if (H.slots > 0) {
                const unsigned long long m = (unsigned long long)H.slots - 1ull;
                for (unsigned long long slot = h & m;; slot = (slot + 1ull) & m) {
                    const unsigned long long v = H.table[slot];
                    if (v == 0) break;
                    if ((v >> 32) != (h >> 32)) continue;
                    const int32_t u = (int32_t)(v & 0xffffffffull) - 1;
                    const int64_t ua = H.off[u];
                    if (H.off[u + 1] - ua != n) continue;
                    bool differ = false;
                    for (int64_t j = lane; j < n; j += nl) differ = differ || !chist_same(src[at + j], held[ua + j]);
                    if (__ballot(differ) == 0) { id = u; break; }
                }
            }
            if (lane == 0) {
                H.src_hash[t] = h;
                H.src_id[t] = id;
                if (id >= 0 && mark != 0 && atomicExch(&H.stamp[id], H.serial) == H.serial) H.counters[2] = 1;
            }
        }
        stitch_wave_sync();   // ... before the next chunk clears the sums
    }
}

struct ChistScan {                   // the view k_sig_scan_* scan the misses over
    ChistSrc S;
    ChistDev H;
    __device__ __forceinline__ unsigned long long packed(int64_t t) const {
        return H.src_id[t] < 0 ? ((1ull << 32) | (unsigned long long)(uint32_t)(S.off[t + 1] - S.off[t])) : 0ull;
    }
    __device__ __forceinline__ unsigned long long* chunks() const { return H.chunk_sum; }
    __device__ __forceinline__ void total(unsigned long long run) const { H.counters[0] = run; }
    // (after the store has grown: the new class' id, hash, mark and the two ends of its entries -- its neighbour writes the same ends)
    __device__ __forceinline__ void emit(int64_t t, unsigned long long run) const {
        const int64_t k = (int64_t)(run >> 32), id = H.C + k, at = H.E + (int64_t)(run & 0xffffffffull);
        H.src_id[t] = (int32_t)id;
        H.new_src[k] = (int32_t)t;
        H.off[id] = at;
        H.off[id + 1] = at + (S.off[t + 1] - S.off[t]);
        H.hash[id] = H.src_hash[t];
        H.stamp[id] = H.serial;
    }
};

__device__ __forceinline__ int64_t chist_class_identity(int col) { return col == 2 || col == 6 ? INT64_MAX : col == 3 || col == 7 ? INT64_MIN : 0; }

__global__ void __launch_bounds__(256) k_chist_append(ChistSrc S, ChistDev H, int64_t new_classes, int64_t new_entries) {
    const int64_t n_work = stitch_max(new_classes, new_entries);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_work; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < new_entries) {
            const int64_t k = cmp_upper_bound(H.off + H.C, 0, new_classes + 1, H.E + i) - 1;   // (new classes without entries are stepped over)
            const int64_t t = H.new_src[k], j = H.E + i - H.off[H.C + k];
            ((uint4*)H.entries)[H.E + i] = ((const uint4*)S.entries)[S.off[t] + j];
            for (int col = 0; col < kProfCols; col++) H.cell[(int64_t)col * H.ent_cap + H.E + i] = (int64_t)prof_identity(col);
        }
        if (i < new_classes)
            for (int col = 0; col < kChistClassCols; col++) H.cls[(int64_t)col * H.cls_cap + H.C + i] = chist_class_identity(col);
    }
}

// The classes [lo, hi) into the table.  check: a slot that another class of [lo, hi) took with the same hash bits is compared (the
// classes below lo differ from these: the lookup missed them).
__global__ void __launch_bounds__(256) k_chist_insert(ChistDev H, int64_t lo, int64_t hi, int check) {
    const int64_t id = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= hi) return;
    const unsigned long long h = H.hash[id], m = (unsigned long long)H.slots - 1ull;
    const unsigned long long mine = ((h >> 32) << 32) | (unsigned long long)(uint32_t)(id + 1);
    const uint4* held = (const uint4*)H.entries;
    for (unsigned long long slot = h & m;; slot = (slot + 1ull) & m) {
        unsigned long long v = *(volatile unsigned long long*)&H.table[slot];
        if (v == 0) {
            v = atomicCAS(&H.table[slot], 0ull, mine);
            if (v == 0) return;
        }
        if (check != 0 && (v >> 32) == (h >> 32)) {   // (v: the class that holds the slot, whoever was first)
            const int64_t u = (int64_t)(v & 0xffffffffull) - 1;
            const int64_t a = H.off[id], n = H.off[id + 1] - a, ua = H.off[u];
            if (u >= lo && H.off[u + 1] - ua == n) {
                bool same = true;
                for (int64_t j = 0; j < n && same; j++) same = chist_same(held[a + j], held[ua + j]);
                if (same) H.counters[2] = 1;
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_chist_accumulate(ChistSrc S, ChistDev H, int what) {
    const int64_t n_work = stitch_max(S.n_classes, (what & 2) != 0 ? S.n_entries : 0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_work; i += (int64_t)gridDim.x * blockDim.x) {
        if ((what & 2) != 0 && i < S.n_entries) {
            const int64_t t = cmp_upper_bound(S.off, 0, S.n_classes + 1, i) - 1;
            const int64_t at = H.off[H.src_id[t]] + (i - S.off[t]);
            for (int col = 0; col < kProfCols; col++) {
                if (S.cell[col] == nullptr) continue;
                const int64_t v = S.cell[col][i];
                int64_t* p = H.cell + (int64_t)col * H.ent_cap + at;
                *p = col == kProfMin ? stitch_min(*p, v) : col == kProfMax ? stitch_max(*p, v) : (int64_t)((unsigned long long)*p + (unsigned long long)v);
            }
        }
        if (i < S.n_classes) {
            int64_t* p = H.cls + H.src_id[i];
            for (int col = 0; col < kChistClassCols; col++, p += H.cls_cap) {
                const bool wanted = col < 4 ? (what & 1) != 0 : col < 6 ? (what & 2) != 0 : true;
                if (!wanted || (S.cls[col] == nullptr && col < 6)) continue;
                const int64_t v = S.cls[col] != nullptr ? S.cls[col][i] : col == 8 ? 1 : S.epoch;
                *p = col == 2 || col == 6 ? stitch_min(*p, v) : col == 3 || col == 7 ? stitch_max(*p, v) : (int64_t)((unsigned long long)*p + (unsigned long long)v);
            }
        }
    }
}

// (the rule of k_prof_classes, over the catalogue's global entry indices)
__global__ void __launch_bounds__(256) k_chist_derive(ChistDev H, int64_t* path_time, int64_t* top_entry) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= H.C) return;
    int64_t sum = 0, top = -1, best = 0;
    for (int64_t i = H.off[c]; i < H.off[c + 1]; i++) {
        const int64_t pt = H.cell[5 * H.ent_cap + i];
        sum = (int64_t)((unsigned long long)sum + (unsigned long long)pt);
        if (H.cell[6 * H.ent_cap + i] != 0 && (top < 0 || pt > best)) { top = i; best = pt; }   // ties: the smallest index
    }
    path_time[c] = sum;
    top_entry[c] = top;
}

}  // namespace tw

// tw_cmp.h -- two cohorts of the latency distributions compared on the device (tw_compare_cohorts): the two-sample KS gap, twice the
// Mann-Whitney U, quantile shifts, and a permutation test of all three.
//
// Replaces: the comparison the delay-culprit query leaves to its reader, src/query_engine/delay_culprit.py:80-97 -- two lists of span
// latencies per service, looked at side by side -- and the numpy loop of traces.compare_distributions for cohort against cohort.
// It works on what tw_latency_distributions works on: the sorted values of every segment (DistDev: values, seg_off, seg_count).
// include/traceweaver_amd.h has the definitions (rows pair * (3 G + 1) + r, A and B, the pooled values M, the selection-sampling rule).
//
//   k_cmp_rank    one lane per item of every compared row (rows with an empty side own no lanes).  Two binary searches into the other
//                 side's slice give the item's position in M (A before B among equal values); the lane writes the value there (the
//                 pool) and, where it is the last item of a run of equal values, |g(x)| beside it (else ~0).  An item of A adds
//                 2 #{B > v} + #{B = v} to u2.  The lanes of a wavefront that meet on one row add their u2 and take the maximum of
//                 their |g| by shuffles; one lane per wavefront and row then does one atomicAdd and one atomicMax.
//   k_cmp_at      one lane per pool position: the least position whose |g| is the row's maximum, as an atomicMin by the first such
//                 lane per wavefront and row (the pool ascends, so the least position holds the smallest x).  The position is kept
//                 instead of the sign-flipped value: it orders the same way and the value is read back from the pool.
//   k_cmp_final   one lane per row: sizes, ks_at = pool[position], ks_gap = g(ks_at) by two searches (the sign), u2, the quantile
//                 shifts (gathers at the index of k_dist_quantiles), and perm_* = 0 (the row will be permuted) or -1.
//   k_cmp_perm    one wavefront per (row, block of 64 permutations), lane = permutation.  The walk over M is sequential; its index k
//                 is the same in every lane, so M[k] is one load for the wavefront, and the end of a run is a uniform branch.  Per
//                 lane: c (items given to A'), c at the start of the run, the running maximum of |g|, u2, and 8 + 8 quantile captures
//                 (the position in M, 32 bits; the values are gathered after the walk) in fixed unrolled arrays (registers, no scratch).  A lane stops hashing once n_a - c is 0 or N - k.  The counts of
//                 permutations at least as extreme leave the wavefront as one ballot / popcount add per statistic.
//
// Every output is a function of the inputs alone: integers throughout but the one product prob * n of the quantile index (a single
// binary64 multiplication); the atomics are integer adds, maxima and minima of which only the result is read.
#pragma once
#include "tw_dist.h"

namespace tw {

constexpr int kCmpMaxPairs = 64;
constexpr int kCmpMaxQ = 8;
constexpr int kCmpMaxPerm = 65536;
constexpr int kCmpWaves = 4;
constexpr unsigned long long kCmpGold = 0x9E3779B97F4A7C15ull;
constexpr unsigned long long kCmpNone = ~0ull;   // gabs of an item that does not end a run; ks_pos before the first candidate

struct CmpDev {
    int32_t n_pairs, n_q, n_perm;
    int64_t per;                     // 3 G + 1
    int64_t n_rows, n_items;         // n_pairs * per; the sum of n_a + n_b over the rows with both sides non-empty
    int64_t max_pool;
    unsigned long long seed;
    double probs[kCmpMaxQ];
    const int32_t* pairs;            // [n_pairs][2]
    const int64_t* row_off;          // [n_rows + 1]: row owns pool[row_off[row] .. row_off[row + 1])
    int64_t* pool;                   // [n_items]
    unsigned long long* gabs;        // [n_items]
    unsigned long long *ks_abs, *ks_pos, *u2_acc;   // [n_rows]
    int64_t *n_a, *n_b, *ks_gap, *ks_at, *u2, *ge_ks, *ge_u;   // [n_rows]
    int64_t *shift, *ge_q;           // [n_rows][n_q]
};

// first position in [a, b) whose value is above x
__device__ __forceinline__ int64_t cmp_upper_bound(const int64_t* v, int64_t a, int64_t b, int64_t x) {
    while (a < b) {
        const int64_t mid = a + (b - a) / 2;
        if (v[mid] <= x) a = mid + 1;
        else b = mid;
    }
    return a;
}

// the row that owns pool position t: the last one whose offset is not above t (rows without items are stepped over)
__device__ __forceinline__ int32_t cmp_row_of(const CmpDev& M, int64_t t) { return (int32_t)(cmp_upper_bound(M.row_off, 0, M.n_rows + 1, t) - 1); }

__device__ __forceinline__ unsigned long long cmp_abs(int64_t v) { return v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v; }

__device__ __forceinline__ int64_t cmp_q_index(double p, int64_t n) { return stitch_min(n - 1, (int64_t)(p * (double)n)); }

__device__ __forceinline__ bool cmp_permuted(const CmpDev& M, int64_t na, int64_t nb) {
    return M.n_perm > 0 && na > 0 && nb > 0 && (M.max_pool == 0 || na + nb <= M.max_pool);
}

struct CmpRow {                      // the two segments of a row
    int64_t a0, na, b0, nb;
};
__device__ __forceinline__ CmpRow cmp_row(const DistDev& D, const CmpDev& M, int64_t row) {
    const int64_t pi = row / M.per, r = row - pi * M.per;
    const int64_t sa = (int64_t)M.pairs[2 * pi] * M.per + r, sb = (int64_t)M.pairs[2 * pi + 1] * M.per + r;
    return CmpRow{D.seg_off[sa], (int64_t)D.seg_count[sa], D.seg_off[sb], (int64_t)D.seg_count[sb]};
}

__device__ __forceinline__ unsigned long long cmp_wave_max(unsigned long long v, int nl) {
    for (int off = 32; off >= 1; off >>= 1)
        if (off < nl) v = dist_umax(v, (unsigned long long)__shfl_xor((long long)v, off));
    return v;
}

__global__ void __launch_bounds__(256) k_cmp_rank(DistDev D, CmpDev M) {
    const int nl = (int)stitch_min(blockDim.x, 64), lane = threadIdx.x % 64;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < M.n_items; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = base + threadIdx.x;
        const bool has = t < M.n_items;
        int32_t row = -1;
        unsigned long long u = 0, ga = 0;   // ga: |g(x)| where the item ends a run, else 0 (no candidate for the maximum is lost: it is >= 0)
        if (has) {
            row = cmp_row_of(M, t);
            const CmpRow R = cmp_row(D, M, row);
            const int64_t off = M.row_off[row], li = t - off;
            const int64_t* v = D.values;
            int64_t x, pos, cA, cB;
            bool last;
            if (li < R.na) {
                x = v[R.a0 + li];
                const int64_t lb = dist_lower_bound(v, R.b0, R.b0 + R.nb, x) - R.b0;
                const int64_t ub = cmp_upper_bound(v, R.b0 + lb, R.b0 + R.nb, x) - R.b0;
                pos = li + lb;
                u = (unsigned long long)(2 * (R.nb - ub) + (ub - lb));
                last = ub == lb && (li + 1 == R.na || v[R.a0 + li + 1] != x);
                cA = li + 1; cB = ub;
            } else {
                const int64_t j = li - R.na;
                x = v[R.b0 + j];
                cA = cmp_upper_bound(v, R.a0, R.a0 + R.na, x) - R.a0;
                pos = j + cA;
                last = j + 1 == R.nb || v[R.b0 + j + 1] != x;
                cB = j + 1;
            }
            M.pool[off + pos] = x;   // (pos < n_a + n_b: the positions of a row are a permutation of its lanes)
            if (last) ga = cmp_abs(cA * R.nb - cB * R.na);
            M.gabs[off + pos] = last ? ga : kCmpNone;
        }
        // one round per distinct row among the lanes; the control flow is the same in every lane
        unsigned long long todo = __ballot(has);
        while (todo != 0) {
            const int leader = __ffsll((long long)todo) - 1;
            const int32_t k = __shfl(row, leader);
            const bool mine = has && row == k;
            const unsigned long long m = __ballot(mine);
            todo &= ~m;
            unsigned long long us = mine ? u : 0ull, gm = mine ? ga : 0ull;
            if (__popcll(m) > 1) {
                us = dist_wave_sum(us, nl);
                gm = cmp_wave_max(gm, nl);
            }
            if (lane == leader) {
                if (us != 0) atomicAdd(&M.u2_acc[k], us);
                if (gm != 0) atomicMax(&M.ks_abs[k], gm);
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_cmp_at(CmpDev M) {
    const int lane = threadIdx.x % 64;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < M.n_items; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = base + threadIdx.x;
        int32_t row = -1;
        bool cand = false;
        if (q < M.n_items) {
            row = cmp_row_of(M, q);
            const unsigned long long g = M.gabs[q];
            cand = g != kCmpNone && g == M.ks_abs[row];
        }
        unsigned long long todo = __ballot(cand);
        while (todo != 0) {   // the leader is the first candidate of its row in the wavefront: the least position among them
            const int leader = __ffsll((long long)todo) - 1;
            const int32_t k = __shfl(row, leader);
            todo &= ~__ballot(cand && row == k);
            if (lane == leader) atomicMin(&M.ks_pos[k], (unsigned long long)(q - M.row_off[k]));
        }
    }
}

__global__ void __launch_bounds__(256) k_cmp_final(DistDev D, CmpDev M) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= M.n_rows) return;
    const CmpRow R = cmp_row(D, M, row);
    const bool both = R.na > 0 && R.nb > 0;
    int64_t gap = 0, at = INT64_MIN, u2 = 0;
    if (both) {
        const unsigned long long pos = M.ks_pos[row];   // (a candidate exists: the last x of M has g = 0; the test keeps the read inside the row regardless)
        at = M.pool[M.row_off[row] + (pos < (unsigned long long)(R.na + R.nb) ? (int64_t)pos : 0)];
        const int64_t cA = cmp_upper_bound(D.values, R.a0, R.a0 + R.na, at) - R.a0, cB = cmp_upper_bound(D.values, R.b0, R.b0 + R.nb, at) - R.b0;
        gap = cA * R.nb - cB * R.na;
        u2 = (int64_t)M.u2_acc[row];
    }
    M.n_a[row] = R.na; M.n_b[row] = R.nb;
    M.ks_gap[row] = gap; M.ks_at[row] = at; M.u2[row] = u2;
    const int64_t ge = cmp_permuted(M, R.na, R.nb) ? 0 : -1;
    for (int j = 0; j < M.n_q; j++) {
        int64_t s = 0;
        if (both) s = D.values[R.b0 + cmp_q_index(M.probs[j], R.nb)] - D.values[R.a0 + cmp_q_index(M.probs[j], R.na)];
        M.shift[row * M.n_q + j] = s;
        if (M.n_perm > 0) M.ge_q[row * M.n_q + j] = ge;
    }
    if (M.n_perm > 0) { M.ge_ks[row] = ge; M.ge_u[row] = ge; }
}

// splitmix64's finaliser
__device__ __forceinline__ unsigned long long cmp_mix(unsigned long long x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// (h * m) >> 64 for m < 2^32: the high word's product cannot carry out of 64 bits with the low word's upper half added
__device__ __forceinline__ unsigned long long cmp_mulhi(unsigned long long h, uint32_t m) {
    const unsigned long long lo = (h & 0xFFFFFFFFull) * m, hi = (h >> 32) * m;
    return (hi + (lo >> 32)) >> 32;
}

__global__ void __launch_bounds__(64 * kCmpWaves) k_cmp_perm(CmpDev M) {
    const int nl = (int)stitch_min(blockDim.x, 64), lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const int wpb = (int)stitch_max(blockDim.x / 64, 1);
    const int64_t n_blk = (M.n_perm + 63) / 64, n_work = M.n_rows * n_blk;
    for (int64_t w = (int64_t)blockIdx.x * wpb + wave; w < n_work; w += (int64_t)gridDim.x * wpb) {
        const int32_t row = __builtin_amdgcn_readfirstlane((int32_t)(w / n_blk));   // (the same in every lane: the walk's loads and branches are scalar)
        const int32_t blk = __builtin_amdgcn_readfirstlane((int32_t)(w % n_blk));
        const int64_t na = M.n_a[row], nb = M.n_b[row], N = na + nb;
        if (!cmp_permuted(M, na, nb)) continue;
        const int64_t* __restrict__ pool = M.pool + M.row_off[row];
        const unsigned long long obs_ks = cmp_abs(M.ks_gap[row]), obs_u = cmp_abs(M.u2[row] - na * nb);
        const unsigned long long row_key = cmp_mix(M.seed + kCmpGold * (unsigned long long)(row + 1));
        const uint32_t n32 = (uint32_t)N, na32 = (uint32_t)na;   // N < 2^32: the walk counts in 32 bits
        const int nq = M.n_q;
        uint32_t ia[kCmpMaxQ], ib[kCmpMaxQ];                      // ~0: no quantile (a count stays below N <= 2^32 - 1)
        unsigned long long obs_q[kCmpMaxQ];
#pragma unroll
        for (int j = 0; j < kCmpMaxQ; j++) {
            const bool on = j < M.n_q;
            ia[j] = on ? (uint32_t)cmp_q_index(M.probs[j], na) : ~0u;
            ib[j] = on ? (uint32_t)cmp_q_index(M.probs[j], nb) : ~0u;
            obs_q[j] = on ? cmp_abs(M.shift[(int64_t)row * M.n_q + j]) : 0ull;
        }
        for (int sub = lane; sub < 64; sub += nl) {
            const int64_t p = (int64_t)blk * 64 + sub;
            const bool active = p < M.n_perm;
            unsigned long long big = 0, u2 = 0;
            uint32_t qa[kCmpMaxQ], qb[kCmpMaxQ];   // where in M the quantiles of A' and B' lie (the values are read after the walk)
#pragma unroll
            for (int j = 0; j < kCmpMaxQ; j++) { qa[j] = 0; qb[j] = 0; }
            if (active) {
                const unsigned long long key = cmp_mix(row_key + kCmpGold * (unsigned long long)(p + 1));
                uint32_t c = 0, c0 = 0, run0 = 0;
                int64_t x = pool[0];
                for (uint32_t k = 0; k < n32; k++) {
                    const int64_t next = k + 1 < n32 ? pool[k + 1] : x;
                    const uint32_t rem = na32 - c, left = n32 - k;
                    const bool take = rem > 0 && (rem == left || cmp_mulhi(cmp_mix(key + kCmpGold * (unsigned long long)(k + 1)), left) < (unsigned long long)rem);
                    if (take) {
#pragma unroll
                        for (int j = 0; j < kCmpMaxQ; j++) if (j < nq && c == ia[j]) qa[j] = k;
                        c++;
                    } else {
                        const uint32_t cb = k - c;
#pragma unroll
                        for (int j = 0; j < kCmpMaxQ; j++) if (j < nq && cb == ib[j]) qb[j] = k;
                    }
                    if (k + 1 == n32 || next != x) {   // the end of a run of equal values
                        // 32-bit factors: g = c n_b - (k + 1 - c) n_a = c N - (k + 1) n_a, whose second product is the same in every lane
                        const uint32_t ra = c - c0, rb = (k + 1 - run0) - ra;
                        u2 += (unsigned long long)rb * (2ull * c0 + ra);
                        big = dist_umax(big, cmp_abs((int64_t)((unsigned long long)c * n32) - (int64_t)((unsigned long long)(k + 1) * na32)));
                        c0 = c; run0 = k + 1;
                    }
                    x = next;
                }
            }
            const unsigned long long b_ks = __ballot(active && big >= obs_ks);
            const unsigned long long b_u = __ballot(active && cmp_abs((int64_t)u2 - na * nb) >= obs_u);
            if (lane == 0) {
                if (b_ks != 0) atomicAdd((unsigned long long*)&M.ge_ks[row], (unsigned long long)__popcll(b_ks));
                if (b_u != 0) atomicAdd((unsigned long long*)&M.ge_u[row], (unsigned long long)__popcll(b_u));
            }
#pragma unroll
            for (int j = 0; j < kCmpMaxQ; j++) {
                if (j < M.n_q) {
                    const unsigned long long b_q = __ballot(active && cmp_abs(pool[qb[j]] - pool[qa[j]]) >= obs_q[j]);
                    if (lane == 0 && b_q != 0) atomicAdd((unsigned long long*)&M.ge_q[(int64_t)row * M.n_q + j], (unsigned long long)__popcll(b_q));
                }
            }
        }
    }
}

}  // namespace tw

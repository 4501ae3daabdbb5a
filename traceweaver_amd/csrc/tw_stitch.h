// tw_stitch.h -- from parent arrays to whole traces on the device (tw_set_span_rows / tw_stitch_traces).
//
// Replaces: ConstructEndToEndTraces (helpers/utils.py:216-252) and the join across services a caller of the engine
// otherwise writes.  The engine's result is one parent[E][n_in] array per service; a trace is what these arrays say
// *together*.  Two kinds of hop make up a trace:
//   server row -> client row of the same RPC   observed (both sides log the call): the span table's parent column
//   client row -> the request that made it     predicted: parent[e][i] = x  <=>  call x of endpoint e belongs to request i
// Their union is a forest over the span-table rows (`link[row]`, -1 = none); its trees are the reconstructed traces.  A
// hole (a call no request took, a skip span, a service that is not in the batch) stays a hole: the rows below it form a
// tree of their own, a *fragment*.  Ground truth never fills one.
//
//   k_stitch_init     link[row] = the observed hop of a server row, -1 otherwise; clears the per-row flags
//   k_stitch_links    one thread per (request, endpoint): link[out_row(x)] = in_row(i)
//   k_stitch_jump     pointer doubling on a packed (depth << 32 | root) word per row, double-buffered
//   k_stitch_count    root / depth columns, rows per root, the cycle check, rows whose tree differs from the true one
//   k_stitch_scan_*   exclusive scan of (trees, rows) over the roots in row order: trees in ascending order of root row
//   k_stitch_scatter  rows grouped by tree (CSR)
//   k_stitch_group    a tree's rows ordered by (start, row), one wavefront per kStitchTrees consecutive trees in LDS
//                     (a tree of more than kStitchCap rows: the same rank sort on global memory), and -- the rows are
//                     at hand -- the per-tree figures (stitch_stats: spans, latency, flags)
//
// Every output is a pure function of the inputs: the atomics are integer adds whose sum is all that is read (rows per
// root), cursors whose order of arrival the sort by (start, row) removes again, and stores of the constant 1.
#pragma once
#include "tw_device.h"

namespace tw {

#ifdef TW_TILE_SMALL   // the tiny tables of the tests' host build: both the packed and the global-memory route occur
constexpr int kStitchCap = 12;
constexpr int kStitchTrees = 4;
#else
constexpr int kStitchCap = 512;     // rows a wavefront sorts in LDS (12 B each; the shipped shapes' traces hold <= 200 spans)
constexpr int kStitchTrees = 16;    // consecutive trees a wavefront takes together when their rows fit
#endif
constexpr int kStitchMaxRounds = 32;   // 2^32 links: a chain longer than the table has rows is a cycle
constexpr int kStitchScanItems = 8;    // rows per thread of the scan kernels
constexpr int kStitchWaves = 4;        // wavefronts per workgroup of k_stitch_group

struct StitchDev {
    int64_t n_rows;
    // inputs (tw_set_span_rows)
    const int32_t *in_row, *out_row;   // layouts of in_start / out_start
    const int32_t* row_link;           // >= 0 observed caller / true parent, -1 root of the span table, -2 caller not in the table
    const uint8_t* row_kind;           // 1 server, 2 client, 0 absent
    const int64_t *row_start, *row_end;
    // forest
    int32_t* link;
    unsigned long long *state_a, *state_b;
    int32_t *root, *depth, *true_root;
    uint8_t *una, *bad;                // per row: a request with an unassigned endpoint / root of a tree that differs from the true one
    // grouping
    int32_t* cursor;                   // rows per root, then the next free position of the root's tree
    unsigned long long* chunk_sum;
    int32_t *rows_tmp, *tree_rows, *tree_root;
    int64_t *tree_off, *tree_latency;
    uint8_t* tree_flags;
    unsigned long long* totals;        // [0] trees << 32 | rows, [1] whole traces, [2] trees with an unassigned endpoint, [3] exact trees
    int32_t* changed;                  // [kStitchMaxRounds] a round of k_stitch_jump moved some row
    int32_t* err;
};

__device__ __forceinline__ int64_t stitch_min(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t stitch_max(int64_t a, int64_t b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned long long stitch_seed(int32_t link, int64_t r) {
    return link >= 0 ? ((1ull << 32) | (unsigned long long)(uint32_t)link) : (unsigned long long)r;
}
__device__ __forceinline__ unsigned long long stitch_packed_count(int32_t c) {
    return c > 0 ? ((1ull << 32) | (unsigned long long)(uint32_t)c) : 0ull;
}

__global__ void __launch_bounds__(256) k_stitch_init(StitchDev S) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= S.n_rows) return;
    const int32_t l = S.row_link[r];
    S.link[r] = (S.row_kind[r] == 1 && l >= 0) ? l : -1;
    S.una[r] = 0;
    S.bad[r] = 0;
    S.cursor[r] = 0;
}

// src: the parent arrays of a pass, or the true ones (layout of tw_results.parent).  Span consumption gives a call to
// at most one request, so no two threads write the same link.
__global__ void __launch_bounds__(kTile) k_stitch_links(Dev P, StitchDev S, const int32_t* src) {
    const TileDev Tl = P.tiles[blockIdx.x];
    const UnitDev& U = P.units[Tl.unit];
    const int e = blockIdx.y, i = Tl.first + threadIdx.x;
    if (e >= U.E || i >= U.n_in) return;
    const int32_t x = src[ie_index(U, e, i)];
    const int32_t req = S.in_row[U.in_off + i];
    if (x >= 0) {
        if ((int64_t)x < U.ep_off[e + 1] - U.ep_off[e]) S.link[S.out_row[U.ep_off[e] + x]] = req;
    } else if (x == -1) {
        S.una[req] = 1;   // (-2, a skip span, is an answer: the request made no such call)
    }
}

// One round: state'[r] = (root of state[root of state[r]], sum of the two depths).  A root holds (0, itself).  In the
// first round the state is read off the link table (stitch_seed), so that it is never written in its initial form.
__global__ void __launch_bounds__(256) k_stitch_jump(StitchDev S, const unsigned long long* a, unsigned long long* b, int first, int round) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool moved = false;
    if (r < S.n_rows) {
        unsigned long long s = first ? stitch_seed(S.link[r], r) : a[r];
        const uint32_t p = (uint32_t)s;
        if ((int64_t)p != r) {
            const unsigned long long t = first ? stitch_seed(S.link[p], (int64_t)p) : a[p];
            if ((uint32_t)t != p) {
                moved = true;
                s = (((s >> 32) + (t >> 32)) << 32) | (unsigned long long)(uint32_t)t;
            }
        }
        b[r] = s;
    }
    const unsigned long long any = __ballot(moved);
    if (any != 0 && (threadIdx.x & 63) == 0) S.changed[round] = 1;
}

// The final state as columns.  A row that is its own root although it has a link sits on a cycle (a valid link table
// has none: a server row links to the client row of its RPC, a client row to a request of its own unit).
__global__ void __launch_bounds__(256) k_stitch_count(StitchDev S, const unsigned long long* state, int32_t* root_out, int32_t* depth_out,
                                                      int count, const int32_t* true_root) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= S.n_rows) return;
    const unsigned long long s = state[r];
    const int32_t R = (int32_t)(uint32_t)s;
    root_out[r] = R;
    if (depth_out != nullptr) depth_out[r] = (int32_t)(s >> 32);
    if ((int64_t)R == r && S.link[r] >= 0) *S.err = TW_ERR_ARG;
    if (count) atomicAdd(&S.cursor[R], 1);
    if (true_root != nullptr) {
        const int32_t T = true_root[r];
        if (T != R) { S.bad[R] = 1; S.bad[T] = 1; }
    }
}

// Exclusive scan of (1, rows) over the roots in row order, packed as trees << 32 | rows: a workgroup's share of
// blockDim * kStitchScanItems rows is summed, the sums are scanned by one workgroup, the third kernel writes per root its
// tree number, the tree's first position and the cursor k_stitch_scatter counts on from.
__device__ __forceinline__ unsigned long long stitch_thread_sum(const StitchDev& S, int64_t first) {
    unsigned long long sum = 0;
    for (int k = 0; k < kStitchScanItems; k++)
        if (first + k < S.n_rows) sum += stitch_packed_count(S.cursor[first + k]);
    return sum;
}

__global__ void __launch_bounds__(256) k_stitch_scan_sums(StitchDev S) {
    __shared__ unsigned long long sh[256];
    const int64_t first = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * kStitchScanItems;
    sh[threadIdx.x] = stitch_thread_sum(S, first);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (int t = 0; t < (int)blockDim.x; t++) total += sh[t];
        S.chunk_sum[blockIdx.x] = total;
    }
}

__global__ void __launch_bounds__(256) k_stitch_scan_chunks(StitchDev S, int64_t n_chunks) {
    __shared__ unsigned long long sh[256];
    const int64_t per = (n_chunks + blockDim.x - 1) / blockDim.x;
    const int64_t lo = stitch_min((int64_t)threadIdx.x * per, n_chunks), hi = stitch_min(lo + per, n_chunks);
    unsigned long long sum = 0;
    for (int64_t c = lo; c < hi; c++) sum += S.chunk_sum[c];
    sh[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < (int)blockDim.x; t++) { const unsigned long long v = sh[t]; sh[t] = run; run += v; }
        S.totals[0] = run;
        S.tree_off[run >> 32] = (int64_t)(run & 0xffffffffull);   // = n_rows: the end of the last tree
    }
    __syncthreads();
    unsigned long long run = sh[threadIdx.x];
    for (int64_t c = lo; c < hi; c++) { const unsigned long long v = S.chunk_sum[c]; S.chunk_sum[c] = run; run += v; }
}

__global__ void __launch_bounds__(256) k_stitch_scan_write(StitchDev S) {
    __shared__ unsigned long long sh[256];
    const int64_t first = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * kStitchScanItems;
    sh[threadIdx.x] = stitch_thread_sum(S, first);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < (int)blockDim.x; t++) { const unsigned long long v = sh[t]; sh[t] = run; run += v; }
    }
    __syncthreads();
    unsigned long long run = S.chunk_sum[blockIdx.x] + sh[threadIdx.x];
    for (int k = 0; k < kStitchScanItems; k++) {
        const int64_t r = first + k;
        if (r >= S.n_rows) break;
        const int32_t c = S.cursor[r];
        if (c > 0) {
            const int64_t t = (int64_t)(run >> 32);
            const int32_t at = (int32_t)(uint32_t)run;
            S.tree_off[t] = at;
            S.tree_root[t] = (int32_t)r;
            S.cursor[r] = at;
            run += stitch_packed_count(c);
        }
    }
}

__global__ void __launch_bounds__(256) k_stitch_scatter(StitchDev S) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= S.n_rows) return;
    S.rows_tmp[atomicAdd(&S.cursor[S.root[r]], 1)] = (int32_t)r;
}

__device__ __forceinline__ void stitch_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// k_stitch_stats of the design, run where the tree's rows are at hand: flags bit 0 the root is a root of the span table
// (a whole trace), bit 1 some request of the tree has an unassigned endpoint, bit 2 (truth set) the tree is whole and
// its row set is the true trace's.
__device__ __forceinline__ void stitch_stats(const StitchDev& S, int64_t t, int64_t latest_end, bool una, int has_truth,
                                             unsigned& n_whole, unsigned& n_una, unsigned& n_exact) {
    const int32_t R = S.tree_root[t];
    const bool whole = S.row_kind[R] == 1 && S.row_link[R] == -1;
    const bool exact = has_truth != 0 && whole && S.bad[R] == 0;
    S.tree_latency[t] = latest_end - S.row_start[R];
    S.tree_flags[t] = (uint8_t)((whole ? 1 : 0) | (una ? 2 : 0) | (exact ? 4 : 0));
    n_whole += whole; n_una += una; n_exact += exact;
}

__global__ void __launch_bounds__(64 * kStitchWaves) k_stitch_group(StitchDev S, int has_truth) {
    __shared__ int64_t s_key[kStitchWaves][kStitchCap];
    __shared__ int32_t s_row[kStitchWaves][kStitchCap];
    const int nl = (int)stitch_min(blockDim.x, 64), lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const int wpb = (int)stitch_max(blockDim.x / 64, 1);
    int64_t* key = s_key[wave];
    int32_t* row = s_row[wave];
    const int64_t n_trees = (int64_t)(S.totals[0] >> 32);
    const int64_t n_chunks = (n_trees + kStitchTrees - 1) / kStitchTrees;
    unsigned n_whole = 0, n_una = 0, n_exact = 0;
    for (int64_t c = (int64_t)blockIdx.x * wpb + wave; c < n_chunks; c += (int64_t)gridDim.x * wpb) {
        const int64_t c0 = c * kStitchTrees, c1 = stitch_min(c0 + kStitchTrees, n_trees);
        const bool packed = S.tree_off[c1] - S.tree_off[c0] <= kStitchCap;
        // the chunk's trees together when their rows fit, else tree by tree
        for (int64_t t0 = c0; t0 < c1; t0 = packed ? c1 : t0 + 1) {
            const int64_t t1 = packed ? c1 : t0 + 1;
            const int64_t a = S.tree_off[t0];
            const int m = (int)stitch_min(S.tree_off[t1] - a, (int64_t)kStitchCap + 1);
            if (m <= kStitchCap) {
                for (int k = lane; k < m; k += nl) {
                    const int32_t r = S.rows_tmp[a + k];
                    row[k] = r;
                    key[k] = S.row_start[r];
                }
                stitch_wave_sync();
                for (int k = lane; k < m; k += nl) {
                    int64_t t = t0;
                    while (t + 1 < t1 && S.tree_off[t + 1] <= a + k) t++;
                    const int lo = (int)(S.tree_off[t] - a), hi = (int)(S.tree_off[t + 1] - a);
                    const int64_t kk = key[k];
                    const int32_t rk = row[k];
                    int rank = 0;
                    for (int j = lo; j < hi; j++) rank += (key[j] < kk || (key[j] == kk && row[j] < rk)) ? 1 : 0;
                    S.tree_rows[a + lo + rank] = rk;
                }
                stitch_wave_sync();   // every lane has read the start times before they make room for the end times
                for (int k = lane; k < m; k += nl) {
                    const int32_t r = row[k];
                    key[k] = S.row_end[r];
                    row[k] = S.una[r];
                }
                stitch_wave_sync();
                for (int64_t t = t0 + lane; t < t1; t += nl) {
                    const int lo = (int)(S.tree_off[t] - a), hi = (int)(S.tree_off[t + 1] - a);
                    int64_t latest = key[lo];
                    bool una = false;
                    for (int j = lo; j < hi; j++) { latest = stitch_max(latest, key[j]); una = una || row[j] != 0; }
                    stitch_stats(S, t, latest, una, has_truth, n_whole, n_una, n_exact);
                }
                stitch_wave_sync();   // ... and the figures before the next trees overwrite them
            } else {
                // a tree that outgrows the wavefront's LDS: the same rank sort on global memory (quadratic in the tree's rows)
                const int64_t n = S.tree_off[t0 + 1] - a;
                int64_t latest = INT64_MIN;
                int una = 0;
                for (int64_t k = lane; k < n; k += nl) {
                    const int32_t rk = S.rows_tmp[a + k];
                    const int64_t kk = S.row_start[rk];
                    int64_t rank = 0;
                    for (int64_t j = 0; j < n; j++) {
                        const int32_t rj = S.rows_tmp[a + j];
                        const int64_t kj = S.row_start[rj];
                        rank += (kj < kk || (kj == kk && rj < rk)) ? 1 : 0;
                    }
                    S.tree_rows[a + rank] = rk;
                    latest = stitch_max(latest, S.row_end[rk]);
                    una |= S.una[rk];
                }
                for (int off = 32; off >= 1; off >>= 1)
                    if (off < nl) { latest = stitch_max(latest, (int64_t)__shfl_xor((long long)latest, off)); una |= __shfl_xor(una, off); }
                if (lane == 0) stitch_stats(S, t0, latest, una != 0, has_truth, n_whole, n_una, n_exact);
            }
        }
    }
    for (int off = 32; off >= 1; off >>= 1)
        if (off < nl) { n_whole += __shfl_xor(n_whole, off); n_una += __shfl_xor(n_una, off); n_exact += __shfl_xor(n_exact, off); }
    if (lane == 0) {
        if (n_whole) atomicAdd(&S.totals[1], (unsigned long long)n_whole);
        if (n_una) atomicAdd(&S.totals[2], (unsigned long long)n_una);
        if (n_exact) atomicAdd(&S.totals[3], (unsigned long long)n_exact);
    }
}

}  // namespace tw

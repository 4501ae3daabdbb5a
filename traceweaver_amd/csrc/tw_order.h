// tw_order.h -- the call-order DAG from timestamps alone (no ground truth).
//
// Replaces: FindConstraintsUsingFit (executor.py:152-212), the reference's greedy search over ordered endpoint pairs: add the
// edge a -> b, run FindAssignments, keep the edge iff no request is left unassigned -- up to E(E-1) full solves per service.
// The search itself runs on the host (traceweaver_amd/order.py); this file holds its two device pieces:
//   k_order_bound    a necessary condition per ordered pair, from the timestamps alone: the solves it proves to fail are never run
//   k_order_gather   the staged span table of a batch (endpoints in partition-key order) gathered into the topological order
//                    of a candidate graph, device to device: a candidate costs no upload of spans
//
// The bound.  Endpoints in partition-key order, every list sorted by (start, end).  viol[a][b] = the number of requests r for
// which no pair (x of a, y of b) has x and y contained in r (in_start <= start, end <= in_end) and end_a[x] <= start_b[y]; every
// comparison is non-strict.  Per (request, endpoint) two values decide it:
//   m_e(r)  the earliest end   among the endpoint's spans contained in r   (INT64_MAX if there is none)
//   M_e(r)  the latest start   among them                                  (INT64_MIN if there is none)
// and the pair is violated iff m_a(r) > M_b(r) -- which the two sentinels make true whenever either endpoint holds no contained
// span.  A request without a feasible tuple is counted in cnt_unassigned (traceweaver_v3.py:1201-1217), so viol[a][b] > 0
// proves that the reference's test of the edge a -> b fails.  Integer arithmetic only; the atomics are 64-bit integer adds of
// which only the sum is read: the table does not depend on scheduling.
#pragma once
#include "tw_device.h"

namespace tw {

struct OrderBoundDev {
    const int64_t* unit_in_off;   // [n_units + 1]
    const int32_t* unit_E;        // [n_units]
    const int64_t* ep_base;       // [n_units]  index of the unit's first endpoint in ep_off
    const int64_t* ep_off;        // global offsets into out_start / out_end (tw_batch layout)
    const int64_t* viol_off;      // [n_units]  base of the unit's E x E block in viol
    const int64_t *in_start, *in_end, *out_start, *out_end;
    unsigned long long* viol;     // [sum E * E], zeroed by the caller
};

// One lane per request (blockIdx.y = unit), a loop over the endpoints: a binary search for the first start >= in_start[r], a walk
// while start <= in_end[r]; the E x E comparison in registers; per pair a ballot and one atomic add per wavefront.
__global__ void k_order_bound(OrderBoundDev O) {
    const int u = blockIdx.y;
    const int64_t base = O.unit_in_off[u], n = O.unit_in_off[u + 1] - base;
    const int E = O.unit_E[u];
    const int64_t* eo = O.ep_off + O.ep_base[u];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    int64_t m[kMaxEp], M[kMaxEp];
#pragma unroll
    for (int e = 0; e < kMaxEp; e++) {
        m[e] = INT64_MAX; M[e] = INT64_MIN;
        if (live && e < E) {
            const int64_t lo_t = O.in_start[base + i], hi_t = O.in_end[base + i];
            const int64_t a = eo[e], len = eo[e + 1] - a;
            int64_t lo = 0, hi = len;
            while (lo < hi) {   // first span with start >= in_start[r]
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (O.out_start[a + mid] < lo_t) lo = mid + 1; else hi = mid;
            }
            for (int64_t x = lo; x < len; x++) {
                const int64_t s = O.out_start[a + x];
                if (s > hi_t) break;
                const int64_t t = O.out_end[a + x];
                if (t <= hi_t) { m[e] = t < m[e] ? t : m[e]; M[e] = s > M[e] ? s : M[e]; }
            }
        }
    }
    unsigned long long* v = O.viol + O.viol_off[u];
#pragma unroll
    for (int a = 0; a < kMaxEp; a++)
#pragma unroll
        for (int b = 0; b < kMaxEp; b++)
            if (a != b && a < E && b < E) {   // (uniform: E is the unit's)
                const unsigned long long mask = __ballot(live && m[a] > M[b]);
                if ((threadIdx.x & 63) == 0 && mask != 0) atomicAdd(&v[a * E + b], (unsigned long long)__popcll(mask));
            }
}

// Segment copies of the staged table: segment g = blockIdx.y moves len[g] (start, end) pairs from src[g] to dst[g].
struct OrderGatherDev {
    const int64_t *seg_src, *seg_dst, *seg_len;   // [n_seg]
    const int64_t *src_start, *src_end;
    int64_t *dst_start, *dst_end;
};

__global__ void k_order_gather(OrderGatherDev G) {
    const int g = blockIdx.y;
    const int64_t s = G.seg_src[g], d = G.seg_dst[g], len = G.seg_len[g];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x) {
        G.dst_start[d + i] = G.src_start[s + i];
        G.dst_end[d + i] = G.src_end[s + i];
    }
}

}  // namespace tw

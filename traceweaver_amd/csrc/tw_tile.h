// tw_tile.h -- k_enumerate_tile<E>: the candidate-window builder and the short enumerations of a tile of incoming spans,
// by the whole workgroup (included by tw_kernels.h).
//
// Reference functions: FindCutoffs traceweaver_v3.py:182-217, DfsTraverseX / DfsTraverse3 :236-351 (feasibility :328-347),
// ScoreAssignmentAsPerInvocationGraph traceweaver_v1.py:305-361, the size-5 heap of traceweaver_v3.py:304-307.
//
// One workgroup per tile of P.tile_spans consecutive incoming spans of one service.  A thread per span only does what is
// per span (its cut-offs); everything else is spread over the lanes by *item*, so that a span with 60 tuples beside spans
// with two does not hold a wavefront (the per-thread kernel this replaces ran with a quarter of its lanes active and 744
// dependent global loads per wavefront):
//   1. cut-offs per span (pass 1: galloping searches in global memory, kept in c_lo / c_hi; pass 2 reads them back);
//   2. the union of the tile's candidate windows per endpoint -- neighbouring spans' windows overlap and the lists are in
//      start order, so the union is one contiguous slice -- is loaded ONCE, coalesced, into LDS as 32-bit offsets from the
//      tile's first start time; containment (traceweaver_v3.py:328-333) becomes a bit mask per (span, endpoint);
//   3. items = (span, endpoint, contained candidate): the root / closing terms (traceweaver_v1.py:349-357) are evaluated one
//      item per lane into LDS tables -- in pass 2 a term is a mixture log-likelihood of ~1.5 k instructions, and every lane
//      has one to evaluate;
//   4. grid points = (span, tuple of contained candidates), one per lane: call-order feasibility (traceweaver_v3.py:343-347),
//      the tuple's score from the tables in the reference's order of additions (bit-identical), tuple count and the
//      bitmap of candidates that occur in a feasible tuple;
//   5. the five largest tuples of a span by counting: rank = number of the span's tuples that are greater under Python's
//      order of (score, [spans]) -- score, then start_mus of the first differing span.  That order is a strict partial
//      order (two tuples whose first differing spans start together are incomparable), and CPython's heap returns exactly
//      the tuples of rank < 5, in rank order, whenever none of those is incomparable with another tuple of equal score:
//      such a tuple is comparable with everything, so whenever it is the root of the six-entry heap it is its true minimum,
//      has five greater tuples and rank >= 5 -- a tuple of rank < 5 is never popped.  A span where a tuple of rank < 5 has
//      an incomparable partner goes to the wavefront kernel, which replays CPython's heap push by push.  A span of more than
//      kRankDirect slots is counted among its survivors only: the tuples that reach a lower bound of its fifth-largest score.
// Spans whose enumeration is longer than kTileMax tuples, whose windows are wider than 32 spans or reach beyond the staged
// slice, or that are too long for 32-bit offsets go to the work lists of k_enumerate_heavy, as before.
#pragma once

namespace tw {

#ifndef TW_TILE_MAX
#define TW_TILE_MAX 256
#endif
constexpr int kTileMax = TW_TILE_MAX;   // largest enumeration (product of the contained candidates) the tile kernel takes itself
#ifndef TW_TILE_REPLAY_MAX
#define TW_TILE_REPLAY_MAX 256
#endif
constexpr int kTileReplayMax = TW_TILE_REPLAY_MAX;   // most feasible tuples of a span whose heap its own thread replays (phase 5b); the others go to the wavefront kernel
// Phase 5 ranks a span of more than kRankDirect (padded) tuple slots among its survivors only: the feasible tuples whose score reaches a
// lower bound L of the span's fifth-largest score.  Shorter spans keep the in-place loop over all their slots.
#ifndef TW_TILE_RANK_DIRECT
#define TW_TILE_RANK_DIRECT 32
#endif
constexpr int kRankDirect = TW_TILE_RANK_DIRECT;
constexpr int kRankMinLong = (kRankDirect & ~3) + 4;   // fewest slots of a long span (slot counts are multiples of four): the long spans of a segment start at least this far apart
constexpr int kRankBuckets = 5;                        // = kTopK disjoint subsets of a span's slots; L = the smallest of their maxima
static_assert(kRankDirect >= 24, "the maxima and counters of a segment's long spans lie in one byte per tuple slot");
// the upper half of a score's order-preserving unsigned key (-0.0 taken for +0.0 first): a score with a smaller key is strictly
// smaller, scores with equal keys may differ; no score has the key 0
__device__ __forceinline__ uint32_t score_key32(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v + 0.0);
    return (uint32_t)(((u >> 63) ? ~u : (u | (1ull << 63))) >> 32);
}
// items of a span before those of endpoint e (contained candidates per endpoint, 8 bits each, in pk)
__device__ __forceinline__ int pos_base(unsigned long long pk, int e) {
    int acc = 0;
    for (int f = 0; f < e; f++) acc += (int)((pk >> (8 * f)) & 255ull);
    return acc;
}
#ifndef TW_TILE_ITEMS
#define TW_TILE_ITEMS 768
#define TW_TILE_GRID 1024
#endif
// SPANS = incoming spans a workgroup serves: kTile, or kTile / 8 for the sub-tile launches of a class of few tiles (the deep call
// graphs of a small batch) -- with tables sized for those 16 spans: 15 KB of LDS instead of 48 KB.  (The sub-tile workgroups of one
// such class used to ask for all the LDS of the GPU, 912 x 43 KB; workgroups that need a third of a CU's LDS at once are not placed
// while smaller ones -- the wavefront kernels of the other classes -- keep taking what becomes free: the classes' tile kernels ran one
// after the other.)
constexpr int kSubTileSpans = kTile / 8;
#ifndef TW_TILE_PAIR_ITEMS
#define TW_TILE_PAIR_ITEMS 512
#define TW_TILE_PAIR_GRID 1024
#endif
// PAIR: the tables of the two-endpoint path (a span has at most 64 items; its tuple slots are not padded) -- a tile of the media
// shape holds about 420 items and 430 tuples, one segment.  As many slots as the general path: a tile of the saturated nodejs shape
// (840 items, 1 800 tuples) took 2.9 segments with 768 slots where the general path takes 2.4 -- every segment pays its barriers, a
// last trip of mostly idle lanes and a replay phase as long as its longest replay (profiles/HISTORY.md, "Round 10").  31.5 KB of LDS
template <int E, int SPANS = kTile, bool PAIR = false>
struct TileCfg {
#ifdef TW_TILE_SMALL   // host-emulation build of the tests: tiny tables, so that segments and slice overflows occur
    static constexpr int kSlice = 24, kItems = PAIR ? 2 * 32 : kMaxEp * 32, kGrid = kTileMax > 64 ? kTileMax : 64;
#else
    static constexpr int kSlice = SPANS < kTile ? 64 : (E <= 4 ? 192 : 160);   // outgoing spans staged per endpoint
    static constexpr int kItems = SPANS < kTile ? kMaxEp * 32 : (PAIR ? TW_TILE_PAIR_ITEMS : TW_TILE_ITEMS);   // (span, endpoint, candidate) items per segment of the tile
    static constexpr int kGrid = SPANS < kTile ? (kTileMax > 512 ? kTileMax : 512) : (PAIR ? TW_TILE_PAIR_GRID : TW_TILE_GRID);   // tuple slots per segment (a span's slots are padded to a multiple of four; PAIR: not padded)
#endif
    static_assert(kItems >= (PAIR ? 2 : kMaxEp) * 32 && kGrid >= ((kTileMax + 3) & ~3) && kGrid % 4 == 0, "a single span must fit a segment");
};

// rest / c for 0 <= rest <= 4096, 1 <= c <= 64: (rest + 0.5) / c is at least 0.5 / c away from an integer, far more than the
// rounding of the reciprocal and the product -- exact on the GPU (v_rcp_f32) and in the host emulation alike
__device__ __forceinline__ uint32_t div_small(uint32_t rest, uint32_t c) {
#ifdef TW_HOST_EMULATION
    const float rc = 1.0f / (float)c;
#else
    const float rc = __builtin_amdgcn_rcpf((float)c);
#endif
    return (uint32_t)(((float)rest + 0.5f) * rc);
}

// the value, as one the compiler takes for new: addresses formed from it are formed where they are used, not ahead of a loop and
// held in registers through it
__device__ __forceinline__ int fresh(int v) {
#ifndef TW_HOST_EMULATION
    asm volatile("" : "+v"(v));
#endif
    return v;
}

// Phase 5 of a segment for its long spans (more than kRankDirect slots), shared by the general and the two-endpoint path.  A long
// span's slots fall into five subsets by slot number mod 5; L = the smallest of the subsets' largest feasible scores (none: everything
// survives), taken on 32-bit keys as phase 4 forms the scores.  Five distinct tuples reach L, so a tuple whose key is below L has five
// strictly greater ones: rank >= 5, which is all that is ever stored of it.  A tuple that reaches L survives, and so does every tuple
// that is greater than or equal to it: its count of greater tuples, its equal partners and their comparisons are those of the whole
// span.  The survivors (about eleven of a span, all of them when the scores are equal) are listed twice: per span from the span's own
// first slot on, to be scanned, and in one list of the segment, a lane each.  A long span is found by its first slot / MINLONG (the
// fewest slots of a long span: the long spans of a segment start at least that far apart).
template <int GRID, int MINLONG>
struct SurvivorRanks {
    static constexpr int kLong = (GRID - MINLONG) / MINLONG + 1;
    static constexpr int kAuxWords = kLong * (kRankBuckets + 1) + 1;
    uint32_t* aux;          // [kLong][kRankBuckets] keys, 0: no feasible tuple; then [kLong] survivors of the span, [1]: of the segment
    uint8_t* g_rank;        // [GRID] the tuple's rank
    uint16_t* r_sub;        // [GRID] a span's survivors from its first slot on
    uint16_t* r_all;        // [GRID] the survivors of the segment
    const double* g_sc;     // [GRID] the scores of phase 4 (NaN: infeasible)
    const uint8_t* g_span;  // [GRID] the slot's span
    const int32_t* s_grid0; // prefix sums of the slots over the spans
    int g0;                 // ... of the segment's first span
    __device__ __forceinline__ uint32_t* r_max() const { return aux; }
    __device__ __forceinline__ int32_t* r_cnt() const { return reinterpret_cast<int32_t*>(aux + kLong * kRankBuckets); }
    __device__ __forceinline__ void clear(int t, int nt) const { for (int x = t; x < kAuxWords; x += nt) aux[x] = 0u; }
    // phase 4, a feasible tuple of a long span (slot g, the gi-th of its span): the largest key of the slot's subset
    __device__ __forceinline__ void note(int g, int gi, double sj) const {
        uint32_t* b = r_max() + ((g - gi) / MINLONG) * kRankBuckets + gi % kRankBuckets;
        const uint32_t key = score_key32(sj);
        if (key > *(volatile uint32_t*)b) atomicMax(b, key);   // (most lanes find a greater one there already)
    }
    // the survivors of the long spans into the two lists (the same trips for every lane: the appends are the wavefront's)
    __device__ __forceinline__ void collect(int nG, int tr, int nt) const {
        for (int gb = 0; gb < nG; gb += nt) {
            const int g = gb + tr, lane = tr & 63;
            bool surv = false;
            int sub0 = 0;   // a survivor: the first slot of its span
            if (g < nG) {
                const double my = g_sc[g];
                const int s = g_span[g];
                const int gs = s_grid0[s] - g0, ge = s_grid0[s + 1] - g0;
                if (ge - gs > kRankDirect && my == my) {
                    const uint32_t* b = r_max() + (gs / MINLONG) * kRankBuckets;
                    uint32_t lk = b[0];
#pragma unroll
                    for (int j = 1; j < kRankBuckets; j++) lk = b[j] < lk ? b[j] : lk;
                    surv = score_key32(my) >= lk;   // (lk = 0, a subset without a feasible tuple: everything survives)
                    sub0 = gs;
                }
            }
            const int at = wave_append(&r_cnt()[kLong], surv, lane);
            if (surv) r_all[at] = (uint16_t)g;
            // the span's own list: one atomic per wavefront and span that has survivors among the lanes
            unsigned long long todo = __ballot(surv);
            while (todo != 0ull) {
                const int leader = __ffsll((long long)todo) - 1;
                const int lead0 = __shfl(sub0, leader);
                const bool with = surv && sub0 == lead0;
                const unsigned long long m = __ballot(with);
                int base = 0;
                if (lane == leader) base = atomicAdd(&r_cnt()[lead0 / MINLONG], __popcll(m));
                base = __shfl(base, leader);
                if (with) r_sub[lead0 + base + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)g;
                todo &= ~m;
            }
        }
    }
    // a survivor per lane (behind a barrier after collect): the greater ones, the equal ones, among the survivors of its span.
    // mine_of(s, gi): what order(s, mine, hrel) needs of the tuple itself; order: +1 the other one (slot hrel of the span) is greater
    // under Python's order of equal scores, -1 smaller, 0 incomparable; undecided(s): a tuple of rank < 5 has an incomparable partner
    template <class MINE, class ORDER, class UNDECIDED>
    __device__ __forceinline__ void rank(int t, int nt, const MINE& mine_of, const ORDER& order, const UNDECIDED& undecided) const {
        const int nsv = r_cnt()[kLong];
        for (int k = t; k < nsv; k += nt) {
            const int g = r_all[k];
            const double my = g_sc[g];
            const int s = g_span[g];
            const int gs = s_grid0[s] - g0;
            const int n = r_cnt()[gs / MINLONG];
            const uint16_t* sub = r_sub + gs;
            int rank = 0, eq = 0;
            for (int h = 0; h < n && rank < kTopK; h++) {
                const double o = g_sc[sub[h]];
                rank += (o > my);
                eq += (o == my);
            }
            bool partner = false;
            if (eq > 1 && rank < kTopK) {
                const auto mine = mine_of(s, g - gs);
                for (int h = 0; h < n; h++) {
                    const int hg = sub[h];
                    if (hg == g || !(g_sc[hg] == my)) continue;
                    const int ord = order(s, mine, hg - gs);
                    if (ord > 0) rank++;
                    else if (ord == 0) partner = true;
                }
            }
            if (partner && rank < kTopK) undecided(s);
            g_rank[g] = (uint8_t)(rank < kTopK ? rank : kTopK);
        }
    }
};

// a term from the gap itself (score_term computes x = (double)(t2 - t1) and then exactly this)
__device__ __forceinline__ double score_term_gap(const Scorer& S, int slot, long long gap) {
    const double x = (double)gap;
    if (S.pass == 1) {
        const double* g = S.gp + slot * 4;
        return term_gauss(g[0], g[3], g[2], x);
    }
    return score_term_mix_x(S, slot, x);
}

// Optional phase timers (build with -DTW_PROFILE_TILE; read back through tw_debug_profile): 10 ns ticks of thread 0 of every
// workgroup of the class TW_PROFILE_TILE_E (4) per phase -- [0] cut-offs, [1] slices, [2] masks / lists / prefix sums, [3] terms, [4] tuples,
// [5] ranks, [6] results, [7] workgroup lifetime, [8] workgroups, [9] segments, [10] items, [11] tuples.  Compiled out by default.
#ifdef TW_PROFILE_TILE
#ifndef TW_PROFILE_TILE_E
#define TW_PROFILE_TILE_E 4   // the endpoint-count class that is timed
#endif
#define TW_TILE_T0() long long _tp = wall_clock64(); const long long _tb = _tp; long long _ta[7] = {0, 0, 0, 0, 0, 0, 0}
#define TW_TILE_TICK(k) do { const long long _n = wall_clock64(); _ta[k] += _n - _tp; _tp = _n; } while (0)
#define TW_TILE_COUNT(k, v) do { if (E == TW_PROFILE_TILE_E && threadIdx.x == 0) atomicAdd((unsigned long long*)&P.prof[k], (unsigned long long)(v)); } while (0)
#define TW_TILE_FLUSH() do { if (E == TW_PROFILE_TILE_E && threadIdx.x == 0) { for (int _k = 0; _k < 7; _k++) atomicAdd((unsigned long long*)&P.prof[_k], (unsigned long long)_ta[_k]); \
    atomicAdd((unsigned long long*)&P.prof[7], (unsigned long long)(wall_clock64() - _tb)); atomicAdd((unsigned long long*)&P.prof[8], 1ull); } } while (0)
#else
#define TW_TILE_T0() do {} while (0)
#define TW_TILE_TICK(k) do {} while (0)
#define TW_TILE_COUNT(k, v) do {} while (0)
#define TW_TILE_FLUSH() do {} while (0)
#endif

// (phase 5b's heap in registers took the kernel from 64 to 135 registers for four endpoints: three workgroups per CU where the LDS lets four
// in, 20.0 -> 20.3 ms on the headline.  Up to four endpoints the compiler is held to four wavefronts per SIMD -- 128 registers)
#ifdef TW_HOST_EMULATION
#define TW_TILE_ATTR
#else
#ifndef TW_TILE_PAIR_WAVES
// wavefronts per SIMD the two-endpoint path is compiled for.  5 fits (96 registers, no scratch, five workgroups per CU by its LDS) and makes the
// kernel itself shortest, but the step is shorter with 4 (the compiler then takes 97 registers): the class' tile kernel shares the SIMDs with the four-endpoint
// one, whose chain is the pass, and at five wavefronts it takes them from it (profiles/HISTORY.md, "Round 10")
#define TW_TILE_PAIR_WAVES 4
#endif
#define TW_TILE_ATTR __attribute__((amdgpu_waves_per_eu(SINGLE ? 8 : (PAIR ? TW_TILE_PAIR_WAVES : (E <= 4 ? 4 : 2)))))
#endif
// SINGLE (one endpoint only): a tuple is an item -- the lean path below, TW_TILE_SINGLE=0 launches the general one instead
// PAIR (two endpoints only): items named by their span's thread, a tuple decoded by one division, unpadded slots, tables sized for
// the class -- the second lean path below, TW_TILE_PAIR=0 launches the general one instead
template <int E, int SPANS = kTile, bool SINGLE = false, bool PAIR = false>
__global__ void __launch_bounds__(4 * kTile) TW_TILE_ATTR k_enumerate_tile(Dev P, int pass, const int32_t* tile_ids, int n_tiles_e, int sub_tiles) {
    static_assert(!SINGLE || E == 1, "the lean path is the one of a single endpoint");
    static_assert(!PAIR || (E == 2 && !SINGLE), "the pair path is the one of two endpoints");
    if (*P.err != 0) return;  // e.g. NaN parameters (hazard H3): nothing downstream is meaningful
    typedef TileCfg<E, SPANS, PAIR> C;
    constexpr int SL = C::kSlice;
    // sub_tiles > 1: a class of few tiles (the deep call graphs of a small batch: 57 tiles on 256 CUs, each a millisecond of
    // segments one after the other) is launched with sub_tiles workgroups per tile, each serving a stretch of the tile's spans
    const int vb = xcd_tile(blockIdx.x, n_tiles_e * sub_tiles);
    const int tile = tile_ids[vb / sub_tiles];
    const TileDev T = P.tiles[tile];
    const UnitDev& U = P.units[T.unit];
    const int t = threadIdx.x, nt = blockDim.x;
    const int sub_spans = P.tile_spans / sub_tiles, first = T.first + (vb % sub_tiles) * sub_spans;
    const int ns = min(sub_spans, min(P.tile_spans, U.n_in - T.first) - (vb % sub_tiles) * sub_spans);   // spans of this workgroup; thread t < ns owns span t
    if (ns <= 0) return;
    __shared__ int32_t s_is[SPANS], s_ie[SPANS];          // start / end of the incoming spans as offsets from `base`
    __shared__ int32_t sl_st[E][SL], sl_en[E][SL];        // the staged slice of every endpoint list, same offsets (clamped)
    __shared__ int32_t s_A[E], s_B[E];                    // the slice = positions [A, B) of the endpoint's list
    __shared__ uint16_t s_lo[E][SPANS];                   // first position of the span's window, relative to A
    __shared__ uint32_t s_cm[E][SPANS];                   // bit r: position lo + r holds a contained candidate
    __shared__ uint32_t s_bits[E][SPANS];                 // ... that occurs in a feasible tuple
    __shared__ int32_t s_item0[SPANS + 1], s_grid0[SPANS + 1], s_leaves[SPANS];
    __shared__ uint8_t s_amb[SPANS];
    __shared__ unsigned long long s_cn[SPANS];            // contained candidates per endpoint, 8 bits each
    __shared__ int32_t s_wtot[4 * kTile / 64][2];
    __shared__ double t_root[C::kItems], t_close[C::kItems];
    __shared__ uint16_t it_idx[C::kItems];                // slice position of the item's candidate
    __shared__ double g_sc[C::kGrid + (PAIR ? 4 : 0)];    // (PAIR: the rank loop reads four scores a step without padding)
    __shared__ uint8_t g_span[C::kGrid];                   // the tuple's span (tile-local); an infeasible grid point has score NaN
    __shared__ uint32_t g_aux[C::kGrid / 4];               // phase 5 of a segment: the long spans' subset maxima and survivor counts (the ranks themselves: in t_root)
    __shared__ int32_t s_segend, s_anyamb;                 // ... any span of the segment whose top five the ranks do not decide (phase 5b)
    const bool live = t < ns;
    const int i = first + (live ? t : 0);
    const int64_t base = P.in_start[U.in_off + first];
    const int64_t in_start = P.in_start[U.in_off + i], in_end = P.in_end[U.in_off + i];
    const int64_t* os[E];
    const int64_t* oe[E];
#pragma unroll
    for (int e = 0; e < E; e++) { os[e] = P.out_start + U.ep_off[e]; oe[e] = P.out_end + U.ep_off[e]; }
    for (int x = t; x < E; x += nt) { s_A[x] = 0x7fffffff; s_B[x] = 0; }
    // the unit's call-order DAG in (scalar) registers: predecessor masks, predecessor counts, and per endpoint the predecessor
    // list in in_edges() order packed 4 bits each (index | primary << 3)
    uint32_t dag_pm[E], dag_np[E], dag_pl[E];
    uint32_t ordered = 0;   // any call-order constraint at all?  (without: every grid point is a tuple)
#pragma unroll
    for (int e = 0; e < E; e++) {
        dag_pm[e] = U.pred_mask[e];
        dag_np[e] = U.npred[e];
        uint32_t pk = 0;
#pragma unroll
        for (int j = 0; j < E; j++) pk |= (j < (int)dag_np[e] ? ((uint32_t)U.pred_list[e][j] | ((uint32_t)U.pred_prim[e][j] << 3)) : 0u) << (4 * j);
        dag_pl[e] = pk;
        ordered |= dag_pm[e];
    }
    TW_TILE_T0();
    // ---- 1. cut-offs ------------------------------------------------------------------------------------------------
    int32_t lo[E], hi[E];
    // (a wavefront none of whose threads owns a span -- the upper half of a workgroup of two threads per span -- does none of the
    // per-span work: empty windows, which nothing below searches, reads back, tests for containment or stores)
    if ((t & ~63) >= ns) {
#pragma unroll
        for (int e = 0; e < E; e++) { lo[e] = 0; hi[e] = -1; }
    } else if (pass == 1) {   // FindCutoffs (traceweaver_v3.py:182-217), reverse topological order
#pragma unroll
        for (int e = E - 1; e >= 0; e--) {
            const int n = (int)(U.ep_off[e + 1] - U.ep_off[e]);
            int64_t tmax = in_end;
#pragma unroll
            for (int f = e + 1; f < E; f++) {
                if (!((U.succ_mask[e] >> f) & 1)) continue;
                const int nf = (int)(U.ep_off[f + 1] - U.ep_off[f]);
                const int anchor = hi[f] >= 0 ? hi[f] : nf - 1;  // Python's [-1] wrap (hazard H10)
                const int64_t st = os[f][anchor];
                if (st < tmax) tmax = st;
            }
            if (U.skip) {   // lists as handed over, possibly out of order: exactly Python's bisect_left / bisect_right
                lo[e] = lower_bound_i64(os[e], n, in_start);
                hi[e] = upper_bound_i64(os[e], n, tmax) - 1;
            } else {
                lo[e] = bound_near<false>(os[e], n, in_start, i);
                hi[e] = bound_near<true>(os[e], n, tmax, lo[e]) - 1;
            }
        }
        if (live) {
#pragma unroll
            for (int e = 0; e < E; e++) { P.c_lo[ie_index(U, e, i)] = lo[e]; P.c_hi[ie_index(U, e, i)] = hi[e]; }
        }
    } else {
#pragma unroll
        for (int e = 0; e < E; e++) { lo[e] = P.c_lo[ie_index(U, e, i)]; hi[e] = P.c_hi[ie_index(U, e, i)]; }
    }
    bool wide = false, empty = false, narrow = true;
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int w = hi[e] - lo[e] + 1;
        wide |= (w > 64 * kCandWords);
        narrow &= (w <= kNarrow);
        empty |= (w <= 0);
    }
    if (live && wide) { raise_err(P, TW_ERR_WINDOW_WIDTH); }
    group_sync();
    TW_TILE_TICK(0);
    // ---- 2. the tile's slice of every endpoint list ------------------------------------------------------------------
    {   // (one pair of LDS atomics per wavefront and endpoint, not per lane: same-address atomics serialise)
        const bool in = live && !empty && !wide;
#pragma unroll
        for (int e = 0; e < E; e++) {
            int a = in ? lo[e] : 0x7fffffff, b = in ? hi[e] + 1 : 0;
            for (int off = 32; off >= 1; off >>= 1) { const int a2 = __shfl_xor(a, off), b2 = __shfl_xor(b, off); a = a2 < a ? a2 : a; b = b2 > b ? b2 : b; }
            if ((t & 63) == 0) { atomicMin(&s_A[e], a); atomicMax(&s_B[e], b); }
        }
    }
    group_sync();
    int32_t cnt[E];
#pragma unroll
    for (int e = 0; e < E; e++) { const int c = s_B[e] - s_A[e]; cnt[e] = c < 0 ? 0 : (c > SL ? SL : c); }
    // (a class whose every span goes to the wavefront kernel -- TW_TILE_MAX_DEEP = 0 -- only classifies here: no slice)
    if (E >= P.lean_min_e && P.tile_max_deep == 0) {
#pragma unroll
        for (int e = 0; e < E; e++) cnt[e] = 0;
    }
    auto clamp32 = [](long long v) -> int32_t { return (int32_t)(v > 0x7fffffffll ? 0x7fffffffll : (v < -0x7fffffffll ? -0x7fffffffll : v)); };
    for (int x0 = 0; x0 < SL; x0 += nt) {   // (one round with the production sizes: the loads of all endpoints are in flight together)
        const int x = x0 + t;
        int64_t a[E], b[E];
#pragma unroll
        for (int e = 0; e < E; e++) { a[e] = 0; b[e] = 0; if (x < cnt[e]) { a[e] = os[e][s_A[e] + x]; b[e] = oe[e][s_A[e] + x]; } }
#pragma unroll
        for (int e = 0; e < E; e++) if (x < cnt[e]) { sl_st[e][x] = clamp32(a[e] - base); sl_en[e][x] = clamp32(b[e] - base); }
    }
    group_sync();
    TW_TILE_TICK(1);
    // ---- containment masks, the size of the span's enumeration, who enumerates it ------------------------------------
    const long long iso = in_start - base, ieo = in_end - base;
    // (offsets beyond 32 bits: not for this kernel; the clamped ends of the slice compare correctly against anything inside)
    const bool far = iso < 0 || ieo >= 0x7fffffffll || in_end < in_start || in_end - in_start >= (1ll << 31);
    uint32_t cm[E];
    bool fits = narrow && !far && !empty;
    long long prod = empty ? 0 : 1;
#pragma unroll
    for (int e = 0; e < E; e++) {
        cm[e] = 0;
        const int rel = lo[e] - s_A[e], w = hi[e] - lo[e] + 1;
        if (fits && (rel < 0 || rel + w > cnt[e])) fits = false;   // the window reaches beyond the staged slice
        if (fits) {
            for (int r = 0; r < w; r++)
                if (sl_st[e][rel + r] >= (int32_t)iso && sl_en[e][rel + r] <= (int32_t)ieo) cm[e] |= 1u << r;
            prod = prod <= kTileMax ? prod * __popcll((unsigned long long)cm[e]) : prod;
        }
    }
    // (the deep call graphs: every tuple costs this kernel a term per primary call-order edge -- in pass 2 a mixture term of ~1.5 k
    // instructions --, the wavefront kernel tabulates those per pair of candidates: its classes hand over from P.tile_max_deep tuples on)
    const long long tile_max = E >= P.lean_min_e ? (long long)P.tile_max_deep : (long long)kTileMax;
    const bool mine = live && !wide && (empty || (fits && prod <= tile_max));   // this kernel enumerates the span
    {   // the others: listed for the wavefront kernel with what it needs to plan (k_enumerate_heavy)
        long long hprod = 0;
        int first_cands = 0;
        bool twins_any = false;
        if (live && !mine && !wide) {
            // the windows also hold spans that start inside the incoming span but end after it; what the enumeration
            // costs is the product of the *contained* candidates (a third of the raw product on the bench workload)
            hprod = 1;
            bool twins = false;   // two candidates of one endpoint that start together: Python's order of tuples may not decide
#pragma unroll
            for (int e = 0; e < E; e++) {
                int v = 0;
                const int rel = lo[e] - s_A[e], w = hi[e] - lo[e] + 1;
                if (!far && rel >= 0 && rel + w <= cnt[e]) {   // the window lies in the staged slice
                    int32_t prev = -0x7fffffff - 1;
                    for (int r = 0; r < w; r++) {
                        const int32_t st = sl_st[e][rel + r];
                        if (st >= (int32_t)iso && sl_en[e][rel + r] <= (int32_t)ieo) { v++; twins |= st == prev; prev = st; }
                    }
                } else {
                    int64_t prev = INT64_MIN;
                    for (int cx = lo[e]; cx <= hi[e]; cx++) {
                        const int64_t st = os[e][cx];
                        if (st >= in_start && oe[e][cx] <= in_end) { v++; twins |= st == prev; prev = st; }
                    }
                }
                if (hprod <= (1ll << 40)) hprod *= v;
                if (e == 0) first_cands = v;
            }
            // with twins the parts cannot settle the top five among themselves (millisecond-granular traces: nearly always): they
            // replay CPython's heap on their shares and log what entered it (log mode, see heavy_append)
            if (twins && P.split_twins == 0) first_cands = 0;
            twins_any = twins;
            if (E >= P.lean_min_e) first_cands = 0;   // (k_enumerate_lean's classes are never cut by the first endpoint's candidate)
            // a class that defers its long spans cuts them by their listed prefixes once their tuples are counted (kListSplitFlag)
            if (E >= 3 && E >= P.defer_min_e) {
                uint32_t any_order = 0;
#pragma unroll
                for (int e = 0; e < E; e++) any_order |= U.pred_mask[e];
                if (any_order != 0) first_cands = 0;
            }
        }
        heavy_append<E>(P, live && !mine && !wide, narrow, hprod > kBigProduct, T.unit, i, hprod, U.skip ? 0 : first_cands, twins_any);
    }
    const bool some = mine && !empty && prod > 0;   // has tuples to enumerate here
    int nitem = 0;
    unsigned long long cnpack = 0;   // contained candidates per endpoint, 8 bits each
    if (live) {
#pragma unroll
        for (int e = 0; e < E; e++) {
            const int rel = lo[e] - s_A[e], c = some ? __popcll((unsigned long long)cm[e]) : 0;
            s_lo[e][t] = (uint16_t)(some ? rel : 0);
            s_cm[e][t] = some ? cm[e] : 0u;
            if constexpr (!SINGLE) s_bits[e][t] = 0u;
            nitem += c;
            cnpack |= (unsigned long long)c << (8 * e);
        }
        s_is[t] = (int32_t)iso; s_ie[t] = (int32_t)ieo;
        s_amb[t] = 0;
        if constexpr (!SINGLE) { s_cn[t] = cnpack; s_leaves[t] = (some && !ordered) ? (int)prod : 0; }
    }
    {   // inclusive prefix sums of the items and of the tuple slots (a span's slots padded to a multiple of four: the rank
        // loop reads four scores a step) over the spans: wavefront scans by shuffles, then the wavefronts' totals through LDS
        // (a single endpoint: the items are the tuples, one prefix sum)
        // (two endpoints: the tuples as they are, no padding)
        int a = live ? nitem : 0, b = (!SINGLE && live && some) ? (PAIR ? (int)prod : (((int)prod + 3) & ~3)) : 0;
        const int lane = t & 63, wv = t >> 6;
        for (int off = 1; off < 64; off <<= 1) {
            const int a2 = __shfl_up(a, off);
            if (lane >= off) a += a2;
            if constexpr (!SINGLE) { const int b2 = __shfl_up(b, off); if (lane >= off) b += b2; }
        }
        if (lane == 63 || t == nt - 1) { s_wtot[wv][0] = a; if constexpr (!SINGLE) s_wtot[wv][1] = b; }
        group_sync();
        for (int w = 0; w < wv; w++) { a += s_wtot[w][0]; if constexpr (!SINGLE) b += s_wtot[w][1]; }
        if (live) { s_item0[t + 1] = a; if constexpr (!SINGLE) s_grid0[t + 1] = b; }
        if (t == 0) { s_item0[0] = 0; if constexpr (!SINGLE) s_grid0[0] = 0; }
        group_sync();
    }
    TW_TILE_TICK(2);
    Scorer S;
    S.pass = pass;
    S.mix_n = P.mix_n + U.slot_off;
    S.mix_c = P.mix_c + (int64_t)U.slot_off * kMaxComp * 4;
    auto span_of = [&](const int32_t* pre, int first, int last, int x) -> int {   // largest s in [first, last) with pre[s] <= x
        int a = first, b = last - 1;
        while (a < b) { const int mid = (a + b + 1) >> 1; if (pre[mid] <= x) a = mid; else b = mid - 1; }
        return a;
    };
    // grid point -> the tuple's candidates: digits (last endpoint fastest, the reference's order), item numbers, slice positions
    auto decode = [&](int s, int gi, int it_first, int32_t (&kx)[E], int32_t (&ix)[E]) {
        uint32_t rest = (uint32_t)gi;
        const unsigned long long pk = s_cn[s];
        int below[E], acc = s_item0[s] - it_first;
#pragma unroll
        for (int e = 0; e < E; e++) { below[e] = acc; acc += (int)((pk >> (8 * e)) & 255ull); }
#pragma unroll
        for (int e = E - 1; e >= 0; e--) {
            const uint32_t c = (uint32_t)((pk >> (8 * e)) & 255ull);
            const uint32_t q = c == 1 ? rest : div_small(rest, c);
            kx[e] = below[e] + (int32_t)(rest - q * c);
            rest = q;
            ix[e] = it_idx[kx[e]];
        }
    };
    // ---- a single endpoint: a tuple is an item.  No tuple slots, no decoding, one score per item in the reference's order of additions
    // ((0.0 + root) + closing, as phase 4 forms it), the rank counted among the span's own items; 13 KB of LDS instead of 31 ---------
    if constexpr (SINGLE) {
        __shared__ double s_sc[C::kItems];                     // the item's score
        __shared__ uint8_t it_span[C::kItems], it_rank[C::kItems];   // its span (tile-local), its rank
        // (what a span's thread needs again after the scores -- its mask, its window's place in the slice, whether the span is this
        // kernel's -- is read back from LDS where it is needed: held in registers through the term it would not fit 64 of them)
        __shared__ uint8_t s_mine[SPANS];
        const bool is_root = dag_np[0] == 0;
        if (live) s_mine[t] = mine ? 1 : 0;
        for (int seg = 0; seg < ns;) {
            if (t == 0) { s_segend = fresh(ns); s_anyamb = 0; }   // (fresh: a copy of the constant made here, not kept from before the loop)
            group_sync();
            const int tq = fresh(t);
            if (live && t >= seg && s_item0[tq + 1] - s_item0[seg] > C::kItems) atomicMin(&s_segend, t);
            group_sync();
            const int send = s_segend;
            const int it0 = s_item0[seg], nIt = s_item0[send] - it0;
            const bool here = live && t >= seg && t < send;
            const int ks = (live ? s_item0[tq] : 0) - it0;   // the first item of this thread's span, the items (= tuples) it has
            const int nitem1 = live ? s_item0[tq + 1] - s_item0[tq] : 0;
            TW_TILE_TICK(2);
            TW_TILE_COUNT(9, 1); TW_TILE_COUNT(10, nIt); TW_TILE_COUNT(11, nIt);
            // the span's thread names its items: span and slice position (contained candidates in list order)
            if (here) {
                int k = ks;
                const int rel0 = s_lo[0][tq];
                for (uint32_t m = s_cm[0][tq]; m != 0; m &= m - 1, k++) { it_span[k] = (uint8_t)t; it_idx[k] = (uint16_t)(rel0 + __ffs((int)m) - 1); }
            }
            group_sync();
            // ---- 3 + 4. the tuple's score, one item per lane ---------------------------------------------------------------
            for (int k = t; k < nIt; k += nt) {
                const int s = it_span[k], idx = it_idx[k];
                S.gp = P.gparam + (U.gp_off + (int64_t)((first + s) / P.batch_size) * U.nslot) * 4;
                // (0.0 + root) + closing: one copy of the term in the kernel, inlined, run for the root and for the closing gap
                double sj = 0.0;
#pragma unroll 1
                for (int h = is_root ? 0 : 1; h < 2; h++) {
                    const int slot = h == 0 ? slot_root(E, 0) : slot_close(E, 0);
                    const double x = (double)(h == 0 ? (long long)sl_st[0][idx] - s_is[s] : (long long)s_ie[s] - sl_en[0][idx]);
                    double term;
                    if (pass == 1) { const double* g = S.gp + slot * 4; term = term_gauss(g[0], g[3], g[2], x); }
                    else {
                        const int n = S.mix_n[slot];
                        const double* c = S.mix_c + (int64_t)slot * kMaxComp * 4;
                        term = n <= 0 ? term_gauss(c[0], c[1], c[2], x) : term_mix_inline(n, c, x);
                    }
                    sj += term;
                }
                s_sc[k] = sj;
            }
            group_sync();
            TW_TILE_TICK(3);
            TW_TILE_TICK(4);
            // ---- 5. rank of every item among the items of its span: the greater scores; on equal scores Python compares the
            // candidates' start_mus -- equal starts: an incomparable partner, the span is undecided (a NaN score ranks nowhere) -----
            for (int k = t; k < nIt; k += nt) {
                const double my = s_sc[k];
                int rank = kTopK;
                if (my == my) {
                    const int s = it_span[k];
                    const int hs0 = s_item0[s] - it0, he = s_item0[s + 1] - it0;
                    const int32_t a = sl_st[0][it_idx[k]];
                    rank = 0;
                    bool partner = false;
                    for (int h = hs0; h < he && rank < kTopK; h++) {
                        const double o = s_sc[h];
                        if (o > my) rank++;
                        else if (o == my && h != k) {
                            const int32_t b = sl_st[0][it_idx[h]];
                            if (b > a) rank++;
                            else if (b == a) partner = true;
                        }
                    }
                    if (partner && rank < kTopK) { s_amb[s] = 1; s_anyamb = 1; }
                }
                it_rank[k] = (uint8_t)(rank < kTopK ? rank : kTopK);
            }
            group_sync();
            TW_TILE_TICK(5);
            // ---- results: the items of rank < 5 write themselves ------------------------------------------------------------
            for (int k = t; k < nIt; k += nt) {
                if (it_rank[k] >= kTopK) continue;
                const int s = it_span[k];
                if (s_amb[s]) continue;
                const int r = it_rank[k], si = first + s;
                P.tk_score[tks_index(U, r, si)] = s_sc[k];
                P.tk_idx[tk_index(U, r, 0, si)] = s_A[0] + (int)it_idx[k];
            }
            // ---- 5b. an undecided span: CPython's heap over the span's items in list order by the span's own thread, in registers;
            // when every thread has read its scores (the barrier) the score and rank tables are free: kTopK + 1 slots of each per
            // span hold the heap for CPython's list.sort
            const int tl = fresh(t);
            const bool replay = s_anyamb != 0 && here && s_mine[tl] && s_amb[tl] && (tl + 1) * (kTopK + 1) <= C::kItems && nitem1 <= kTileReplayMax;
            auto start_of = [&](int, int pos) -> int32_t { return sl_st[0][it_idx[ks + pos]]; };
            RegHeap RH;
            RH.clear(E);
            if (replay) {
                for (int pos = 0; pos < nitem1; pos++) {
                    const double sc = s_sc[ks + pos];
                    if (!(sc == sc) || RH.below_root(sc)) continue;   // strictly below the root of a full heap: the push leaves the array as it is
                    RH.push(sc, (unsigned long long)pos, start_of);
                }
            }
            if (s_anyamb != 0) group_sync();   // (the flag is the same for all since the barrier after the ranks)
            if (replay) {
                double* hs = s_sc + tl * (kTopK + 1);
                uint8_t* hx = it_rank + tl * (kTopK + 1);
#pragma unroll
                for (int k = 0; k < kTopK; k++) { hs[k] = RH.s[k]; hx[k] = (uint8_t)RH.x[k]; }
                py_sort_desc(hs, hx, RH.n, [&](double sa, unsigned long long xa, double sb, unsigned long long xb) { return RH.lt(sa, xa, sb, xb, start_of); });
                const int si = first + tl;
                for (int k = 0; k < RH.n; k++) {
                    P.tk_score[tks_index(U, k, si)] = hs[k];
                    P.tk_idx[tk_index(U, k, 0, si)] = s_A[0] + (int)it_idx[ks + (int)hx[k]];
                }
                s_amb[tl] = 0;   // (read again only by this thread: below, and when the tile hands its undecided spans on)
            }
            if (here && s_mine[tl] && !s_amb[tl]) {
                const int i1 = first + tl;
                const int64_t g = U.in_off + i1;
                P.tk_n[g] = nitem1 < kTopK ? nitem1 : kTopK;
                P.leaves[g] = nitem1;
                if (pass == 1) P.leaves0[g] = nitem1;
                P.rep[g] = 0;
                if (pass == 1) {
                    P.c_bits[ie_index(U, 0, i1) * kCandWords] = (uint64_t)s_cm[0][tl];
                    for (int w = 1; w < kCandWords; w++) P.c_bits[ie_index(U, 0, i1) * kCandWords + w] = (uint64_t)(uint32_t)fresh(0);
                }
            }
            group_sync();
            TW_TILE_TICK(6);
            seg = send;
        }
        TW_TILE_FLUSH();
        const int te = fresh(t);
        heavy_append<E>(P, live && s_mine[te] != 0 && s_amb[te] != 0, true, false, T.unit, first + (live ? te : 0), 0, 0, false, te & 63);   // (as below)
        return;
    } else if constexpr (PAIR) {
        // ---- two endpoints.  The endpoints are in topological order of the DAG (tw_load_batch refuses anything else): endpoint 0 is a
        // root, endpoint 1 is a root too (no call order: every grid point is a tuple) or follows endpoint 0, block-uniformly.  A span's
        // thread names its items and its tuple slots, a tuple finds its two items by one division and keeps their slice positions as two
        // bytes for the ranks and the results; nothing searches the prefix sums.  The slots are the tuples (no padding), the tables are
        // sized for the class.  The score is phase 4's of the general path for E = 2 in its order of additions ---------------------------
        static_assert(SL <= 256, "the slice positions of a tuple's two candidates lie in a byte each");
        __shared__ uint8_t it_span[C::kItems];   // the item's span (tile-local); its endpoint is bit 15 of it_idx
        __shared__ uint16_t g_ix[C::kGrid];      // the slice positions of the tuple's candidates: endpoint 0 | endpoint 1 << 8
        // (what a span's thread needs again behind the tuples -- whether the span is this kernel's, its first item, its candidates --
        // is read back from LDS where it is needed, from a fresh copy of the thread's number: held in registers through the segment
        // it would not fit the 96 registers of five wavefronts per SIMD)
        __shared__ uint8_t s_mine[SPANS];
        if (live) s_mine[t] = mine ? 1 : 0;
        typedef SurvivorRanks<C::kGrid, kRankDirect + 1> SR;   // (unpadded: a long span has at least kRankDirect + 1 slots)
        constexpr bool kRankFits = SR::kAuxWords <= C::kGrid / 4 && C::kGrid * 4 <= C::kItems * 8 && C::kGrid <= 65536;
        static_assert(C::kGrid <= C::kItems * 8, "a rank per slot in t_root");
        uint8_t* const g_rank = reinterpret_cast<uint8_t*>(t_root);   // [kGrid] the tuple's rank (from phase 5 on; the term tables are free by then)
        const bool compact = kRankFits && P.tile_rank != 0;
        const bool prim = dag_np[1] != 0 && (dag_pl[1] & 8u) != 0;   // the call-order edge 0 -> 1 is scored per tuple
        for (int seg = 0; seg < ns;) {
            if (compact) SR{g_aux, g_rank, nullptr, nullptr, g_sc, g_span, s_grid0, 0}.clear(t, nt);
            if (t == 0) { s_segend = ns; s_anyamb = 0; }
            group_sync();
            if (live && t >= seg && (s_item0[t + 1] - s_item0[seg] > C::kItems || s_grid0[t + 1] - s_grid0[seg] > C::kGrid)) atomicMin(&s_segend, t);
            group_sync();
            const int send = s_segend;
            const int it0 = s_item0[seg], nIt = s_item0[send] - it0, g0 = s_grid0[seg], nG = s_grid0[send] - g0;
            const SR sr{g_aux, g_rank, reinterpret_cast<uint16_t*>(t_close), reinterpret_cast<uint16_t*>(t_close) + C::kGrid, g_sc, g_span, s_grid0, g0};
            const int tq = fresh(t);
            const bool here = tq < ns && tq >= seg && tq < send;
            TW_TILE_TICK(2);
            TW_TILE_COUNT(9, 1); TW_TILE_COUNT(10, nIt); TW_TILE_COUNT(11, nG);
            // the span's thread names its items (span, endpoint, slice position; contained candidates in list order) and its slots
            if (here) {
                int k = s_item0[tq] - it0;
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const int rel = s_lo[e][tq];
                    for (uint32_t m = s_cm[e][tq]; m != 0; m &= m - 1, k++) { it_span[k] = (uint8_t)tq; it_idx[k] = (uint16_t)((rel + __ffs((int)m) - 1) | (e << 15)); }
                }
                for (int g = s_grid0[tq] - g0, ge = s_grid0[tq + 1] - g0; g < ge; g++) g_span[g] = (uint8_t)tq;
            }
            group_sync();
            // ---- 3. root / closing terms, one item per lane -------------------------------------------------------------------
            for (int k = t; k < nIt; k += nt) {
                const int s = it_span[k], e = it_idx[k] >> 15, idx = it_idx[k] & 0x7fff;
                const int32_t st = sl_st[e][idx], en = sl_en[e][idx];
                const bool is_root = (e == 0 ? dag_np[0] : dag_np[1]) == 0;
                S.gp = P.gparam + (U.gp_off + (int64_t)((first + s) / P.batch_size) * U.nslot) * 4;
                t_root[k] = is_root ? score_term_gap(S, slot_root(E, e), (long long)st - s_is[s]) : 0.0;
                t_close[k] = score_term_gap(S, slot_close(E, e), (long long)s_ie[s] - en);
            }
            group_sync();
            TW_TILE_TICK(3);
            // ---- 4. tuples, one per lane (last endpoint fastest, the reference's order): feasibility and score -------------------
            for (int g = t; g < nG; g += nt) {
                const int s = g_span[g];
                const int gi = g - (s_grid0[s] - g0);
                const uint32_t pk = (uint32_t)s_cn[s], n0 = pk & 255u, n1 = (pk >> 8) & 255u;
                const uint32_t k0 = n1 == 1 ? (uint32_t)gi : div_small((uint32_t)gi, n1), k1 = (uint32_t)gi - k0 * n1;
                const int kx0 = s_item0[s] - it0 + (int)k0, kx1 = s_item0[s] - it0 + (int)(n0 + k1);
                const int ix0 = it_idx[kx0], ix1 = it_idx[kx1] & 0x7fff;
                const int32_t st0 = sl_st[0][ix0], en0 = sl_en[0][ix0], st1 = sl_st[1][ix1], en1 = sl_en[1][ix1];
                const bool ok = !((dag_pm[1] & 1u) && en0 > st1);   // traceweaver_v3.py:343-347
                double sj = 0.0;
                if (ok) {
                    // ScoreAssignmentAsPerInvocationGraph, no-skip branch (traceweaver_v1.py:305-361)
                    const bool last1 = en1 > en0;
                    if (dag_np[0] == 0) sj += t_root[kx0];
                    if (!last1) sj += t_close[kx0];
                    if (prim) {
                        S.gp = P.gparam + (U.gp_off + (int64_t)((first + s) / P.batch_size) * U.nslot) * 4;
                        sj += score_term_gap(S, slot_prim(E, 0, 1), (long long)st1 - en0);
                    }
                    if (dag_np[1] == 0) sj += t_root[kx1];
                    if (last1) sj += t_close[kx1];
                    if (ordered) {
                        atomicAdd(&s_leaves[s], 1);
                        if (pass == 1) { atomicOr(&s_bits[0][s], 1u << (ix0 - (int)s_lo[0][s])); atomicOr(&s_bits[1][s], 1u << (ix1 - (int)s_lo[1][s])); }
                    }
                }
                g_sc[g] = ok ? sj : dnan();
                g_ix[g] = (uint16_t)(ix0 | (ix1 << 8));
                if (compact && ok && s_grid0[s + 1] - s_grid0[s] > kRankDirect) sr.note(g, gi, sj);   // a long span: the largest key of the slot's subset
            }
            group_sync();
            TW_TILE_TICK(4);
            // ---- 5. rank of every tuple among the tuples of its span.  Python's order of two tuples with equal scores: start_mus of
            // the first differing span (spans.py:51-52).  +1: the other one is greater, -1: smaller, 0: incomparable
            auto order_equal = [&](uint32_t a, uint32_t b) -> int {
                const int e = (a & 255u) != (b & 255u) ? 0 : 1;
                const int32_t sa = sl_st[e][(a >> (8 * e)) & 255u], sb = sl_st[e][(b >> (8 * e)) & 255u];
                return sb > sa ? 1 : (sb < sa ? -1 : 0);
            };
            if (compact) sr.collect(nG, t, nt);
            for (int g = t; g < nG; g += nt) {
                const double my = g_sc[g];
                int rank = kTopK;
                const int s = g_span[g];
                const int gs = s_grid0[s] - g0, ge = s_grid0[s + 1] - g0;
                if (compact && ge - gs > kRankDirect) { g_rank[g] = (uint8_t)kTopK; continue; }   // (a survivor's own rank follows behind the barrier)
                if (my == my) {   // (a NaN score ranks nowhere)
                    rank = 0;
                    bool partner = false;
                    // four scores a step: how many are greater, how many are equal -- the tuple itself is one of the equal ones.  (No
                    // padding: what lies behind the span's last slot is another span's or nobody's, and is not counted; g_sc has
                    // three entries to spare behind the segment's last)
                    int eq = 0;
                    for (int h0 = gs; h0 < ge && rank < kTopK; h0 += 4) {
                        const double o0 = g_sc[h0], o1 = g_sc[h0 + 1], o2 = g_sc[h0 + 2], o3 = g_sc[h0 + 3];
                        const bool in1 = h0 + 1 < ge, in2 = h0 + 2 < ge, in3 = h0 + 3 < ge;
                        rank += (o0 > my) + (in1 && o1 > my) + (in2 && o2 > my) + (in3 && o3 > my);
                        eq += (o0 == my) + (in1 && o1 == my) + (in2 && o2 == my) + (in3 && o3 == my);
                    }
                    if (eq > 1 && rank < kTopK) {   // equal scores (millisecond-granular data): the equal ones that are greater, one that is incomparable
                        const uint32_t mine_ix = g_ix[g];
                        for (int h = gs; h < ge; h++) {
                            if (h == g || !(g_sc[h] == my)) continue;
                            const int ord = order_equal(mine_ix, g_ix[h]);
                            if (ord > 0) rank++;
                            else if (ord == 0) partner = true;
                        }
                    }
                    if (partner && rank < kTopK) { s_amb[s] = 1; s_anyamb = 1; }
                }
                g_rank[g] = (uint8_t)(rank < kTopK ? rank : kTopK);
            }
            if (compact) {   // a survivor per lane: the greater ones, the equal ones, among the survivors of its span
                group_sync();
                sr.rank(t, nt,
                        [&](int s, int gi) -> uint32_t { return g_ix[s_grid0[s] - g0 + gi]; },
                        [&](int s, uint32_t mine_ix, int hrel) { return order_equal(mine_ix, g_ix[s_grid0[s] - g0 + hrel]); },
                        [&](int s) { s_amb[s] = 1; s_anyamb = 1; });
            }
            group_sync();
            TW_TILE_TICK(5);
            // ---- results: the tuples of rank < 5 write themselves; then one thread per span ---------------------------------------
            for (int g = t; g < nG; g += nt) {
                if (g_rank[g] >= kTopK) continue;
                const int s = g_span[g];
                if (s_amb[s]) continue;
                const int k = g_rank[g], si = first + s;
                const uint32_t ix = g_ix[g];
                P.tk_score[tks_index(U, k, si)] = g_sc[g];
                P.tk_idx[tk_index(U, k, 0, si)] = s_A[0] + (int)(ix & 255u);
                P.tk_idx[tk_index(U, k, 1, si)] = s_A[1] + (int)(ix >> 8);
            }
            // ---- 5b. a span whose top five the ranks do not decide: CPython's heap over the span's tuples in enumeration order by the
            // span's own thread, in registers, on the scores of phase 4.  Behind the barrier the term tables (the ranks, the survivor
            // lists) and the position table are free: kTopK + 1 slots per span hold the heap for CPython's list.sort -- the scores of
            // the lower half of the spans in t_root, of the upper half in t_close, the tuples in g_ix
            if (s_anyamb != 0) group_sync();   // (the flag is the same for all since the barrier after the ranks; the lanes above skip the tuples of undecided spans: s_amb is cleared only when all have passed)
            const int tl = fresh(t);
            const bool mine_here = tl < ns && tl >= seg && tl < send && s_mine[tl] != 0;
            const int th = tl < SPANS / 2 ? tl : tl - SPANS / 2;
            const bool replay = s_anyamb != 0 && mine_here && s_amb[tl] && (th + 1) * (kTopK + 1) <= C::kItems && (tl + 1) * (kTopK + 1) <= C::kGrid && s_leaves[tl] <= kTileReplayMax;
            if (replay) {
                const int ks = s_item0[tl] - it0;                       // the first item of this thread's span
                const int c0 = (int)((uint32_t)s_cn[tl] & 255u);        // ... its candidates of endpoint 0
                auto start_of = [&](int e, int pos) -> int32_t { return sl_st[e][it_idx[ks + (e != 0 ? c0 : 0) + pos] & 0x7fff]; };
                RegHeap RH;
                RH.clear(E);
                const int gs = s_grid0[tl] - g0, nT = s_grid0[tl + 1] - s_grid0[tl];
                const uint32_t n1 = ((uint32_t)s_cn[tl] >> 8) & 255u;
                uint32_t k0 = 0, k1 = 0;
                for (int gi = 0; gi < nT; gi++) {
                    const double sc = g_sc[gs + gi];
                    const unsigned long long x = (unsigned long long)(k0 | (k1 << 8));   // positions among the span's candidates, 8 bits per endpoint
                    if (++k1 == n1) { k1 = 0; k0++; }
                    if (!(sc == sc) || RH.below_root(sc)) continue;   // infeasible / strictly below the root of a full heap: the push leaves the array as it is
                    RH.push(sc, x, start_of);
                }
                double* hs = (tl < SPANS / 2 ? t_root : t_close) + th * (kTopK + 1);
                uint16_t* hx = g_ix + tl * (kTopK + 1);
#pragma unroll
                for (int k = 0; k < kTopK; k++) { hs[k] = RH.s[k]; hx[k] = (uint16_t)RH.x[k]; }
                py_sort_desc(hs, hx, RH.n, [&](double sa, unsigned long long xa, double sb, unsigned long long xb) { return RH.lt(sa, xa, sb, xb, start_of); });
                const int si = first + tl;
                for (int k = 0; k < RH.n; k++) {
                    P.tk_score[tks_index(U, k, si)] = hs[k];
                    P.tk_idx[tk_index(U, k, 0, si)] = s_A[0] + (int)it_idx[ks + (int)(hx[k] & 255u)];
                    P.tk_idx[tk_index(U, k, 1, si)] = s_A[1] + (int)(it_idx[ks + c0 + (int)(hx[k] >> 8)] & 0x7fff);
                }
                s_amb[tl] = 0;   // (read again only by this thread: below, and when the tile hands its undecided spans on)
            }
            if (mine_here && !s_amb[tl]) {
                const int i = first + tl;
                // a span's list has min(5, feasible tuples) entries in every pass; the unused entries keep the -1 / NaN
                // pattern of tw_load_batch and are never written
                const int64_t g = U.in_off + i;
                const int leaves = s_leaves[tl];
                P.tk_n[g] = leaves < kTopK ? leaves : kTopK;
                P.leaves[g] = leaves;
                if (pass == 1) P.leaves0[g] = leaves;
                P.rep[g] = 0;
                if (pass == 1) {
#pragma unroll
                    for (int e = 0; e < 2; e++) {
                        P.c_bits[ie_index(U, e, i) * kCandWords] = (uint64_t)(ordered ? s_bits[e][tl] : s_cm[e][tl]);
                        for (int w = 1; w < kCandWords; w++) P.c_bits[ie_index(U, e, i) * kCandWords + w] = 0;
                    }
                }
            }
            group_sync();
            TW_TILE_TICK(6);
            seg = send;
        }
        TW_TILE_FLUSH();
        const int te = fresh(t);
        heavy_append<E>(P, te < ns && s_mine[te] != 0 && s_amb[te] != 0, true, false, T.unit, first + (te < ns ? te : 0), 0, 0, false, te & 63);
        return;
    } else
    // ---- segments of the tile: as many spans as the tables hold ------------------------------------------------------
    for (int seg = 0; seg < ns;) {
        // Phase 5 ranks a long span (more than kRankDirect slots) among its survivors only (SurvivorRanks).  The term tables are free
        // between phase 4 and phase 5b: t_root holds the ranks, t_close the two lists of 16-bit slot numbers.
        typedef SurvivorRanks<C::kGrid, kRankMinLong> SR;
        constexpr bool kRankFits = SR::kAuxWords <= C::kGrid / 4 && C::kGrid * 4 <= C::kItems * 8 && C::kGrid <= 65536;
        static_assert(kRankBuckets == kTopK && C::kGrid <= C::kItems * 8, "a subset of slots per entry of the list; a rank per slot in t_root");
        uint8_t* const g_rank = reinterpret_cast<uint8_t*>(t_root);                        // [kGrid] the tuple's rank (from phase 5 on)
        const bool compact = kRankFits && P.tile_rank != 0;   // (an instantiation whose tables do not hold the lists keeps the loop over all slots)
        if (compact) SR{g_aux, g_rank, nullptr, nullptr, g_sc, g_span, s_grid0, 0}.clear(fresh(t), nt);
        if (t == 0) { s_segend = ns; s_anyamb = 0; }
        group_sync();
        if (live && t >= seg && (s_item0[t + 1] - s_item0[seg] > C::kItems || s_grid0[t + 1] - s_grid0[seg] > C::kGrid)) atomicMin(&s_segend, t);
        group_sync();
        const int send = s_segend;
        const int it0 = s_item0[seg], nIt = s_item0[send] - it0, g0 = s_grid0[seg], nG = s_grid0[send] - g0;
        const SR sr{g_aux, g_rank, reinterpret_cast<uint16_t*>(t_close), reinterpret_cast<uint16_t*>(t_close) + C::kGrid, g_sc, g_span, s_grid0, g0};
        TW_TILE_TICK(2);
        TW_TILE_COUNT(9, 1); TW_TILE_COUNT(10, nIt); TW_TILE_COUNT(11, nG);
        // ---- 3. root / closing terms, one (span, endpoint, candidate) per lane ----------------------------------------
        for (int k = t; k < nIt; k += nt) {
            const int s = span_of(s_item0, seg, send, it0 + k);
            int j = it0 + k - s_item0[s], es = 0;
            uint32_t m = 0;
            bool found = false;
#pragma unroll
            for (int e = 0; e < E; e++)
                if (!found) { m = s_cm[e][s]; const int c = __popcll((unsigned long long)m); if (j < c) { es = e; found = true; } else j -= c; }
            const int idx = (int)s_lo[es][s] + nth_set_bit((unsigned long long)m, j);
            int32_t st = 0, en = 0;
            bool is_root = false;
#pragma unroll
            for (int e = 0; e < E; e++) if (e == es) { st = sl_st[e][idx]; en = sl_en[e][idx]; is_root = dag_np[e] == 0; }
            S.gp = P.gparam + (U.gp_off + (int64_t)((first + s) / P.batch_size) * U.nslot) * 4;
            t_root[k] = is_root ? score_term_gap(S, slot_root(E, es), (long long)st - s_is[s]) : 0.0;
            t_close[k] = score_term_gap(S, slot_close(E, es), (long long)s_ie[s] - en);
            it_idx[k] = (uint16_t)idx;
        }
        group_sync();
        TW_TILE_TICK(3);
        // ---- 4. tuples, one per lane: feasibility and score ----------------------------------------------------------
        for (int g = t; g < nG; g += nt) {
            const int s = span_of(s_grid0, seg, send, g0 + g);
            int32_t kx[E], ix[E], st[E], en[E];
            const int gi = g0 + g - s_grid0[s];
            uint32_t real = 1;   // tuples of the span (its slots beyond are padding)
            {
                const unsigned long long pk = s_cn[s];
#pragma unroll
                for (int e = 0; e < E; e++) real *= (uint32_t)((pk >> (8 * e)) & 255ull);
            }
            bool ok = (uint32_t)gi < real;
            decode(s, ok ? gi : 0, it0, kx, ix);
#pragma unroll
            for (int e = 0; e < E; e++) {
                st[e] = sl_st[e][ix[e]]; en[e] = sl_en[e][ix[e]];
#pragma unroll
                for (int p = 0; p < e; p++)
                    if (((dag_pm[e] >> p) & 1) && en[p] > st[e]) ok = false;   // traceweaver_v3.py:343-347
            }
            double sj = 0.0;
            if (ok) {
                // ScoreAssignmentAsPerInvocationGraph, no-skip branch (traceweaver_v1.py:305-361)
                int last = 0;
                int32_t last_end = en[0];
#pragma unroll
                for (int e = 1; e < E; e++) if (en[e] > last_end) { last_end = en[e]; last = e; }
                S.gp = P.gparam + (U.gp_off + (int64_t)((first + s) / P.batch_size) * U.nslot) * 4;
#pragma unroll
                for (int e = 0; e < E; e++) {
                    const int np = (int)dag_np[e];
#pragma unroll
                    for (int j = 0; j < E; j++) {
                        if (j >= np) continue;
                        const uint32_t pj = (dag_pl[e] >> (4 * j)) & 15u;
                        if (!(pj & 8u)) continue;
                        const int p = (int)(pj & 7u);
                        int32_t pend = 0;
#pragma unroll
                        for (int q = 0; q < E; q++) if (q == p) pend = en[q];
                        sj += score_term_gap(S, slot_prim(E, p, e), (long long)st[e] - pend);
                    }
                    if (np == 0) sj += t_root[kx[e]];
                    if (e == last) sj += t_close[kx[e]];
                }
                if (ordered) {
                    atomicAdd(&s_leaves[s], 1);
                    if (pass == 1) {
#pragma unroll
                        for (int e = 0; e < E; e++) atomicOr(&s_bits[e][s], 1u << (ix[e] - (int)s_lo[e][s]));
                    }
                }
            }
            g_sc[g] = ok ? sj : dnan();
            g_span[g] = (uint8_t)s;
            if (compact && ok && s_grid0[s + 1] - s_grid0[s] > kRankDirect) sr.note(g, gi, sj);   // a long span: the largest key of the slot's subset
        }
        group_sync();
        TW_TILE_TICK(4);
        // ---- 5. rank of every tuple among the tuples of its span ------------------------------------------------------
        // Python's order of two tuples of a span with equal scores: start_mus of the first differing span (spans.py:51-52).
        // +1: the other one (slot hrel of the span) is greater, -1: smaller, 0: incomparable
        auto order_equal = [&](int s, const int32_t (&ia)[E], int hrel) -> int {
            int32_t kb[E], ib[E];
            decode(s, hrel, it0, kb, ib);
            int ord = 0;
            bool done = false;
#pragma unroll
            for (int e = 0; e < E; e++)
                if (!done && ia[e] != ib[e]) {
                    const int32_t a = sl_st[e][ia[e]], b = sl_st[e][ib[e]];
                    ord = b > a ? 1 : (b < a ? -1 : 0);
                    done = true;
                }
            return ord;
        };
        if (compact) sr.collect(nG, fresh(t), nt);   // (fresh: what the lists' addresses are formed from, here, not ahead of the segment loop)
        for (int g = t; g < nG; g += nt) {
            const double my = g_sc[g];
            int rank = kTopK;
            const int s = g_span[g];
            const int gs = s_grid0[s] - g0, ge = s_grid0[s + 1] - g0;
            if (compact && ge - gs > kRankDirect) { g_rank[g] = (uint8_t)kTopK; continue; }   // (a survivor's own rank follows behind the barrier)
            if (my == my) {
                rank = 0;
                bool partner = false;
                // four scores a step (the span's slots are padded to a multiple of four with NaN, which compares as neither
                // greater nor equal): how many are greater, how many are equal -- the tuple itself is one of the equal ones
                int eq = 0;
                for (int h0 = gs; h0 < ge && rank < kTopK; h0 += 4) {
                    const double o0 = g_sc[h0], o1 = g_sc[h0 + 1], o2 = g_sc[h0 + 2], o3 = g_sc[h0 + 3];
                    rank += (o0 > my) + (o1 > my) + (o2 > my) + (o3 > my);
                    eq += (o0 == my) + (o1 == my) + (o2 == my) + (o3 == my);
                }
                if (eq > 1 && rank < kTopK) {
                    // equal scores (millisecond-granular data): Python compares the span lists -- start_mus of the first differing
                    // span (spans.py:51-52); count the equal ones that are greater, note one that is incomparable
                    int32_t ka[E], ia[E];
                    decode(s, g - gs, it0, ka, ia);
                    for (int h = gs; h < ge; h++) {
                        if (h == g || !(g_sc[h] == my)) continue;
                        const int ord = order_equal(s, ia, h - gs);
                        if (ord > 0) rank++;
                        else if (ord == 0) partner = true;
                    }
                }
                if (partner && rank < kTopK) { s_amb[s] = 1; s_anyamb = 1; }
            }
            g_rank[g] = (uint8_t)(rank < kTopK ? rank : kTopK);
        }
        if (compact) {   // a survivor per lane: the greater ones, the equal ones, among the survivors of its span
            group_sync();
            struct Mine { int32_t ia[E]; };
            sr.rank(fresh(t), nt,
                    [&](int s, int gi) { Mine m; int32_t ka[E]; decode(s, gi, it0, ka, m.ia); return m; },
                    [&](int s, const Mine& m, int hrel) { return order_equal(s, m.ia, hrel); },
                    [&](int s) { s_amb[s] = 1; s_anyamb = 1; });
        }
        group_sync();
        TW_TILE_TICK(5);
        // ---- results: the tuples of rank < 5 write themselves; then one thread per span ---------------------------------
        for (int g = t; g < nG; g += nt) {
            if (g_rank[g] >= kTopK) continue;
            const int s = g_span[g];
            if (s_amb[s]) continue;
            int32_t kx[E], ix[E];
            decode(s, g0 + g - s_grid0[s], it0, kx, ix);
            const int k = g_rank[g], si = first + s;
            P.tk_score[tks_index(U, k, si)] = g_sc[g];
#pragma unroll
            for (int e = 0; e < E; e++) P.tk_idx[tk_index(U, k, e, si)] = s_A[e] + ix[e];
        }
        // ---- 5b. a span whose top five the ranks do not decide (s_amb: equal scores, tuples Python's order does not compare --
        // millisecond-granular traces have them in a third of their spans): the reference's procedure itself, by the span's own
        // thread -- CPython's heap over the span's tuples in enumeration order (traceweaver_v3.py:304-307), then its list.sort --
        // on the scores of phase 4.  (Such a span used to go to the wavefront kernel, which staged its windows and evaluated its terms
        // again for a wavefront's ~90 us: 10.7 of the 29 ms of a pass on the nodejs shape at 14.4 M spans.)  The term tables of the
        // segment are free by now: kTopK + 1 slots of each per span hold the heap for the sort.
        if (s_anyamb != 0) group_sync();   // (the lanes above skip the tuples of undecided spans: s_amb is cleared only when all have passed; the flag is the same for all since the barrier after the ranks)
        if (s_anyamb != 0 && live && t >= seg && t < send && mine && s_amb[t] && (t + 1) * (kTopK + 1) <= C::kItems && s_leaves[t] <= kTileReplayMax) {
            RegHeap RH;
            RH.clear(E);
            const unsigned long long pk = s_cn[t];
            auto start_of = [&](int e, int pos) -> int32_t { return sl_st[e][it_idx[s_item0[t] - it0 + pos_base(pk, e) + pos]]; };
            uint32_t real = 1;
#pragma unroll
            for (int e = 0; e < E; e++) real *= (uint32_t)((pk >> (8 * e)) & 255ull);
            const int gs = s_grid0[t] - g0;
            for (uint32_t gi = 0; gi < real; gi++) {
                const double sc = g_sc[gs + gi];
                if (!(sc == sc) || RH.below_root(sc)) continue;   // infeasible / strictly below the root of a full heap: the push leaves the array as it is
                unsigned long long x = 0;
                uint32_t rest = gi;
#pragma unroll
                for (int e = E - 1; e >= 0; e--) {
                    const uint32_t c = (uint32_t)((pk >> (8 * e)) & 255ull);
                    const uint32_t q = c == 1 ? rest : div_small(rest, c);
                    x |= (unsigned long long)(rest - q * c) << (8 * e);
                    rest = q;
                }
                RH.push(sc, x, start_of);
            }
            double* hs = t_root + t * (kTopK + 1);
            unsigned long long* hx = reinterpret_cast<unsigned long long*>(t_close + t * (kTopK + 1));
#pragma unroll
            for (int k = 0; k < kTopK; k++) { hs[k] = RH.s[k]; hx[k] = RH.x[k]; }
            py_sort_desc(hs, hx, RH.n, [&](double sa, unsigned long long xa, double sb, unsigned long long xb) { return RH.lt(sa, xa, sb, xb, start_of); });
            const int si = first + t;
            for (int k = 0; k < RH.n; k++) {
                P.tk_score[tks_index(U, k, si)] = hs[k];
#pragma unroll
                for (int e = 0; e < E; e++)
                    P.tk_idx[tk_index(U, k, e, si)] = s_A[e] + (int)it_idx[s_item0[t] - it0 + pos_base(pk, e) + (int)((hx[k] >> (8 * e)) & 255ull)];
            }
            s_amb[t] = 0;   // (read again only by this thread: below, and when the tile hands its undecided spans on)
        }
        if (live && t >= seg && t < send && mine && !s_amb[t]) {
            // a span's list has min(5, feasible tuples) entries in every pass; the unused entries keep the -1 / NaN
            // pattern of tw_load_batch and are never written (most lists are short: this halves the store traffic)
            const int64_t g = U.in_off + i;
            const int leaves = s_leaves[t];
            P.tk_n[g] = leaves < kTopK ? leaves : kTopK;
            P.leaves[g] = leaves;
            if (pass == 1) P.leaves0[g] = leaves;
            P.rep[g] = 0;
            if (pass == 1) {
#pragma unroll
                for (int e = 0; e < E; e++) {
                    P.c_bits[ie_index(U, e, i) * kCandWords] = (uint64_t)(ordered ? s_bits[e][t] : s_cm[e][t]);
                    for (int w = 1; w < kCandWords; w++) P.c_bits[ie_index(U, e, i) * kCandWords + w] = 0;
                }
            }
        }
        group_sync();
        TW_TILE_TICK(6);
        seg = send;
    }
    TW_TILE_FLUSH();
    // rare (millisecond-granular data): CPython's heapq / list.sort must be replayed push by push -- the wavefront kernel does
    heavy_append<E>(P, mine && s_amb[live ? t : 0] != 0, true, false, T.unit, i);
}

}  // namespace tw

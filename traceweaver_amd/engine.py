"""numpy-level wrapper around the C-ABI (include/traceweaver_amd.h).

A *unit* is one call of the reference's TraceWeaverV3.FindAssignments (traceweaver_v3.py:1087): one
service, its incoming spans and its outgoing spans per endpoint.  Units of a batch are independent and
are solved together on one GPU.
"""
import ctypes
import os
import warnings

import numpy as np

from . import _ffi


class EngineError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("%s (%d): %s" % (_ffi.STATUS.get(code, "TW_ERR"), code, message))
        self.code = code


class UnitArrays(object):
    """Structure-of-arrays form of one unit: endpoints in topological order of the call-order DAG
    (traceweaver_v1.py:37-39), every span list sorted by (start, end) (executor.py:1112)."""

    AFTER_CUT, BEFORE_CUT = 1, 2   # tw_batch.unit_part

    def __init__(self, in_start, in_end, out_off, out_start, out_end, dag, key_rank=None, time_scale=None, part=0):
        # time_scale: None = int64 microseconds.  A power of two = the timestamps are exact images of binary64
        # values in units of time_scale microseconds (load-scaled units, traceweaver_amd.transforms).
        self.time_scale = None if time_scale is None else float(time_scale)
        # part: the unit is a stretch of a service's requests between cuts (sharding.split_unit): AFTER_CUT / BEFORE_CUT
        self.part = int(part)
        self.in_start = np.ascontiguousarray(in_start, dtype=np.int64)
        self.in_end = np.ascontiguousarray(in_end, dtype=np.int64)
        self.out_off = np.ascontiguousarray(out_off, dtype=np.int64)
        self.out_start = np.ascontiguousarray(out_start, dtype=np.int64)
        self.out_end = np.ascontiguousarray(out_end, dtype=np.int64)
        self.E = len(self.out_off) - 1
        self.n_in = len(self.in_start)
        self.dag = np.ascontiguousarray(dag, dtype=np.uint8).reshape(self.E, self.E)
        self.key_rank = np.ascontiguousarray(np.arange(self.E) if key_rank is None else key_rank, dtype=np.int32)
        if len(self.in_end) != self.n_in or len(self.out_start) != self.out_off[-1] or len(self.out_end) != len(self.out_start):
            raise ValueError("inconsistent unit arrays")

    @property
    def nslot(self):
        return self.E * self.E + 2 * self.E

    @property
    def n_spans(self):
        return self.n_in + len(self.out_start)


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else ctypes.c_void_p(0)


class _PinnedPool(object):
    """Page-locked staging arrays for Engine.load (tw_host_alloc): the concatenation of the units' arrays has to be
    written somewhere anyway -- written into pinned memory, tw_load_batch moves it at the full host-link rate."""

    def __init__(self, lib):
        self._lib = lib
        self._bufs = {}

    def array(self, name, count, dtype):
        dtype = np.dtype(dtype)
        need = max(int(count) * dtype.itemsize, 8)
        buf = self._bufs.get(name)
        if buf is None or buf[1] < need:
            if buf is not None:
                self._lib.tw_host_free(buf[0])
            p = ctypes.c_void_p(0)
            cap = need + need // 4
            if self._lib.tw_host_alloc(cap, ctypes.byref(p)) != 0 or not p.value:
                raise MemoryError("tw_host_alloc(%d) failed" % cap)
            buf = (p, cap)
            self._bufs[name] = buf
        raw = (ctypes.c_char * need).from_address(buf[0].value)
        return np.frombuffer(raw, dtype=dtype, count=int(count))

    def close(self):
        for p, _ in self._bufs.values():
            self._lib.tw_host_free(p)
        self._bufs = {}


class Engine(object):
    def __init__(self, device=0, lib_path=None):
        self._lib = _ffi.load(lib_path)
        self._h = ctypes.c_void_p(0)
        rc = self._lib.tw_create(int(device), ctypes.byref(self._h))
        if rc != 0:
            raise EngineError(rc, "tw_create failed on device %d" % device)
        self.units = []
        self._keep = None
        self._n_traces = 0
        self._pinned = _PinnedPool(self._lib)
        self.last_load_s = {}

    def close(self):
        if self._h:
            self._keep = None
            self._pinned.close()
            self._lib.tw_destroy(self._h)
            self._h = ctypes.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self._lib.tw_last_error(self._h).decode())

    # ------------------------------------------------------------------------------------------
    _warned_queues = False

    def load(self, units, batch_size=100, batch_size_mis=30, skip=None):
        """Copy a list of UnitArrays into HBM.  skip: None, or per unit a skipmode.SkipPlan (time windows, skip-span pools,
        (mean, std) table) -- the batch then runs the reference's one-pass skip mode (run_pass1 only)."""
        self.units = list(units)
        self.skip_mode = skip is not None
        in_off = np.zeros(len(units) + 1, dtype=np.int64)
        np.cumsum([u.n_in for u in units], out=in_off[1:])
        unit_E = np.array([u.E for u in units], dtype=np.int32)
        # every endpoint-count class runs on a stream of its own; the HIP runtime maps a process' streams onto GPU_MAX_HW_QUEUES
        # hardware queues (4 unless the host exports more BEFORE HIP initialises) and classes that share a queue run one after the
        # other: 9.5 instead of 6.3 ms per pass on an eight-class batch (tw_create).  The library leaves the variable alone
        # (it holds for the whole process): tell a host that embeds the engine, once.
        if len(set(unit_E.tolist())) > 3 and "GPU_MAX_HW_QUEUES" not in os.environ and not Engine._warned_queues:
            Engine._warned_queues = True
            warnings.warn("traceweaver_amd: this batch has %d endpoint-count classes and GPU_MAX_HW_QUEUES is not set: their streams share the "
                          "runtime's 4 hardware queues and partly serialise.  Export GPU_MAX_HW_QUEUES=12 before the process touches the GPU "
                          "(or TW_SET_HW_QUEUES=1 before importing traceweaver_amd)." % len(set(unit_E.tolist())))
        ep_off = [0]
        base = 0
        for u in units:
            ep_off.extend((base + u.out_off[1:]).tolist())
            base += int(u.out_off[-1])
        arrays = {
            "unit_in_off": in_off, "unit_E": unit_E, "ep_off": np.array(ep_off, dtype=np.int64),
            "dag": np.concatenate([u.dag.ravel() for u in units]),
            "key_rank": np.concatenate([u.key_rank for u in units]),
        }
        self._keep = None   # views of the pinned buffers of the previous batch
        n_in_total, n_out_total = int(in_off[-1]), int(base)
        for name, total in (("in_start", n_in_total), ("in_end", n_in_total), ("out_start", n_out_total), ("out_end", n_out_total)):
            dst = self._pinned.array(name, total, np.int64)   # the span arrays (16 B per span) go through page-locked memory
            np.concatenate([getattr(u, name) for u in units], out=dst)
            arrays[name] = dst
        scaled = [u.time_scale is not None for u in units]
        if any(scaled) and not all(scaled):
            raise ValueError("a batch holds either integer-microsecond units or load-scaled units, not both")
        arrays["unit_time_scale"] = np.array([u.time_scale for u in units], dtype=np.float64) if all(scaled) else None
        arrays["unit_part"] = np.array([u.part for u in units], dtype=np.uint8) if any(u.part for u in units) else None
        skip_arr = None
        if skip is not None:
            if len(skip) != len(units):
                raise ValueError("one skip plan per unit")
            skip_arr = (_ffi.SkipUnit * len(units))()
            for k, (u, sp) in enumerate(zip(units, skip)):
                tw = np.ascontiguousarray(sp.tw_start, dtype=np.int64)
                pool = np.ascontiguousarray(sp.pool, dtype=np.int32).reshape(u.E, len(tw))
                dist = np.ascontiguousarray(sp.dist, dtype=np.float64).reshape(u.E + 1, u.E + 1, 2)
                arrays["skip%d" % k] = (tw, pool, dist)
                skip_arr[k] = _ffi.SkipUnit(len(tw), _vp(tw), _vp(pool), _vp(dist))
            arrays["skip"] = skip_arr
        self._keep = arrays
        b = _ffi.Batch(len(units), *[_vp(arrays[k]) for k in (
            "unit_in_off", "unit_E", "ep_off", "dag", "key_rank", "in_start", "in_end", "out_start", "out_end")],
            batch_size, batch_size_mis, _ffi.TW_TOPK, _vp(arrays["unit_time_scale"]),
            ctypes.cast(skip_arr, ctypes.c_void_p) if skip_arr is not None else ctypes.c_void_p(0), _vp(arrays["unit_part"]))
        self._check(self._lib.tw_load_batch(self._h, ctypes.byref(b), 0))
        self._n_cohorts = 1                                           # (the cohort labels go with the row maps)
        self._last_pass, self._n_rows = 0, 0
        self._in_off = in_off
        self._ie_off = np.concatenate([[0], np.cumsum([u.n_in * u.E for u in units])]).astype(np.int64)
        self._slot_off = np.concatenate([[0], np.cumsum([u.nslot for u in units])]).astype(np.int64)
        self._gap_off = np.concatenate([[0], np.cumsum([u.nslot * u.n_in for u in units])]).astype(np.int64)
        self._nblk = [(u.n_in + batch_size - 1) // batch_size for u in units]
        self._gp_off = np.concatenate([[0], np.cumsum([nb * u.nslot for nb, u in zip(self._nblk, units)])]).astype(np.int64)

    def run_pass1(self):
        self._check(self._lib.tw_run_pass1(self._h))
        self._last_pass = 1

    def run_pass2(self):
        self._check(self._lib.tw_run_pass2(self._h))
        self._last_pass = 2

    def gaps(self):
        """Per unit: [nslot, n_in] gap samples of the pass-1 assignment (NaN = dropped / unscored slot)."""
        g = np.empty(int(self._gap_off[-1]), dtype=np.float64)
        self._check(self._lib.tw_get_gaps(self._h, _vp(g)))
        return [g[self._gap_off[k]:self._gap_off[k + 1]].reshape(u.nslot, u.n_in) for k, u in enumerate(self.units)]

    def set_gaps(self, gaps):
        """Per unit [nslot, n_in] gap samples (NaN = none) in place of the ones pass 1 produced: the input of fit_mixtures
        for a service whose requests were solved in parts (traceweaver_amd/sharding.py)."""
        g = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in gaps]))
        if len(g) != self._gap_off[-1]:
            raise ValueError("gap rows do not match the loaded batch")
        self._check(self._lib.tw_set_gaps(self._h, _vp(g)))

    class _DeviceArray(object):
        """A device buffer of the engine as the CUDA array interface describes it (torch.as_tensor takes it without a copy)."""

        def __init__(self, ptr, count, typestr):
            self.__cuda_array_interface__ = {"data": (int(ptr), False), "shape": (int(count),), "typestr": typestr, "version": 2}

    def device_views(self):
        """(parent, gaps): the engine's device buffers of the two exchange steps (tw_device_buffers) as objects with
        `__cuda_array_interface__` -- int32 [sum E * n_in] parent indices of the last pass run, float64 gap rows of pass 1;
        `torch.as_tensor(view, device="cuda")` wraps them in place for an all-gather over RCCL (sharding.py)."""
        v = _ffi.DeviceView()
        self._check(self._lib.tw_device_buffers(self._h, ctypes.byref(v)))
        return (Engine._DeviceArray(v.parent or 0, v.parent_count, "<i4"), Engine._DeviceArray(v.gaps or 0, v.gaps_count, "<f8"))

    def set_gaps_device(self, ptr):
        """set_gaps with a device pointer (int): the gathered rows stay in HBM."""
        self._check(self._lib.tw_set_gaps_device(self._h, ctypes.c_void_p(int(ptr))))

    def set_mixtures(self, mix_n, mix_p):
        """mix_n / mix_p: per unit arrays [nslot] int32 and [nslot, 5, 3] (weight, mean, precision_cholesky)."""
        n = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.int32).ravel() for a in mix_n]), dtype=np.int32)
        p = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1, _ffi.TW_MAX_COMP, 3) for a in mix_p]))
        if len(n) != self._slot_off[-1] or len(p) != len(n):
            raise ValueError("mixture tables do not match the loaded batch")
        self._check(self._lib.tw_set_mixtures(self._h, _vp(n), _vp(p)))

    FIT_ROW_DRAWS = (0, 1, 4, 11, 21, 34)   # uniforms the model-selection fits of a row draw, by min(5, #unique)

    def fit_mixtures(self, tape=None, slot_off=None, seed=None, unit_seeds=None):
        """The reference's refit of every scored edge on the device, from the pass-1 gap samples (csrc/tw_fit.h).
        Without a tape the k-means++ draws come from the engine's own MT19937 (`seed` reseeds it first) or, with
        `unit_seeds`, from one MT19937 per unit (a unit's fit then does not depend on its batch); with (tape, slot_off) --
        per unit arrays of offsets [nslot] into one tape -- from the caller (see fit_rows)."""
        if unit_seeds is not None:
            sd = np.ascontiguousarray(unit_seeds, dtype=np.uint32)
            if len(sd) != len(self.units):
                raise ValueError("one seed per unit")
            self._check(self._lib.tw_fit_mixtures_seeded(self._h, _vp(sd)))
            return
        if tape is None:
            if seed is not None:
                self._check(self._lib.tw_set_fit_seed(self._h, int(seed)))
            self._check(self._lib.tw_fit_mixtures(self._h))
            return
        t = np.ascontiguousarray(tape, dtype=np.float64)
        o = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.int64).ravel() for a in slot_off]), dtype=np.int64)
        if len(o) != self._slot_off[-1]:
            raise ValueError("tape offsets do not match the loaded batch")
        self._check(self._lib.tw_fit_mixtures_tape(self._h, _vp(t), len(t), _vp(o)))

    def fit_rows(self):
        """Per unit [nslot]: min(5, #distinct samples) of every gap row of the pass-1 result (0 = nothing to fit) -- the
        number of model-selection fits of that edge, hence the uniforms they draw (FIT_ROW_DRAWS)."""
        m = np.empty(int(self._slot_off[-1]), dtype=np.int32)
        self._check(self._lib.tw_fit_rows(self._h, _vp(m)))
        return [m[self._slot_off[k]:self._slot_off[k + 1]] for k in range(len(self.units))]

    def fit_order(self):
        """The order tables of the last refit (tw_get_fit_order): (order_seed [4 S], order_em [5 S], order_row [S]) for the batch's S
        slots -- block (5 - count) * S + slot, or the row, that each workgroup of the refit's launches served, the longest fits first --
        or None: the refit ran in grid order (TW_FIT_ORDER=0)."""
        s = int(self._slot_off[-1])
        seed, em, row = np.empty(4 * s, dtype=np.int32), np.empty(5 * s, dtype=np.int32), np.empty(s, dtype=np.int32)
        present = ctypes.c_int32(0)
        self._check(self._lib.tw_get_fit_order(self._h, _vp(seed), _vp(em), _vp(row), ctypes.byref(present)))
        return (seed, em, row) if present.value else None

    def mixtures(self):
        """Per unit (mix_n [nslot], mix_p [nslot, 5, 3]) currently resident on the device."""
        n = np.empty(int(self._slot_off[-1]), dtype=np.int32)
        p = np.empty((int(self._slot_off[-1]), _ffi.TW_MAX_COMP, 3), dtype=np.float64)
        self._check(self._lib.tw_get_mixtures(self._h, _vp(n), _vp(p)))
        return [(n[self._slot_off[k]:self._slot_off[k + 1]], p[self._slot_off[k]:self._slot_off[k + 1]])
                for k in range(len(self.units))]

    def gauss_params(self):
        """Per unit: [nblk, nslot, 3] = mean, std, log(std used) of pass 1 (NaN for unscored slots)."""
        g = np.empty((int(self._gp_off[-1]), 3), dtype=np.float64)
        self._check(self._lib.tw_get_gauss_params(self._h, _vp(g)))
        return [g[self._gp_off[k]:self._gp_off[k + 1]].reshape(self._nblk[k], u.nslot, 3) for k, u in enumerate(self.units)]

    _FIELDS = ("parent", "topk_idx", "topk_score", "topk_n", "chosen", "leaves", "window_end", "unit_stats")

    def results(self, which, fields=None):
        """Per unit dict: parent [E,n], topk_idx [5,E,n], topk_score [5,n], topk_n, chosen, leaves, window_end
        and the counters.  `fields` restricts what is copied back from the device."""
        fields = self._FIELDS if fields is None else tuple(fields)
        n_in = int(self._in_off[-1])
        n_ie = int(self._ie_off[-1])
        K = _ffi.TW_TOPK
        shapes = {
            "parent": (n_ie, np.int32), "topk_idx": (n_ie * K, np.int32), "topk_score": (n_in * K, np.float64),
            "topk_n": (n_in, np.int32), "chosen": (n_in, np.int32), "leaves": (n_in, np.int64),
            "window_end": (n_in, np.uint8), "unit_stats": ((len(self.units), 8), np.int64),
        }
        buf = {k: (np.empty(*shapes[k]) if k in fields else None) for k in self._FIELDS}
        r = _ffi.Results(*[_vp(buf[k]) for k in self._FIELDS])
        self._check(self._lib.tw_get_results(self._h, int(which), ctypes.byref(r)))
        out = []
        for k, u in enumerate(self.units):
            a, b = int(self._in_off[k]), int(self._in_off[k + 1])
            ia, ib = int(self._ie_off[k]), int(self._ie_off[k + 1])
            o = {}
            if buf["parent"] is not None:
                o["parent"] = buf["parent"][ia:ib].reshape(u.E, u.n_in)
            if buf["topk_idx"] is not None:
                o["topk_idx"] = buf["topk_idx"][K * ia:K * ib].reshape(K, u.E, u.n_in)
            if buf["topk_score"] is not None:
                o["topk_score"] = buf["topk_score"][K * a:K * b].reshape(K, u.n_in)
            for name in ("topk_n", "chosen", "leaves", "window_end"):
                if buf[name] is not None:
                    o[name] = buf[name][a:b]
            if buf["unit_stats"] is not None:
                st = buf["unit_stats"][k]
                o.update({"not_best_count": int(st[0]), "cnt_unassigned": int(st[1]), "n_windows": int(st[2]),
                          "repaired_windows": int(st[3]), "budget_windows": int(st[4]), "search_nodes": int(st[5]),
                          "dp_windows": int(st[6]), "dfs_components": int(st[7])})
            out.append(o)
        return out

    # ------------------------------------------------------------------------------------------
    def scale_load(self, factors, trace_rank=None):
        """helpers/transforms.py:10-40 (repeat_change_spans) on the resident table (tw_scale_load): per unit an integer load
        factor; trace_rank = per unit [n_in] ranks of the requests' trace ids (tie order of the re-sort; None = current
        order).  Needs set_truth.  Every call scales the table as uploaded.  Returns per unit (in_perm [n_in],
        [out_perm_e [n_in]] * E, time_scale) -- old index of every new position.  (self.units keeps the arrays as uploaded.)"""
        f = np.ascontiguousarray(np.asarray(factors, dtype=np.int32))
        if len(f) != len(self.units):
            raise ValueError("one load factor per unit")
        tr = None
        if trace_rank is not None:
            tr = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.int32).ravel() for a in trace_rank]), dtype=np.int32)
            if len(tr) != self._in_off[-1]:
                raise ValueError("trace_rank does not match the loaded batch")
        n_out = int(sum(int(u.out_off[-1]) for u in self.units))
        ip = np.zeros(int(self._in_off[-1]), dtype=np.int32)
        op = np.zeros(n_out, dtype=np.int32)
        ts = np.zeros(len(self.units), dtype=np.float64)
        self._check(self._lib.tw_scale_load(self._h, _vp(f), _vp(tr), _vp(ip), _vp(op), _vp(ts)))
        self._n_cohorts = 1
        self._last_pass = 0
        out, o = [], 0
        for k, u in enumerate(self.units):
            a, b = int(self._in_off[k]), int(self._in_off[k + 1])
            outs = []
            for e in range(u.E):
                m = int(u.out_off[e + 1] - u.out_off[e])
                outs.append(op[o:o + m].copy())
                o += m
            out.append((ip[a:b].copy(), outs, float(ts[k])))
        return out

    def worklists(self):
        """Sizes of the device work lists of the last pass (debug aid, tw_debug_worklists): windows sent to the exact
        search, spans sent to the wavefront enumeration per endpoint count, spans whose enumeration was split into parts
        and, of those, the ones enumerated once more as a whole (order of equal scores not decided by the parts); items the lean wavefront
        kernel handed to k_enumerate_heavy, spans that were refused parts (budget of extra list entries / arena exhausted), list parts."""
        out = np.zeros(16, dtype=np.int32)
        self._lib.tw_debug_worklists.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._check(self._lib.tw_debug_worklists(self._h, _vp(out)))
        return {"select_windows": int(out[0]), "enumerate_spans": [int(x) for x in out[1:10]], "split_spans": int(out[10]), "split_redone": int(out[11]),
                "handed_to_heavy": int(out[12]), "parts_refused": int(out[13]), "list_parts": int(out[14])}

    def set_truth(self, true_parent, in_trace=None, n_traces=0):
        """Ground truth of the loaded batch: per unit [E, n_in] index of the true outgoing span; optionally per
        unit [n_in] trace numbers in [0, n_traces) for the per-trace (end-to-end) accuracy."""
        t = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.int32).ravel() for a in true_parent]), dtype=np.int32)
        if len(t) != self._ie_off[-1]:
            raise ValueError("truth does not match the loaded batch")
        tr = None
        if in_trace is not None:
            tr = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.int32).ravel() for a in in_trace]), dtype=np.int32)
            if len(tr) != self._in_off[-1]:
                raise ValueError("in_trace does not match the loaded batch")
        self._n_traces = int(n_traces) if tr is not None else 0
        self._check(self._lib.tw_set_truth(self._h, _vp(t), _vp(tr), int(n_traces)))

    def evaluate(self, trace_flags=False):
        """helpers/utils.py:62-145 on the device, for the last pass run.  Returns per unit
        {n_in, correct, correct_topk, unassigned, accuracy, topk_accuracy} and, when trace numbers were given,
        (traces right, traces right under top-5) -- plus the raw [2, n_traces] wrong-flags if asked for."""
        per = np.zeros((len(self.units), 4), dtype=np.int64)
        flags = np.zeros((2, self._n_traces), dtype=np.uint8) if (trace_flags and self._n_traces) else None
        e2e = np.zeros(2, dtype=np.int64) if self._n_traces else None
        self._check(self._lib.tw_evaluate(self._h, _vp(per), _vp(flags), _vp(e2e)))
        out = [{"n_in": int(r[0]), "correct": int(r[1]), "correct_topk": int(r[2]), "unassigned": int(r[3]),
                "accuracy": float(r[1]) / max(int(r[0]), 1), "topk_accuracy": float(r[2]) / max(int(r[0]), 1)} for r in per]
        if e2e is None:
            return out
        return (out, (int(e2e[0]), int(e2e[1])), flags) if trace_flags else (out, (int(e2e[0]), int(e2e[1])))

    # ------------------------------------------------------------------------------------------
    def set_span_rows(self, in_rows, out_rows, row_link, row_kind, row_start, row_end):
        """The span-table rows of the loaded batch and the table's observed links (tw_set_span_rows; traces.rows_from_units
        builds the arguments): per unit in_rows [n_in] and out_rows = one array per endpoint, then the table's columns
        [n_rows].  load() and scale_load() drop them."""
        ir = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.int32).ravel() for a in in_rows]), dtype=np.int32)
        flat = [np.asarray(a, dtype=np.int32).ravel() for per in out_rows for a in per]
        orow = np.ascontiguousarray(np.concatenate(flat) if flat else np.zeros(0, np.int32), dtype=np.int32)
        if len(ir) != self._in_off[-1] or len(orow) != sum(int(u.out_off[-1]) for u in self.units) or \
                any(len(a) != int(u.out_off[e + 1] - u.out_off[e]) for u, per in zip(self.units, out_rows) for e, a in enumerate(per)):
            raise ValueError("row maps do not match the loaded batch")
        link = np.ascontiguousarray(row_link, dtype=np.int32)
        kind = np.ascontiguousarray(row_kind, dtype=np.uint8)
        start = np.ascontiguousarray(row_start, dtype=np.int64)
        end = np.ascontiguousarray(row_end, dtype=np.int64)
        if not (len(link) == len(kind) == len(start) == len(end)):
            raise ValueError("the table's columns differ in length")
        self._check(self._lib.tw_set_span_rows(self._h, len(link), _vp(ir), _vp(orow), _vp(link), _vp(kind), _vp(start), _vp(end)))
        self._n_rows = len(link)
        self._n_cohorts = 1

    def set_parents(self, parents):
        """An assignment that this engine's last pass did not produce (per unit [E, n_in]; services solved one after the
        other, or gathered from other ranks): stitch(pass_=0) stitches it (tw_set_parents)."""
        p = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.int32).ravel() for a in parents]), dtype=np.int32)
        if len(p) != self._ie_off[-1]:
            raise ValueError("parent arrays do not match the loaded batch")
        self._check(self._lib.tw_set_parents(self._h, _vp(p)))

    def stitch(self, pass_=None, truth=False):
        """The assignment of a pass (None = the last pass run) -- or, with truth=True, the true one of set_truth -- joined
        with the observed links into whole traces on the device (tw_stitch_traces).  Returns traces.StitchedTraces."""
        from .traces import StitchedTraces

        n = int(getattr(self, "_n_rows", 0))
        root, depth, tree_rows = (np.empty(n, dtype=np.int32) for _ in range(3))
        tree_off = np.empty(n + 1, dtype=np.int64)
        tree_root = np.empty(n, dtype=np.int32)
        tree_latency = np.empty(n, dtype=np.int64)
        tree_flags = np.empty(n, dtype=np.uint8)
        out = _ffi.Stitched(*[_vp(a) for a in (root, depth, tree_off, tree_rows, tree_root, tree_latency, tree_flags)])
        nt = ctypes.c_int64(0)
        counts = np.zeros(4, dtype=np.int64)
        which = int(getattr(self, "_last_pass", 0)) if pass_ is None else int(pass_)
        self._check(self._lib.tw_stitch_traces(self._h, which, 1 if truth else 0, ctypes.byref(out), ctypes.byref(nt), _vp(counts)))
        k = int(nt.value)
        self._n_trees = k
        self._tree_root = tree_root[:k].copy()
        return StitchedTraces(root, depth, tree_off[:k + 1].copy(), tree_rows, tree_root[:k].copy(), tree_latency[:k].copy(),
                              tree_flags[:k].copy(), counts)

    def stitch_timing(self):
        """The last stitch on the device (HIP events, ms): whole (without the copies to the host), link table, doubling
        rounds, rows per root + scan + scatter, per-tree order and figures; `rounds` = doubling rounds."""
        ms = np.zeros(16, dtype=np.float64)
        self._check(self._lib.tw_get_timing(self._h, _vp(ms), 16))
        return dict(zip(("stitch", "links", "jump", "scatter", "group", "rounds"), ms[10:16].tolist()))

    def set_row_groups(self, row_group, n_groups):
        """The group of every span-table row, in [0, n_groups) or -1 = not counted (tw_set_row_groups; traces.groups_from_table
        groups by service).  Call it after set_span_rows; dropped with the row maps."""
        g = np.ascontiguousarray(row_group, dtype=np.int32)
        if len(g) != int(getattr(self, "_n_rows", 0)):
            raise ValueError("row_group does not match the span rows")
        self._check(self._lib.tw_set_row_groups(self._h, int(n_groups), _vp(g)))
        self._n_groups = int(n_groups)

    def attribute(self, percentile=0.0, start_min=None, start_max=None, need_flags=1, skip_flags=2):
        """Latency attribution on the forest of the last stitch() (tw_attribute_traces): per row self time and critical-path
        time, per tree the top group, per group the totals over the selected trees -- the eligible trees (flags hold need_flags,
        none of skip_flags; default: whole traces without an unassigned call) from rank int(percentile * n_eligible) by
        latency on, whose root starts in [start_min, start_max).  Returns traces.Attribution."""
        from .traces import Attribution

        n, G = int(getattr(self, "_n_rows", 0)), int(getattr(self, "_n_groups", 0))
        lo = np.iinfo(np.int64).min if start_min is None else int(start_min)
        hi = np.iinfo(np.int64).max if start_max is None else int(start_max)
        q = _ffi.AttrQuery(float(percentile), lo, hi, int(need_flags), int(skip_flags))
        link = np.empty(n, dtype=np.int32)
        self_time, path_time = (np.empty(n, dtype=np.int64) for _ in range(2))
        top, path_rows = (np.empty(n, dtype=np.int32) for _ in range(2))
        selected = np.empty(n, dtype=np.uint8)
        groups = np.zeros((7, max(G, 1)), dtype=np.int64)
        out = _ffi.Attribution(*[_vp(a) for a in (link, self_time, path_time, top, selected, path_rows)] + [_vp(groups[c]) for c in range(7)])
        summary = np.zeros(6, dtype=np.int64)
        self._check(self._lib.tw_attribute_traces(self._h, ctypes.byref(q), ctypes.byref(out), _vp(summary)))
        k = int(summary[5])
        return Attribution(link, self_time, path_time, top[:k].copy(), selected[:k].copy(), path_rows[:k].copy(), groups[:, :G].copy(), summary[:5])

    def attribute_timing(self):
        """The last attribute() on the device (HIP events, ms): per-tree kernel, selection (flags, sort, mark), group reduction."""
        ms = np.zeros(19, dtype=np.float64)
        self._check(self._lib.tw_get_timing(self._h, _vp(ms), 19))
        return dict(zip(("tree", "select", "reduce"), ms[16:19].tolist()))

    def decisions(self, pass_=None):
        """The decision of every request of the resident pass (None = the last pass run; tw_get_decisions): per unit a dict
        rank [n_in] (= chosen, -1 none), list_n [n_in] (length of the list the selection chose from: the one enumerated again
        on the remaining spans where that happened) and margin [n_in] (float64: rank 0: best score less the runner-up's, +inf
        for a list of one; rank > 0: the chosen score less the best, <= 0; rank -1: NaN)."""
        n = int(self._in_off[-1])
        rank, list_n, margin = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float64)
        which = int(getattr(self, "_last_pass", 0)) if pass_ is None else int(pass_)
        self._check(self._lib.tw_get_decisions(self._h, which, _vp(rank), _vp(list_n), _vp(margin)))
        return [{"rank": rank[a:b], "list_n": list_n[a:b], "margin": margin[a:b]} for a, b in zip(self._in_off[:-1].tolist(), self._in_off[1:].tolist())]

    def score_traces(self, threshold=0.0, edges=()):
        """Confidence of the traces of the last stitch() of a pass (tw_score_traces): the per-request decisions reduced over
        every tree, the calibration table over the whole trees with bucket edges `edges` (ascending, at most 15), and the
        CONFIDENT bit (not_best == 0 and min_margin >= threshold) set in the forest attribute() works on:
        attribute(need_flags=traces.WHOLE | traces.CONFIDENT).  Returns traces.TraceConfidence."""
        from .traces import TraceConfidence

        n, rows = int(self._in_off[-1]), int(getattr(self, "_n_rows", 0))
        ed = np.ascontiguousarray(edges, dtype=np.float64).ravel()
        q = _ffi.ConfQuery(float(threshold), len(ed), _vp(ed) if len(ed) else ctypes.c_void_p(0))
        rank, list_n, row_request = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty(rows, dtype=np.int32)
        margin = np.empty(n, dtype=np.float64)
        dec, nb, una, weakest = (np.empty(rows, dtype=np.int32) for _ in range(4))
        min_margin = np.empty(rows, dtype=np.float64)
        confident = np.empty(rows, dtype=np.uint8)
        calib = np.zeros((min(len(ed), _ffi.TW_CONF_MAX_EDGES) + 2, 3), dtype=np.int64)
        out = _ffi.Confidence(*[_vp(a) for a in (rank, list_n, margin, row_request, dec, nb, una, min_margin, weakest, confident, calib)])
        summary = np.zeros(5, dtype=np.int64)
        self._check(self._lib.tw_score_traces(self._h, ctypes.byref(q), ctypes.byref(out), _vp(summary)))
        k = int(self._n_trees)                                        # (of the stitch the call worked on: it succeeded)
        return TraceConfidence(rank, list_n, margin, row_request, dec[:k].copy(), nb[:k].copy(), una[:k].copy(), min_margin[:k].copy(),
                               weakest[:k].copy(), confident[:k].copy(), calib, summary, float(threshold), ed)

    def score_timing(self):
        """The last score_traces() on the device (HIP events, ms): decision kernel, row map + per-tree reduction, calibration."""
        ms = np.zeros(22, dtype=np.float64)
        self._check(self._lib.tw_get_timing(self._h, _vp(ms), 22))
        return dict(zip(("decisions", "trees", "calibration"), ms[19:22].tolist()))

    def set_row_cohorts(self, labels, n_cohorts):
        """The cohort label of every span-table row, in [0, n_cohorts) or -1 = the row says nothing (tw_set_row_cohorts): a
        tree's cohort is the smallest label among its rows.  labels=None with n_cohorts=1: back to one cohort that holds every
        tree.  Call it after set_span_rows; dropped with the row maps."""
        if labels is None:
            self._check(self._lib.tw_set_row_cohorts(self._h, int(n_cohorts), None))
            self._n_cohorts = 1
            return
        c = np.ascontiguousarray(labels, dtype=np.int32)
        if len(c) != int(getattr(self, "_n_rows", 0)):
            raise ValueError("labels do not match the span rows")
        self._check(self._lib.tw_set_row_cohorts(self._h, int(n_cohorts), _vp(c)))
        self._n_cohorts = int(n_cohorts)

    def distributions(self, probs=(0.5, 0.9, 0.95, 0.99), edges=None, values=True):
        """The populations behind the last attribute() (tw_latency_distributions): per cohort, metric (span latency, self time,
        path time, trace latency) and group the sorted values of the selected trees, their count and sum, the quantiles at
        `probs` and, with `edges` (strictly ascending integers, at most 63), a histogram.  values=False leaves the sorted values on
        the device (`values` is then empty).  Returns traces.LatencyDistributions."""
        from .traces import LatencyDistributions

        G, C = int(getattr(self, "_n_groups", 0)), int(getattr(self, "_n_cohorts", 1))
        n_seg = C * (3 * G + 1)
        pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
        ed = np.ascontiguousarray(() if edges is None else edges, dtype=np.int64).ravel()
        q = _ffi.DistQuery(len(pr), _vp(pr) if len(pr) else ctypes.c_void_p(0), len(ed), _vp(ed) if len(ed) else ctypes.c_void_p(0))
        nq, bins = min(len(pr), _ffi.TW_DIST_MAX_Q), min(len(ed), _ffi.TW_DIST_MAX_EDGES) + 1
        tree_cohort = np.empty(max(int(getattr(self, "_n_trees", 0)), 1), dtype=np.int32)
        seg_count, seg_sum = np.zeros(n_seg, dtype=np.int64), np.zeros(n_seg, dtype=np.int64)
        seg_off = np.zeros(n_seg + 1, dtype=np.int64)
        quantile = np.zeros((n_seg, nq), dtype=np.int64)
        hist = np.zeros((n_seg, bins), dtype=np.int64)
        summary = np.zeros(4, dtype=np.int64)
        out = _ffi.Distributions(_vp(tree_cohort), _vp(seg_count), _vp(seg_sum), _vp(seg_off), None, _vp(quantile) if nq else None, _vp(hist))
        self._check(self._lib.tw_latency_distributions(self._h, ctypes.byref(q), ctypes.byref(out), _vp(summary)))
        values = np.empty(int(summary[0]) if values else 0, dtype=np.int64)   # the sorted items are resident: the second call only copies them
        if len(values):
            only = _ffi.Distributions(None, None, None, None, _vp(values), None, None)
            self._check(self._lib.tw_latency_distributions(self._h, ctypes.byref(q), ctypes.byref(only), None))
        return LatencyDistributions(tree_cohort[:int(self._n_trees)].copy(), seg_count, seg_sum, seg_off, values, quantile, hist, summary, C, G, pr, ed)

    def distributions_timing(self):
        """The last distributions() on the device (HIP events, ms): items and counts (cohorts, the two sweeps over the rows);
        sort, offsets and values; quantiles and histogram."""
        ms = np.zeros(25, dtype=np.float64)
        self._check(self._lib.tw_get_timing(self._h, _vp(ms), 25))
        return dict(zip(("items", "sort", "quantiles"), ms[22:25].tolist()))

    def compare_cohorts(self, pairs=((0, 1),), probs=(0.5, 0.95, 0.99), permutations=0, seed=0, max_pool=0):
        """Pairs of cohorts (a, b) compared segment by segment on the device (tw_compare_cohorts), on what distributions() works
        on: per (pair, metric, group) the sizes, the two-sample KS gap and where it lies, twice the Mann-Whitney U of b over a,
        the quantile shifts Q_b - Q_a at `probs` (at most 8) and, with `permutations` > 0 (at most 65536), how many permutations
        of the pooled values are at least as extreme in each of them (`seed` selects the draws; rows of more than `max_pool`
        pooled values, when it is > 0, are not permuted).  Returns traces.CohortComparison."""
        return self._compare(self._lib.tw_compare_cohorts, int(getattr(self, "_n_groups", 0)), pairs, probs, permutations, seed, max_pool)

    def _compare(self, call, G, pairs, probs, permutations, seed, max_pool):
        """tw_compare_cohorts / tw_history_compare: the query, the output arrays of n_pairs * (3 G + 1) rows, the call."""
        from .traces import CohortComparison

        pa = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
        n_rows = min(len(pa), _ffi.TW_CMP_MAX_PAIRS) * (3 * G + 1)
        nq, n_perm = min(len(pr), _ffi.TW_CMP_MAX_Q), int(permutations)
        q = _ffi.CmpQuery(len(pa), _vp(pa) if len(pa) else ctypes.c_void_p(0), len(pr), _vp(pr) if len(pr) else ctypes.c_void_p(0),
                          n_perm, int(seed) & ((1 << 64) - 1), int(max_pool))
        one = [np.zeros(n_rows, dtype=np.int64) for _ in range(5)]
        shift = np.zeros((n_rows, nq), dtype=np.int64)
        ge_ks, ge_u = np.full(n_rows, -1, dtype=np.int64), np.full(n_rows, -1, dtype=np.int64)   # (not written with permutations=0)
        ge_q = np.full((n_rows, nq), -1, dtype=np.int64)
        summary = np.zeros(4, dtype=np.int64)
        out = _ffi.CohortComparison(*([_vp(x) for x in one] + [_vp(shift) if shift.size else None, _vp(ge_ks), _vp(ge_u), _vp(ge_q) if ge_q.size else None]))
        self._check(call(self._h, ctypes.byref(q), ctypes.byref(out), _vp(summary)))
        return CohortComparison(one[0], one[1], one[2], one[3], one[4], shift, ge_ks, ge_u, ge_q, summary, pa, pr, G, n_perm)

    def compare_timing(self):
        """The last compare_cohorts() on the device (HIP events, ms): ranks, pool and observed statistics; the permutation walk."""
        ms = np.zeros(35, dtype=np.float64)
        self._check(self._lib.tw_get_timing(self._h, _vp(ms), 35))
        return dict(zip(("observed", "permutations"), ms[33:35].tolist()))

    # ---- the history: distributions kept across batches (tw_history_*, csrc/tw_hist.h) ----
    def history_reset(self):
        """Empties the history (tw_history_reset): no cohorts, the number of groups open again."""
        self._check(self._lib.tw_history_reset(self._h))

    def history_push(self, cohort_map=None):
        """Merges the sorted items of the last attribute() -- those distributions() returns -- into the history on the device
        (tw_history_push): the batch's cohort c goes to history cohort cohort_map[c] (-1 = not kept, None = the identity; the
        entries >= 0 distinct).  The history survives loads, new row maps, stitches and passes; only history_reset() and close()
        end it.  Returns summary4: items added, items held, cohorts of the history, pushes and merges since the reset."""
        summary = np.zeros(4, dtype=np.int64)
        if cohort_map is None:
            n_map, m = int(getattr(self, "_n_cohorts", 1)), None
        else:
            m = np.ascontiguousarray(cohort_map, dtype=np.int32).ravel()
            n_map = len(m)
        self._check(self._lib.tw_history_push(self._h, n_map, _vp(m) if m is not None and len(m) else None, _vp(summary)))
        return summary

    def history_merge(self, source, cohort_map=None):
        """The same from the host (tw_history_merge): `source` is a traces.LatencyDistributions (another engine's, or a history
        read back) or a tuple (n_cohorts, n_groups, seg_off, values) as traces.read_history_npz returns.  Every segment must
        ascend (checked on the device before anything is merged)."""
        if hasattr(source, "seg_off"):
            source = (source.n_cohorts, source.n_groups, source.seg_off, source.values)
        C, G = int(source[0]), int(source[1])
        off = np.ascontiguousarray(source[2], dtype=np.int64).ravel()
        values = np.ascontiguousarray(source[3], dtype=np.int64).ravel()
        if C < 1 or G < 1 or len(off) != C * (3 * G + 1) + 1 or (len(off) and len(values) != int(off[-1])):
            raise ValueError("history_merge: seg_off and values do not match n_cohorts * (3 * n_groups + 1) segments")
        m = None if cohort_map is None else np.ascontiguousarray(cohort_map, dtype=np.int32).ravel()
        if m is not None and len(m) != C:
            raise ValueError("history_merge: cohort_map does not match the source's cohorts")
        summary = np.zeros(4, dtype=np.int64)
        self._check(self._lib.tw_history_merge(self._h, C, G, _vp(off), _vp(values) if len(values) else None, _vp(m) if m is not None else None, _vp(summary)))
        return summary

    def history_info(self):
        """tw_history_info: cohorts, groups, segments, items, pushes (and merges) since the reset, capacity in items; all 0 for an
        empty history."""
        out = np.zeros(6, dtype=np.int64)
        self._check(self._lib.tw_history_info(self._h, _vp(out)))
        return dict(zip(("cohorts", "groups", "segments", "items", "pushes", "capacity"), out.tolist()))

    def history_distributions(self, probs=(0.5, 0.9, 0.95, 0.99), edges=None, values=True):
        """distributions() over the history (tw_history_distributions): per history cohort, metric and group the sorted values of
        everything pushed so far, counts, sums, quantiles and a histogram.  With probs=() and no edges it reads the history back.
        Returns traces.LatencyDistributions (tree_cohort empty; summary = items, non-empty segments, cohorts, pushes)."""
        from .traces import LatencyDistributions

        info = self.history_info()
        C, G, n_seg = info["cohorts"], info["groups"], info["segments"]
        pr = np.ascontiguousarray(probs, dtype=np.float64).ravel()
        ed = np.ascontiguousarray(() if edges is None else edges, dtype=np.int64).ravel()
        q = _ffi.DistQuery(len(pr), _vp(pr) if len(pr) else ctypes.c_void_p(0), len(ed), _vp(ed) if len(ed) else ctypes.c_void_p(0))
        nq, bins = min(len(pr), _ffi.TW_DIST_MAX_Q), min(len(ed), _ffi.TW_DIST_MAX_EDGES) + 1
        seg_count, seg_sum = np.zeros(n_seg, dtype=np.int64), np.zeros(n_seg, dtype=np.int64)
        seg_off = np.zeros(n_seg + 1, dtype=np.int64)
        quantile = np.zeros((n_seg, nq), dtype=np.int64)
        hist = np.zeros((n_seg, bins), dtype=np.int64)
        held = np.empty(info["items"] if values else 0, dtype=np.int64)
        summary = np.zeros(4, dtype=np.int64)
        out = _ffi.Distributions(None, _vp(seg_count) if n_seg else None, _vp(seg_sum) if n_seg else None, _vp(seg_off), _vp(held) if len(held) else None,
                                 _vp(quantile) if quantile.size else None, _vp(hist) if hist.size else None)
        self._check(self._lib.tw_history_distributions(self._h, ctypes.byref(q), ctypes.byref(out), _vp(summary)))
        return LatencyDistributions(np.zeros(0, dtype=np.int32), seg_count, seg_sum, seg_off, held, quantile, hist, summary, C, G, pr, ed)

    def history_compare(self, pairs=((0, 1),), probs=(0.5, 0.95, 0.99), permutations=0, seed=0, max_pool=0):
        """compare_cohorts() over the history (tw_history_compare): pairs of history cohorts -- batch against batch.  Returns
        traces.CohortComparison."""
        return self._compare(self._lib.tw_history_compare, self.history_info()["groups"], pairs, probs, permutations, seed, max_pool)

    def history_timing(self):
        """The history on the device (HIP events, ms): plan and merge of the last history_push() / history_merge(); quantiles
        and histogram of the last history_distributions(); observed statistics and permutation walk of the last history_compare()."""
        ms = np.zeros(43, dtype=np.float64)
        self._check(self._lib.tw_get_timing(self._h, _vp(ms), 43))
        return dict(zip(("plan", "merge", "quantiles", "observed", "permutations"), ms[38:43].tolist()))

    def signatures(self, mode="levels", need_flags=1, skip_flags=0, keep_reference=False, compare=False):
        """The trees of the last stitch() grouped by call-graph signature (tw_trace_signatures): per eligible tree (flags hold
        need_flags, none of skip_flags; default: whole traces, those with an unassigned call included) the run-length encoded,
        sorted list of its (level, caller group, group) items -- mode "levels": the caller group left out, the reference's
        signature; "edges": with it --, the classes of equal signatures numbered by their first tree, and per class its trees,
        latency sum / min / max and entries.  keep_reference stores the signatures on the device, keyed by root row;
        compare=True sets tree_same against that set.  Needs set_row_groups.  Returns traces.TraceSignatures."""
        from .traces import SIGNATURE_MODES, TraceSignatures

        m = SIGNATURE_MODES.index(mode) if isinstance(mode, str) else int(mode)
        n, nt = int(getattr(self, "_n_rows", 0)), max(int(getattr(self, "_n_trees", 0)), 1)
        q = _ffi.SigQuery(m, int(need_flags), int(skip_flags), 1 if keep_reference else 0, 1 if compare else 0)
        level, tree_class, rep = (np.empty(k, dtype=np.int32) for k in (max(n, 1), nt, nt))
        items, trees, lsum, lmin, lmax = (np.empty(nt, dtype=np.int64) for _ in range(5))
        same = np.empty(nt, dtype=np.uint8)
        off = np.empty(nt + 1, dtype=np.int64)
        summary = np.zeros(6, dtype=np.int64)
        out = _ffi.Signatures(*[_vp(a) for a in (level, tree_class, items, same, rep, trees, lsum, lmin, lmax, off)] + [None])
        self._check(self._lib.tw_trace_signatures(self._h, ctypes.byref(q), ctypes.byref(out), _vp(summary)))
        entries = np.empty((int(summary[3]), 4), dtype=np.int32)   # the result is resident: the second call only copies the entries
        if len(entries):
            only = _ffi.Signatures(*([None] * 10 + [_vp(entries)]))
            self._check(self._lib.tw_trace_signatures(self._h, ctypes.byref(q), ctypes.byref(only), None))
        k, c = int(self._n_trees), int(summary[1])
        self._sig_resident = (m, off[:c + 1].copy(), entries)         # what class_profiles() sizes and labels its result by
        return TraceSignatures(level[:n].copy(), tree_class[:k].copy(), items[:k].copy(), same[:k].copy(), rep[:c].copy(), trees[:c].copy(),
                               lsum[:c].copy(), lmin[:c].copy(), lmax[:c].copy(), off[:c + 1].copy(), entries, summary, m, self._tree_root)

    def signatures_timing(self):
        """The last signatures() that ran kernels on the device (HIP events, ms): items and levels; sort, run lengths and hash;
        classes, comparison and per-class reduction."""
        ms = np.zeros(28, dtype=np.float64)
        self._check(self._lib.tw_get_timing(self._h, _vp(ms), 28))
        return dict(zip(("items", "sort", "classes"), ms[25:28].tolist()))

    def class_profiles(self):
        """The aggregate trace of every call-graph class (tw_class_profiles): per entry of the last signatures() the rows, durations,
        self and critical-path times and start offsets over the trees of the class that the last attribute() selected, and per
        class the counted trees, their latency, the path time and the entry that holds most of it.  Takes no query: it joins the
        resident signature result with the resident attribution (both on the forest of the last stitch()).  Returns
        traces.ClassProfiles."""
        from .traces import ClassProfiles

        mode, off, entries = getattr(self, "_sig_resident", (0, np.zeros(1, dtype=np.int64), np.zeros((0, 4), dtype=np.int32)))
        nc, ne = len(off) - 1, len(entries)
        cap = max(int(getattr(self, "_n_rows", 0)), ne, nc, 1)        # (entries and classes never outnumber the rows)
        arrays = [np.empty(cap, dtype=np.int64) for _ in range(13)]
        summary = np.zeros(6, dtype=np.int64)
        out = _ffi.ClassProfile(*[_vp(a) for a in arrays])
        self._check(self._lib.tw_class_profiles(self._h, ctypes.byref(out), _vp(summary)))
        return ClassProfiles(*([a[:ne].copy() for a in arrays[:9]] + [a[:nc].copy() for a in arrays[9:]] + [summary]),
                             class_off=off, class_entries=entries, mode=mode)

    def profiles_timing(self):
        """The last class_profiles() that ran kernels on the device (HIP events, ms): the sweep over the rows; the per-tree and
        per-class pass; the copies."""
        ms = np.zeros(31, dtype=np.float64)
        self._check(self._lib.tw_get_timing(self._h, _vp(ms), 31))
        return dict(zip(("sweep", "classes", "copies"), ms[28:31].tolist()))

    def filter_traces(self, clauses=(), need_flags=1, skip_flags=0):
        """Selects the trees of the last stitch() by a predicate, on the device (tw_filter_traces): `clauses` are traces.clause(...)
        tuples (or what traces.parse_filter returns), clauses of one term ANDed, the terms ORed; an eligible tree (flags hold
        need_flags, none of skip_flags) matches when some term holds, every eligible tree with no clause at all.  The match becomes
        bit traces.MATCH of the forest's flags on the device: attribute(need_flags=WHOLE | MATCH), signatures(need_flags=WHOLE |
        MATCH) and what follows them then work on the matched traces.  Clauses on self / path time need the last attribute(), a
        class clause the last signatures().  Returns traces.TraceFilter."""
        from .traces import TraceFilter

        clauses = [tuple(int(x) for x in c) for c in clauses]
        nt, nc = max(int(getattr(self, "_n_trees", 0)), 1), len(clauses)
        table = (_ffi.FilterClause * max(nc, 1))(*[_ffi.FilterClause(*c) for c in clauses])
        q = _ffi.FilterQuery(int(need_flags), int(skip_flags), nc, table)
        match = np.zeros(nt, dtype=np.uint8)
        listed = np.empty(nt, dtype=np.int32)
        value = np.empty((nt, nc), dtype=np.int64)
        clause_trees, term_trees, summary = np.zeros(nc, dtype=np.int64), np.zeros(_ffi.TW_FILT_MAX_TERMS, dtype=np.int64), np.zeros(6, dtype=np.int64)
        out = _ffi.FilterResult(*[_vp(a) for a in (match, listed, value, clause_trees, term_trees)])
        self._check(self._lib.tw_filter_traces(self._h, ctypes.byref(q), ctypes.byref(out), _vp(summary)))
        k = int(getattr(self, "_n_trees", 0))
        return TraceFilter(match[:k].copy(), listed[:int(summary[1])].copy(), value[:k].copy(), clause_trees, term_trees, summary, clauses)

    def filter_timing(self):
        """The last filter_traces() on the device (HIP events, ms): the tree kernel (rows, clauses, terms, the bit); the list of the
        matched trees; the copies."""
        ms = np.zeros(49, dtype=np.float64)
        self._check(self._lib.tw_get_timing(self._h, _vp(ms), 49))
        return dict(zip(("trees", "list", "copies"), ms[46:49].tolist()))

    def extract_traces(self, mode="top", order="slowest", limit=0, probs=(), trees=None, need_flags=1, skip_flags=0):
        """Hands out trees of the last stitch() as a packed sub-forest, built on the device (tw_extract_traces, tw_get_extracted): every
        selected tree in pre-order with local parent indices.  mode "top": the eligible trees (flags hold need_flags, none of
        skip_flags -- the device's flags, so traces.CONFIDENT and traces.MATCH can be named) in the order "tree" / "slowest" /
        "fastest", the first `limit` of them (0: all); "quantiles": the trees at `probs` of the eligible trees' latency, the exemplars;
        "list": the trees `trees` names (match_trees of a filter), in that order, flags not applied.  The self / path times of the last
        attribute() and the row groups are gathered where resident.  Returns traces.ExtractedTraces."""
        from .traces import EXTRACT_MODES, EXTRACT_ORDERS, ExtractedTraces, _extract_code

        probs = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        listed = np.ascontiguousarray([] if trees is None else trees, dtype=np.int32).reshape(-1)
        q = _ffi.ExtractQuery(int(need_flags), int(skip_flags), _extract_code(EXTRACT_MODES, mode, "mode"), _extract_code(EXTRACT_ORDERS, order, "order"),
                              int(limit), len(probs), len(listed), probs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                              listed.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        summary = np.zeros(6, dtype=np.int64)
        self._check(self._lib.tw_extract_traces(self._h, ctypes.byref(q), _vp(summary)))
        n_sel, n_rows, times = int(summary[1]), int(summary[2]), bool(summary[5])
        cols = {}
        for k in ExtractedTraces.FIELDS[:-1]:
            n = n_sel + 1 if k == "out_off" else n_sel if k in ExtractedTraces.TREE_FIELDS else n_rows if times or k not in ("self_time", "path_time") else 0
            cols[k] = np.zeros(n, dtype=ExtractedTraces.DTYPES.get(k, np.int64))
        out = _ffi.Extracted(*[_vp(cols[k]) if len(cols[k]) or k == "out_off" else None for k in ExtractedTraces.FIELDS[:-1]])
        self._check(self._lib.tw_get_extracted(self._h, ctypes.byref(out)))
        return ExtractedTraces(summary, **cols)

    def extract_timing(self):
        """The last extract_traces() on the device (HIP events, ms): selection, sizes and offsets; the tree kernel; the copies."""
        ms = np.zeros(52, dtype=np.float64)
        self._check(self._lib.tw_get_timing(self._h, _vp(ms), 52))
        return dict(zip(("select", "trees", "copies"), ms[49:52].tolist()))

    # ---- the class catalogue: call-graph classes kept across batches (tw_class_history_*, csrc/tw_chist.h) ----
    def class_history_reset(self):
        """Empties the class catalogue (tw_class_history_reset): no classes, mode and number of groups open again."""
        self._check(self._lib.tw_class_history_reset(self._h))

    def class_history_push(self, what=3, epoch=0):
        """Adds the classes of the last signatures() -- and, with what & 2, the figures of the last class_profiles() -- to the
        catalogue on the device (tw_class_history_push): a class whose signature the catalogue holds keeps that class' id, the
        others are appended in the batch's order.  what: 1 the signature result's trees and latencies, 2 the profile's figures
        only, 3 both -- which falls back to 1 when no profile is resident.  epoch: a label of the caller's, kept as first / last
        epoch per class.  The catalogue survives loads, new row maps, stitches and passes; only class_history_reset() and
        close() end it.  Returns (class_map [the batch's classes] = catalogue ids, summary6 = new classes, classes held, new
        entries, entries held, pushes and merges since the reset, classes of the batch)."""
        off = getattr(self, "_sig_resident", (0, np.zeros(1, dtype=np.int64), None))[1]
        class_map = np.full(max(len(off) - 1, 1), -1, dtype=np.int32)
        summary = np.zeros(6, dtype=np.int64)
        rc = self._lib.tw_class_history_push(self._h, int(what), int(epoch), _vp(class_map), _vp(summary))
        if rc == -4 and int(what) == 3 and b"what & 2" in self._lib.tw_last_error(self._h):   # the default without a resident profile
            rc = self._lib.tw_class_history_push(self._h, 1, int(epoch), _vp(class_map), _vp(summary))
        self._check(rc)
        return class_map[:int(summary[5])].copy(), summary

    def class_history_match(self):
        """The catalogue ids of the classes of the last signatures(), -1 for a class the catalogue does not hold
        (tw_class_history_match); changes nothing.  With TraceSignatures.tree_class it names the traces of a shape never seen."""
        off = getattr(self, "_sig_resident", (0, np.zeros(1, dtype=np.int64), None))[1]
        class_map = np.full(max(len(off) - 1, 1), -1, dtype=np.int32)
        summary = np.zeros(6, dtype=np.int64)
        self._check(self._lib.tw_class_history_match(self._h, _vp(class_map), _vp(summary)))
        return class_map[:int(summary[5])].copy()

    def class_history_merge(self, source, epoch=0):
        """A push from the host (tw_class_history_merge).  source: a traces.ClassHistory -- a catalogue read back, another
        engine's, one of traces.read_class_history_npz, or ClassHistory.from_batch(signatures, profiles or None, n_groups) of
        another engine's batch.  Figures that are None add nothing.  The source's entries are checked on the device before
        anything changes.  Returns (class_map, summary6) as class_history_push()."""
        from .traces import ClassHistory

        src = source
        nc, ne = src.n_classes, src.n_entries
        off = np.ascontiguousarray(src.class_off, dtype=np.int64).ravel()
        entries = np.ascontiguousarray(src.class_entries, dtype=np.int32).reshape(-1, 4)
        if len(off) != nc + 1:
            raise ValueError("class_history_merge: class_off does not match the source's classes")
        figures = []
        for k, n in [(k, nc) for k in ClassHistory.CLASS_FIELDS] + [(k, ne) for k in ClassHistory.ENTRY_FIELDS]:
            a = getattr(src, k)
            a = None if a is None else np.ascontiguousarray(a, dtype=np.int64).ravel()
            if a is not None and len(a) != n:
                raise ValueError("class_history_merge: %s does not match the source's classes and entries" % k)
            figures.append(a)
        ptr = lambda a: None if a is None or a.size == 0 else _vp(a)                    # noqa: E731
        cat = _ffi.ClassCatalogue(nc, len(entries), int(src.mode), int(src.n_groups), _vp(off), ptr(entries), *([ptr(a) for a in figures] + [None, None]))
        class_map = np.full(max(nc, 1), -1, dtype=np.int32)
        summary = np.zeros(6, dtype=np.int64)
        self._check(self._lib.tw_class_history_merge(self._h, ctypes.byref(cat), int(epoch), _vp(class_map), _vp(summary)))
        return class_map[:nc].copy(), summary

    def class_history_info(self):
        """tw_class_history_info: classes, entries, pushes (and merges) since the reset, mode, groups, capacity of the hash table
        in slots; all 0 for an empty catalogue."""
        out = np.zeros(6, dtype=np.int64)
        self._check(self._lib.tw_class_history_info(self._h, _vp(out)))
        return dict(zip(("classes", "entries", "pushes", "mode", "groups", "capacity"), out.tolist()))

    def class_history(self):
        """The catalogue read back (tw_class_history_get: a call for the sizes, a call that copies).  Returns traces.ClassHistory."""
        from .traces import ClassHistory

        sizes = np.zeros(6, dtype=np.int64)
        self._check(self._lib.tw_class_history_get(self._h, None, _vp(sizes)))
        nc, ne = int(sizes[0]), int(sizes[1])
        off = np.zeros(nc + 1, dtype=np.int64)
        entries = np.zeros((ne, 4), dtype=np.int32)
        per_class = [np.zeros(nc, dtype=np.int64) for _ in ClassHistory.CLASS_FIELDS]
        per_entry = [np.zeros(ne, dtype=np.int64) for _ in ClassHistory.ENTRY_FIELDS]
        derived = [np.zeros(nc, dtype=np.int64) for _ in range(2)]
        cat = _ffi.ClassCatalogue(0, 0, 0, 0, *[_vp(a) if a.size else None for a in [off, entries] + per_class + per_entry + derived])
        self._check(self._lib.tw_class_history_get(self._h, ctypes.byref(cat), None))
        return ClassHistory(off, entries, *(per_class + per_entry + derived), mode=int(sizes[3]), n_groups=int(sizes[4]))

    def class_history_timing(self):
        """The last class_history_push() / class_history_merge() on the device (HIP events, ms): hash and lookup; scan, append,
        insert and any rehash; accumulate."""
        ms = np.zeros(46, dtype=np.float64)
        self._check(self._lib.tw_get_timing(self._h, _vp(ms), 46))
        return dict(zip(("lookup", "insert", "accumulate"), ms[43:46].tolist()))

    # ------------------------------------------------------------------------------------------
    def baseline(self, kind):
        """The reference's FCFS ("FCFS", algorithms/fcfs.py) or vPath ("vPath", algorithms/vpath.py; needs set_truth) on the
        resident table (tw_run_baseline).  Per unit parent [E, n_in] int32, -1 = ("NA", "NA")."""
        code = {"FCFS": 4, "vPath": 7}[kind]
        par = np.empty(int(self._ie_off[-1]), dtype=np.int32)
        self._check(self._lib.tw_run_baseline(self._h, code, _vp(par)))
        return [par[int(self._ie_off[k]):int(self._ie_off[k + 1])].reshape(u.E, u.n_in) for k, u in enumerate(self.units)]

    def wap5(self, ep_names, state=None):
        """The reference's WAP5 (algorithms/wap5.py:257-351) on the resident table: tw_wap5_delays -> the delay samples
        added up per callee name in service order (the reference keeps one predictor object for a run; `state` = the dict
        {name: [sum in microseconds, count]} carried from batch to batch) -> tw_wap5_parents.  ep_names: per unit the
        endpoint names in the unit's endpoint order.  Returns (per unit parent [E, n_in]: -1 none, -2 several calls for one
        request -- counted as wrong like the reference does --, state, per unit options[e][i] = the calls given to request i,
        the reference's list-valued assignment)."""
        from fractions import Fraction

        state = {} if state is None else state
        nu = len(self.units)
        sums = np.zeros((nu, _ffi.TW_MAX_EP), dtype=np.int64)
        cnts = np.zeros((nu, _ffi.TW_MAX_EP), dtype=np.int32)
        self._check(self._lib.tw_wap5_delays(self._h, _vp(sums), _vp(cnts), None))
        mean = np.zeros((nu, _ffi.TW_MAX_EP), dtype=np.float64)
        for k, u in enumerate(self.units):
            scale = Fraction(1) if u.time_scale is None else Fraction(u.time_scale)
            for e in np.argsort(u.key_rank, kind="stable"):   # for out_ep in out_span_partitions.keys()
                st = state.setdefault(ep_names[k][int(e)], [Fraction(0), 0])
                st[0] += int(sums[k, e]) * scale
                st[1] += int(cnts[k, e])
                if st[1] == 0:
                    raise ValueError("WAP5: no delay sample for endpoint %r (statistics.mean of an empty list raises in the reference)" % ep_names[k][int(e)])
                mean[k, e] = float(st[0] / st[1])               # statistics.mean: exact, rounded once
        par = np.empty(int(self._ie_off[-1]), dtype=np.int32)
        req = np.empty(int(sum(int(u.out_off[-1]) for u in self.units)), dtype=np.int32)
        self._check(self._lib.tw_wap5_parents(self._h, _vp(mean), _vp(par), _vp(req)))
        options, o = [], 0
        for u in self.units:
            per = []
            for e in range(u.E):
                m = int(u.out_off[e + 1] - u.out_off[e])
                lists = [[] for _ in range(u.n_in)]
                for x in np.flatnonzero(req[o:o + m] >= 0):
                    lists[int(req[o + x])].append(int(x))
                per.append(lists)
                o += m
            options.append(per)
        return [par[int(self._ie_off[k]):int(self._ie_off[k + 1])].reshape(u.E, u.n_in) for k, u in enumerate(self.units)], state, options

    def find_order(self, units, true_parent):
        """executor.py:214-285 (FindOrder) on the device for units that need not be loaded (endpoints in any
        order): per unit the uint8 [E, E] call-order relation implied by the true assignments."""
        units = list(units)
        in_off = np.zeros(len(units) + 1, dtype=np.int64)
        np.cumsum([u.n_in for u in units], out=in_off[1:])
        unit_E = np.array([u.E for u in units], dtype=np.int32)
        ep_off, base = [0], 0
        for u in units:
            ep_off.extend((base + u.out_off[1:]).tolist())
            base += int(u.out_off[-1])
        ep_off = np.array(ep_off, dtype=np.int64)
        os_ = np.ascontiguousarray(np.concatenate([u.out_start for u in units]))
        oe_ = np.ascontiguousarray(np.concatenate([u.out_end for u in units]))
        t = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.int32).ravel() for a in true_parent]), dtype=np.int32)
        dag = np.zeros(int(sum(int(e) * int(e) for e in unit_E)), dtype=np.uint8)
        self._check(self._lib.tw_find_order(self._h, len(units), _vp(in_off), _vp(unit_E), _vp(ep_off), _vp(os_), _vp(oe_), _vp(t), _vp(dag)))
        out, p = [], 0
        for e in unit_E:
            out.append(dag[p:p + int(e) * int(e)].reshape(int(e), int(e)).copy())
            p += int(e) * int(e)
        return out

    # ------------------------------------------------------------------------------------------
    # the call-order DAG without ground truth (csrc/tw_order.h; the search itself: traceweaver_amd/order.py)
    @staticmethod
    def _soa(units):
        """The descriptor and span arrays of tw_batch for a list of units (their dag / key_rank left out)."""
        in_off = np.zeros(len(units) + 1, dtype=np.int64)
        np.cumsum([u.n_in for u in units], out=in_off[1:])
        unit_E = np.array([u.E for u in units], dtype=np.int32)
        ep_off, base = [0], 0
        for u in units:
            ep_off.extend((base + u.out_off[1:]).tolist())
            base += int(u.out_off[-1])
        cat = lambda name: np.ascontiguousarray(np.concatenate([getattr(u, name) for u in units]), dtype=np.int64)
        return in_off, unit_E, np.array(ep_off, dtype=np.int64), cat("in_start"), cat("in_end"), cat("out_start"), cat("out_end")

    def order_bound(self, units):
        """tw_order_bound for units that need not be loaded, endpoints in partition-key order: per unit the int64 [E, E] table
        viol[a, b] = requests in which no call to a that lies inside the request ends before (or when) some call to b inside
        it starts.  viol[a, b] > 0 proves that a solve under any graph with the edge a -> b leaves a request unassigned."""
        units = list(units)
        in_off, unit_E, ep_off, i_s, i_e, o_s, o_e = self._soa(units)
        viol = np.zeros(int(sum(int(e) * int(e) for e in unit_E)), dtype=np.int64)
        self._check(self._lib.tw_order_bound(self._h, len(units), _vp(in_off), _vp(unit_E), _vp(ep_off), _vp(i_s), _vp(i_e), _vp(o_s), _vp(o_e), _vp(viol)))
        out, p = [], 0
        for e in unit_E:
            out.append(viol[p:p + int(e) * int(e)].reshape(int(e), int(e)).copy())
            p += int(e) * int(e)
        return out

    def order_bound_ms(self):
        """The last order_bound's kernel on the device (HIP events, ms)."""
        ms = np.zeros(32, dtype=np.float64)
        self._check(self._lib.tw_get_timing(self._h, _vp(ms), 32))
        return float(ms[31])

    def order_stage(self, units, batch_size=100, batch_size_mis=30, skip=None):
        """Upload the span table of a no-skip batch once, endpoints in partition-key order (the units' dag / key_rank are not
        read), for order_load (tw_order_stage).  Skip-mode batches (`skip`, or an endpoint short of spans), load-scaled units
        and parts of a split service are refused (TW_ERR_UNSUPPORTED)."""
        units = list(units)
        in_off, unit_E, ep_off, i_s, i_e, o_s, o_e = self._soa(units)
        scaled = [u.time_scale is not None for u in units]
        ts = np.array([u.time_scale if s else 1.0 for u, s in zip(units, scaled)], dtype=np.float64) if any(scaled) else None
        part = np.array([u.part for u in units], dtype=np.uint8) if any(u.part for u in units) else None
        skip_arr = (_ffi.SkipUnit * len(units))() if skip is not None else None
        b = _ffi.Batch(len(units), _vp(in_off), _vp(unit_E), _vp(ep_off), None, None, _vp(i_s), _vp(i_e), _vp(o_s), _vp(o_e),
                       batch_size, batch_size_mis, _ffi.TW_TOPK, _vp(ts),
                       ctypes.cast(skip_arr, ctypes.c_void_p) if skip_arr is not None else ctypes.c_void_p(0), _vp(part))
        self._check(self._lib.tw_order_stage(self._h, ctypes.byref(b)))
        self._staged = units
        self._stage_sizes = (int(batch_size), int(batch_size_mis))

    def order_load(self, active, dags):
        """Load the staged units `active` (ascending indices into the staged batch) under the candidate graphs `dags` (per
        listed unit uint8 [E, E] in key order, dag[a, b] = 1 <=> a -> b): the topological order on the host, the endpoint
        segments gathered into it on the device, then the usual load (tw_order_load).  Afterwards the engine -- and self.units,
        the permuted units with dag and key_rank in that order -- is as after load() of those units."""
        from .order import permuted_unit

        active = np.ascontiguousarray(active, dtype=np.int32)
        staged = getattr(self, "_staged", None)
        if staged is None:
            raise EngineError(-4, "order_load before order_stage")
        if len(dags) != len(active):
            raise ValueError("one candidate graph per listed unit")
        flat = np.ascontiguousarray(np.concatenate([np.asarray(d, dtype=np.uint8).ravel() for d in dags]), dtype=np.uint8)
        if any(k < 0 or k >= len(staged) for k in active.tolist()) or len(flat) != sum(staged[k].E ** 2 for k in active.tolist()):
            raise ValueError("candidate graphs do not match the staged units")
        self._check(self._lib.tw_order_load(self._h, len(active), _vp(active), _vp(flat)))
        units = [permuted_unit(staged[k], d, lazy=True) for k, d in zip(active.tolist(), dags)]
        self.units = units
        self.skip_mode = False
        self._keep = None
        self._n_cohorts = 1
        self._last_pass, self._n_rows = 0, 0
        batch_size = self._stage_sizes[0]
        self._in_off = np.concatenate([[0], np.cumsum([u.n_in for u in units])]).astype(np.int64)
        self._ie_off = np.concatenate([[0], np.cumsum([u.n_in * u.E for u in units])]).astype(np.int64)
        self._slot_off = np.concatenate([[0], np.cumsum([u.nslot for u in units])]).astype(np.int64)
        self._gap_off = np.concatenate([[0], np.cumsum([u.nslot * u.n_in for u in units])]).astype(np.int64)
        self._nblk = [(u.n_in + batch_size - 1) // batch_size for u in units]
        self._gp_off = np.concatenate([[0], np.cumsum([nb * u.nslot for nb, u in zip(self._nblk, units)])]).astype(np.int64)

    def build_distributions(self, start, dur, ep, large_delay, E):
        """The sweep of BuildDistributions (traceweaver_v3.py:120-169) on the device: per span of the merged, start-ordered
        list the pair index a * (E + 1) + b its delay sample belongs to (-1 none) and the sample."""
        start = np.ascontiguousarray(start, dtype=np.int64)
        dur = np.ascontiguousarray(dur, dtype=np.int64)
        ep = np.ascontiguousarray(ep, dtype=np.uint8)
        key = np.empty(len(start), dtype=np.int32)
        val = np.empty(len(start), dtype=np.int64)
        self._check(self._lib.tw_build_distributions(self._h, len(start), _vp(start), _vp(dur), _vp(ep), int(large_delay), int(E), _vp(key), _vp(val)))
        return key, val

    def hbm_copy_gbps(self, nbytes=1 << 30, iters=10):
        """Measured HBM rate of a plain streaming copy kernel on this device (read + written GB/s)."""
        g = ctypes.c_double(0.0)
        self._check(self._lib.tw_measure_hbm_copy(self._h, int(nbytes), int(iters), ctypes.byref(g)))
        return float(g.value)

    def timing(self):
        """ms of the last pass: total, enumerate kernel, select kernel, windows, claim+detect+repair, params (HIP events); the last
        refit; repair rounds; host wall clock of submitting the first enumeration and of the whole pass call."""
        ms = np.zeros(10, dtype=np.float64)
        self._check(self._lib.tw_get_timing(self._h, _vp(ms), 10))
        return dict(zip(("pass", "enumerate", "select", "windows", "repair", "params", "fit", "rounds", "host_enum_submit", "host_pass"), ms.tolist()))

    def gated_stages(self):
        """Class stages of the last pass that were queued behind the stage gate (tw_get_timing slot 32): 0 = the pass was not gated --
        TW_STAGE_GATE=0, a batch that is not staged, or a deepest class that the general path of the tile kernel does not serve."""
        ms = np.zeros(33, dtype=np.float64)
        self._check(self._lib.tw_get_timing(self._h, _vp(ms), 33))
        return int(ms[32])

    def fit_spec(self):
        """(hits, misses) of the last refit (tw_get_timing slots 35, 36): rows whose final fit ran beside the model selection and was
        adopted -- the row selected the largest admissible count, min(5, #distinct) -- and rows that were fitted after the selection.
        (0, 0) = TW_FIT_SPEC=0, or no refit yet."""
        ms = np.zeros(37, dtype=np.float64)
        self._check(self._lib.tw_get_timing(self._h, _vp(ms), 37))
        return int(ms[35]), int(ms[36])

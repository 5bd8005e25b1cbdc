"""An E-member hybrid forecast on one rank: one reservoir context holding E members
(Reservoirs.set_members) beside E SPEEDY models, one Dynamics per member.

Every member is the hybrid loop of speedy_ml_amd.hybrid on its own (parallelmain.f90:204-270:
predict, sendrecievegrid's assembly, run_model, the re-tiling), bit for bit; what the members
share is the stream of the reservoir weights.  The split step makes that sharing pay in a
hybrid forecast: the members' update and v_ml (begin_members, about 98 % of the bytes) run on
the reservoir's CUs while the E windows run one after the other on SPEEDY's, and only the v_p
finish (finish_assemble_members: local models tiled from the E forecasts, the members' outvecs,
the E assembled grids) waits for the forecasts.

Schedule of step(), in the order of the native loop's predict and advance (sml_hybrid.hip), so
that every member is that loop:
  host         the date of step t + 1, then the tisr table's hour of step t (in that order:
               the two share the calendar's February latch), once for all members
  main stream  the slab ocean's predict on a slab step (sml_slab_predict: the E ring means,
               the slab reservoirs' step for all members, the new sst into the exchange rows)
               finish_assemble_members(f4, f2 -> lm, ov, g4, g2, pr)
               after a change of the slab sst: the E wholegrid_sst grids and the feedbacks'
               sst entries (sml_slab_sst), each grid into its member's window (set_hybrid_sst)
               tile_feedback_members into fb, the table's tisr field (tile_tisr_field_members),
               the slab ring's column (sml_slab_ring): one launch each        -> event
               begin_members(fb): the next step's update and v_ml (the states run one update
               ahead, as the pipelined HybridLoop's do; cancel_step() rolls them back)
               with set_products: the ensemble mean and spread of g4, g2, pr and the step's
               row of scores (sml_ens_moments, sml_ens_scores) behind the begin -- the grids
               are complete by then and stay as they are until the next step's finish
  side stream  waits for the event, then for e = 0 .. E - 1: dyns[e].fordate(date) with the
               calendar on, dyns[e].run_model(g4[e], g2[e] -> f4[e], f2[e]); the host waits
               for window e (its safety flag, then the stream) before it enqueues window e + 1.
That host wait is a safety rule, not a convenience: every Dynamics has a check stream whose
kernel polls in-kernel, an in-kernel wait holds its hardware queue, and
the E contexts' streams share the process's few queues -- so no window is enqueued while
another context's window or check is outstanding.

EnsembleProducts is that reduction over the members on its own.

The slab ocean (`slab=`), run_model's calendar (set_calendar) and get_tisr_by_date
(set_tisr_table) are HybridLoop's, with the same refusals.

Out of scope here: more than one rank (world > 1: `res` holds every region in global order),
concurrent windows, and a native (sml_hybrid_*) form of this loop.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from ._lib import SmlError, check, lib, ptr
from .dynamics import ALPH, DELT
from .hybrid import slab_state_copy


def _member_stride(a, shape, what):
    """The member stride in doubles of a members' device array [E, *shape] whose members
    are packed."""
    if a.dtype != torch.float64 or not a.is_cuda or tuple(a.shape[1:]) != shape or not a[0].is_contiguous():
        raise ValueError(f"{what}: a float64 device tensor [E, {', '.join(map(str, shape))}] with packed members expected")
    return int(a.stride(0)) if a.shape[0] > 1 else int(np.prod(shape))


class EnsembleProducts:
    """What an E-member forecast is run for (sml_ens_*, include/speedy_ml.h): the per-point
    ensemble mean and spread of the members' grids g4 [E, 8, 48, 96, 4], g2 [E, 48, 96],
    pr [E, 48, 96] or None, and per step a row of area-weighted scores of each of the 34
    fields (4 k + v: level k, variable v; 32 logp; 33 precip) against a verifying analysis:
    scores [capacity, 34, 4] = rmse of the mean, spread, fair CRPS, bias, and the rank
    histogram ranks [capacity, 34, 33].  The tables live on the device; read() copies rows
    to the host.  Calls on one object are to be made in stream order."""

    RMSE, SPREAD, CRPS, BIAS = 0, 1, 2, 3

    def __init__(self, members: int, capacity: int, device):
        self.dev = torch.device(device)
        self._h = None
        h = ctypes.c_void_p()
        with torch.cuda.device(self.dev):
            check(lib().sml_ens_create(int(members), int(capacity), ctypes.byref(h)))
        self._h = h
        self.members, self.capacity = int(members), int(capacity)
        n = [ctypes.c_int() for _ in range(3)]
        check(lib().sml_ens_info(h, None, None, *[ctypes.byref(x) for x in n]))
        self.fields, self.nscores, self.rank_bins = (x.value for x in n)

    def _inputs(self, g4, g2, pr):
        if g4.shape[0] != self.members or g2.shape[0] != self.members or (pr is not None and pr.shape[0] != self.members):
            raise ValueError(f"{self.members} members expected")
        s4, s2 = _member_stride(g4, (8, 48, 96, 4), "g4"), _member_stride(g2, (48, 96), "g2")
        if pr is not None and _member_stride(pr, (48, 96), "pr") != s2:
            raise ValueError("pr: the member stride of g2 expected")
        return ptr(g4), s4, ptr(g2), ptr(pr), s2

    def moments(self, g4, g2, pr=None, mean=True, spread=True, out=None, stream=None):
        """(mean4, mean2, meanpr, spread4, spread2, spreadpr) in the single-member layouts;
        None where not asked for (mean / spread off, pr None).  `out`: such a tuple of
        tensors to write into instead of new ones."""
        a = self._inputs(g4, g2, pr)
        if out is None:
            z = lambda on, *s: torch.empty(s, dtype=torch.float64, device=self.dev) if on else None  # noqa: E731
            out = (z(mean, 8, 48, 96, 4), z(mean, 48, 96), z(mean and pr is not None, 48, 96),
                   z(spread, 8, 48, 96, 4), z(spread, 48, 96), z(spread and pr is not None, 48, 96))
        s = stream if stream is not None else torch.cuda.current_stream(self.dev)
        check(lib().sml_ens_moments(self._h, *a, *[ptr(o) for o in out], ctypes.c_void_p(s.cuda_stream)))
        return out

    def scores(self, g4, g2, pr, truth, t: int, stream=None):
        """Row t of the tables.  truth: None (only the row's spread is written), or
        (truth4 [8, 48, 96, 4], truth2 [48, 96], truthpr [48, 96] or None)."""
        a = self._inputs(g4, g2, pr)
        t4, t2, tp = truth if truth is not None else (None, None, None)
        for x, shape in ((t4, (8, 48, 96, 4)), (t2, (48, 96)), (tp, (48, 96))):
            if x is not None and (x.dtype != torch.float64 or not x.is_cuda or tuple(x.shape) != shape
                                  or not x.is_contiguous()):
                raise ValueError(f"truth: contiguous float64 device tensors expected, one of them {shape}")
        s = stream if stream is not None else torch.cuda.current_stream(self.dev)
        check(lib().sml_ens_scores(self._h, *a, ptr(t4), ptr(t2), ptr(tp), int(t), ctypes.c_void_p(s.cuda_stream)))

    def reset(self, stream=None):
        """Quiet NaN into every score, 0 into every rank bin."""
        s = stream if stream is not None else torch.cuda.current_stream(self.dev)
        check(lib().sml_ens_reset(self._h, ctypes.c_void_p(s.cuda_stream)))

    def read(self, t0: int = 0, count: int | None = None):
        """Host rows (scores [count, 34, 4], ranks [count, 34, 33]); waits for the device."""
        if count is None:
            count = self.capacity - t0
        sc = np.empty((max(count, 0), self.fields, self.nscores))
        rk = np.empty((max(count, 0), self.fields, self.rank_bins), dtype=np.int32)
        check(lib().sml_ens_read(self._h, int(t0), int(count), ptr(sc), ptr(rk)))
        return sc, rk

    @staticmethod
    def weights():
        """The weight of one point of each of the 48 rows; 96 * sum = 1."""
        w = np.empty(48)
        check(lib().sml_ens_weights(ptr(w)))
        return w

    def close(self):
        if getattr(self, "_h", None):
            check(lib().sml_ens_destroy(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EnsembleLoop:
    """res: Reservoirs holding every region in global order with set_members(len(dyns))
    done; dyns: one Dynamics per member, each with its own state, forcing and physics;
    tisr: [nlocal, 16] standardized tisr inputs (device) or None; slab: None, or a SlabOcean
    (speedy_ml_amd.hybrid) whose `res` has set_members(len(dyns)) done -- the exchange rows
    then carry each region's slab sst beside its outvec.  Owns the members' strided buffers
    fb [E, tot], lm [E, nlocal, ncs], ov [E, nlocal, exchange_width], g4 / f4
    [E, 8, 48, 96, 4], g2 / pr / f2 [E, 48, 96] and two library streams on the CU split
    HybridLoop uses: SPEEDY on CUs [0, speedy_cus), the reservoir on the rest.  As
    HybridLoop does, it moves each Dynamics' safety check to a CU-masked stream on the
    reservoir's CUs (sml_dyn_set_check_cus) and lifts the reservoir's read-wave cap; a window
    of such a Dynamics must not be run on the legacy default stream afterwards (a CU-masked
    stream synchronises with it, and the window and its in-kernel check would wait for each
    other until the check's time-out)."""

    def __init__(self, res, dyns, device, tisr=None, nleap: int = 24, delt: float = DELT,
                 speedy_cus: int | None = None, slab=None):
        self.res, self.dyns, self.tisr, self.slab = res, list(dyns), tisr, slab
        self._slab_h = None
        self.E = len(self.dyns)
        if self.E < 1 or res.members != self.E:
            raise ValueError(f"dyns: {self.E} models for a context of {res.members} members (set_members first)")
        if res.nlocal != res.numregions or list(res.region_ids) != list(range(res.numregions)):
            raise ValueError("res: every region of the decomposition, in global order, expected (world 1)")
        if slab is not None and slab.res.members != self.E:
            raise ValueError(f"slab: a context of {slab.res.members} members for {self.E} models (set_members first)")
        self.nleap, self.delt = nleap, delt
        self.dev = torch.device(device)
        E, nl = self.E, res.nlocal
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=self.dev)  # noqa: E731
        self.fb = z(E, int(res.fb_offsets[-1]))
        self.lm, self.ov = z(E, nl, max(res.ncs, 1)), z(E, nl, res.nout)
        # variables3d(4, 96, 48, 8) / logp(96, 48) / precip(96, 48) in Fortran order, per member
        self.g4, self.g2, self.pr = z(E, 8, 48, 96, 4), z(E, 48, 96), z(E, 48, 96)
        self.f4, self.f2 = z(E, 8, 48, 96, 4), z(E, 48, 96)
        if speedy_cus is None:
            speedy_cus = int(os.environ.get("SML_SPEEDY_CUS", "64"))
        ncu = torch.cuda.get_device_properties(self.dev).multi_processor_count
        self._streams = []
        with torch.cuda.device(self.dev):
            if 0 < speedy_cus < ncu:
                self.speedy_cus, self.res_cus = speedy_cus, ncu - speedy_cus
                self.side = self._cu_stream(0, speedy_cus)
                self.main = self._cu_stream(speedy_cus, self.res_cus)
                for d in self.dyns:  # the windows' safety checks beside them, never on SPEEDY's CUs
                    check(lib().sml_dyn_set_check_cus(d._h, speedy_cus, self.res_cus))
                res.set_read_waves(0)  # pacing pays only on shared CUs
                res.set_update_cus(self.res_cus)
            else:
                self.speedy_cus = self.res_cus = 0
                self.side, self.main = self._cu_stream(0, ncu), self._cu_stream(0, ncu)
        self._tiled = torch.cuda.Event()
        self._started, self._slab_started = set(), set()
        self._flags = [True] * E
        # the steps done, and the calendar run_model's date and the tisr table share
        self.t = 0
        self._cal_on, self._table = False, None
        self._startyear, self._base, self._step_hours, self._feb29 = 0, 0, 6, 0
        self.exchange_width = res.nout
        self._prod, self._prod_t, self._truth, self._prod_fields = None, 0, None, False
        self.mean4 = self.mean2 = self.meanpr = self.spread4 = self.spread2 = self.spreadpr = None
        if slab is not None:
            self._set_slab(slab)

    def _set_slab(self, slab):
        """sml_slab_create: sml_hybrid_set_slab's checks, the index tables, the members' slab
        buffers; the atmo context's outvec rows widen to the exchange width."""
        h = ctypes.c_void_p()
        try:
            with torch.cuda.device(self.dev):
                check(lib().sml_slab_create(self.res.handle, slab.res.handle, ptr(slab.base_sst), ptr(slab.sea_mask),
                                            int(slab.timestep), int(slab.timestep_slab), float(slab.sst_bias),
                                            ctypes.byref(h)))
        except SmlError as err:  # the native loop's refusals, with their reason
            raise ValueError(f"slab: {err}") from None
        self._slab_h = h
        w = ctypes.c_int()
        check(lib().sml_slab_info(h, None, ctypes.byref(w), None, None, None, None))
        self.exchange_width = w.value
        self.res.set_outvec_ld(w.value)  # (set by the create already: the binding's copy of it)
        self.ov = torch.zeros((self.E, self.res.nlocal, w.value), dtype=torch.float64, device=self.dev)
        if self.res_cus > 0:  # the slab step runs on the main stream too
            slab.res.set_update_cus(self.res_cus)

    def _strides(self):
        return int(self.ov.stride(0)), int(self.fb.stride(0))

    def _cu_stream(self, first, count):
        h = ctypes.c_void_p()
        check(lib().sml_stream_create_cu_range(int(first), int(count), ctypes.byref(h)))
        self._streams.append(h)
        return torch.cuda.ExternalStream(h.value, device=self.dev)

    def _tile_feedback(self, e):
        # (the start's feedback takes the fixed tisr with a table set too, as sml_hybrid_start's)
        self.res.tile_feedback(self.g4[e], self.g2[e], self.pr[e], self.tisr, self.fb[e], stream=self.main)

    def set_calendar(self, startyear: int, hours_base: int, step_hours: int = 6):
        """run_model's calendar (HybridLoop.set_calendar): step t hands every member's window
        the date of hour hours_base + t * step_hours and refreshes its forcing at that date
        (Dynamics.fordate; every Dynamics needs set_surface).  Shared with the tisr table's;
        the step count restarts."""
        if step_hours <= 0 or hours_base < 0:
            raise ValueError("set_calendar: step_hours > 0 and hours_base >= 0 expected")
        self._startyear, self._base, self._step_hours = int(startyear), int(hours_base), int(step_hours)
        self._feb29, self.t, self._cal_on = 0, 0, True

    def set_tisr_table(self, table, startyear: int, hours_base: int, step_hours: int = 6):
        """get_tisr_by_date (HybridLoop.set_tisr_table): hourly global tisr fields `table`
        [nhours >= 8760, 48, 96] (device) shared by the members; None switches back to the
        fixed tisr.  The step count restarts."""
        if table is not None:
            if step_hours <= 0 or hours_base < 0 or table.dim() != 3 or table.shape[0] < 8760 \
                    or tuple(table.shape[1:]) != (48, 96) or not table.is_contiguous() \
                    or table.dtype != torch.float64 or not table.is_cuda:
                raise ValueError("set_tisr_table: a contiguous float64 device table [>= 8760, 48, 96], "
                                 "step_hours > 0 and hours_base >= 0 expected")
        self._table = table
        self._startyear, self._base, self._step_hours = int(startyear), int(hours_base), int(step_hours)
        self._feb29, self.t = 0, 0

    def set_products(self, capacity, truth=None, fields=True):
        """Ensemble products of every step from here on (EnsembleProducts): step s = 0, 1, ..
        after this call fills row s of the score tables from the assembled hybrid grids
        g4, g2, pr, verified against truth[s] -- truth: None (only the spread is scored), or
        device tensors ([T, 8, 48, 96, 4], [T, 48, 96], [T, 48, 96] or None) with
        T >= capacity -- and, with `fields`, leaves their mean and spread in mean4 / mean2 /
        meanpr and spread4 / spread2 / spreadpr.  The launches follow begin_members on the
        main stream, off the chain between the finish and the windows; no loop buffer
        changes.  A step past `capacity` refuses before anything is enqueued.
        capacity None switches the products off: step() is then the loop without them."""
        if capacity is not None:
            if int(capacity) < 1:
                raise ValueError("set_products: capacity >= 1 expected")
            if truth is not None:
                t4, t2, tp = truth
                for x, shape, optional in ((t4, (8, 48, 96, 4), False), (t2, (48, 96), False), (tp, (48, 96), True)):
                    if x is None and optional:
                        continue
                    if x is None or x.dtype != torch.float64 or not x.is_cuda or not x.is_contiguous() \
                            or tuple(x.shape[1:]) != shape or x.shape[0] < int(capacity):
                        raise ValueError(f"set_products: truth [T >= {int(capacity)}, {', '.join(map(str, shape))}], "
                                         "contiguous float64 device tensors, expected")
        self.sync()
        if self._prod is not None:
            self._prod.close()
        self._prod, self._prod_t, self._truth, self._prod_fields = None, 0, None, False
        self.mean4 = self.mean2 = self.meanpr = self.spread4 = self.spread2 = self.spreadpr = None
        if capacity is None:
            return
        self._prod = EnsembleProducts(self.E, int(capacity), self.dev)
        self._truth, self._prod_fields = truth, bool(fields)
        if fields:
            z = lambda *s: torch.zeros(s, dtype=torch.float64, device=self.dev)  # noqa: E731
            self.mean4, self.mean2, self.meanpr = z(8, 48, 96, 4), z(48, 96), z(48, 96)
            self.spread4, self.spread2, self.spreadpr = z(8, 48, 96, 4), z(48, 96), z(48, 96)

    def products(self, t0=0, count=None):
        """Host rows [t0, t0 + count) of the score tables (count None: up to the last step
        done): scores [count, 34, 4] = rmse, spread, crps, bias and ranks [count, 34, 33].
        Waits for the device."""
        if self._prod is None:
            raise RuntimeError("no products in this loop (set_products)")
        return self._prod.read(t0, self._prod_t - t0 if count is None else count)

    def _enqueue_products(self):
        p, s = self._prod, self._prod_t
        if self._prod_fields:
            p.moments(self.g4, self.g2, self.pr, out=(self.mean4, self.mean2, self.meanpr, self.spread4, self.spread2,
                                                      self.spreadpr), stream=self.main)
        truth = None
        if self._truth is not None:
            t4, t2, tp = self._truth
            truth = (t4[s], t2[s], tp[s] if tp is not None else None)
        p.scores(self.g4, self.g2, self.pr, truth, s, stream=self.main)
        self._prod_t = s + 1

    def _date(self, t, feb29):
        d = (ctypes.c_int * 4)()
        check(lib().sml_calendar_delta_hour(self._startyear, self._base + t * self._step_hours, ctypes.byref(feb29), d))
        return tuple(d)

    def window_date(self):
        """(year, month, day, hour) of the next step's windows."""
        if not self._cal_on:
            raise RuntimeError("no calendar (set_calendar)")
        return self._date(self.t + 1, ctypes.c_int(self._feb29))

    def start(self, e, g4, g2, pr, f4, f2):
        """start_prediction analogue for member e: its analysis grid (g4, g2, pr) and a
        SPEEDY forecast from it (f4, f2) into the loop's buffers, its first feedback tiled.
        After the last member's start the first begin_members is issued.  A start after that
        is a restart: the pending begin is discarded and every member is to be started again."""
        if not 0 <= e < self.E:
            raise ValueError(f"member {e} out of range [0, {self.E})")
        torch.cuda.synchronize(self.dev)
        if len(self._started) == self.E or self.res.step_begun():
            # a restart (every member is started again): the begin in flight, if the host has
            # not discarded it already, was built from the old feedback
            self.res.cancel_step()
            self._started.clear()
            self._slab_started.clear()
        self._slab_started.discard(e)
        with torch.cuda.stream(self.main):
            for dst, src in ((self.g4, g4), (self.g2, g2), (self.pr, pr), (self.f4, f4), (self.f2, f2)):
                dst[e].copy_(src)
        self._tile_feedback(e)
        self._started.add(e)
        if len(self._started) == self.E:
            self.res.begin_members(self.fb, stream=self.main)
        self.main.synchronize()

    def start_slab(self, e, slab_outvec):
        """start_prediction_slab's hand-over for member e, after its start: the slab
        reservoirs' sst [nslab, 4] (device) until their first prediction (sml_slab_start;
        their states are the host's to synchronize, slab.res.set_state(..., member=e))."""
        if self._slab_h is None:
            raise RuntimeError("no slab ocean in this loop (slab=)")
        if not 0 <= e < self.E:
            raise ValueError(f"member {e} out of range [0, {self.E})")
        if e not in self._started:
            raise RuntimeError(f"start_slab of member {e} before its start")
        ovs, _ = self._strides()
        check(lib().sml_slab_start(self._slab_h, int(e), ptr(slab_outvec), ptr(self.ov), ovs, self.main.cuda_stream))
        self._slab_started.add(e)

    def slab_state(self, e):
        """Host copies of member e's slab state (after the loop's work completes), as
        HybridLoop.slab_state: wholegrid_sst [48, 96], the ring [ratio - 1, tot], the last
        slab feedback [tot] and slab outvecs [nslab, 4]."""
        if self._slab_h is None:
            raise RuntimeError("no slab ocean in this loop (slab=)")
        if not 0 <= e < self.E:
            raise ValueError(f"member {e} out of range [0, {self.E})")
        p = [ctypes.c_void_p() for _ in range(4)]
        st = [ctypes.c_int64() for _ in range(4)]
        args = [x for pair in zip(p, st) for x in (ctypes.byref(pair[0]), ctypes.byref(pair[1]))]
        check(lib().sml_slab_buffers(self._slab_h, *args))
        cols, n = ctypes.c_int(), ctypes.c_int()
        check(lib().sml_slab_info(self._slab_h, None, None, None, ctypes.byref(cols), ctypes.byref(n), None))
        return slab_state_copy(p, [s.value for s in st], e, cols.value, n.value, self.slab.res.nlocal)

    def step(self):
        """One hybrid time step of every member.  Returns when the E windows are done; the
        next step's begin may still run on the main stream (`sync()` waits for it)."""
        if len(self._started) != self.E:
            raise RuntimeError("EnsembleLoop.step before every member's start")
        if self._slab_h is not None and len(self._slab_started) != self.E:
            raise RuntimeError("EnsembleLoop.step before every member's start_slab")
        if self._prod is not None and self._prod_t >= self._prod.capacity:
            raise RuntimeError(f"EnsembleLoop.step: the products' {self._prod.capacity} rows are full "
                               "(set_products with a larger capacity, or None)")
        res, L, m = self.res, lib(), self.main.cuda_stream
        # the date of step t + 1 and the table's hour of step t, once for all members and ahead
        # of any launch (a refusal leaves the loop as it was); the date first: the two lookups
        # share the calendar's February latch, and run_model's comes first in the reference
        feb29, date, field = ctypes.c_int(self._feb29), None, None
        if self._cal_on:
            date = self._date(self.t + 1, feb29)
        if self._table is not None:
            idx = ctypes.c_int()
            check(L.sml_tisr_date_index(self._startyear, self._base + self.t * self._step_hours, ctypes.byref(feb29),
                                        ctypes.byref(idx)))
            if not 1 <= idx.value <= self._table.shape[0]:
                raise ValueError(f"tisr hour {idx.value} outside the table's {self._table.shape[0]} hours")
            field = self._table[idx.value - 1]
        self._feb29 = feb29.value
        ovs, fbs = self._strides()
        if self._slab_h is not None:  # predict_slab_ml of every member, on a slab step
            check(L.sml_slab_predict(self._slab_h, self.t + 1, ptr(self.ov), ovs, m, None))
        res.finish_assemble_members(self.f4, self.f2, self.lm if res.ncs else None, self.ov, self.g4, self.g2,
                                    self.pr, stream=self.main)
        if self._slab_h is not None:  # a new SST: the grids, the feedbacks' sst entries, the windows' sst_am
            wrote = ctypes.c_int()
            check(L.sml_slab_sst(self._slab_h, ptr(self.ov), ovs, ptr(self.fb), fbs, m, ctypes.byref(wrote)))
            if wrote.value:
                sst, stride = ctypes.c_void_p(), ctypes.c_int64()
                check(L.sml_slab_buffers(self._slab_h, ctypes.byref(sst), ctypes.byref(stride), None, None, None, None,
                                         None, None))
                for e, dyn in enumerate(self.dyns):
                    check(L.sml_dyn_set_hybrid_sst(dyn._h, ctypes.c_void_p(sst.value + 8 * e * stride.value),
                                                   float(self.slab.sst_bias), m))
        self.t += 1
        res.tile_feedback_members(self.g4, self.g2, self.pr, None if field is not None else self.tisr, self.fb,
                                  stream=self.main)
        if field is not None:  # get_tisr_by_date(..., timestep - 1, ...) for the next feedback
            res.tile_tisr_field_members(field, self.fb, stream=self.main)
        if self._slab_h is not None:  # averaged_atmo_input_vec(:, mod(t-1, R-1)+1)
            check(L.sml_slab_ring(self._slab_h, self.t, ptr(self.fb), fbs, m))
        self._tiled.record(self.main)
        res.begin_members(self.fb, stream=self.main)
        if self._prod is not None:  # behind the begin: g4, g2, pr stay as they are until the next finish
            self._enqueue_products()
        self.side.wait_event(self._tiled)
        for e, dyn in enumerate(self.dyns):
            if date is not None:  # the window's forcing at the date, behind any new SST
                dyn.fordate(date[0], date[1], date[2], stream=self.side)
            dyn.run_model(self.g4[e], self.g2[e], self.f4[e], self.f2[e], nleap=self.nleap, delt=self.delt,
                          alph=ALPH, stream=self.side)
            # the safety rule: window e and its check are done before window e + 1 is enqueued
            self._flags[e] = dyn.last_safe()[0]
            self.side.synchronize()

    def run_speedy(self):
        """run_speedy of the last step, per member: False where that member's window entry
        failed iogrid(30)'s safety check (the reference ends the prediction there)."""
        return list(self._flags)

    def cancel_step(self):
        """Discard the begin issued for the next step: every member's state is then the one
        the last finished step computed.  The next step() needs a start() of every member."""
        self.res.cancel_step()
        self._started.clear()
        self._slab_started.clear()

    def sync(self):
        self.main.synchronize()
        self.side.synchronize()

    def close(self):
        """Wait for the loop's work and release its streams."""
        if getattr(self, "_streams", None):
            self.sync()
            for h in self._streams:
                check(lib().sml_stream_destroy(h))
            self._streams = []
        if getattr(self, "_slab_h", None):
            check(lib().sml_slab_destroy(self._slab_h))
            self._slab_h = None
        if getattr(self, "_prod", None) is not None:
            self._prod.close()
            self._prod = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

"""An E-member hybrid forecast on one rank: one reservoir context holding E members
(Reservoirs.set_members) beside E SPEEDY models, one Dynamics per member.

Every member is the hybrid loop of speedy_ml_amd.hybrid on its own (parallelmain.f90:204-270:
predict, sendrecievegrid's assembly, run_model, the re-tiling), bit for bit; what the members
share is the stream of the reservoir weights.  The split step makes that sharing pay in a
hybrid forecast: the members' update and v_ml (begin_members, about 98 % of the bytes) run on
the reservoir's CUs while the E windows run one after the other on SPEEDY's, and only the v_p
finish (finish_assemble_members: local models tiled from the E forecasts, the members' outvecs,
the E assembled grids) waits for the forecasts.

Schedule of step():
  main stream  finish_assemble_members(f4, f2 -> lm, ov, g4, g2, pr)
               tile_feedback per member into fb[e]                      -> event
               begin_members(fb): the next step's update and v_ml (the states run one update
               ahead, as the pipelined HybridLoop's do; cancel_step() rolls them back)
  side stream  waits for the event, then for e = 0 .. E - 1: dyns[e].run_model(g4[e], g2[e] ->
               f4[e], f2[e]); the host waits for window e (its safety flag, then the stream)
               before it enqueues window e + 1.
That host wait is a safety rule, not a convenience: every Dynamics has a check stream whose
kernel polls in-kernel, an in-kernel wait holds its hardware queue, and
the E contexts' streams share the process's few queues -- so no window is enqueued while
another context's window or check is outstanding.

Out of scope here: more than one rank (world > 1: `res` holds every region in global order),
the slab ocean, the calendar and the tisr table (a fixed tisr or none), concurrent windows, and
a native (sml_hybrid_*) form of this loop.
"""
from __future__ import annotations

import ctypes
import os

import torch

from ._lib import check, lib
from .dynamics import ALPH, DELT


class EnsembleLoop:
    """res: Reservoirs holding every region in global order with set_members(len(dyns))
    done; dyns: one Dynamics per member, each with its own state, forcing and physics;
    tisr: [nlocal, 16] standardized tisr inputs (device) or None.  Owns the members'
    strided buffers fb [E, tot], lm [E, nlocal, ncs], ov [E, nlocal, nout], g4 / f4
    [E, 8, 48, 96, 4], g2 / pr / f2 [E, 48, 96] and two library streams on the CU split
    HybridLoop uses: SPEEDY on CUs [0, speedy_cus), the reservoir on the rest.  As
    HybridLoop does, it moves each Dynamics' safety check to a CU-masked stream on the
    reservoir's CUs (sml_dyn_set_check_cus) and lifts the reservoir's read-wave cap; a window
    of such a Dynamics must not be run on the legacy default stream afterwards (a CU-masked
    stream synchronises with it, and the window and its in-kernel check would wait for each
    other until the check's time-out)."""

    def __init__(self, res, dyns, device, tisr=None, nleap: int = 24, delt: float = DELT,
                 speedy_cus: int | None = None):
        self.res, self.dyns, self.tisr = res, list(dyns), tisr
        self.E = len(self.dyns)
        if self.E < 1 or res.members != self.E:
            raise ValueError(f"dyns: {self.E} models for a context of {res.members} members (set_members first)")
        if res.nlocal != res.numregions or list(res.region_ids) != list(range(res.numregions)):
            raise ValueError("res: every region of the decomposition, in global order, expected (world 1)")
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
        self._started = set()
        self._flags = [True] * E

    def _cu_stream(self, first, count):
        h = ctypes.c_void_p()
        check(lib().sml_stream_create_cu_range(int(first), int(count), ctypes.byref(h)))
        self._streams.append(h)
        return torch.cuda.ExternalStream(h.value, device=self.dev)

    def _tile_feedback(self, e):
        self.res.tile_feedback(self.g4[e], self.g2[e], self.pr[e], self.tisr, self.fb[e], stream=self.main)

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
        with torch.cuda.stream(self.main):
            for dst, src in ((self.g4, g4), (self.g2, g2), (self.pr, pr), (self.f4, f4), (self.f2, f2)):
                dst[e].copy_(src)
        self._tile_feedback(e)
        self._started.add(e)
        if len(self._started) == self.E:
            self.res.begin_members(self.fb, stream=self.main)
        self.main.synchronize()

    def step(self):
        """One hybrid time step of every member.  Returns when the E windows are done; the
        next step's begin may still run on the main stream (`sync()` waits for it)."""
        if len(self._started) != self.E:
            raise RuntimeError("EnsembleLoop.step before every member's start")
        res = self.res
        res.finish_assemble_members(self.f4, self.f2, self.lm if res.ncs else None, self.ov, self.g4, self.g2,
                                    self.pr, stream=self.main)
        for e in range(self.E):
            self._tile_feedback(e)
        self._tiled.record(self.main)
        res.begin_members(self.fb, stream=self.main)
        self.side.wait_event(self._tiled)
        for e, dyn in enumerate(self.dyns):
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

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

#!/usr/bin/env python
"""The members' split step against what it replaces (profiles/members.md).

A configs[1]-shaped context as tools/probe_members.py builds it (every region of the
decomposition at its own n, fp32 storage) at E members; three pairs, each alternating in one
process, --repeats windows of --window seconds after a warm-up:
  begin   : begin_members (update + v_ml) against predict_members (the one-pass step), each
            call between a pair of device events of its own (the begin's finish runs outside
            its pair)
  finish  : finish_assemble_members at each finish tile TF (the library's measurement hook
            sml_res_dbg_set_finish_tile; 1 = the single-member k_res_finish_grid<kAsm>
            launched once per member on the members' pointers), each call between a pair of
            device events, behind an untimed begin_members
  loop    : one EnsembleLoop.step (the split step beside E serial SPEEDY windows) against the
            host sequence a host holding E members runs without it -- predict_members, then
            per member assemble, tile_feedback, run_model and its wait, tile_local_model --
            by the host clock around steps that end in a device synchronise.  The host
            sequence runs on a library stream of its own, never on the default stream: once a
            loop has moved a Dynamics' safety check to a CU-masked stream
            (sml_dyn_set_check_cus), that stream is a blocking one, and a window on the legacy
            default stream and its in-kernel check would then wait for each other until the
            check's time-out
--host-only runs the host sequence alone: with SML_LIB naming another build of the library
(the parent commit's) it is that build's side of the loop comparison on the same machine.
--slab, --calendar and --tisr-table (any of them) add a fourth pair:
  options : EnsembleLoop.step with the chosen options against the plain loop on the same
            context and SPEEDY models, alternating in one process: every window restarts the
            members, warms up and times a whole number of slab cycles (timestep_slab /
            timestep steps: one slab step in each) by the host clock.  The slab reservoirs are
            full size (n 4000 + the sst) unless --n-override reduces them too.
--products adds a pair of its own:
  products: EnsembleLoop.step with set_products(capacity, truth) against the same loop with
            products off, alternating in one process by the host clock, and the products' own
            launches (sml_ens_moments + sml_ens_scores on the loop's grids) between a pair of
            device events.  With SML_LIB naming a build without the sml_ens_* entry points (the
            parent commit's) only the loop with products off is timed: that build's side of
            the "off against the parent" comparison.
--loop-only skips the begin, finish and host-sequence pairs.
Prints one JSON line per E and markdown tables.  Needs the GPU; there is no CPU path.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speedy-ml-1_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=1152)
    ap.add_argument("--members", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--tiles", type=int, nargs="+", default=[1, 2, 4], help="finish tiles to try (1 = looped single)")
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timed window (>= 0.2)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n-override", type=int, default=None, help="reduced n (a rehearsal, not a measurement)")
    ap.add_argument("--host-only", action="store_true", help="the host sequence alone (any build of the library)")
    ap.add_argument("--slab", action="store_true", help="the options pair: the slab ocean (1027 slab reservoirs)")
    ap.add_argument("--calendar", action="store_true", help="the options pair: run_model's date drives fordate")
    ap.add_argument("--tisr-table", action="store_true", help="the options pair: tisr by date from an hourly table")
    ap.add_argument("--products", action="store_true", help="the products pair: set_products on against off")
    ap.add_argument("--loop-only", action="store_true", help="skip the begin, finish and host-sequence pairs")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    args = ap.parse_args()

    import torch

    from speedy_ml_amd import domain
    from speedy_ml_amd._lib import check, lib
    from speedy_ml_amd.dynamics import Dynamics
    from speedy_ml_amd.reservoir import Reservoirs
    from speedy_ml_amd.synthetic import dyn_state, initial_state, phys_boundary, region_weights, synthetic_grids

    if not torch.cuda.is_available():
        sys.exit("probe_members_split needs the GPU")
    if args.regions != 1152:
        sys.exit("the assembly needs every region of the 1152-region decomposition on this rank")
    dev = torch.device("cuda", 0)
    mask = domain.load_sst_mask()
    regions = list(range(args.regions))
    t0 = time.time()

    def weights(r):
        return region_weights(r, bool(mask[r]), climatology=True, n_override=args.n_override)

    if args.n_override is None:
        sizes = [domain.reservoir_sizes(r, bool(mask[r])) for r in regions]
        ws_n, ws_k = [s.n for s in sizes], [s.k for s in sizes]
    else:
        ws_n, ws_k = (list(v) for v in zip(*((w.n, w.k) for w in map(weights, regions))))
    res = Reservoirs(regions, [mask[r] for r in regions], ws_n, ws_k, weight_dtype="f32")
    for i, r in enumerate(regions):
        res.load_region_weights(i, weights(r))
        if i % 288 == 0:
            print(f"loaded {i}/{len(regions)} regions ({time.time() - t0:.1f}s)", flush=True)
    nl, ncs, nout = res.nlocal, res.ncs, res.nout
    tot = int(res.fb_offsets[-1])
    res.set_read_waves(0)  # the v_ml launch uncapped, as EnsembleLoop runs it on CUs of its own
    emax = max(args.members)
    x0 = [initial_state(r, n) for r, n in zip(regions, ws_n)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    tisr = t(np.random.default_rng(13).standard_normal((nl, 16)))
    st0, forcing = dyn_state()

    options = args.slab or args.calendar or args.tisr_table
    if args.host_only and (options or args.loop_only or args.products):
        sys.exit("--host-only runs the host sequence alone")

    def dynamics():
        d = Dynamics()
        d.set_forcing(**forcing)
        d.set_state(st0)
        bc = phys_boundary(d, forcing["phis"])
        if options:  # the date-driven forcing's inputs, as bench.py's loop has them
            from speedy_ml_amd.synthetic import surface_climatology
            surf, clim = surface_climatology(bc["fmask1"])
            bc["fmask1"] = surf["fmask_l"]
        d.set_physics(bc)
        if options:
            d.set_surface(surf)
            d.set_climatology(clim)
        return d

    slab = table = None
    if args.slab:
        from speedy_ml_amd.synthetic import slab_fields, slab_start_outvec, slab_weights

        sreg = [r for r in regions if mask[r]]
        sws = [slab_weights(r, n_override=args.n_override and 200) for r in sreg]
        slab = Reservoirs(sreg, [0] * len(sreg), [w.n for w in sws], [w.k for w in sws], chunk_speedy=0, nout=4,
                          ninp=[w.ninp for w in sws], out_index=[35] * 4, weight_dtype="f32")
        for j, w in enumerate(sws):
            slab.load_region_weights(j, w)
        sx0 = [initial_state(r, w.n, seed=17) for r, w in zip(sreg, sws)]
        del sws
        base, smask, _, _ = slab_fields()
        print(f"loaded {len(sreg)} slab reservoirs ({time.time() - t0:.1f}s)", flush=True)
    if args.tisr_table:
        table = torch.from_numpy(300.0 + 100.0 * np.random.default_rng(21).random((8760, 48, 96))).to(dev)

    dyns = [dynamics() for _ in range(emax)]
    hh = ctypes.c_void_p()  # the host sequence's stream: every CU, not the default stream
    check(lib().sml_stream_create_cu_range(0, torch.cuda.get_device_properties(dev).multi_processor_count,
                                           ctypes.byref(hh)))
    hstream = torch.cuda.ExternalStream(hh.value, device=dev)
    print(f"context and {emax} SPEEDY models ready ({time.time() - t0:.1f}s)", flush=True)

    def set_members(E):
        if res.step_begun():
            res.cancel_step()
        res.set_members(E)
        for e in range(E):  # perturbed copies of one start
            for i in range(nl):
                res.set_state(i, x0[i] * (1.0 - 0.01 * e), member=e)

    def paired(before, timed, after, ncalls):
        """Mean device time of `timed` alone, in ms: a pair of events around every call."""
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ncalls)]
        for a, b in ev:
            before()
            a.record()
            timed()
            b.record()
            after()
        torch.cuda.synchronize()
        return float(np.mean([a.elapsed_time(b) for a, b in ev]))

    def calls_for(before, timed, after):
        paired(before, timed, after, 5)
        ms = paired(before, timed, after, 10)
        return max(20, min(2000, int(np.ceil(args.window * 1e3 / max(ms, 1e-3)))))

    def host_clock(step, sync, nsteps):
        sync()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(nsteps):
            step()
        sync()
        torch.cuda.synchronize()
        return (time.perf_counter() - t1) * 1e3 / nsteps

    def options_pair(E, rec, starts, flags, healthy):
        """EnsembleLoop.step with the options against the plain loop, alternating."""
        from speedy_ml_amd.ensemble import EnsembleLoop
        from speedy_ml_amd.hybrid import SlabOcean

        set_members(E)
        cycle = 28  # timestep_slab / timestep of the reference (168 h / 6 h): one slab step a cycle
        cal = (1981, 227520 + 24 * 40)
        ocean = sov = None
        if slab is not None:
            slab.set_members(E)
            sov = t(np.stack([slab_start_outvec(r) for r in sreg]))
            ocean = SlabOcean(slab, t(base), t(smask))  # timestep 6 h, timestep_slab 168 h
        variants = {"plain": EnsembleLoop(res, dyns[:E], dev, tisr=tisr),
                    "options": EnsembleLoop(res, dyns[:E], dev, tisr=tisr, slab=ocean)}
        full = variants["options"]
        widths = {"plain": res.nout, "options": full.exchange_width}

        def restart(name):
            loop = variants[name]
            if res.step_begun():
                res.cancel_step()
            res.set_outvec_ld(widths[name])  # the two loops' outvec rows differ by the slab's sst columns
            if name == "options":
                if args.tisr_table:
                    loop.set_tisr_table(table, *cal)
                if args.calendar:
                    loop.set_calendar(*cal)
            for e in range(E):
                loop.start(e, *starts[e])
                if name == "options" and slab is not None:
                    for j in range(len(sreg)):
                        slab.set_state(j, sx0[j] * (1.0 - 0.01 * e), member=e)
                    loop.start_slab(e, sov)
            return loop

        for name in variants:  # warm every shape, the slab step included
            loop = restart(name)
            ms = host_clock(loop.step, loop.sync, 1)
            flags[:] = loop.run_speedy()
            healthy(f"EnsembleLoop.step ({name}), first step", ms)
            ms = host_clock(loop.step, loop.sync, cycle)
        ncyc = max(1, min(8, int(np.ceil(args.window * 1e3 / (ms * cycle)))))
        rec["options"] = dict(slab=args.slab, calendar=args.calendar, tisr_table=args.tisr_table,
                              steps_per_window=ncyc * cycle)
        rec["plain_ms"], rec["options_ms"] = [], []
        for _ in range(args.repeats):
            for name in variants:
                loop = restart(name)
                host_clock(loop.step, loop.sync, 3)  # (every timed cycle holds one slab step, whatever its phase)
                rec[name + "_ms"].append(round(host_clock(loop.step, loop.sync, ncyc * cycle), 4))
                flags[:] = loop.run_speedy()
                healthy(f"EnsembleLoop.step ({name}) window", rec[name + "_ms"][-1])
        for loop in variants.values():
            loop.sync()
        if res.step_begun():
            res.cancel_step()
        for loop in variants.values():
            loop.close()
        res.set_outvec_ld(res.nout)

    def products_pair(E, rec, starts, flags, healthy):
        """EnsembleLoop.step with the ensemble products on against off, alternating; then the
        products' own launches between device events."""
        from speedy_ml_amd.ensemble import EnsembleLoop

        have = hasattr(lib(), "sml_ens_create")
        set_members(E)
        for d in dyns[:E]:
            d.set_state(st0)
        loop = EnsembleLoop(res, dyns[:E], dev, tisr=tisr)
        for e in range(E):
            loop.start(e, *starts[e])
        ms = host_clock(loop.step, loop.sync, 1)
        flags[:] = loop.run_speedy()
        healthy("EnsembleLoop.step (products pair), first step", ms)
        host_clock(loop.step, loop.sync, 10)
        ms = host_clock(loop.step, loop.sync, 10)
        nsteps = max(10, min(400, int(np.ceil(args.window * 1e3 / ms))))
        rec["products_steps_per_window"] = nsteps
        rec["products_off_ms"], rec["products_on_ms"] = [], []
        truth = None
        if have:
            g = torch.Generator(device="cpu").manual_seed(7)
            truth = tuple(torch.randn((nsteps + 3,) + s, dtype=torch.float64, generator=g).to(dev)
                          for s in ((8, 48, 96, 4), (48, 96), (48, 96)))
        for _ in range(args.repeats):
            if have:
                loop.set_products(None)
            rec["products_off_ms"].append(round(host_clock(loop.step, loop.sync, nsteps), 4))
            flags[:] = loop.run_speedy()
            healthy("EnsembleLoop.step, products off, window", rec["products_off_ms"][-1])
            if have:
                loop.set_products(nsteps + 3, truth)
                host_clock(loop.step, loop.sync, 3)
                rec["products_on_ms"].append(round(host_clock(loop.step, loop.sync, nsteps), 4))
                flags[:] = loop.run_speedy()
                healthy("EnsembleLoop.step, products on, window", rec["products_on_ms"][-1])
        if have:
            from speedy_ml_amd.ensemble import EnsembleProducts

            loop.set_products(None)
            loop.sync()
            prod = EnsembleProducts(E, 1, dev)
            out = tuple(torch.zeros(s, dtype=torch.float64, device=dev)
                        for s in ((8, 48, 96, 4), (48, 96), (48, 96)) * 2)
            tr0 = tuple(a[0] for a in truth)

            def launches():
                prod.moments(loop.g4, loop.g2, loop.pr, out=out, stream=hstream)
                prod.scores(loop.g4, loop.g2, loop.pr, tr0, 0, stream=hstream)

            with torch.cuda.stream(hstream):
                n = calls_for(nop, launches, nop)
                rec["products_launch_ms"] = [round(paired(nop, launches, nop, n), 5) for _ in range(args.repeats)]
            grid = (147456 + 2 * 4608) * 8
            # each kernel reads the E members once from memory (the moments' second pass and the
            # scores' pair term re-read what the thread has just loaded); means, spreads, truth
            rec["products_bytes"] = 2 * E * grid + 3 * grid
            prod.close()
        loop.sync()
        if res.step_begun():
            res.cancel_step()
        loop.close()

    nop = lambda: None  # noqa: E731
    lines = []
    for E in args.members:
        rec = dict(E=E, n_override=args.n_override, lib=os.environ.get("SML_LIB") or "built")
        set_members(E)
        g = torch.Generator(device="cpu").manual_seed(5)
        fb = torch.randn((E, tot), dtype=torch.float64, generator=g).to(dev)
        lm = torch.randn((E, nl, ncs), dtype=torch.float64, generator=g).to(dev)
        ov = torch.zeros((E, nl, nout), dtype=torch.float64, device=dev)
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)  # noqa: E731
        g4, g2, pr = z(E, 8, 48, 96, 4), z(E, 48, 96), z(E, 48, 96)
        f4, f2 = z(E, 8, 48, 96, 4), z(E, 48, 96)
        starts = []
        for e in range(E):
            a4, a2, ap_ = synthetic_grids(11 + 10 * e)
            b4, b2, _ = synthetic_grids(12 + 10 * e)
            starts.append(tuple(t(a) for a in (a4, a2, ap_, b4, b2)))
            f4[e].copy_(starts[e][3])
            f2[e].copy_(starts[e][4])

        if not args.host_only and not args.loop_only:
            # ---- begin_members against predict_members
            begin = lambda: res.begin_members(fb)  # noqa: E731
            finish = lambda: res.finish_members(lm, ov)  # noqa: E731
            onepass = lambda: res.predict_members(fb, lm, ov)  # noqa: E731
            nb, ns = calls_for(nop, begin, finish), calls_for(nop, onepass, nop)
            rec["begin_ms"], rec["step_members_ms"] = [], []
            for _ in range(args.repeats):
                rec["begin_ms"].append(round(paired(nop, begin, finish, nb), 4))
                rec["step_members_ms"].append(round(paired(nop, onepass, nop, ns), 4))
            # ---- the finish with assembly at each tile
            L = lib()
            L.sml_res_dbg_set_finish_tile.argtypes = [ctypes.c_void_p, ctypes.c_int]
            L.sml_res_dbg_set_finish_tile.restype = ctypes.c_int
            fin = lambda: res.finish_assemble_members(f4, f2, lm, ov, g4, g2, pr)  # noqa: E731
            tiles = [tf for tf in args.tiles if tf <= max(E, 1)]
            rec["finish_ms"] = {str(tf): [] for tf in tiles}
            ncalls = {}
            for tf in tiles:
                check(L.sml_res_dbg_set_finish_tile(res.handle, tf))
                ncalls[tf] = calls_for(begin, fin, nop)
            for _ in range(args.repeats):
                for tf in tiles:
                    check(L.sml_res_dbg_set_finish_tile(res.handle, tf))
                    rec["finish_ms"][str(tf)].append(round(paired(begin, fin, nop, ncalls[tf]), 5))
            check(L.sml_res_dbg_set_finish_tile(res.handle, 0))
            print(f"E {E} begin {rec['begin_ms']} one pass {rec['step_members_ms']} finish {rec['finish_ms']}",
                  flush=True)
            rec["finish_tile_of_the_build"] = res.member_finish_tile()

        # ---- the loop: the host sequence, and (this build) EnsembleLoop.step
        hs = dict(fb=z(E, tot), lm=z(E, nl, ncs), ov=z(E, nl, nout), g4=z(E, 8, 48, 96, 4), g2=z(E, 48, 96),
                  pr=z(E, 48, 96), f4=z(E, 8, 48, 96, 4), f2=z(E, 48, 96))
        flags = [True] * E

        def host_start():
            set_members(E)
            for e in range(E):
                for k, src in zip(("g4", "g2", "pr", "f4", "f2"), starts[e]):
                    hs[k][e].copy_(src)
                torch.cuda.synchronize()
                res.tile_inputs(hs["g4"][e], hs["g2"][e], hs["pr"][e], hs["f4"][e], hs["f2"][e], tisr, hs["fb"][e],
                                hs["lm"][e], stream=hstream)
            hstream.synchronize()

        def host_step():
            S = hstream
            res.predict_members(hs["fb"], hs["lm"], hs["ov"], stream=S)
            for e in range(E):
                res.assemble(hs["ov"][e], hs["g4"][e], hs["g2"][e], hs["pr"][e], stream=S)
                res.tile_feedback(hs["g4"][e], hs["g2"][e], hs["pr"][e], tisr, hs["fb"][e], stream=S)
            for e in range(E):
                dyns[e].run_model(hs["g4"][e], hs["g2"][e], hs["f4"][e], hs["f2"][e], stream=S)
                flags[e] = dyns[e].last_safe()[0]  # one window outstanding at a time, as in EnsembleLoop
                S.synchronize()
                res.tile_local_model(hs["f4"][e], hs["f2"][e], hs["lm"][e], stream=S)

        def healthy(what, ms):
            # a window that waits for a time-out takes seconds: stop there instead of timing it
            print(f"E {E} {what}: {ms:.3f} ms / step, run_speedy {flags}", flush=True)
            if ms > 50.0 * E or not all(flags):
                sys.exit(f"E {E} {what}: {ms:.1f} ms per step, run_speedy {flags}: not a measurement")

        for d in dyns[:E]:
            d.set_state(st0)
        rec["host_sequence_ms"], rec["loop_step_ms"] = [], []
        loop = None
        if not args.loop_only:
            host_start()
            healthy("host sequence, first step", host_clock(host_step, hstream.synchronize, 1))
            host_clock(host_step, hstream.synchronize, 5)
            ms = host_clock(host_step, hstream.synchronize, 5)
            healthy("host sequence", ms)
            nsteps = max(10, min(400, int(np.ceil(args.window * 1e3 / ms))))
        if not args.host_only and not args.loop_only:
            from speedy_ml_amd.ensemble import EnsembleLoop

            set_members(E)
            loop = EnsembleLoop(res, dyns[:E], dev, tisr=tisr)
            for e in range(E):
                loop.start(e, *starts[e])
            ms = host_clock(loop.step, loop.sync, 1)
            flags[:] = loop.run_speedy()
            healthy("EnsembleLoop.step, first step", ms)
            host_clock(loop.step, loop.sync, 10)
        for _ in range(0 if args.loop_only else args.repeats):
            if loop is not None:
                rec["loop_step_ms"].append(round(host_clock(loop.step, loop.sync, nsteps), 4))
                flags[:] = loop.run_speedy()
                healthy("EnsembleLoop.step window", rec["loop_step_ms"][-1])
                loop.sync()
                res.cancel_step()  # the host sequence steps in one pass
            rec["host_sequence_ms"].append(round(host_clock(host_step, hstream.synchronize, nsteps), 4))
            healthy("host sequence window", rec["host_sequence_ms"][-1])
            if loop is not None:
                for e in range(E):  # and the loop goes on from where the host sequence left the members
                    loop.start(e, hs["g4"][e], hs["g2"][e], hs["pr"][e], hs["f4"][e], hs["f2"][e])
        rec["run_speedy"] = [bool(f) for f in (loop.run_speedy() if loop is not None else flags)]
        if loop is not None:
            loop.sync()
            res.cancel_step()
            loop.close()
        if options:
            options_pair(E, rec, starts, flags, healthy)
        if args.products:
            products_pair(E, rec, starts, flags, healthy)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    med = lambda v: float(np.median(v))  # noqa: E731
    spread = lambda v: float(max(v) - min(v))  # noqa: E731
    if not args.host_only and not args.loop_only:
        print("\n| E | begin_members ms | spread | predict_members ms | spread |")
        print("|---|---|---|---|---|")
        for r in lines:
            print(f"| {r['E']} | {med(r['begin_ms']):.3f} | {spread(r['begin_ms']):.3f} | "
                  f"{med(r['step_members_ms']):.3f} | {spread(r['step_members_ms']):.3f} |")
        print("\n| E | finish + assembly, TF: ms (spread) |")
        print("|---|---|")
        for r in lines:
            cells = ", ".join(f"TF {tf}: {med(v):.4f} ({spread(v):.4f})" for tf, v in r["finish_ms"].items())
            print(f"| {r['E']} | {cells} |")
    if not args.loop_only:
        print("\n| E | EnsembleLoop.step ms | spread | host sequence ms | spread | library |")
        print("|---|---|---|---|---|---|")
        for r in lines:
            ls = r["loop_step_ms"]
            print(f"| {r['E']} | " + (f"{med(ls):.3f} | {spread(ls):.3f}" if ls else "- | -") +
                  f" | {med(r['host_sequence_ms']):.3f} | {spread(r['host_sequence_ms']):.3f} | {r['lib']} |")
    if options:
        on = ", ".join(k for k in ("slab", "calendar", "tisr_table") if getattr(args, k))
        print(f"\n| E | plain EnsembleLoop.step ms | spread | with {on} ms | spread | difference ms |")
        print("|---|---|---|---|---|---|")
        for r in lines:
            a, b = r["plain_ms"], r["options_ms"]
            print(f"| {r['E']} | {med(a):.3f} | {spread(a):.3f} | {med(b):.3f} | {spread(b):.3f} | "
                  f"{med(b) - med(a):+.3f} |")
    if args.products:
        print("\n| E | products off ms | spread | products on ms | spread | difference ms | own launches ms | bytes / 8 TB/s ms | library |")
        print("|---|---|---|---|---|---|---|---|---|")
        for r in lines:
            a, b = r["products_off_ms"], r["products_on_ms"]
            if b:
                own = r["products_launch_ms"]
                print(f"| {r['E']} | {med(a):.3f} | {spread(a):.3f} | {med(b):.3f} | {spread(b):.3f} | "
                      f"{med(b) - med(a):+.3f} | {med(own):.4f} | {r['products_bytes'] / 8e9:.4f} | {r['lib']} |")
            else:
                print(f"| {r['E']} | {med(a):.3f} | {spread(a):.3f} | - | - | - | - | - | {r['lib']} |")
    hstream.synchronize()
    check(lib().sml_stream_destroy(hh))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

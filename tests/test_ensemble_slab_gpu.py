"""The E-member hybrid loop with the slab ocean, run_model's calendar and the tisr table
(speedy_ml_amd.ensemble.EnsembleLoop, the sml_slab_* stage, sml_res_tile_*_members) against
single-member HybridLoops with the same options, bit for bit.

Shapes are tests/test_slab_gpu.py::test_slab_loop_date_forcing's: all 1152 regions at n 96, the
1027 slab reservoirs at n 200, nleap 2, timestep_slab 24 h (a ring of 3 columns, a slab step
every 4th step), the calendar from 1981-02-27 06 h.  E = 3: one full member tile of 2 and a
partial one.  Every member has its own start grids, reservoir states, slab states and slab
start outvec.  No tolerance anywhere: tests/test_slab_gpu.py holds the single-member loop to
the oracle chain, and bitwise equality with that loop carries the parity to every member.

The weights, the device contexts and the single-member references are built once for the
module and shared; the references are never modified."""
import ctypes

import numpy as np
import pytest

from speedy_ml_amd import domain
from speedy_ml_amd.synthetic import initial_state, region_weights, slab_fields, slab_start_outvec, slab_weights

pytestmark = pytest.mark.gpu

E = 3
KEYS = ("ov", "g4", "g2", "pr", "fb", "f4", "f2", "lm")
SLAB_KEYS = ("sst", "ring", "feedback", "outvec")
PROBE = (0, 500, 1151)
CAL = (1981, 24 * 58 + 6)  # 9 steps: two slab steps, three wraps of the ring, a day and the month boundary
# the table run starts in a leap year (1984: the calendar's February latch sets at the first
# lookup) at 02-28 12 h, so that its 5 steps cross into the 29th the latch gives February
TABLE_CAL = (1981, 3 * 8760 + 24 * 59 + 12)


class World:
    """Host weights and fields, the device contexts (one member and E members), and the
    single-member reference runs, each computed once."""

    def __init__(self, cuda):
        import torch

        from speedy_ml_amd.reservoir import Reservoirs

        self.cuda = cuda
        self.t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
        self.mask = domain.load_sst_mask()
        self.ws = [region_weights(r, bool(self.mask[r]), climatology=True, n_override=96) for r in range(1152)]
        self.sreg = [r for r in range(1152) if self.mask[r]]
        self.sws = [slab_weights(r, n_override=200) for r in self.sreg]
        self.sprobe = (0, len(self.sreg) // 2, len(self.sreg) - 1)
        self.base, self.smask, self.sice, self.tice = slab_fields()
        self.d_base, self.d_mask = self.t(self.base), self.t(self.smask)
        self.tisr = self.t(np.random.default_rng(13).standard_normal((1152, 16)))
        self._table = None
        self._refs = {}

        def atmo(members):
            res = Reservoirs(list(range(1152)), self.mask, [w.n for w in self.ws], [w.k for w in self.ws])
            for i, w in enumerate(self.ws):
                res.load_region_weights(i, w)
            res.set_members(members)
            return res

        def slab(members):
            res = Reservoirs(self.sreg, [0] * len(self.sreg), [w.n for w in self.sws], [w.k for w in self.sws],
                             chunk_speedy=0, nout=4, ninp=[w.ninp for w in self.sws], out_index=[35] * 4)
            for j, w in enumerate(self.sws):
                res.load_region_weights(j, w)
            res.set_members(members)
            return res

        self.single, self.sslab = atmo(1), slab(1)
        self.res, self.slab = atmo(E), slab(E)

    def close(self):
        for c in (self.single, self.sslab, self.res, self.slab):
            c.close()

    def table(self):
        if self._table is None:
            self._table = self.t(300.0 + 100.0 * np.random.default_rng(21).random((8760, 48, 96)))
        return self._table

    def ocean(self, slab):
        from speedy_ml_amd.hybrid import SlabOcean

        return SlabOcean(slab, self.d_base, self.d_mask, timestep=6, timestep_slab=24)

    def dynamics(self):
        """A SPEEDY model with the date-driven forcing on, as tests/test_slab_gpu.py::_run's."""
        from speedy_ml_amd._lib import check, lib, ptr
        from speedy_ml_amd.dynamics import Dynamics
        from speedy_ml_amd.synthetic import dyn_state, phys_boundary, surface_climatology

        st0, forcing = dyn_state()
        dyn = Dynamics()
        dyn.set_forcing(**forcing)
        dyn.set_state(st0)
        bc = phys_boundary(dyn, forcing["phis"])
        surf, clim = surface_climatology(bc["fmask1"])
        bc["fmask1"] = surf["fmask_l"]
        dyn.set_physics(bc)
        check(lib().sml_dyn_set_sea_ice(dyn._h, ptr(np.ascontiguousarray(self.sice)),
                                        ptr(np.ascontiguousarray(self.tice))))
        dyn.set_surface(surf)
        dyn.set_climatology(clim)
        return dyn

    def grids(self, e):
        from speedy_ml_amd.synthetic import synthetic_grids

        g4, g2, pr = synthetic_grids(11 + 10 * e)
        f4, f2, _ = synthetic_grids(12 + 10 * e)
        return [self.t(a) for a in (g4, g2, pr, f4, f2)]

    def slab_start(self, e):
        return self.t(np.stack([slab_start_outvec(r, seed=88 + e) for r in self.sreg]))

    def set_states(self, res, slab, e, member):
        """Member e's own atmo and slab reservoir states into `member` of the contexts."""
        for i, w in enumerate(self.ws):
            res.set_state(i, initial_state(w.region, w.n, seed=99 + e), member=member)
        for j, w in enumerate(self.sws):
            slab.set_state(j, initial_state(self.sreg[j], w.n, seed=17 + e), member=member)

    def reference(self, table):
        """Member e = 0 .. E - 1 on a serial single-member HybridLoop of its own: per step its
        buffers and slab state, then the probed states and the fordate count."""
        if table in self._refs:
            return self._refs[table]
        import torch

        from speedy_ml_amd.exchange import OutvecExchange
        from speedy_ml_amd.hybrid import HybridLoop

        steps, cal = (5, TABLE_CAL) if table else (9, CAL)
        out = []
        for e in range(E):
            self.set_states(self.single, self.sslab, e, member=0)
            dyn = self.dynamics()
            loop = HybridLoop(self.single, dyn, OutvecExchange(1152, 1, 0, device=self.cuda), self.cuda,
                              tisr=self.tisr, overlap=False, nleap=2, slab=self.ocean(self.sslab))
            assert loop.exchange_width == 140
            if table:
                loop.set_tisr_table(self.table(), cal[0], cal[1], 6)
            loop.set_calendar(cal[0], cal[1], 6)
            loop.start(*self.grids(e))
            loop.start_slab(self.slab_start(e))
            loop.sync()
            snaps, dates = [], []
            for _ in range(steps):
                dates.append(loop.window_date())
                loop.step()
                loop.sync()
                torch.cuda.synchronize()
                assert loop.run_speedy()
                snap = {k: getattr(loop, k).cpu().numpy().copy() for k in KEYS}
                snap.update(loop.slab_state())
                snaps.append(snap)
            out.append({"snaps": snaps, "dates": dates, "x": [self.single.get_state(i) for i in PROBE],
                        "sx": [self.sslab.get_state(j) for j in self.sprobe], "fordate": dyn.fordate_count()})
            loop.close()
            dyn.close()
            torch.cuda.synchronize()
        self._refs[table] = out
        return out


@pytest.fixture(scope="module")
def world(cuda):
    w = World(cuda)
    yield w
    w.close()


def _run_ensemble(w, res, slab, members, table):
    """EnsembleLoop over `members` (the references' member numbers) on (res, slab), compared
    with the references after every step; returns the last step's buffers."""
    import torch

    from speedy_ml_amd.ensemble import EnsembleLoop

    ref = w.reference(table)
    steps, cal = (5, TABLE_CAL) if table else (9, CAL)
    n = len(members)
    for k, e in enumerate(members):
        w.set_states(res, slab, e, member=k)
    dyns = [w.dynamics() for _ in members]
    ens = EnsembleLoop(res, dyns, w.cuda, tisr=w.tisr, nleap=2, slab=w.ocean(slab))
    assert ens.exchange_width == 140 and tuple(ens.ov.shape) == (n, 1152, 140)
    if table:
        ens.set_tisr_table(w.table(), cal[0], cal[1], 6)
    ens.set_calendar(cal[0], cal[1], 6)
    for k, e in enumerate(members):
        ens.start(k, *w.grids(e))
        ens.start_slab(k, w.slab_start(e))
    for s in range(steps):
        assert ens.window_date() == ref[members[0]]["dates"][s]
        ens.step()
        ens.sync()
        torch.cuda.synchronize()
        assert ens.run_speedy() == [True] * n, f"step {s}: {ens.run_speedy()}"
        got = {k: getattr(ens, k).cpu().numpy() for k in KEYS}
        for k, e in enumerate(members):
            want = ref[e]["snaps"]
            for key in KEYS[:-1]:
                np.testing.assert_array_equal(got[key][k], want[s][key], err_msg=f"step {s} member {e} {key}")
            if s >= 1:  # lm is written by the next finish: one step late
                np.testing.assert_array_equal(got["lm"][k], want[s - 1]["lm"], err_msg=f"step {s} member {e} lm")
            state = ens.slab_state(k)
            for key in SLAB_KEYS:
                # (the single-member loop's slab feedback is unwritten memory until its first
                # slab step, the 4th: there is nothing to compare before that)
                if key != "feedback" or s >= 3:
                    np.testing.assert_array_equal(state[key], want[s][key], err_msg=f"step {s} member {e} slab {key}")
    # the atmo states run one update ahead; rolled back they are the serial loops'
    assert res.step_begun()
    ens.cancel_step()
    assert not res.step_begun()
    for k, e in enumerate(members):
        for j, i in enumerate(PROBE):
            np.testing.assert_array_equal(res.get_state(i, member=k), ref[e]["x"][j], err_msg=f"member {e} region {i}")
        for j, i in enumerate(w.sprobe):
            np.testing.assert_array_equal(slab.get_state(i, member=k), ref[e]["sx"][j], err_msg=f"member {e} slab {i}")
        assert dyns[k].fordate_count() == ref[e]["fordate"], (e, dyns[k].fordate_count(), ref[e]["fordate"])
    got["sst"] = np.stack([ens.slab_state(k)["sst"] for k in range(n)])
    assert np.isfinite(got["f4"]).all() and np.isfinite(got["f2"]).all() and np.isfinite(got["ov"]).all()
    assert all(np.abs(got["f4"][k]).max() > 0 for k in range(n))
    ens.close()
    for d in dyns:
        d.close()
    torch.cuda.synchronize()
    return got


def test_ensemble_slab_loop_is_bitwise_the_single_member_loops(world):
    """E = 3 over 9 steps with the slab ocean and the calendar: after every step every member's
    ov (all 140 columns), g4, g2, pr, fb, f4, f2, lm (one step late) and slab state (sst grid,
    ring, slab feedback, slab outvecs) are its serial HybridLoop's; after cancel_step so are
    the probed atmo and slab reservoir states; the fordate counts agree; every run_speedy flag
    is true; the last forecast is finite and nonzero; members 0 and 1 end with different SSTs."""
    ref = world.reference(False)
    dates = ref[0]["dates"]
    assert len({d[:3] for d in dates}) >= 3 and {d[1] for d in dates} == {2, 3}, dates  # a day and the month boundary
    assert sum((s * 6) % 24 == 0 for s in range(1, 10)) == 2  # two slab steps
    got = _run_ensemble(world, world.res, world.slab, (0, 1, 2), table=False)
    assert not np.array_equal(got["sst"][0], got["sst"][1])
    assert not np.array_equal(got["f4"][0], got["f4"][1]) and not np.array_equal(got["f4"][1], got["f4"][2])


def test_ensemble_tisr_table_is_bitwise_the_single_member_loops(world):
    """The same comparison over 5 steps with get_tisr_by_date from a table shared by the
    members, across 28 / 29 February of a leap year (the calendar's February latch, which the
    date and the table lookups share, sets at the first lookup)."""
    dates = world.reference(True)[0]["dates"]
    assert (1984, 2, 28) in {d[:3] for d in dates} and (1984, 2, 29) in {d[:3] for d in dates}, dates
    _run_ensemble(world, world.res, world.slab, (0, 1, 2), table=True)


def test_one_member_ensemble_with_the_slab(world):
    """E = 1 (the single-member kernels behind the members calls) against the same HybridLoop."""
    _run_ensemble(world, world.single, world.sslab, (0,), table=False)


def _slab_handle(w):
    from speedy_ml_amd._lib import check, lib, ptr

    h = ctypes.c_void_p()
    check(lib().sml_slab_create(w.res.handle, w.slab.handle, ptr(w.d_base), ptr(w.d_mask), 6, 24, 0.0, ctypes.byref(h)))
    return h


def _buffers(w, h, e_count):
    """Host copies of the stage's own buffers [E, ...]."""
    from speedy_ml_amd._lib import check, lib, ptr

    p = [ctypes.c_void_p() for _ in range(4)]
    st = [ctypes.c_int64() for _ in range(4)]
    check(lib().sml_slab_buffers(h, *[ctypes.byref(x) for pair in zip(p, st) for x in pair]))
    cols, n = ctypes.c_int(), ctypes.c_int()
    check(lib().sml_slab_info(h, None, None, None, ctypes.byref(cols), ctypes.byref(n), None))
    shapes = {"sst": (48, 96), "ring": (cols.value, n.value), "feedback": (n.value,), "outvec": (len(w.sreg), 4)}
    out = {}
    for (key, shape), src, stride in zip(shapes.items(), p, st):
        assert stride.value >= int(np.prod(shape)), key  # member strides in doubles, checked against the packed size
        a = np.zeros((e_count,) + shape)
        for e in range(e_count):
            check(lib().sml_copy_to_host(ptr(a[e]), ctypes.c_void_p(src.value + 8 * e * stride.value), a[e].nbytes))
        out[key] = a
    return out


def test_slab_stage_through_the_c_abi(world):
    """sml_slab_start / _sst / _ring / _predict on their own, the members' outvecs and
    feedbacks with strides larger than packed.  A NaN in one member's slab outvec reaches only
    that member's sst grid, at that region's point, and only the feedback entries whose
    overlap tile holds that point; regions without sst read exactly 272 K; land points read
    base_sst; values below 272 K are floored; nothing but the sst entries of the feedbacks and
    the sst columns of the outvecs is written; the ring column and the ring mean are the
    plain gathers and column-by-column sums."""
    import torch

    from speedy_ml_amd._lib import SmlError, check, lib, ptr

    w, L = world, lib()
    h = _slab_handle(w)
    assert w.res.members == E
    tot = int(w.res.fb_offsets[-1])
    ovs, fbs = 1152 * 140 + 13, tot + 7
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ov = torch.full((E, ovs), -5.0, dtype=torch.float64, device=w.cuda)
    rng = np.random.default_rng(3)
    fb_h = rng.standard_normal((E, fbs))
    fb = w.t(fb_h)
    with pytest.raises(SmlError, match="ov_stride"):
        check(L.sml_slab_start(h, 0, ptr(w.slab_start(0)), ptr(ov), 1152 * 140 - 1, stream))
    with pytest.raises(SmlError, match="out of range"):
        check(L.sml_slab_start(h, E, ptr(w.slab_start(0)), ptr(ov), ovs, stream))
    with pytest.raises(SmlError, match="sml_slab_start of member 0 first"):
        check(L.sml_slab_predict(h, 4, ptr(ov), ovs, stream, None))
    # a sea region and its point for the NaN, another for a value below the floor
    sea = [j for j, r in enumerate(w.sreg) if 200 < r < 900 and not w.smask[_points(r)].any()]
    jn, jf = sea[0], sea[len(sea) // 2]
    sov = np.stack([np.stack([slab_start_outvec(r, seed=88 + e) for r in w.sreg]) for e in range(E)])
    sov[1, jn, 2] = np.nan
    sov[2, jf, 1] = 250.0
    for e in range(E):
        check(L.sml_slab_start(h, e, ptr(w.t(sov[e])), ptr(ov), ovs, stream))
    wrote = ctypes.c_int(-1)
    with pytest.raises(SmlError, match="fb_stride"):
        check(L.sml_slab_sst(h, ptr(ov), ovs, ptr(fb), tot - 1, stream, ctypes.byref(wrote)))
    check(L.sml_slab_sst(h, ptr(ov), ovs, ptr(fb), fbs, stream, ctypes.byref(wrote)))
    assert wrote.value == 1
    check(L.sml_slab_sst(h, ptr(ov), ovs, ptr(fb), fbs, stream, ctypes.byref(wrote)))
    assert wrote.value == 0  # nothing changed since
    torch.cuda.synchronize()
    got = _buffers(w, h, E)
    ov_h = ov.cpu().numpy()
    rows = ov_h[:, :1152 * 140].reshape(E, 1152, 140)
    np.testing.assert_array_equal(rows[:, :, :136], -5.0)  # the outvec proper is not the stage's
    np.testing.assert_array_equal(ov_h[:, 1152 * 140:], -5.0)  # nor the padding
    nosst = [r for r in range(1152) if not w.mask[r]]
    np.testing.assert_array_equal(rows[:, nosst, 136:], 272.0)
    np.testing.assert_array_equal(rows[:, w.sreg, 136:], sov)
    np.testing.assert_array_equal(got["outvec"], sov)
    np.testing.assert_array_equal(got["ring"], 0.0)
    # wholegrid_sst of every member, from the region geometry
    yy, xx, rr, cc = _grid_index()
    land = w.smask > 0.0
    ms = np.array([[sw.mean[35], sw.std[35]] for sw in w.sws])
    o = w.res.fb_offsets
    want_fb = fb_h.copy()
    for e in range(E):
        sst = np.empty((48, 96))
        sst[yy, xx] = rows[e, rr, 136 + cc]
        sst = np.where(land, w.base, sst)
        sst = np.where(sst < 272.0, 272.0, sst)
        np.testing.assert_array_equal(got["sst"][e], sst, err_msg=f"member {e} sst grid")
        np.testing.assert_array_equal(got["sst"][e][land], w.base[land])
        for j, r in enumerate(w.sreg):
            g = domain.region_geometry(r)
            in2d = g.inx * g.iny
            tile = np.array([sst[g.in_ystart - 1 + p // g.inx, g.input_x(p % g.inx + 1) - 1] for p in range(in2d)])
            at = o[r] + 32 * in2d + 2 * in2d
            want_fb[e, at:at + in2d] = (tile - ms[j, 0]) / ms[j, 1]
    np.testing.assert_array_equal(fb.cpu().numpy(), want_fb)  # the sst entries, and nothing else
    # the NaN: one point of member 1's grid, none of the others'; the floor: member 2's point
    gn, gf = domain.region_geometry(w.sreg[jn]), domain.region_geometry(w.sreg[jf])
    nan_at = np.argwhere(np.isnan(got["sst"]))
    assert nan_at.tolist() == [[1, gn.res_ystart - 1 + 1, gn.res_xstart - 1 + 0]], nan_at  # column 2 = (lx 0, ly 1)
    assert got["sst"][2, gf.res_ystart - 1, gf.res_xstart - 1 + 1] == 272.0
    assert not np.isnan(want_fb[0]).any() and not np.isnan(want_fb[2]).any()
    assert 1 <= np.isnan(want_fb[1]).sum() <= 9  # the overlap tiles of the region and its neighbours that hold the point
    # the ring's columns: gathers of the atmo feedbacks; the ring mean on a slab step
    idx = np.concatenate([o[r] + _slab_input_index(r) for r in w.sreg])
    fbs_h = []
    for t in (1, 2, 3):
        fb_t = rng.standard_normal((E, fbs))
        fbs_h.append(fb_t)
        check(L.sml_slab_ring(h, t, ptr(w.t(fb_t)), fbs, stream))
    predicted = ctypes.c_int(-1)
    check(L.sml_slab_predict(h, 3, ptr(ov), ovs, stream, ctypes.byref(predicted)))
    assert predicted.value == 0
    for e in range(E):
        for j in w.sprobe:
            w.slab.set_state(j, initial_state(w.sreg[j], w.sws[j].n, seed=17 + e), member=e)
    check(L.sml_slab_predict(h, 4, ptr(ov), ovs, stream, ctypes.byref(predicted)))
    assert predicted.value == 1
    torch.cuda.synchronize()
    got = _buffers(w, h, E)
    for e in range(E):
        for c in range(3):
            np.testing.assert_array_equal(got["ring"][e, c], fbs_h[c][e, idx], err_msg=f"member {e} ring column {c}")
        acc = np.zeros(len(idx))
        for c in range(3):
            acc = acc + got["ring"][e, c]
        np.testing.assert_array_equal(got["feedback"][e], acc / 3.0, err_msg=f"member {e} ring mean")
    rows = ov.cpu().numpy()[:, :1152 * 140].reshape(E, 1152, 140)
    np.testing.assert_array_equal(rows[:, w.sreg, 136:], got["outvec"])  # the new sst in the exchange rows
    np.testing.assert_array_equal(rows[:, nosst, 136:], 272.0)
    np.testing.assert_array_equal(rows[:, :, :136], -5.0)
    assert np.isfinite(got["outvec"]).all() and not np.array_equal(got["outvec"], sov)
    check(L.sml_slab_sst(h, ptr(ov), ovs, ptr(fb), fbs, stream, ctypes.byref(wrote)))
    assert wrote.value == 1
    torch.cuda.synchronize()
    check(L.sml_slab_destroy(h))


def _points(r):
    """(rows, columns) of region r's own points in a [48, 96] grid."""
    g = domain.region_geometry(r)
    ys = np.arange(g.res_ystart - 1, g.res_yend)
    xs = np.arange(g.res_xstart - 1, g.res_xend)
    return np.repeat(ys, len(xs)), np.tile(xs, len(ys))


def _grid_index():
    """For every point of every region: its grid row and column, the region, and its sst
    column lx + resx * ly in the region's exchange row."""
    yy, xx, rr, cc = [], [], [], []
    for r in range(1152):
        g = domain.region_geometry(r)
        y, x = _points(r)
        yy.append(y)
        xx.append(x)
        rr.append(np.full(len(y), r))
        cc.append((x - (g.res_xstart - 1)) + g.resx * (y - (g.res_ystart - 1)))
    return tuple(np.concatenate(a) for a in (yy, xx, rr, cc))


def _slab_input_index(r):
    """atmo_training_data_idx of region r's feedback: the lowest level's four variables, logp,
    the sst and the tisr (not the precipitation)."""
    g = domain.region_geometry(r)
    in2d = g.inx * g.iny
    natmo = 32 * in2d
    return np.concatenate([np.arange(natmo - 4 * in2d, natmo + in2d), np.arange(natmo + 2 * in2d, natmo + 4 * in2d)])


def test_member_tilings_are_bitwise_the_single_calls(world):
    """sml_res_tile_feedback_members / sml_res_tile_tisr_field_members in one launch against E
    single calls, with member strides larger than packed and with a null tisr; the sst entries
    and the padding are left alone."""
    import torch

    from speedy_ml_amd._lib import SmlError, check, lib, ptr
    from speedy_ml_amd.synthetic import synthetic_grids

    w, res = world, world.res
    tot = int(res.fb_offsets[-1])
    pad = lambda a, extra: torch.cat([a, torch.full((E, extra), 9.5, dtype=torch.float64, device=w.cuda)], 1)  # noqa: E731
    gs = [synthetic_grids(31 + e) for e in range(E)]
    g4 = pad(w.t(np.stack([g[0].ravel() for g in gs])), 24)
    g2 = pad(w.t(np.stack([g[1].ravel() for g in gs])), 8)
    pr = pad(w.t(np.stack([g[2].ravel() for g in gs])), 8)
    field = w.t(300.0 + 100.0 * np.random.default_rng(8).random((48, 96)))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for tisr in (w.tisr, None):
        fb = torch.full((E, tot + 11), 3.25, dtype=torch.float64, device=w.cuda)
        want = torch.full((E, tot + 11), 3.25, dtype=torch.float64, device=w.cuda)
        check(lib().sml_res_tile_feedback_members(res.handle, ptr(g4), g4.stride(0), ptr(g2), ptr(pr), g2.stride(0),
                                                  ptr(tisr), ptr(fb), fb.stride(0), stream))
        for e in range(E):
            res.tile_feedback(g4[e], g2[e], pr[e], tisr, want[e])
        torch.cuda.synchronize()
        np.testing.assert_array_equal(fb.cpu().numpy(), want.cpu().numpy())
        kept = (fb == 3.25).sum(1).cpu().numpy()  # the padding, the sst entries and, without a tisr, the tisr entries
        assert (kept > 11).all() and (kept < tot).all()
        check(lib().sml_res_tile_tisr_field_members(res.handle, ptr(field), ptr(fb), fb.stride(0), stream))
        for e in range(E):
            check(lib().sml_res_tile_tisr_field(res.handle, ptr(field), ptr(want[e]), stream))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(fb.cpu().numpy(), want.cpu().numpy())
        assert (fb[:, tot:] == 3.25).all()
    # the wrapper on [E, ...] tensors gives the same
    fb2 = torch.full((E, tot + 11), 3.25, dtype=torch.float64, device=w.cuda)
    res.tile_feedback_members(g4[:, :147456].reshape(E, 8, 48, 96, 4), g2[:, :4608].reshape(E, 48, 96),
                              pr[:, :4608].reshape(E, 48, 96), None, fb2)
    res.tile_tisr_field_members(field, fb2)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(fb2.cpu().numpy(), fb.cpu().numpy())
    for bad in ("g4", "g2", "fb"):
        s4, s2, sf = (147455 if bad == "g4" else g4.stride(0), 4607 if bad == "g2" else g2.stride(0),
                      tot - 1 if bad == "fb" else fb.stride(0))
        with pytest.raises(SmlError, match="stride"):
            check(lib().sml_res_tile_feedback_members(res.handle, ptr(g4), s4, ptr(g2), ptr(pr), s2, None, ptr(fb),
                                                      sf, stream))
    with pytest.raises(SmlError, match="fb_stride"):
        check(lib().sml_res_tile_tisr_field_members(res.handle, ptr(field), ptr(fb), tot - 1, stream))


def test_ensemble_loop_refusals(world):
    """A slab context whose member count is not E, start_slab before start, step before every
    member's start_slab (again after a restart), a table index outside the table, a table
    shorter than a year, window_date without a calendar: refused with the reason."""
    import torch

    from speedy_ml_amd.ensemble import EnsembleLoop

    w = world
    dyns = [w.dynamics() for _ in range(E)]
    with pytest.raises(ValueError, match="members"):
        EnsembleLoop(w.res, dyns, w.cuda, tisr=w.tisr, nleap=2, slab=w.ocean(w.sslab))
    ens = EnsembleLoop(w.res, dyns, w.cuda, tisr=w.tisr, nleap=2, slab=w.ocean(w.slab))
    with pytest.raises(RuntimeError, match="no calendar"):
        ens.window_date()
    with pytest.raises(ValueError, match="8760"):
        ens.set_tisr_table(w.table()[:100], 1981, 0)
    with pytest.raises(RuntimeError, match="before its start"):
        ens.start_slab(0, w.slab_start(0))
    with pytest.raises(ValueError, match="out of range"):
        ens.start_slab(E, w.slab_start(0))
    for k in range(E):
        w.set_states(w.res, w.slab, k, member=k)
        ens.start(k, *w.grids(k))
    for k in range(E - 1):
        ens.start_slab(k, w.slab_start(k))
    with pytest.raises(RuntimeError, match="start_slab"):
        ens.step()
    ens.start_slab(E - 1, w.slab_start(E - 1))
    # a table index outside the table.  set_tisr_table refuses a table shorter than a year, as
    # the native loop does, and the reference's index wraps past 8760, so no table that the
    # setter accepts can be missed; the step's own guard is shown by shortening the table
    # behind the setter.  It refuses before anything is launched: the step count is unchanged.
    ens.set_tisr_table(w.table(), TABLE_CAL[0], TABLE_CAL[1])
    ens._table = w.table()[:100]
    with pytest.raises(ValueError, match="outside the table's 100 hours"):
        ens.step()
    assert ens.t == 0 and w.res.step_begun()
    # a restart needs every member's slab started again
    ens.set_tisr_table(None, 1981, CAL[1])
    ens.set_calendar(CAL[0], CAL[1], 6)
    ens.start(0, *w.grids(0))
    for k in range(1, E):
        ens.start(k, *w.grids(k))
    with pytest.raises(RuntimeError, match="start_slab"):
        ens.step()
    for k in range(E):
        ens.start_slab(k, w.slab_start(k))
    ens.step()
    ens.sync()
    torch.cuda.synchronize()
    assert ens.run_speedy() == [True] * E and ens.t == 1
    ens.cancel_step()
    ens.close()
    for d in dyns:
        d.close()
    torch.cuda.synchronize()

"""Generate tests/golden/phys_edges_ref.npz and phys_edges_ref_b.npz (one file per case,
each within the size limit of a committed file): the reference's own phypar on the state
fixture of tests/_phys_edges.py (a polar cap and a plateau with psg near 0.6, a cold
top, a hot surface, a dry region, saturated levels, a hot saturated boundary layer),
so that the oracle is pinned to the reference on the branches that phys_ref.npz's
synthetic state never takes.

Run in the survey/build container after `make -C oracle ref`:

    python tests/golden/make_phys_edges_golden.py

Drives oracle/_ref/libspeedy_ref_dyn.so like make_phys_golden.py: reference
initialisation (inifft, indyns, inphys, radset), sol_oz(tyear of phys_ref.npz), the
fixture's boundary fields written into the reference's modules, then
  * case "a": S_A, lradsw = .true.  -> geop(1), phypar with zero input tendencies;
  * case "b": S_B (its own boundary fields), lradsw = .false. on the radiation state
    that "a" left in the reference's modules.
Stored at every 4th longitude (all latitudes), as in phys_ref.npz: the grid inputs
phypar computed (mod_physvar ug1..pslg1), its tendencies, and after "a" the radiation
state.  phypar clips its qg1 in place (phy_phypar.f90:87), so the stored qg1 is
max(q, 0).  The spectral states themselves are not stored: tests/_phys_edges.py rebuilds
them from its seeds, and the tests hold the oracle's phys_inputs to the stored ones.
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _path in (HERE, os.path.join(REPO, "tests"), os.path.join(REPO, "oracle"), os.path.join(REPO, "speedy-ml-1_amd")):
    if _path not in sys.path:
        sys.path.insert(0, _path)
from make_dyn_golden import IL, IX, KX, MX, NX, Ref, _int, _p  # noqa: E402

import _phys_edges as pe  # noqa: E402

NGP = IX * IL
PATHS = {"a": os.path.join(HERE, "phys_edges_ref.npz"), "b": os.path.join(HERE, "phys_edges_ref_b.npz")}


def main():
    R = Ref()
    L = R.L
    pg = pe.golden("phys_ref.npz")
    L.inifft_()
    L.indyns_()
    hsg = R.var("mod_dyncon1", "hsg", (KX + 1,))
    fsg = R.var("mod_dyncon1", "fsg", (KX,))
    radang = R.var("mod_dyncon1", "radang", (IL,))
    ppl = np.ascontiguousarray(fsg.copy())
    L.inphys_(_p(hsg), _p(ppl), _p(radang))
    L.radset_()
    ty = ctypes.c_double(float(pg["tyear"]))
    L.sol_oz_(ctypes.byref(ty))

    vor = R.var("mod_dynvar", "vor", (MX, NX, KX, 2), np.complex128)
    div = R.var("mod_dynvar", "div", (MX, NX, KX, 2), np.complex128)
    t = R.var("mod_dynvar", "t", (MX, NX, KX, 2), np.complex128)
    ps = R.var("mod_dynvar", "ps", (MX, NX, 2), np.complex128)
    tr = R.var("mod_dynvar", "tr", (MX, NX, KX, 2, 1), np.complex128)
    phi = R.var("mod_dynvar", "phi", (MX, NX, KX), np.complex128)
    phis = R.var("mod_dynvar", "phis", (MX, NX), np.complex128)

    def load(s):
        st, bc = s["state"], s["bc"]
        vor[...] = st["vor"].transpose(3, 2, 1, 0)
        div[...] = st["div"].transpose(3, 2, 1, 0)
        t[...] = st["t"].transpose(3, 2, 1, 0)
        tr[..., 0] = st["tr"].transpose(3, 2, 1, 0)
        ps[...] = st["ps"].transpose(2, 1, 0)
        phis[...] = s["forcing"]["phis"].T
        for name in ("fmask1", "phis0"):
            R.var("mod_surfcon", name, (IX, IL))[...] = bc[name].reshape(IL, IX).T
        for name, mod in (("sst_am", "mod_var_sea"), ("stl_am", "mod_var_land"), ("soilw_am", "mod_var_land"),
                          ("alb_l", "mod_radcon"), ("alb_s", "mod_radcon"), ("snowc", "mod_radcon"),
                          ("albsfc", "mod_radcon"), ("forog", "mod_sflcon")):
            R.var(mod, name, (NGP,))[...] = bc[name]
        R.var("mod_var_sea", "ssti_om", (NGP,))[...] = bc["sst_am"]
        for k in ("fsol", "ozone", "ozupp", "zenit", "stratz"):  # sol_oz above gave the fixture's own values
            assert np.array_equal(R.var("mod_radcon", k, (NGP,)), bc[k]), k

    def physics(lradsw):
        R.scalar_logical("mod_lflags", "lradsw", lradsw)
        L.geop_(_int(1))
        tend = [np.zeros((KX, IL, IX)) for _ in range(4)]
        L.phypar_(_p(vor), _p(div), _p(t), _p(tr), _p(phi), _p(ps), *[_p(x) for x in tend])
        ins = {k: R.var("mod_physvar", k, (NGP, KX)).T.copy() for k in ("ug1", "vg1", "tg1", "qg1", "phig1")}
        ins["pslg1"] = R.var("mod_physvar", "pslg1", (NGP,)).copy()
        return ins, np.stack([x.reshape(KX, NGP) for x in tend])

    sets = pe.state()
    out = {"sel": pe.SEL, "seed": np.int64(pe.STATE_SEED)}
    for case, lradsw in (("a", True), ("b", False)):
        load(sets[case.upper()])
        ins, tend = physics(lradsw)
        assert np.all(np.isfinite(tend)), case
        for k, v in ins.items():
            out[f"{case}_{k}"] = v[..., pe.SEL]
        out[f"{case}_tend"] = tend[..., pe.SEL]
        if case == "a":
            tau2 = R.var("mod_radcon", "tau2", (NGP, KX, 4)).transpose(2, 1, 0)
            out["a_tau2"] = tau2[..., pe.SEL].copy()
            out["a_stratc"] = R.var("mod_radcon", "stratc", (NGP, 2)).T[:, pe.SEL].copy()
            out["a_tt_rsw"] = R.var("mod_physvar", "tt_rsw", (NGP, KX)).T[:, pe.SEL].copy()
            out["a_ssrd"] = R.var("mod_physvar", "ssrd", (NGP,))[pe.SEL].copy()
        cb = R.var("mod_physvar", "cbmf", (NGP,))
        pl = R.var("mod_physvar", "precls", (NGP,))
        print(case, "convective columns", int((cb > 0).sum()), "lsc columns", int((pl > 0).sum()),
              "max |tend|", [float(np.abs(x).max()) for x in tend])
    for case, path in PATHS.items():
        np.savez_compressed(path, **{k: v for k, v in out.items() if k in ("sel", "seed") or k.startswith(case + "_")})
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""W_out ridge training on the GPU (libspeedyml sml_train_*).

Mirrors the reference's training tail for a batch of regions:
chunking_matmul (src/mod_reservoir.f90:1643-1699) accumulates G = S S^T and
B = T S^T over batches of time steps, fit_chunk_hybrid / fit_chunk_ml
(:1233-1332 / :1175-1231) regularise and solve through mldivide
(src/mod_linalg.f90:109-151).

Layouts (C order of the reference's Fortran arrays): per region S is
augmented_states(naug, m) == C (m, naug), T is targetdata(nout, m) == C (m, nout),
W_out is wout(nout, naug) == C (naug, nout).  Device buffers are float64 CUDA
tensors packing the regions back to back.

The front end (get_training_data: the standardisation statistics and the tiling of the
truth and the SPEEDY forecasts) runs on the device too, from a series of global grids:
fit_standardisation, tile_series, train_from_grids (sml_res_series_stats,
sml_res_set_mean_std_device, sml_res_tile_series).  The slab-ocean reservoirs train from the
same grids: slab_series, train_slab_from_grids (sml_slab_train_series, sml_res_set_target_index).

The reference never feeds a reservoir the clean input: every W_in product wraps it in
gaussian_noise_1d_function[_precip] (mod_reservoir.f90:1091-1170), the regulariser of the
free-running forecast.  noise=InputNoise(...) on train_wout, train_from_grids and
train_slab_from_grids does the same on the device (Reservoirs.input_noise), reproducibly: the
discard phase and every batch are driven by the noised blocks, the targets stay clean
(Reservoirs.train_drive(target_inputs=...)).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from ._lib import check, lib, ptr, stream_ptr

NOUT = 136


@dataclass(frozen=True)
class InputNoise:
    """The input noise of a training run (Reservoirs.set_input_noise): the reference's
    noisemag, the seed every draw is a function of, and model_parameters%precip_epsilon
    (0: precipitation entries take the plain formula, its precip_bool = .false.)."""
    noisemag: float
    seed: int
    precip_epsilon: float = 0.0


class Trainer:
    def __init__(self, naug, nout: int = NOUT):
        self.naug = [int(x) for x in naug]
        self.nout = nout
        arr = np.asarray(self.naug, dtype=np.int32)
        h = ctypes.c_void_p()
        check(lib().sml_train_create(len(self.naug), ptr(arr), nout, ctypes.byref(h)))
        self._h = h
        n = ctypes.c_int()
        check(lib().sml_train_npad(h, ctypes.byref(n)))
        self.npad = n.value

    def close(self):
        if self._h:
            lib().sml_train_destroy(self._h)
            self._h = None

    __del__ = close

    def set_panel(self, panel: int):
        """Block columns per Cholesky panel (sml_train_set_panel; default 8)."""
        check(lib().sml_train_set_panel(self._h, int(panel)))

    def reset(self, stream=None):
        check(lib().sml_train_reset(self._h, stream_ptr(stream)))

    def accumulate(self, states, targets, m: int, stream=None):
        """states: packed device tensor, sum(naug) * m doubles (region i's
        (m, naug_i) block after region i-1's); targets: len(naug) * m * nout."""
        if states.numel() != sum(self.naug) * m or targets.numel() != len(self.naug) * m * self.nout:
            raise ValueError("states / targets sizes do not match the regions and m")
        check(lib().sml_train_accumulate(self._h, ptr(states), ptr(targets), m, stream_ptr(stream)))

    def solve(self, ncs: int = 132, beta_res: float = 0.001, beta_model: float = 1.0, using_prior: bool = True,
              prior_val: float = 0.0, out=None, stream=None):
        """Regularise + solve (consumes the accumulators).  Returns (wout packed
        device tensor, per-region potrf info after synchronisation)."""
        import torch

        total = sum(self.naug) * self.nout
        if out is None:
            out = torch.empty(total, dtype=torch.float64, device="cuda")
        info = np.zeros(len(self.naug), dtype=np.int32)
        check(lib().sml_train_solve(self._h, ncs, beta_res, beta_model, int(using_prior), prior_val, ptr(out),
                                    ptr(info), stream_ptr(stream)))
        torch.cuda.synchronize()
        return out, info

    def wout_views(self, packed):
        """Per-region (naug_i, nout) views (C order == Fortran wout(nout, naug_i))."""
        views, off = [], 0
        for n in self.naug:
            views.append(packed[off:off + n * self.nout].view(n, self.nout))
            off += n * self.nout
        return views

    def gram(self, i: int):
        """Host copies: G (npad, npad) lower triangle valid (C order = transposed
        Fortran), B as (nout, npad) C order = B(j, o) at j + npad*o."""
        G = np.zeros((self.npad, self.npad))
        B = np.zeros((self.nout, self.npad))
        check(lib().sml_train_get_gram(self._h, i, ptr(G), ptr(B)))
        return G, B


def _fit_wout(res, blocks, sync_chunk: int, discard: int, batch: int, nbatches: int, ncs: int, beta_res: float,
              beta_model: float, using_prior: bool, prior_val: float, dtype, device, stream, noise=None):
    """The loop train_wout and train_from_grids share: states to zero, the discard phase
    (Reservoirs.synchronize over at most sync_chunk blocks a call), per batch one
    Reservoirs.train_drive + Trainer.accumulate, then Trainer.solve.  blocks(t0, m): the
    packed input blocks t0 .. t0 + m - 1 and their model blocks (None when ncs == 0).
    With noise (an InputNoise), blocks t0 .. t0 + m - 1 are noised with t = t0 .. into one
    reused buffer (Reservoirs.input_noise) that the discard phase and the drives read; the
    drives' targets come from the clean blocks."""
    import torch

    naug = [ncs + int(n) for n in res.n]
    for i, n in enumerate(res.n):
        res.set_state(i, np.zeros(int(n)))
    if discard == 0:
        res.synchronize(blocks(0, 0)[0], 0, stream=stream)
    noisy = None
    if noise is not None:
        res.set_input_noise(noise.noisemag, noise.seed, noise.precip_epsilon)
        tot = int(res.fb_offsets[-1])
        noisy = torch.empty(max(max(min(sync_chunk, discard), batch) * tot, 1), dtype=torch.float64, device=device)
    t = 0
    while t < discard:
        m = min(sync_chunk, discard - t)
        d_in = blocks(t, m)[0]
        res.synchronize(d_in if noisy is None else res.input_noise(d_in, noisy, t, m, stream=stream), m, stream=stream)
        t += m
    tr = Trainer(naug, res.nout)
    tr.reset(stream=stream)
    states = torch.empty(sum(naug) * batch, dtype=torch.float64, device=device)
    targets = torch.empty(len(naug) * batch * res.nout, dtype=torch.float64, device=device)
    for b in range(nbatches):
        d_in, d_mod = blocks(discard + b * batch, batch)
        if noisy is None:
            res.train_drive(d_in, batch, d_mod if ncs else None, states, targets, stream=stream)
        else:
            res.input_noise(d_in, noisy, discard + b * batch, batch, stream=stream)
            res.train_drive(noisy, batch, d_mod if ncs else None, states, targets, stream=stream, target_inputs=d_in)
        tr.accumulate(states, targets, batch, stream=stream)
    packed, info = tr.solve(ncs=ncs, beta_res=beta_res, beta_model=beta_model, using_prior=using_prior,
                            prior_val=prior_val, stream=stream)
    wouts = [v.cpu().numpy().astype(dtype) for v in tr.wout_views(packed)]
    tr.close()
    return wouts, info


def train_wout(res, d_inputs, d_model, discard: int, batch: int, nbatches: int, ncs: int = 132,
               beta_res: float = 0.001, beta_model: float = 1.0, using_prior: bool = True, prior_val: float = 0.0,
               dtype=np.float32, stream=None, noise=None):
    """Train W_out of every local region of `res` (a Reservoirs with A and W_in loaded:
    genres.generate draws them and scales A to its spectral radius, gen_res + the W_in
    fill of train_reservoir) from a training series on the device: the reference's train_reservoir tail,
    reservoir_layer_chunking_hybrid + chunking_matmul + fit_chunk_hybrid
    (src/mod_reservoir.f90:1065-1173, :1643-1699, :1233-1332).

    d_inputs: (discard + batch * nbatches, total feedback) packed input blocks;
    d_model:  the same number of (nlocal, ncs) model blocks (None when ncs == 0).
    The states start at zero and run `discard` updates (Reservoirs.synchronize); batch b
    is then one Reservoirs.train_drive over blocks discard + b * batch .. + batch - 1
    followed by Trainer.accumulate; Trainer.solve closes.  noise=None uses the series as
    given; noise=InputNoise(noisemag, seed, precip_epsilon) adds the reference's input noise
    (gaussian_noise_1d_function[_precip]) on the device: block t, noised with step t, drives
    the discard phase (at most `batch` blocks a call then) and the batches, whose targets
    stay the clean blocks'.

    Returns (wouts, info): per region W_out as a float32 (ncs + n, nout) array -- C order
    of the file's wout(nout, ncs + n), NF90_REAL, ready for write_region_netcdf /
    Reservoirs.load_region -- and the per-region potrf info.  dtype=np.float64 keeps
    the solve's own precision (the float32 arrays are its rounding)."""
    if ncs != res.ncs:
        raise ValueError(f"ncs {ncs} differs from the context's chunk_speedy {res.ncs}")
    nblocks = discard + batch * nbatches
    tot = int(res.fb_offsets[-1])
    d_inputs = d_inputs.reshape(-1)
    if d_inputs.numel() < nblocks * tot:
        raise ValueError("d_inputs holds fewer than discard + batch * nbatches input blocks")
    nmod = res.nlocal * ncs
    if ncs:
        d_model = d_model.reshape(-1)
        if d_model.numel() < nblocks * nmod:
            raise ValueError("d_model holds fewer than discard + batch * nbatches model blocks")

    def blocks(t0, m):
        return d_inputs[t0 * tot:], (d_model[t0 * nmod:] if ncs else None)

    return _fit_wout(res, blocks, max(discard, 1) if noise is None else max(batch, 1), discard, batch, nbatches, ncs,
                     beta_res, beta_model, using_prior, prior_val, dtype, d_inputs.device, stream, noise=noise)


# ---- from a series of global grids (sml_res_series_stats, sml_res_tile_series)
G4_SHAPE, G2_SHAPE = (8, 48, 96, 4), (48, 96)


def _series(t, what, shape):
    """A float64 device series [T, *shape] whose steps are dense: (T, its step stride)."""
    import torch

    if t.dtype != torch.float64 or not t.is_cuda:
        raise ValueError(f"{what}: a float64 device tensor expected")
    if t.dim() != len(shape) + 1 or tuple(t.shape[1:]) != tuple(shape) or t.shape[0] < 1:
        raise ValueError(f"{what}: shape (T,) + {tuple(shape)} expected, got {tuple(t.shape)}")
    if not t[0].is_contiguous():
        raise ValueError(f"{what}: a step's grid must be packed, got strides {t.stride()}")
    packed = int(np.prod(shape))
    stride = int(t.stride(0)) if t.shape[0] > 1 else packed
    if stride < packed:
        raise ValueError(f"{what}: the step stride {stride} is below the packed {packed}")
    return int(t.shape[0]), stride


def _truth_series(g4, g2, pr, sst, tisr):
    """(T, g4 stride, common stride of the 2-d series)."""
    T, s4 = _series(g4, "g4", G4_SHAPE)
    s2 = None
    for name, a in (("g2", g2), ("pr", pr), ("sst", sst), ("tisr", tisr)):
        if a is None:
            continue
        Ta, sa = _series(a, name, G2_SHAPE)
        if Ta != T:
            raise ValueError(f"{name}: {Ta} steps, g4 has {T}")
        if T > 1 and s2 is not None and sa != s2:
            raise ValueError(f"{name}: step stride {sa}, the 2-d series share one ({s2})")
        s2 = sa if s2 is None else s2
    return T, s4, s2


def series_stats(res, g4, g2, pr, sst=None, tisr=None, stream=None):
    """sml_res_series_stats: the [nlocal, 72] device table (mean then std per region) and
    the [nlocal] device int32 sst_change of a series g4 [T, 8, 48, 96, 4], g2 / pr / sst /
    tisr [T, 48, 96] (the 2-d series with one common step stride).  Stream-ordered."""
    import torch

    T, s4, s2 = _truth_series(g4, g2, pr, sst, tisr)
    table = torch.empty((res.nlocal, 72), dtype=torch.float64, device=g4.device)
    change = torch.zeros(res.nlocal, dtype=torch.int32, device=g4.device)
    check(lib().sml_res_series_stats(res.handle, ptr(g4), s4, ptr(g2), ptr(pr), ptr(sst), ptr(tisr), s2, T, ptr(table),
                                     ptr(change), stream_ptr(stream)))
    return table, change


def fit_standardisation(res, g4, g2, pr, sst=None, tisr=None, adopt: bool = True, stream=None):
    """The standardisation statistics of every local region of `res` over a series of
    global grids (get_training_data's standardize_data_5d_logp_tisr, standardize_data_3d,
    standardize_sst_data_3d), computed on the device.  Returns (mean [nlocal, 36],
    std [nlocal, 36], sst_change [nlocal]) as numpy arrays; adopt=True makes them the
    context's (sml_res_set_mean_std_device).  Raises ValueError naming the local regions
    whose sst flag is set while sst_change is 0 (the reference would drop their sst
    input; a context's ninp is fixed at create), before anything is adopted."""
    import torch

    table, change = series_stats(res, g4, g2, pr, sst, tisr, stream=stream)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.current_stream().synchronize()
    ms = table.cpu().numpy()
    sst_change = change.cpu().numpy()
    bad = [int(i) for i in range(res.nlocal) if res.sst[i] and not sst_change[i]]
    if bad:
        raise ValueError(f"local regions {bad} (ids {[int(res.region_ids[i]) for i in bad]}) have the sst flag "
                         "but an sst series that does not vary (sst_change 0)")
    if adopt:
        check(lib().sml_res_set_mean_std_device(res.handle, ptr(table), stream_ptr(stream)))
    return ms[:, :36].copy(), ms[:, 36:].copy(), sst_change


def tile_series(res, g4, g2, pr, sst=None, tisr=None, fc4=None, fc2=None, inputs=None, model=None,
                in_stride: int | None = None, model_stride: int | None = None, stream=None):
    """sml_res_tile_series: the T standardised input blocks of a series (and, with fc4
    [T, 8, 48, 96, 4] / fc2 [T, 48, 96], its T model blocks [nlocal, ncs]) in one launch
    each, with the context's mean / std.  inputs / model: flat float64 device tensors
    holding T blocks of in_stride / model_stride doubles (the packed sizes unless
    given); allocated when None.  sst / tisr None: those entries are not written.
    Returns (inputs, model)."""
    import torch

    T, s4, s2 = _truth_series(g4, g2, pr, sst, tisr)
    tot, nmod = int(res.fb_offsets[-1]), res.nlocal * res.ncs
    in_stride = tot if in_stride is None else int(in_stride)
    model_stride = nmod if model_stride is None else int(model_stride)
    if inputs is None:
        inputs = torch.zeros(T * in_stride, dtype=torch.float64, device=g4.device)
    if inputs.numel() < (T - 1) * in_stride + tot:
        raise ValueError("inputs holds fewer than T blocks of in_stride doubles")
    f4s = f2s = 0
    if (fc4 is None) != (fc2 is None):
        raise ValueError("fc4 and fc2 are given together")
    if fc4 is not None:
        Tf, f4s = _series(fc4, "fc4", G4_SHAPE)
        Tg, f2s = _series(fc2, "fc2", G2_SHAPE)
        if Tf != T or Tg != T:
            raise ValueError(f"fc4 / fc2: {Tf} / {Tg} steps, the truth has {T}")
        if model is None:
            model = torch.zeros(T * model_stride, dtype=torch.float64, device=g4.device)
        if model.numel() < (T - 1) * model_stride + nmod:
            raise ValueError("model holds fewer than T blocks of model_stride doubles")
    elif model is not None:
        raise ValueError("model without fc4 / fc2")
    check(lib().sml_res_tile_series(res.handle, ptr(g4), s4, ptr(g2), ptr(pr), ptr(sst), ptr(tisr), s2, ptr(fc4), f4s,
                                    ptr(fc2), f2s, T, ptr(inputs), in_stride, ptr(model), model_stride,
                                    stream_ptr(stream)))
    return inputs, model


def train_from_grids(res, truth, model, discard: int, batch: int, nbatches: int, ncs: int = 132,
                     beta_res: float = 0.001, beta_model: float = 1.0, using_prior: bool = True,
                     prior_val: float = 0.0, dtype=np.float32, stream=None, noise=None):
    """From a series of global grids to W_out, on the device.  truth = (g4, g2, pr, sst,
    tisr): the training series, g4 [T, 8, 48, 96, 4], the others [T, 48, 96] (sst None on a
    context without sst regions, tisr None to leave the tisr entries zero); model =
    (fc4, fc2), the SPEEDY forecasts of the same steps, or None when ncs == 0;
    T >= discard + batch * nbatches.

    fit_standardisation over the whole series, adopted; then train_wout's loop, with the
    blocks it reads tiled `batch` steps at a time into one reused buffer (tile_series):
    the series is never tiled as a whole.  noise: as train_wout takes it -- each tiled
    batch of clean blocks is noised into a second reused buffer with t = the blocks' steps in
    the series, and its precipitation branch reads the statistics adopted here.  Returns
    (wouts, info, mean, std): train_wout's results and the adopted statistics [nlocal, 36]."""
    import torch

    if ncs != res.ncs:
        raise ValueError(f"ncs {ncs} differs from the context's chunk_speedy {res.ncs}")
    if batch < 1:
        raise ValueError("batch must be >= 1")
    g4, g2, pr, sst, tisr = truth
    if ncs and model is None:
        raise ValueError("model: a hybrid context needs the forecast series")
    fc4, fc2 = model if ncs else (None, None)
    T = int(g4.shape[0])
    if T < discard + batch * nbatches:
        raise ValueError("the series holds fewer than discard + batch * nbatches steps")
    mean, std, _ = fit_standardisation(res, g4, g2, pr, sst, tisr, adopt=True, stream=stream)
    tot, nmod = int(res.fb_offsets[-1]), res.nlocal * ncs
    d_in = torch.zeros(batch * tot, dtype=torch.float64, device=g4.device)
    d_mod = torch.zeros(batch * nmod, dtype=torch.float64, device=g4.device) if ncs else None

    def cut(a, t0, m):
        return None if a is None else a[t0:t0 + m]

    def blocks(t0, m):
        if m > 0:
            tile_series(res, cut(g4, t0, m), cut(g2, t0, m), cut(pr, t0, m), cut(sst, t0, m), cut(tisr, t0, m),
                        cut(fc4, t0, m), cut(fc2, t0, m), inputs=d_in, model=d_mod, stream=stream)
        return d_in, d_mod

    wouts, info = _fit_wout(res, blocks, batch, discard, batch, nbatches, ncs, beta_res, beta_model, using_prior,
                            prior_val, dtype, g4.device, stream, noise=noise)
    return wouts, info, mean, std


# ---- the slab-ocean reservoirs (sml_slab_train_series, sml_res_set_target_index)
SLAB_BETA_RES = 0.0001  # initialize_slab_ocean_model: reservoir%beta_res (mod_slab_ocean_reservoir.f90:32)


def _own_slabs(atmo, slab):
    """The local atmo rows of the slab reservoirs; ValueError on a slab context that is not
    the generic ML-only context of atmo's local sst regions, in order."""
    rows = [i for i in range(atmo.nlocal) if atmo.sst[i]]
    ids = [int(atmo.region_ids[i]) for i in rows]
    if slab.numregions != atmo.numregions or slab.ncs != 0 or [int(r) for r in slab.region_ids] != ids:
        raise ValueError("slab: not the ML-only context of the atmo context's local sst regions, in order "
                         f"({len(ids)} sst regions, {slab.nlocal} slab reservoirs)")
    return rows


def slab_series(atmo, slab, g4, g2, pr, sst, tisr=None, window: int = 1, divisor: int = 1, t0: int = 0,
                ncols: int | None = None, out=None, out_stride: int | None = None, stream=None):
    """sml_slab_train_series: columns t0 .. t0 + ncols - 1 (all from t0 when ncols is None) of
    the slab reservoirs' averaged input series, from the grids of a training series (g4
    [T, 8, 48, 96, 4]; g2 / pr / sst / tisr [T, 48, 96]) with atmo's adopted mean / std:
    column t = (z_lo + ... + z_t) / d over the last `window` standardised steps, d the
    number of terms while t + 1 < window, `divisor` afterwards.  (window, divisor) =
    (P + 1, P) is the reference's rolling_average_over_a_period_2d of period P; (P, P) the
    plain mean of P columns, what the loop's ring feeds the slab at prediction.  out: a flat
    float64 device tensor of ncols columns out_stride doubles apart (the slab's packed
    feedback size unless given); allocated (not filled: with a padded out_stride the words
    between the columns hold anything) when None.  Stream-ordered.  Returns out."""
    import torch

    T, s4, s2 = _truth_series(g4, g2, pr, sst, tisr)
    if sst is None:
        raise ValueError("sst: the slab series needs the sst series")
    ncols = T - t0 if ncols is None else int(ncols)
    tot = int(slab.fb_offsets[-1])
    out_stride = tot if out_stride is None else int(out_stride)
    if out is None:
        # not filled: the kernel writes every word of a column's packed feedback, and a fill on
        # torch's current stream would not be ordered against a kernel on `stream` (one double
        # at least: an empty tensor has no address to pass)
        out = torch.empty(max(ncols * out_stride, 1), dtype=torch.float64, device=g4.device)[:max(ncols, 0) * out_stride]
    if ncols > 0 and out.numel() < (ncols - 1) * out_stride + tot:
        raise ValueError("out holds fewer than ncols columns of out_stride doubles")
    check(lib().sml_slab_train_series(atmo.handle, slab.handle, ptr(g4), s4, ptr(g2), ptr(pr), ptr(sst), ptr(tisr), s2,
                                      T, int(window), int(divisor), int(t0), ncols,
                                      ctypes.c_void_p(out.untyped_storage().data_ptr() + 8 * out.storage_offset()), out_stride,
                                      stream_ptr(stream)))
    return out


def train_slab_from_grids(atmo, slab, truth, window: int, divisor: int, phase_stride: int, discard_cols: int,
                          batch: int, nbatches: int, beta_res: float = SLAB_BETA_RES, dtype=np.float32,
                          fit_stats: bool = False, stream=None, noise=None):
    """From the grids of a training period to the slab-ocean reservoirs' W_out, on the device:
    train_slab_ocean_model with get_training_data_from_atmo, reservoir_layer_chunking_ml,
    chunking_matmul_ml and fit_chunk_ml (mod_slab_ocean_reservoir.f90:173-270, 272-376,
    802-887, 1353-1397, 994-1050).

    atmo: the atmospheric context with its standardisation adopted -- fit_standardisation is
    the caller's step (train_from_grids does it); fit_stats=True does it here, over `truth`.
    slab: the generic context of atmo's local sst regions (A and W_in loaded).  truth =
    (g4, g2, pr, sst, tisr) as train_from_grids takes it.

    The averaged series (slab_series with (window, divisor)) is made once for all T steps:
    T * the slab's packed feedback doubles, 0.91 MB a step at full size (1027 reservoirs).
    The slab gets its target index (Reservoirs.set_target_index of slab_target_index).
    Then, for each phase i = 0 .. phase_stride - 1 -- the reference's do i = 1, timestep_slab
    over trainingdata(:, i::timestep_slab) -- on the sub-series i, i + S, i + 2 S, ...:
    states to zero, Reservoirs.synchronize over discard_cols columns, nbatches times
    train_drive + Trainer.accumulate into the same sums across the phases.  One
    Trainer.solve(ncs=0, beta_res) with beta_res on the whole diagonal (fit_chunk_ml)
    closes; the default beta_res is the reference's for the slab (SLAB_BETA_RES).
    noise=None uses the series as given.  noise=InputNoise(...) adds the reference's input
    noise: the averaged series, which exists as a whole, gets a noised copy in one launch
    (Reservoirs.input_noise with t = the column's index in the series and the atmosphere's
    global ids of the sst regions as noise ids; every entry plain, the slab context has no
    geometry); the discard columns and the drives read the copy, the targets the clean
    series.  Every launch goes
    to `stream`; the states' reset of each phase is a host copy, so the host waits for
    `stream` before it (the previous phase's last drive writes the state it zeroes).  A slab
    context without reservoirs (a rank with no sst region) returns empty results at once.

    Returns (wouts, info, mean, std): per slab reservoir W_out (n, nout), ready for
    write_region_netcdf / Reservoirs.load_region, the potrf info, and the [nslab, 36] mean /
    std rows the slab's file carries -- its atmo region's adopted statistics, of which the
    slab reads the sst slot (35).  ValueError when T < phase_stride * (discard_cols + batch *
    nbatches) and on a slab context that does not belong to atmo."""
    import torch

    rows = _own_slabs(atmo, slab)
    g4, g2, pr, sst, tisr = truth
    S = int(phase_stride)
    if S < 1 or batch < 1 or nbatches < 1 or discard_cols < 0:
        raise ValueError("phase_stride, batch, nbatches must be >= 1 and discard_cols >= 0")
    T = int(g4.shape[0])
    if T < S * (discard_cols + batch * nbatches):
        raise ValueError("the series holds fewer than phase_stride * (discard_cols + batch * nbatches) steps")
    if fit_stats:
        fit_standardisation(atmo, g4, g2, pr, sst, tisr, adopt=True, stream=stream)
    if slab.nlocal == 0:
        return [], np.zeros(0, dtype=np.int32), np.zeros((0, 36)), np.zeros((0, 36))
    mean, std = np.zeros((len(rows), 36)), np.zeros((len(rows), 36))
    for j, i in enumerate(rows):
        check(lib().sml_res_mean_std(atmo.handle, i, ptr(mean[j]), ptr(std[j])))
    series = slab_series(atmo, slab, g4, g2, pr, sst, tisr, window, divisor, stream=stream)
    slab.set_target_index(np.stack([slab.slab_target_index(j) for j in range(slab.nlocal)]))
    tot = int(slab.fb_offsets[-1])
    driving = series
    if noise is not None:
        slab.set_input_noise(noise.noisemag, noise.seed, noise.precip_epsilon, ids=slab.region_ids)
        driving = slab.input_noise(series, torch.empty_like(series), 0, T, stream=stream)
    naug = [int(n) for n in slab.n]
    tr = Trainer(naug, slab.nout)
    tr.reset(stream=stream)
    states = torch.empty(sum(naug) * batch, dtype=torch.float64, device=g4.device)
    targets = torch.empty(len(naug) * batch * slab.nout, dtype=torch.float64, device=g4.device)
    for i in range(S):
        # set_state copies from the host with no regard for `stream`, whose last drive (record,
        # then advance) still writes the state being zeroed: wait for it first
        (stream if stream is not None else torch.cuda.current_stream()).synchronize()
        for j, n in enumerate(slab.n):
            slab.set_state(j, np.zeros(int(n)))
        slab.synchronize(driving[i * tot:], discard_cols, stride=S * tot, stream=stream)
        for b in range(nbatches):
            col = i + (discard_cols + b * batch) * S
            if noise is None:
                slab.train_drive(series[col * tot:], batch, None, states, targets, stride=S * tot, stream=stream)
            else:
                slab.train_drive(driving[col * tot:], batch, None, states, targets, stride=S * tot, stream=stream,
                                 target_inputs=series[col * tot:], target_stride=S * tot)
            tr.accumulate(states, targets, batch, stream=stream)
    packed, info = tr.solve(ncs=0, beta_res=beta_res, using_prior=False, stream=stream)
    wouts = [v.cpu().numpy().astype(dtype) for v in tr.wout_views(packed)]
    tr.close()
    return wouts, info, mean, std

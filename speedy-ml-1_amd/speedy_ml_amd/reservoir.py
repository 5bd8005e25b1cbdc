"""Batched reservoir forward + exchange tiling on the GPU (libspeedyml sml_res_*).

Host-side mirror of the reference's reservoir interface for one rank:
  Reservoirs(...)            <- initialize_model_parameters + processor_decomposition +
                                per-region trained_reservoir_prediction
                                (src/parallelmain.f90:30-199, src/mod_reservoir.f90:1781)
  .load_region(...)          <- read_trained_res + allocate_res_new + mklsparse
  .predict(fb, lm, out)      <- predict for every region of the rank (mod_reservoir.f90:1416)
  .assemble / .tile_inputs   <- sendrecievegrid's gather and scatter (mpires.f90:218-780)
Device buffers are torch CUDA tensors (plumbing only).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._lib import SML_F32, SML_F64, check, lib, ptr, stream_ptr
from .domain import CHUNK_PRED, CHUNK_SPEEDY, NUM_REGIONS


class Reservoirs:
    """One rank's reservoirs on the GPU (sml_res_*).  With `ninp` and `out_index` given,
    a generic context (sml_res_create_generic: the slab-ocean reservoir's shape,
    ninp per region, outputs unstandardized with mean/std slot out_index[o])."""

    def __init__(self, region_ids, sst_flags, n, k, numregions: int = NUM_REGIONS,
                 chunk_speedy: int = CHUNK_SPEEDY, nout: int = CHUNK_PRED, weight_dtype: str = "f32",
                 leakage: float = 1.0, ninp=None, out_index=None):
        self.region_ids = np.ascontiguousarray(region_ids, dtype=np.int32)
        self.sst = np.ascontiguousarray(sst_flags, dtype=np.uint8)
        self.n = np.ascontiguousarray(n, dtype=np.int32)
        self.k = np.ascontiguousarray(k, dtype=np.int32)
        self.nlocal = len(self.region_ids)
        self.numregions = numregions
        self.ncs = chunk_speedy
        self.nout = nout
        self.weight_dtype = weight_dtype
        dt = {"f32": SML_F32, "f64": SML_F64}[weight_dtype]
        h = ctypes.c_void_p()
        if ninp is None:
            check(lib().sml_res_create(numregions, self.nlocal, ptr(self.region_ids), ptr(self.sst), ptr(self.n),
                                       ptr(self.k), chunk_speedy, nout, dt, leakage, ctypes.byref(h)))
        else:
            self._ninp = np.ascontiguousarray(ninp, dtype=np.int32)
            self._oidx = np.ascontiguousarray(out_index, dtype=np.int8)
            check(lib().sml_res_create_generic(numregions, self.nlocal, ptr(self.region_ids), ptr(self._ninp),
                                               ptr(self.n), ptr(self.k), chunk_speedy, nout, ptr(self._oidx), dt,
                                               leakage, ctypes.byref(h)))
        self._h = h
        self._ov_ld = nout  # the outvec row stride (set_outvec_ld)
        off = np.zeros(self.nlocal + 1, dtype=np.int64)
        check(lib().sml_res_feedback_offsets(self._h, ptr(off)))
        self.fb_offsets = off

    def close(self):
        if getattr(self, "_h", None):
            lib().sml_res_destroy(self._h)
            self._h = None

    __del__ = close

    @property
    def handle(self):
        return self._h

    def ninp(self, i: int) -> int:
        v = ctypes.c_int()
        check(lib().sml_res_ninp(self._h, i, ctypes.byref(v)))
        return v.value

    def load_region(self, i: int, rows, cols, vals, win, wout, mean, std):
        """Reference layouts: rows/cols 1-based (k,), vals (k,), win (ninp, n) C-order,
        wout (ncs+n, nout) C-order, mean/std (36,)."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        mean = np.ascontiguousarray(mean, dtype=np.float64)
        std = np.ascontiguousarray(std, dtype=np.float64)
        if vals.dtype == np.float32 and win.dtype == np.float32 and wout.dtype == np.float32:
            f = lib().sml_res_load_region_f32
            vals, win, wout = (np.ascontiguousarray(a, dtype=np.float32) for a in (vals, win, wout))
        else:
            f = lib().sml_res_load_region_f64
            vals, win, wout = (np.ascontiguousarray(a, dtype=np.float64) for a in (vals, win, wout))
        check(f(self._h, i, ptr(rows), ptr(cols), ptr(vals), ptr(win), ptr(wout), ptr(mean), ptr(std)))

    def load_region_weights(self, i: int, w):
        self.load_region(i, w.rows, w.cols, w.vals, w.win, w.wout, w.mean, w.std)

    def load_netcdf(self, i: int, path: str):
        """Load region i from a reference weight file (read_trained_res)."""
        d = read_region_netcdf(path)
        self.load_region(i, d["rows"], d["cols"], d["vals"], d["win"], d["wout"],
                         d["mean"].astype(np.float64), d["std"].astype(np.float64))

    def set_state(self, i: int, x, member: int = 0):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if member == 0:  # (the entry point every build of the library has: SML_LIB A/B runs)
            check(lib().sml_res_set_state(self._h, i, ptr(x)))
        else:
            check(lib().sml_res_set_state_member(self._h, int(member), i, ptr(x)))

    def get_state(self, i: int, member: int = 0) -> np.ndarray:
        x = np.zeros(int(self.n[i]))
        if member == 0:
            check(lib().sml_res_get_state(self._h, i, ptr(x)))
        else:
            check(lib().sml_res_get_state_member(self._h, int(member), i, ptr(x)))
        return x

    # --- ensemble members
    def set_members(self, members: int):
        """The number of ensemble members (sml_res_set_members; 1 at create): states of
        every region that advance through the same weights.  Member 0 keeps its state,
        new members start from x = 0.  While members > 1 the single-member calls that
        advance the state (predict, predict_begin, synchronize, ...) are refused."""
        check(lib().sml_res_set_members(self._h, int(members)))

    @property
    def members(self) -> int:
        v = ctypes.c_int()
        check(lib().sml_res_members(self._h, ctypes.byref(v)))
        return v.value

    def member_tile(self) -> dict:
        """The tiles the members kernels run with (sml_res_member_tile): members per
        update block, whether their states are staged in LDS, members per W_out load."""
        v = [ctypes.c_int() for _ in range(3)]
        check(lib().sml_res_member_tile(self._h, *[ctypes.byref(x) for x in v]))
        return dict(update_tile=v[0].value, update_lds=bool(v[1].value), readout_tile=v[2].value)

    @staticmethod
    def _member_rows(t, what, shape, row_min):
        """A float64 device tensor [shape..., >= row_min] whose trailing dimensions are
        dense (a member's block is what the library lays out): its leading stride."""
        import torch

        if t.dtype != torch.float64 or not t.is_cuda:
            raise ValueError(f"{what}: a float64 device tensor expected")
        if t.dim() != len(shape) + 1 or tuple(t.shape[:-1]) != tuple(shape) or t.shape[-1] < row_min:
            raise ValueError(f"{what}: shape {tuple(shape)} + (>= {row_min},) expected, got {tuple(t.shape)}")
        want = 1
        for d in range(t.dim() - 1, 0, -1):  # every dimension but the first is packed
            if t.shape[d] != 1 and t.stride(d) != want:
                raise ValueError(f"{what}: only the first dimension may be strided, got strides {t.stride()}")
            want *= t.shape[d]
        if t.shape[0] > 1 and t.stride(0) < want:
            raise ValueError(f"{what}: the first dimension's stride {t.stride(0)} is below {want}")
        return int(t.stride(0)) if t.shape[0] > 1 else want

    def predict_members(self, d_feedback, d_local_model, d_outvec, stream=None):
        """predict for every member in one stream of the weights (sml_res_step_members):
        d_feedback [E, >= total feedback], d_local_model [E, nlocal, chunk_speedy] (None
        when chunk_speedy == 0), d_outvec [E, nlocal, the outvec row stride].  Member e's
        outvecs and state are bitwise those of predict on a context of its own."""
        E = self.members
        fbs = self._member_rows(d_feedback, "d_feedback", (E,), int(self.fb_offsets[-1]))
        lms = 0
        if self.ncs:
            if d_local_model is None:
                raise ValueError("d_local_model: a hybrid context needs it")
            lms = self._member_rows(d_local_model, "d_local_model", (E, self.nlocal), self.ncs)
            if d_local_model.shape[-1] != self.ncs:
                raise ValueError(f"d_local_model: rows of {self.ncs} doubles expected")
        ovs = self._member_rows(d_outvec, "d_outvec", (E, self.nlocal), self._ov_ld)
        if d_outvec.shape[-1] != self._ov_ld:
            raise ValueError(f"d_outvec: rows of {self._ov_ld} doubles expected (set_outvec_ld)")
        check(lib().sml_res_step_members(self._h, ptr(d_feedback), fbs, ptr(d_local_model if self.ncs else None), lms,
                                         ptr(d_outvec), ovs, stream_ptr(stream)))

    # --- the split step for every member (sml_res_step_begin_members and its finishes)
    def _member_lm_ov(self, d_local_model, d_outvec, lm_optional=False):
        """The strides of d_local_model [E, nlocal, chunk_speedy] (None allowed when
        chunk_speedy == 0, or where the call only writes it) and d_outvec [E, nlocal, ld]."""
        E = self.members
        lms = self.nlocal * self.ncs
        if d_local_model is None or not self.ncs:
            if self.ncs and not lm_optional:
                raise ValueError("d_local_model: a hybrid context needs it")
        else:
            lms = self._member_rows(d_local_model, "d_local_model", (E, self.nlocal), self.ncs)
            if d_local_model.shape[-1] != self.ncs:
                raise ValueError(f"d_local_model: rows of {self.ncs} doubles expected")
        ovs = self._member_rows(d_outvec, "d_outvec", (E, self.nlocal), self._ov_ld)
        if d_outvec.shape[-1] != self._ov_ld:
            raise ValueError(f"d_outvec: rows of {self._ov_ld} doubles expected (set_outvec_ld)")
        return lms, ovs

    def _member_grids(self, g4, g2, names, pr=None):
        """The strides of a members' 4-d grid [E, 8, 48, 96, 4] and 2-d grid(s) [E, 48, 96]
        (pr, when given, with g2's stride)."""
        E = self.members
        s4 = self._member_rows(g4, names[0], (E, 8, 48, 96), 4)
        if g4.shape[-1] != 4:
            raise ValueError(f"{names[0]}: shape ({E}, 8, 48, 96, 4) expected, got {tuple(g4.shape)}")
        s2 = self._member_rows(g2, names[1], (E, 48), 96)
        if g2.shape[-1] != 96:
            raise ValueError(f"{names[1]}: shape ({E}, 48, 96) expected, got {tuple(g2.shape)}")
        if pr is not None:
            sp = self._member_rows(pr, names[2], (E, 48), 96)
            if pr.shape[-1] != 96 or sp != s2:
                raise ValueError(f"{names[2]}: shape ({E}, 48, 96) and {names[1]}'s member stride {s2} expected, "
                                 f"got {tuple(pr.shape)} with stride {sp}")
        return s4, s2

    def begin_members(self, d_feedback, stream=None):
        """predict_begin for every member (sml_res_step_begin_members): d_feedback
        [E, >= total feedback]; every member's update and v_ml, no local model needed."""
        fbs = self._member_rows(d_feedback, "d_feedback", (self.members,), int(self.fb_offsets[-1]))
        check(lib().sml_res_step_begin_members(self._h, ptr(d_feedback), fbs, stream_ptr(stream)))

    def finish_members(self, d_local_model, d_outvec, stream=None):
        """predict_finish for every member (sml_res_step_finish_members): d_local_model
        [E, nlocal, chunk_speedy] (None when chunk_speedy == 0), d_outvec [E, nlocal, ld]."""
        lms, ovs = self._member_lm_ov(d_local_model, d_outvec)
        check(lib().sml_res_step_finish_members(self._h, ptr(d_local_model if self.ncs else None), lms,
                                                ptr(d_outvec), ovs, stream_ptr(stream)))

    def finish_grid_members(self, d_fc4d, d_fc2d, d_local_model, d_outvec, stream=None):
        """predict_finish_grid for every member (sml_res_step_finish_grid_members): member
        e's local model is tiled from its forecast d_fc4d[e] / d_fc2d[e] ([E, 8, 48, 96, 4] /
        [E, 48, 96]); d_local_model (or None) also receives the tiled vectors."""
        s4, s2 = self._member_grids(d_fc4d, d_fc2d, ("d_fc4d", "d_fc2d"))
        lms, ovs = self._member_lm_ov(d_local_model, d_outvec, lm_optional=True)
        check(lib().sml_res_step_finish_grid_members(self._h, ptr(d_fc4d), s4, ptr(d_fc2d), s2,
                                                     ptr(d_local_model if self.ncs else None), lms, ptr(d_outvec),
                                                     ovs, stream_ptr(stream)))

    def finish_assemble_members(self, d_fc4d, d_fc2d, d_local_model, d_outvec, g4, g2, pr, stream=None):
        """predict_finish_assemble for every member (sml_res_step_finish_assemble_members):
        member e's outputs are also scattered into g4[e], g2[e], pr[e] (one rank holding
        every region in order)."""
        s4, s2 = self._member_grids(d_fc4d, d_fc2d, ("d_fc4d", "d_fc2d"))
        g4s, g2s = self._member_grids(g4, g2, ("g4", "g2", "pr"), pr=pr)
        lms, ovs = self._member_lm_ov(d_local_model, d_outvec, lm_optional=True)
        check(lib().sml_res_step_finish_assemble_members(self._h, ptr(d_fc4d), s4, ptr(d_fc2d), s2,
                                                         ptr(d_local_model if self.ncs else None), lms,
                                                         ptr(d_outvec), ovs, ptr(g4), g4s, ptr(g2), ptr(pr), g2s,
                                                         stream_ptr(stream)))

    def tile_feedback_members(self, g4, g2, pr, d_tisr, d_feedback, stream=None):
        """tile_feedback for every member in one launch (sml_res_tile_feedback_members): g4
        [E, 8, 48, 96, 4], g2 / pr [E, 48, 96], d_feedback [E, >= total feedback]; d_tisr
        [nlocal, 16], the members' common one, or None (the tisr entries stay)."""
        g4s, g2s = self._member_grids(g4, g2, ("g4", "g2", "pr"), pr=pr)
        fbs = self._member_rows(d_feedback, "d_feedback", (self.members,), int(self.fb_offsets[-1]))
        check(lib().sml_res_tile_feedback_members(self._h, ptr(g4), g4s, ptr(g2), ptr(pr), g2s, ptr(d_tisr),
                                                  ptr(d_feedback), fbs, stream_ptr(stream)))

    def tile_tisr_field_members(self, d_tisr_grid, d_feedback, stream=None):
        """One hour's global tisr field [48, 96] into every member's feedback
        (sml_res_tile_tisr_field_members)."""
        fbs = self._member_rows(d_feedback, "d_feedback", (self.members,), int(self.fb_offsets[-1]))
        check(lib().sml_res_tile_tisr_field_members(self._h, ptr(d_tisr_grid), ptr(d_feedback), fbs,
                                                    stream_ptr(stream)))

    def member_finish_tile(self) -> int:
        """Members one block of the grid finish serves (sml_res_member_finish_tile); 1 at
        more than one member: the single-member kernel once per member."""
        v = ctypes.c_int()
        check(lib().sml_res_member_finish_tile(self._h, ctypes.byref(v)))
        return v.value

    def cancel_step(self):
        """Discard a begun step, of one member or of all (sml_res_step_cancel): the states
        are what they were before the begin.  Waits for the device."""
        check(lib().sml_res_step_cancel(self._h))

    def step_begun(self) -> bool:
        """Whether a begin's finish is pending (sml_res_step_begun)."""
        v = ctypes.c_int()
        check(lib().sml_res_step_begun(self._h, ctypes.byref(v)))
        return bool(v.value)

    def synchronize_members(self, d_inputs, length: int, stream=None):
        """synchronize for every member (sml_res_synchronize_members): d_inputs
        [>= length, E, >= total feedback]; `length` updates of every member, no readout."""
        import torch

        E, tot = self.members, int(self.fb_offsets[-1])
        if d_inputs.dtype != torch.float64 or not d_inputs.is_cuda:
            raise ValueError("d_inputs: a float64 device tensor expected")
        if d_inputs.dim() != 3 or d_inputs.shape[0] < length or d_inputs.shape[1] != E or d_inputs.shape[2] < tot:
            raise ValueError(f"d_inputs: shape (>= {length}, {E}, >= {tot}) expected, got {tuple(d_inputs.shape)}")
        if d_inputs.shape[2] > 1 and d_inputs.stride(2) != 1:
            raise ValueError("d_inputs: a member's block must be packed")
        stride = int(d_inputs.stride(0)) if d_inputs.shape[0] > 1 else E * max(int(d_inputs.stride(1)), tot)
        mstride = int(d_inputs.stride(1)) if E > 1 else tot
        if mstride < tot or stride < tot:
            raise ValueError(f"d_inputs: strides {d_inputs.stride()} below the packed feedback size {tot}")
        check(lib().sml_res_synchronize_members(self._h, ptr(d_inputs), int(length), stride, mstride,
                                                stream_ptr(stream)))

    # --- device buffers
    def alloc_io(self, device="cuda"):
        import torch

        fb = torch.zeros(int(self.fb_offsets[-1]), dtype=torch.float64, device=device)
        lm = torch.zeros((self.nlocal, max(self.ncs, 1)), dtype=torch.float64, device=device)
        ov = torch.zeros((self.nlocal, self.nout), dtype=torch.float64, device=device)
        return fb, lm, ov

    def predict(self, d_feedback, d_local_model, d_outvec, stream=None):
        check(lib().sml_res_step(self._h, ptr(d_feedback), ptr(d_local_model if self.ncs else None),
                                 ptr(d_outvec), stream_ptr(stream)))

    def predict_begin(self, d_feedback, stream=None):
        """First half of predict: the state update and W_out(:, ncs+1:) x~ (v_ml of
        outvec_component_contribs, mod_reservoir.f90:1456-1459) -- no local_model needed."""
        check(lib().sml_res_step_begin(self._h, ptr(d_feedback), stream_ptr(stream)))

    def predict_finish_grid(self, d_fc4d, d_fc2d, d_local_model, d_outvec, stream=None):
        """tile_local_model + predict_finish in one launch (same results); d_local_model
        (or None) also receives the tiled local-model vectors."""
        check(lib().sml_res_step_finish_grid(self._h, ptr(d_fc4d), ptr(d_fc2d), ptr(d_local_model), ptr(d_outvec),
                                             stream_ptr(stream)))

    def predict_finish_assemble(self, d_fc4d, d_fc2d, d_local_model, d_outvec, g4, g2, pr, stream=None):
        """predict_finish_grid + assemble(d_outvec, g4, g2, pr) in one launch (one rank
        holding every region in order; same results)."""
        check(lib().sml_res_step_finish_assemble(self._h, ptr(d_fc4d), ptr(d_fc2d), ptr(d_local_model),
                                                 ptr(d_outvec), ptr(g4), ptr(g2), ptr(pr), stream_ptr(stream)))

    def set_read_waves(self, waves: int):
        """Cap on the v_ml readout's waves in predict_begin (0 = uncapped)."""
        check(lib().sml_res_set_read_waves(self._h, int(waves)))

    def set_outvec_ld(self, ld: int):
        """Row stride (>= nout) of the outvec arrays the context writes (sml_res_set_outvec_ld)."""
        check(lib().sml_res_set_outvec_ld(self._h, int(ld)))
        self._ov_ld = int(ld)

    def set_update_cus(self, cus: int):
        """The CUs this context's launches get (sml_res_set_update_cus; 0 = the device)."""
        check(lib().sml_res_set_update_cus(self._h, int(cus)))

    def update_balanced(self) -> bool:
        """Whether the state update runs as k_res_update_bal (sml_res_update_balanced)."""
        b = ctypes.c_int()
        check(lib().sml_res_update_balanced(self._h, ctypes.byref(b)))
        return bool(b.value)

    def ell_layout(self, i: int) -> dict:
        """Local region i's compressed A / W_in form (sml_res_ell_layout)."""
        v = [ctypes.c_int() for _ in range(4)]
        check(lib().sml_res_ell_layout(self._h, int(i), *[ctypes.byref(x) for x in v]))
        return dict(a_width=v[0].value, a_overflow=bool(v[1].value), win_q=v[2].value, win_ell=bool(v[3].value))

    def set_reference_paths(self, csr: bool = False, per_region: bool = False, ungrouped_finish: bool = False,
                            stepwise_drive: bool = False, radius_global: bool = False):
        """Force the fallback paths for every region (sml_res_set_reference_paths): A /
        W_in from their CSR copies (before any region is loaded), the per-region state
        update, the v_p finish one thread per output, the training drive one update
        launch per column, spectral_radius's vectors in global scratch -- bitwise the
        defaults."""
        flags = ((1 if csr else 0) | (2 if per_region else 0) | (4 if ungrouped_finish else 0)
                 | (8 if stepwise_drive else 0) | (16 if radius_global else 0))
        check(lib().sml_res_set_reference_paths(self._h, flags))

    def spectral_radius(self, tol: float = 2e-14, max_iter: int = 1000, stream=None):
        """The spectral radius of every local region's A as loaded (sml_res_spectral_radius;
        gen_res's sparse_eigen, mod_reservoir.f90:190): power iteration with the
        Collatz-Wielandt enclosure lo <= rho <= hi, for A without negative entries.
        Returns (lo, hi, iters, info), arrays of nlocal; info 0 = hi - lo <= tol * hi,
        1 = max_iter reached, 2 = A x vanished, 3 = a negative or non-finite entry.
        Waits for the stream."""
        lo, hi = np.zeros(self.nlocal), np.zeros(self.nlocal)
        iters, info = np.zeros(self.nlocal, dtype=np.int32), np.zeros(self.nlocal, dtype=np.int32)
        check(lib().sml_res_spectral_radius(self._h, float(tol), int(max_iter), ptr(lo), ptr(hi), ptr(iters),
                                            ptr(info), stream_ptr(stream)))
        return lo, hi, iters, info

    def target_index(self, i: int) -> np.ndarray:
        """0-based positions of local region i's training targets inside its feedback
        vector (sml_region_target_index)."""
        idx = np.zeros(34 * 96 * 48 // self.numregions, dtype=np.int32)
        cnt = ctypes.c_int()
        check(lib().sml_region_target_index(self.numregions, int(self.region_ids[i]), int(self.sst[i]), ptr(idx),
                                            ctypes.byref(cnt)))
        return idx[:cnt.value]

    def slab_target_index(self, i: int) -> np.ndarray:
        """0-based positions of the slab-ocean reservoir's targets inside the slab feedback
        of local region i (sml_slab_target_index): the sst section's inner tile."""
        idx = np.zeros(96 * 48 // self.numregions, dtype=np.int32)
        cnt = ctypes.c_int()
        check(lib().sml_slab_target_index(self.numregions, int(self.region_ids[i]), ptr(idx), ctypes.byref(cnt)))
        return idx[:cnt.value]

    def set_target_index(self, idx):
        """Give a generic context its training targets (sml_res_set_target_index): idx
        [nlocal, nout], positions in each local region's feedback; train_drive then
        accepts d_targets on it."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        if idx.shape != (self.nlocal, self.nout):
            raise ValueError(f"idx: shape ({self.nlocal}, {self.nout}) expected, got {idx.shape}")
        check(lib().sml_res_set_target_index(self._h, ptr(idx)))

    def set_input_noise(self, noisemag: float, seed: int, precip_epsilon: float = 0.0, ids=None):
        """The configuration of input_noise (sml_res_set_input_noise): the reference's
        gaussian_noise_1d_function of magnitude noisemag, drawn from (seed, the region's noise
        id, step, entry); precip_epsilon > 0 turns on gaussian_noise_1d_function_precip's branch
        for the precipitation entries of a context with a geometry.  ids [nlocal]: the regions'
        noise ids; None: the region ids (the local index on a generic context)."""
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.int32)
            if ids.shape != (self.nlocal,):
                raise ValueError(f"ids: shape ({self.nlocal},) expected, got {ids.shape}")
        check(lib().sml_res_set_input_noise(self._h, float(noisemag), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                            float(precip_epsilon), ptr(ids)))

    def input_noise(self, d_in, d_out, t0: int, m: int, in_stride: int | None = None, out_stride: int | None = None,
                    stream=None):
        """sml_res_input_noise: blocks t0 .. t0 + m - 1 (absolute steps of the series) of
        d_in, noised, into d_out (flat float64 device tensors of m blocks in_stride /
        out_stride doubles apart, the packed feedback size unless given; d_out may be d_in).
        d_in None: the normal draws g themselves.  One launch, stream-ordered.  Returns d_out."""
        tot = int(self.fb_offsets[-1])
        in_stride = tot if in_stride is None else int(in_stride)
        out_stride = tot if out_stride is None else int(out_stride)
        if m < 0:
            raise ValueError("m must be >= 0")
        if m > 0:
            if d_in is not None and d_in.numel() < (m - 1) * in_stride + tot:
                raise ValueError("d_in holds fewer than m blocks of in_stride doubles")
            if d_out.numel() < (m - 1) * out_stride + tot:
                raise ValueError("d_out holds fewer than m blocks of out_stride doubles")
        check(lib().sml_res_input_noise(self._h, ptr(d_in), in_stride, ptr(d_out), out_stride, int(t0), int(m),
                                        stream_ptr(stream)))
        return d_out

    def train_drive(self, d_inputs, m: int, d_model, d_states, d_targets=None, stride: int | None = None,
                    model_stride: int | None = None, stream=None, target_inputs=None,
                    target_stride: int | None = None):
        """The training drive (sml_res_train_drive; reservoir_layer_chunking_hybrid,
        mod_reservoir.f90:1065-1173): for each of the m input blocks of d_inputs, column c
        of every region's block of d_states = [model block c; the current state with its
        odd nodes squared], column c of d_targets = the region's targets of block c, then
        the state advances on block c.  d_states / d_targets are packed as
        Trainer.accumulate reads them.  d_model: m blocks of [nlocal][ncs] (None when
        chunk_speedy == 0).  target_inputs (sml_res_train_drive_from): a second series, m
        blocks target_stride apart, the targets are read from instead -- the clean series
        beside a d_inputs that input_noise has noised, as the reference trains."""
        stride = int(self.fb_offsets[-1]) if stride is None else int(stride)
        model_stride = self.nlocal * self.ncs if model_stride is None else int(model_stride)
        if m < 0:
            raise ValueError("m must be >= 0")
        if m > 0:
            if d_inputs.numel() < (m - 1) * stride + int(self.fb_offsets[-1]):
                raise ValueError("d_inputs holds fewer than m blocks of `stride` doubles")
            if self.ncs and (d_model is None or d_model.numel() < (m - 1) * model_stride + self.nlocal * self.ncs):
                raise ValueError("d_model holds fewer than m blocks of `model_stride` doubles")
            if d_states.numel() < m * (int(self.n.sum()) + self.nlocal * self.ncs):
                raise ValueError("d_states is smaller than m * sum(ncs + n)")
            if d_targets is not None and d_targets.numel() < m * self.nlocal * self.nout:
                raise ValueError("d_targets is smaller than m * nlocal * nout")
        if target_inputs is None:
            check(lib().sml_res_train_drive(self._h, ptr(d_inputs), int(m), stride,
                                            ptr(d_model if self.ncs else None), model_stride, ptr(d_states),
                                            ptr(d_targets), stream_ptr(stream)))
            return
        target_stride = int(self.fb_offsets[-1]) if target_stride is None else int(target_stride)
        if m > 0 and target_inputs.numel() < (m - 1) * target_stride + int(self.fb_offsets[-1]):
            raise ValueError("target_inputs holds fewer than m blocks of `target_stride` doubles")
        check(lib().sml_res_train_drive_from(self._h, ptr(d_inputs), int(m), stride, ptr(target_inputs), target_stride,
                                             ptr(d_model if self.ncs else None), model_stride, ptr(d_states),
                                             ptr(d_targets), stream_ptr(stream)))

    def set_begin_mode(self, mode: int):
        """predict_begin's form: 0 update grid + readout grid, 1 / 2 one fused launch
        (sml_res_set_begin_mode); bit-identical results."""
        check(lib().sml_res_set_begin_mode(self._h, int(mode)))

    @property
    def begin_fused(self) -> bool:
        """Whether predict_begin runs as the fused launch (the mode and this context's shapes)."""
        f = ctypes.c_int()
        check(lib().sml_res_begin_fused(self._h, ctypes.byref(f)))
        return bool(f.value)

    def predict_finish(self, d_local_model, d_outvec, stream=None):
        """Second half: outvec = W_out(:, 1:ncs) local_model + v_ml, unstandardized."""
        check(lib().sml_res_step_finish(self._h, ptr(d_local_model if self.ncs else None), ptr(d_outvec),
                                        stream_ptr(stream)))

    def synchronize(self, d_inputs, length: int, stride: int | None = None, stream=None):
        """synchronize (mod_reservoir.f90:1352-1378): `length` state updates, no
        readout.  d_inputs: device tensor of `length` packed feedback blocks
        (row t = block t, stride = total feedback doubles unless given)."""
        stride = int(self.fb_offsets[-1]) if stride is None else int(stride)
        if d_inputs.numel() < length * stride:
            raise ValueError("d_inputs holds fewer than length * stride doubles")
        check(lib().sml_res_synchronize(self._h, ptr(d_inputs), length, stride, stream_ptr(stream)))

    def start_prediction(self, d_inputs, length: int, d_feedback, stride: int | None = None, stream=None):
        """start_prediction (mod_reservoir.f90:938-959): synchronize_print over the first
        `length` input blocks, block `length` into d_feedback."""
        stride = int(self.fb_offsets[-1]) if stride is None else stride
        check(lib().sml_res_start_prediction(self._h, ptr(d_inputs), length, stride, ptr(d_feedback),
                                             stream_ptr(stream)))

    def predict_slab(self, d_feedback, d_local_model, d_local_model_next, d_outvec, stream=None):
        """predict_slab (mod_slab_ocean_reservoir.f90:1201-1249) on a generic context:
        outvec unstandardized, the raw outvec into d_local_model_next."""
        check(lib().sml_res_step_slab(self._h, ptr(d_feedback), ptr(d_local_model), ptr(d_local_model_next),
                                      ptr(d_outvec), stream_ptr(stream)))

    def predict_host(self, feedback: np.ndarray, local_model: np.ndarray | None) -> np.ndarray:
        fb = np.ascontiguousarray(feedback, dtype=np.float64)
        lm = np.ascontiguousarray(local_model, dtype=np.float64) if local_model is not None else None
        out = np.zeros((self.nlocal, self.nout))
        check(lib().sml_res_step_host(self._h, ptr(fb), ptr(lm), ptr(out)))
        return out

    def assemble(self, d_outvec_all, d_g4, d_g2, d_pr, stream=None):
        check(lib().sml_exchange_assemble(self._h, ptr(d_outvec_all), ptr(d_g4), ptr(d_g2), ptr(d_pr),
                                          stream_ptr(stream)))

    def tile_inputs(self, d_g4, d_g2, d_pr, d_fc4, d_fc2, d_tisr, d_feedback, d_local_model, stream=None):
        check(lib().sml_res_tile_inputs(self._h, ptr(d_g4), ptr(d_g2), ptr(d_pr), ptr(d_fc4), ptr(d_fc2),
                                        ptr(d_tisr), ptr(d_feedback), ptr(d_local_model), stream_ptr(stream)))

    def tile_feedback(self, d_g4, d_g2, d_pr, d_tisr, d_feedback, stream=None):
        check(lib().sml_res_tile_feedback(self._h, ptr(d_g4), ptr(d_g2), ptr(d_pr), ptr(d_tisr), ptr(d_feedback),
                                          stream_ptr(stream)))

    def tile_local_model(self, d_fc4, d_fc2, d_local_model, stream=None):
        check(lib().sml_res_tile_local_model(self._h, ptr(d_fc4), ptr(d_fc2), ptr(d_local_model),
                                             stream_ptr(stream)))

    # --- measurement
    def footprint(self):
        w = ctypes.c_int64()
        a = ctypes.c_int64()
        check(lib().sml_res_footprint(self._h, ctypes.byref(w), ctypes.byref(a)))
        return w.value, a.value

    def enable_timing(self, capacity: int):
        check(lib().sml_res_enable_timing(self._h, capacity))

    def kernel_times(self, max_steps: int = 100000):
        upd = np.zeros(max_steps, dtype=np.float32)
        rd = np.zeros(max_steps, dtype=np.float32)
        cnt = ctypes.c_int()
        check(lib().sml_res_kernel_times(self._h, ptr(upd), ptr(rd), max_steps, ctypes.byref(cnt)))
        return upd[:cnt.value].astype(np.float64), rd[:cnt.value].astype(np.float64)


def read_region_netcdf(path: str) -> dict:
    """Read a worker_XXXX_level_1_<trial>.nc weight file (read_trained_res layout)."""
    dims = np.zeros(6, dtype=np.int64)
    p = os.fsencode(path)
    check(lib().sml_nc_read_region(p, ptr(dims), None, None, None, None, None, None, None))
    n, ninp, nout, ncsn, k, nms = (int(v) for v in dims)
    out = {
        "win": np.zeros((ninp, n), dtype=np.float32),
        "wout": np.zeros((ncsn, nout), dtype=np.float32),
        "rows": np.zeros(k, dtype=np.int32),
        "cols": np.zeros(k, dtype=np.int32),
        "vals": np.zeros(k, dtype=np.float32),
        "mean": np.zeros(nms, dtype=np.float32),
        "std": np.zeros(nms, dtype=np.float32),
    }
    check(lib().sml_nc_read_region(p, ptr(dims), ptr(out["win"]), ptr(out["wout"]), ptr(out["rows"]),
                                   ptr(out["cols"]), ptr(out["vals"]), ptr(out["mean"]), ptr(out["std"])))
    return out


def write_region_netcdf(path: str, win, wout, rows, cols, vals, mean, std) -> None:
    """Write the reference's per-region weight layout (write_trained_res), CDF-1."""
    win = np.ascontiguousarray(win, dtype=np.float32)
    wout = np.ascontiguousarray(wout, dtype=np.float32)
    ninp, n = win.shape
    ncsn, nout = wout.shape
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    mean = np.ascontiguousarray(mean, dtype=np.float32)
    std = np.ascontiguousarray(std, dtype=np.float32)
    check(lib().sml_nc_write_region(os.fsencode(path), n, ninp, nout, ncsn, len(rows), ptr(win), ptr(wout),
                                    ptr(rows), ptr(cols), ptr(vals), ptr(mean), ptr(std)))

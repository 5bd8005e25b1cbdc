/*
 * speedy_ml.h -- C ABI of the MI355X-native SPEEDY-ML hybrid hot path.
 *
 * Plain C: pointers, sizes and status codes; no torch or HIP C++ types.  Every
 * device pointer argument (d_*) is a gfx950 device address; every other pointer
 * is host memory owned by the caller.  Streams are passed as `void*` holding a
 * hipStream_t (NULL = the legacy default stream).  Functions return SML_OK (0)
 * or a negative SML_ERR_* code; sml_last_error() gives the message (per thread).
 *
 * Array layouts are the reference's Fortran layouts (column-major), so a Fortran
 * host passes its arrays unchanged:
 *   spectral field   v(mx2=62, nx=32)            -> 1984 doubles, m fastest
 *   grid field       g(ix=96, il=48)             -> 4608 doubles, x fastest, row 1 south
 *   grid4d           (4, 96, 48, 8)  = (var,x,y,z), var = T,u,v,q[g/kg]
 *   grid2d / precip  (96, 48)
 *   W_in             win(n, ninp)       (NetCDF file: win[win_y=ninp][win_x=n])
 *   W_out            wout(nout, ncs+n)  (NetCDF file: wout[wout_y=ncs+n][wout_x=nout])
 *   A                COO rows/cols (1-based), vals, k entries, duplicates additive
 * Batched calls take fields back to back (field stride 1984 or 4608 doubles).
 *
 * Reference interfaces replaced:
 *   sml_grid_batched     <- grid   (src/spe_spectral.f90:389-401)
 *   sml_spec_batched     <- spec   (src/spe_spectral.f90:403-414)
 *   sml_vdspec_batched   <- vdspec (src/spe_spectral.f90:416-452)
 *   sml_uvspec_batched   <- uvspec (src/spe_spectral.f90:351-387)
 *   sml_spectral_create  <- parmtr + inifft (src/spe_spectral.f90:45-192,
 *                           src/spe_subfft_fftpack.f90:1-11)
 *   sml_res_create / sml_res_load_region_*
 *                        <- trained_reservoir_prediction + read_trained_res +
 *                           allocate_res_new + mklsparse
 *                           (src/mod_reservoir.f90:1781-1884, :78-178;
 *                            src/mod_io.f90:2911-2956; src/mod_linalg.f90:10-25)
 *   sml_res_step         <- predict / predict_ml for every region on the rank
 *                           (src/mod_reservoir.f90:1416-1533, called per region from
 *                            src/parallelmain.f90:225-234)
 *   sml_exchange_assemble <- the root half of sendrecievegrid: outvec tiles into the
 *                           global grid + clips (src/mpires.f90:300-478,
 *                            src/res_domain.f90:769-804)
 *   sml_res_tile_inputs  <- the scatter half of sendrecievegrid: overlap input tiles,
 *                           SPEEDY local vectors, standardisation
 *                           (src/mpires.f90:558-751, src/res_domain.f90:1000-1293)
 *   sml_nc_read_region   <- read_trained_res (src/mod_io.f90:2911-2956), NetCDF-3
 *                           classic reader for the per-region weight files
 *   sml_nc_write_region  <- write_trained_res (src/mod_reservoir.f90:1701-1736,
 *                           src/mod_io.f90:1247-1496)
 *   sml_dyn_create       <- indyns (+ parmtr, inifft) (src/ini_indyns.f90:1-128)
 *   sml_dyn_impint       <- impint (src/ini_impint.f90:1-153, spe_matinv.f90)
 *   sml_dyn_step         <- step (src/dyn_step.f90:1-128: grtend, sptend, implic,
 *                           geop, hordif, timint; dyn_grtend.f90, dyn_sptend.f90,
 *                           dyn_implic.f90, dyn_geop.f90)
 *   sml_dyn_leapfrog     <- the step(2,2,...) loop of stloop (src/dyn_stloop.f90:43)
 *   sml_dyn_window       <- stepone + stloop of one agcm_main window (src/ini_stepone.f90,
 *                           src/dyn_stloop.f90:37-56; run_model, src/mpires.f90:1605)
 *   sml_dyn_from_grid    <- iogrid(30) (src/ppo_iogrid.f90:497-571)
 *   sml_dyn_to_grid      <- iogrid(31) (src/ppo_iogrid.f90:573-595)
 */
#ifndef SPEEDY_ML_H
#define SPEEDY_ML_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SML_OK 0
#define SML_ERR_ARG (-1)
#define SML_ERR_HIP (-2)
#define SML_ERR_NOMEM (-3)
#define SML_ERR_STATE (-4)
#define SML_ERR_IO (-5)
#define SML_ERR_FORMAT (-6)

#define SML_F32 1
#define SML_F64 2

/* T30L8 grid constants (mod_atparam.f90:9-14) */
#define SML_MX 31
#define SML_NX 32
#define SML_MX2 62
#define SML_IX 96
#define SML_IL 48
#define SML_KX 8
#define SML_SPEC_FIELD 1984 /* 62*32 doubles */
#define SML_GRID_FIELD 4608 /* 96*48 doubles */

const char *sml_last_error(void);
int sml_abi_version(void);

/* ----------------------------------------------------------------- spectral */
typedef struct sml_spectral sml_spectral;

/* parmtr(a) + inifft: builds the Gaussian latitudes, Legendre tables (T30) and the
 * Fourier matrices on the host, uploads them to the current device. */
int sml_spectral_create(double radius, sml_spectral **out);
int sml_spectral_destroy(sml_spectral *s);
/* host copies of the tables (any pointer may be NULL):
 * sia[24], wt[24], cpol[24*32*62] (cpol(mx2,nx,iy) column-major), nsh2[32] */
int sml_spectral_tables(const sml_spectral *s, double *sia, double *wt, double *cpol, int *nsh2);

/* grid: spectral -> grid for nfields fields; kcos = 1 (plain) or 2 (x 1/cos lat) */
int sml_grid_batched(sml_spectral *s, const double *d_spec, double *d_grid, int nfields, int kcos, void *stream);
/* spec: grid -> spectral */
int sml_spec_batched(sml_spectral *s, const double *d_grid, double *d_spec, int nfields, void *stream);
/* stage-level entry points (gridy / gridx / specx / specy), Fourier buffers are
 * varm(mx2=62, il=48) per field */
int sml_gridy_batched(sml_spectral *s, const double *d_spec, double *d_varm, int nfields, void *stream);
int sml_gridx_batched(sml_spectral *s, const double *d_varm, double *d_grid, int nfields, int kcos, void *stream);
int sml_specx_batched(sml_spectral *s, const double *d_grid, double *d_varm, int nfields, void *stream);
int sml_specy_batched(sml_spectral *s, const double *d_varm, double *d_spec, int nfields, void *stream);
/* vdspec: (u,v) grid -> (vor,div) spectral, kcos 2: u*1/cos, else u*1/cos^2 */
int sml_vdspec_batched(sml_spectral *s, const double *d_ug, const double *d_vg, double *d_vor, double *d_div,
                       int nfields, int kcos, void *stream);
/* uvspec: (vor,div) spectral -> (u cos, v cos) spectral */
int sml_uvspec_batched(sml_spectral *s, const double *d_vor, const double *d_div, double *d_ucos, double *d_vcos,
                       int nfields, void *stream);
/* host convenience (synchronous, one call = H2D + kernels + D2H): used by the
 * single-field drop-ins and the Fortran binding tests */
int sml_grid_host(sml_spectral *s, const double *spec, double *grid, int nfields, int kcos);
int sml_spec_host(sml_spectral *s, const double *grid, double *spec, int nfields);

/* ---------------------------------------------------------------- reservoirs */
typedef struct sml_reservoirs sml_reservoirs;

/* One context per rank: the regions listed in region_ids (0-based global region
 * numbers of a numregions decomposition, res_domain.f90:31-62), bottom level with
 * logp/precip/tisr inputs, sst input where sst_flags[i] != 0.
 *   n[i], k[i]      reservoir size and nnz of A for local region i
 *   chunk_speedy    132 (hybrid, predict) or 0 (ML-only, predict_ml)
 *   nout            136 (chunk_size_prediction)
 *   weight_dtype    SML_F32: W_in/A/W_out held as fp32 (exact for weights read from
 *                   the NF90_REAL files); SML_F64: held as fp64.  Arithmetic is fp64.
 *   leakage         reservoir%leakage (1.0 in the reference, mod_reservoir.f90:97) */
int sml_res_create(int numregions, int nlocal, const int *region_ids, const unsigned char *sst_flags,
                   const int *n, const int *k, int chunk_speedy, int nout, int weight_dtype, double leakage,
                   sml_reservoirs **out);
int sml_res_destroy(sml_reservoirs *c);
/* A reservoir context for a different reservoir of the same shape: ninp[i] given per
 * region (no geometry-derived inputs, no exchange/tiling tables), nout outputs each
 * unstandardized with mean/std slot out_index[o] (0-based, -1 = none), a local-model
 * block of chunk_speedy columns.  Used for the slab-ocean reservoir
 * (src/mod_slab_ocean_reservoir.f90: inputs averaged atmosphere + sst, outputs the
 * region's sst points, all unstandardized with the sst slot 36 -> out_index 35). */
int sml_res_create_generic(int numregions, int nlocal, const int *region_ids, const int *ninp, const int *n,
                           const int *k, int chunk_speedy, int nout, const signed char *out_index, int weight_dtype,
                           double leakage, sml_reservoirs **out);
/* predict_slab (src/mod_slab_ocean_reservoir.f90:1201-1249) for every local region:
 * x = tanh(A x + W_in feedback), outvec = W_out [local_model; x~] unstandardized, and
 * the raw outvec (before unstandardize) into d_local_model_next -- the reference's
 * local_model = outvec (:1235).  chunk_speedy must equal nout; the two local-model
 * buffers must not alias (swap them between steps). */
int sml_res_step_slab(sml_reservoirs *c, const double *d_feedback, const double *d_local_model,
                      double *d_local_model_next, double *d_outvec, void *stream);
/* ninp of local region i (from geometry + sst flag) */
int sml_res_ninp(const sml_reservoirs *c, int i, int *ninp);
/* packed feedback layout: offsets[nlocal+1] (in doubles) */
int sml_res_feedback_offsets(const sml_reservoirs *c, int64_t *offsets);
/* load region i from reference-layout host arrays (see header comment); mean/std[36] */
int sml_res_load_region_f32(sml_reservoirs *c, int i, const int *rows, const int *cols, const float *vals,
                            const float *win, const float *wout, const double *mean, const double *std);
int sml_res_load_region_f64(sml_reservoirs *c, int i, const int *rows, const int *cols, const double *vals,
                            const double *win, const double *wout, const double *mean, const double *std);
/* state x (current_state) of region i, host arrays of n doubles */
int sml_res_set_state(sml_reservoirs *c, int i, const double *x);
int sml_res_get_state(sml_reservoirs *c, int i, double *x);
/* One prediction step for every local region (predict, mod_reservoir.f90:1416):
 *   d_feedback    packed feedback vectors (sml_res_feedback_offsets)
 *   d_local_model [nlocal][chunk_speedy] standardized SPEEDY vectors (ignored if 0)
 *   d_outvec      [nlocal][nout] unstandardized outputs */
int sml_res_step(sml_reservoirs *c, const double *d_feedback, const double *d_local_model, double *d_outvec,
                 void *stream);
/* The same step in two halves, so the reservoir's share overlaps SPEEDY's window:
 * outvec = W_out(:,1:ncs) local_model + W_out(:,ncs+1:) x~ is split at column ncs
 * exactly as the reference's outvec_component_contribs (v_p + v_ml,
 * src/mod_reservoir.f90:1456-1459).
 *   begin:  x update from d_feedback, then v_ml into a context-owned buffer
 *           (~98 % of the step's bytes; needs no SPEEDY output)
 *   finish: v_p from d_local_model, outvec = v_p + v_ml, unstandardize
 * sml_res_step == begin + finish on one stream.  Each begin needs one finish
 * before the next begin (SML_ERR_STATE otherwise). */
int sml_res_step_begin(sml_reservoirs *c, const double *d_feedback, void *stream);
int sml_res_step_finish(sml_reservoirs *c, const double *d_local_model, double *d_outvec, void *stream);
/* discard a begun step (a begin without its finish, e.g. the pipelined loop's
 * next begin when the host restarts the prediction): waits for the device, then rolls
 * the state back to the one the begin read.  No-op when nothing is begun.
 * sml_res_set_state discards a begun step itself.  sml_res_step_begun: 1 while a
 * begin waits for its finish. */
int sml_res_step_cancel(sml_reservoirs *c);
int sml_res_step_begun(const sml_reservoirs *c, int *begun);
/* finish straight from SPEEDY's forecast grids: the local-model tiling of
 * sml_res_tile_local_model (res_domain.f90:1000-1031, standardize_state_vec_res
 * :1189-1293) fused into sml_res_step_finish, one launch; identical results.
 * d_local_model (may be NULL) also receives the tiled vectors. */
int sml_res_step_finish_grid(sml_reservoirs *c, const double *d_fc4d, const double *d_fc2d, double *d_local_model,
                             double *d_outvec, void *stream);
/* sml_res_step_finish_grid + sml_exchange_assemble of the same outvecs in one launch
 * (sendrecievegrid's assembly with the root's clips, src/mpires.f90:430-478): for a
 * context that holds every region in global order (one rank), where the exchange is
 * the identity.  d_outvec receives the outvecs as well; identical results. */
int sml_res_step_finish_assemble(sml_reservoirs *c, const double *d_fc4d, const double *d_fc2d,
                                 double *d_local_model, double *d_outvec, double *d_grid4d, double *d_grid2d,
                                 double *d_precip, void *stream);
/* cap on the waves of the v_ml readout issued by sml_res_step_begin (0 = one wave per
 * 8-row item, the default cap is 2048).  The cap leaves HBM headroom for SPEEDY when
 * both share CUs; on CUs of their own (sml_stream_create_cu_range) it is not needed. */
int sml_res_set_read_waves(sml_reservoirs *c, int waves);
/* The fallback paths, forced for every region -- the defaults take them only where a
 * region's structure does not fit the fast layout, and give the same bits: A and W_in
 * read from their CSR copies (SML_RES_PATH_CSR; before any region is loaded), the
 * state update one block per (region, part) instead of the balanced persistent grid
 * (SML_RES_PATH_PER_REGION), the v_p finish one thread per output instead of in
 * column groups (SML_RES_PATH_UNGROUPED_FINISH), the training drive one update launch
 * per column after a column-writer launch instead of one persistent launch per batch
 * (SML_RES_PATH_STEPWISE_DRIVE), sml_res_spectral_radius's vectors in the context's
 * global scratch instead of LDS (SML_RES_PATH_RADIUS_GLOBAL).  For tests and for a
 * host bisecting a difference; 0 restores the defaults. */
#define SML_RES_PATH_CSR 1
#define SML_RES_PATH_PER_REGION 2
#define SML_RES_PATH_UNGROUPED_FINISH 4
#define SML_RES_PATH_STEPWISE_DRIVE 8
#define SML_RES_PATH_RADIUS_GLOBAL 16
int sml_res_set_reference_paths(sml_reservoirs *c, int flags);
/* The spectral radius of every local region's A as loaded: gen_res's sparse_eigen
 * (src/mod_reservoir.f90:190; ARPACK dnaupd / dneupd, src/mod_linalg.f90:219-514)
 * for a matrix with no negative entry, which makesparse's is (RANDOM_NUMBER values,
 * src/mod_linalg.f90:191).  Power iteration from x = 1 in the max norm, at most
 * max_iter times:
 *   y = A x      each row summed in the order of its entries, fp64
 *   lo = min, hi = max of y_i / x_i over the rows with x_i > 0
 *   m = max y_i; m == 0 ends with SML_RADIUS_ZERO; x = y / m
 *   hi - lo <= tol * hi ends with SML_RADIUS_OK
 * With x > 0, lo <= rho(A) <= hi (Collatz-Wielandt), so the two outputs enclose the
 * radius up to the rounding of the row sums; min and max leave no summation order
 * open, so the outputs are the same bits on every path.  One launch, a workgroup per
 * region, x and y in LDS where 2 n doubles fit, else in a scratch of the context.
 * lo, hi, iters, info: host arrays of nlocal, filled when the call returns (it waits
 * for `stream`: a set-up call).  A negative or non-finite entry gives that region
 * SML_RADIUS_INVALID; the other regions are not affected. */
#define SML_RADIUS_OK 0      /* hi - lo <= tol * hi */
#define SML_RADIUS_MAXITER 1 /* lo, hi are the last iteration's */
#define SML_RADIUS_ZERO 2    /* A x vanished: lo = hi = 0 */
#define SML_RADIUS_INVALID 3 /* a negative or non-finite entry: lo = hi = NaN */
int sml_res_spectral_radius(sml_reservoirs *c, double tol, int max_iter, double *lo, double *hi, int *iters,
                            int *info, void *stream);
/* One region's untrained reservoir on the host, no GPU: makesparse's A before gen_res
 * scales it (src/mod_linalg.f90:180-218, shuffle: src/mod_utilities.f90:1562-1589) and
 * train_reservoir's block-diagonal W_in (src/mod_reservoir.f90:260-278), from a
 * counter-based generator keyed by (seed, region) alone -- the recipe is in
 * csrc/sml_genres.cpp.  rows / cols [k] 1-based, vals [k] in [0, 1) on the 2^-24 grid;
 * row r of W_in holds win_val[r] (never 0, |.| <= sigma) in column win_col[r] = r / (n / ninp).
 * n in 1..65535, k >= 0, ninp >= 1 dividing n, region >= 0; else SML_ERR_ARG. */
int sml_gen_region(int n, int k, int ninp, uint64_t seed, int region, double sigma, int *rows, int *cols,
                   float *vals, int *win_col, float *win_val);
/* the number of CUs the context's launches get (its stream's CU mask; 0 = the whole
 * device): the balanced state update runs one block per CU over equal shares of all
 * local rows.  sml_res_update_balanced: 1 when the update takes that form (every
 * region's A / W_in in ELL form, n <= 7168, ninp <= 1024), 0 for the per-region form;
 * both give bit-identical states. */
int sml_res_set_update_cus(sml_reservoirs *c, int cus);
int sml_res_update_balanced(sml_reservoirs *c, int *balanced);
/* the compressed form of local region i's A and W_in the state update reads
 * (DESIGN.md §3.1): a_width = A's ELL main slots per row (0: the CSR copy),
 * a_overflow = 1 when rows of a_width + 1 entries keep their last entry in an
 * overflow list, win_q > 0 when W_in is block-diagonal with win_q rows per input (its
 * column i / win_q is computed, not read), win_ell = 1 when W_in is read in ELL form.
 * Layout only: every form gives bit-identical states. */
int sml_res_ell_layout(sml_reservoirs *c, int i, int *a_width, int *a_overflow, int *win_q, int *win_ell);
/* the form of sml_res_step_begin (predict's update + the v_ml half of the readout,
 * src/mod_reservoir.f90:1440-1455): 0 = the update grid, then the readout grid;
 * 1 = one launch, a block per region that updates its state and then streams its
 * W_out rows (k_res_begin, up to 3 blocks per CU); 2 = the same with the W_out loads
 * unrolled twice (1 block per CU).  Every form gives bit-identical states and sums.
 * The fused forms need the 17-row readout and <= 64 KB of LDS per region; otherwise
 * form 0 runs (sml_res_begin_fused says which). */
int sml_res_set_begin_mode(sml_reservoirs *c, int mode);
int sml_res_begin_fused(const sml_reservoirs *c, int *fused);
/* synchronize (src/mod_reservoir.f90:1352-1378), the spin-up of start_prediction
 * (:938-959): `length` updates x = (1-leak) x + leak tanh(A x + W_in u_t) for every
 * local region, no readout.  d_inputs holds `length` blocks in the packed feedback
 * layout, block t at d_inputs + t * stride doubles (stride >= total feedback). */
int sml_res_synchronize(sml_reservoirs *c, const double *d_inputs, int length, int64_t stride, void *stream);
/* start_prediction (src/mod_reservoir.f90:938-959): synchronize_print (:1381-1414) over
 * the first `length` blocks of d_inputs (layout as sml_res_synchronize; the reference
 * uses synclength/timestep - 1 blocks of its prediction data), then block `length`
 * copied into d_feedback.  The local model of the first step comes from SPEEDY's
 * forecast (sml_res_tile_local_model or the hybrid loop's start). */
int sml_res_start_prediction(sml_reservoirs *c, const double *d_inputs, int length, int64_t stride,
                             double *d_feedback, void *stream);
/* The training drive: reservoir_layer_chunking_hybrid (src/mod_reservoir.f90:1065-1173)
 * with the first lines of chunking_matmul (:1662-1675) -- what sml_train_accumulate
 * consumes -- for one batch of m columns and every local region, "record, then advance".
 * For column c = 0 .. m-1, with u_c the region's part of input block c
 * (d_inputs + c * stride, the packed feedback layout; stride as sml_res_synchronize):
 *   rows ncs .. ncs+n-1 of column c of the region's state block = the current state x
 *     with every 0-based odd node squared (states(2:n:2,:)**2, :1133);
 *   rows 0 .. ncs-1 = the region's ncs values of model block c (d_model +
 *     c * model_stride, laid out [nlocal][ncs] like d_local_model; model_stride >=
 *     nlocal * ncs; d_model is ignored and may be NULL when chunk_speedy == 0);
 *   column c of the region's target block = the nout target entries of u_c
 *     (tile_full_input_to_target_data2d, res_domain.f90:602-651; sml_region_target_index);
 *   then x = (1-leak) x + leak tanh(A x + W_in u_c), bitwise sml_res_synchronize's update.
 * d_states: the layout sml_train_accumulate reads -- regions back to back, region i's
 * block (ncs + n_i) x m column-major, starting at m * sum_{j<i} (ncs + n_j).
 * d_targets: per region nout x m column-major, back to back; NULL skips it; non-NULL
 * on a sml_res_create_generic context (no geometry) is SML_ERR_ARG until
 * sml_res_set_target_index has given that context a target table.
 * The discard phase is sml_res_synchronize over the first blocks from x = 0; batch b
 * is then one call on the next m blocks.  Every batch advances from the unsquared
 * state (the reference's ML-only form restarts from the squared column, :1032: a
 * deliberate difference), and the last batch ends with one advance the reference
 * does not make.  m == 0 is a no-op.  Stream-ordered, no host synchronisation.
 * One launch per batch, a workgroup per region with the state in LDS; with
 * SML_RES_PATH_STEPWISE_DRIVE, or where a region's two states + two inputs exceed the
 * device's LDS per workgroup, m launches of the update. */
int sml_res_train_drive(sml_reservoirs *c, const double *d_inputs, int m, int64_t stride, const double *d_model,
                        int64_t model_stride, double *d_states, double *d_targets, void *stream);
/* the targets of a sml_res_create_generic context (the slab-ocean reservoir): idx
 * [nlocal][nout] host ints, idx[i][o] the 0-based position in local region i's feedback
 * of target o.  Afterwards sml_res_train_drive accepts d_targets on that context and
 * writes u_c[idx] per column through both drive forms; the state columns and the final
 * state do not depend on whether targets are written.  Every index is checked before
 * anything changes; the upload waits for the device.  SML_ERR_ARG: a NULL argument; a
 * context with a geometry (its own table stays the only one); a context with members > 1;
 * an index outside [0, ninp[i]).  SML_ERR_STATE inside a begun step.  The slab's
 * positions: sml_slab_target_index. */
int sml_res_set_target_index(sml_reservoirs *c, const int32_t *idx);
/* sml_res_train_drive with the targets of column c read from d_target_inputs +
 * c * target_stride (the packed feedback layout, target_stride >= total feedback; global
 * memory) while the states are driven by d_inputs: the clean series beside the noised one
 * (sml_res_input_noise).  Both drive forms serve it.  With d_target_inputs == d_inputs
 * and equal strides every output is bit for bit sml_res_train_drive's.  d_target_inputs
 * is not read (and may be NULL) when d_targets is NULL. */
int sml_res_train_drive_from(sml_reservoirs *c, const double *d_inputs, int m, int64_t stride,
                             const double *d_target_inputs, int64_t target_stride, const double *d_model,
                             int64_t model_stride, double *d_states, double *d_targets, void *stream);
/* The reference's input noise (gaussian_noise_1d_function, gaussian_noise_1d_function_precip:
 * src/mod_utilities.f90:1380-1456), reproducible: DESIGN.md §3.11.  Entry e (0-based, within
 * its region's feedback) of the block of absolute step t draws, with the generator of
 * sml_gen_region keyed by (seed, the region's noise id),
 *   b1 = draw(stream 4, (t << 20) | e) >> 11,  u1 = (b1 + 1) 2^-53 in (0, 1]
 *   b2 = draw(stream 5, (t << 20) | e) >> 11,  u2 = b2 2^-53 in [0, 1)
 *   g  = sqrt(-2 log(u1)) cospi(2 u2)
 * and becomes x + (g * noisemag) * x; a precipitation entry (slot 34), when precip_epsilon
 * > 0 and the context has a geometry, becomes instead, with its region's adopted mean / std,
 *   p = eps (exp(x std + mean) - 1);  p = |p + g noisemag|;  (log(1 + p / eps) - mean) / std.
 * noisemag == 0 copies x (a -0.0 keeps its sign).  One rounding per operation.
 * sml_res_set_input_noise stores the configuration.  ids: host [nlocal] noise ids (>= 0),
 * or NULL: the context's region ids (the local index on a sml_res_create_generic context),
 * so a rank's share of the regions draws what a context of all regions draws.  SML_ERR_ARG: a
 * negative or non-finite noisemag or precip_epsilon, a NULL context, members > 1, a negative
 * id, a region with ninp >= 2^20.  SML_ERR_STATE inside a begun step.  A context that never
 * calls it allocates and launches nothing new.
 * sml_res_input_noise writes blocks t0 .. t0 + m - 1, block j read at d_in + j * in_stride
 * and written at d_out + j * out_stride (both strides >= total feedback; d_out == d_in with
 * equal strides is allowed).  d_in == NULL writes g itself for every entry.  One launch,
 * stream-ordered, no host synchronisation; m == 0 is a no-op.  SML_ERR_ARG: m < 0, steps
 * outside [0, 2^43), a short stride, a NULL d_out; SML_ERR_STATE before the setter. */
int sml_res_set_input_noise(sml_reservoirs *c, double noisemag, uint64_t seed, double precip_epsilon,
                            const int32_t *ids);
int sml_res_input_noise(sml_reservoirs *c, const double *d_in, int64_t in_stride, double *d_out, int64_t out_stride,
                        int64_t t0, int m, void *stream);
/* the two 53-bit integers b1, b2 above, on the host (no device is touched): the device's
 * own functions.  SML_ERR_ARG: region < 0, t outside [0, 2^43), e outside [0, 2^20), NULL. */
int sml_noise_bits(uint64_t seed, int region, int64_t t, int64_t e, uint64_t *b1, uint64_t *b2);
/* host convenience: H2D, step, D2H (synchronous) */
int sml_res_step_host(sml_reservoirs *c, const double *feedback, const double *local_model, double *outvec);
/* bytes of weights + state resident on the device (for roofline bookkeeping) */
int sml_res_footprint(const sml_reservoirs *c, int64_t *weight_bytes, int64_t *algorithmic_bytes_per_step);
/* timing hook: with capacity > 0, the next `capacity` sml_res_step calls record HIP
 * events around their update and readout kernels on the step's stream (0 = off).
 * sml_res_kernel_times waits for them and returns per-step milliseconds, then
 * rearms the recorder. */
int sml_res_enable_timing(sml_reservoirs *c, int capacity);
int sml_res_kernel_times(sml_reservoirs *c, float *update_ms, float *readout_ms, int max_steps, int *count);
/* Ensemble members: several states of every local region -- forecasts from perturbed
 * initial conditions -- advanced through the same weights, which are then read once
 * per step for a tile of members instead of once per member.
 * sml_res_set_members: 1 .. SML_RES_MAX_MEMBERS members (1 at create: the context as it
 * always was).  Member 0 keeps its state, the members kept on shrinking keep theirs,
 * new members start from x = 0.  A set-up call (it waits for the device); SML_ERR_STATE
 * inside a begun step, SML_ERR_ARG out of range.
 * sml_res_set_state / _get_state are member 0 of the _member pair; setting a state
 * discards a begun step.
 * sml_res_step_members: sml_res_step for every member.  Member e's packed feedback is
 * at d_feedback + e * fb_stride, its [nlocal][chunk_speedy] local model at
 * d_local_model + e * lm_stride (ignored when chunk_speedy is 0), its [nlocal][ld]
 * outvecs (ld: sml_res_set_outvec_ld) at d_outvec + e * ov_stride, strides in doubles;
 * fb_stride >= the packed feedback size, lm_stride >= nlocal * chunk_speedy, ov_stride
 * >= nlocal * ld, else SML_ERR_ARG.  Stream-ordered, no host synchronisation; every
 * member advances in the one call.  The timing hook stamps it like sml_res_step.
 * sml_res_synchronize_members: sml_res_synchronize for every member, block t of member
 * e at d_inputs + t * stride + e * member_stride.
 * For every member, outvecs and state are bit for bit those of sml_res_step
 * (sml_res_synchronize) on a single-member context of the same weights started from
 * that member's state and given that member's inputs.
 * While the context holds more than one member, the single-member calls that advance
 * the state -- sml_res_step, _step_begin, _step_slab, _synchronize, _start_prediction,
 * _train_drive, _step_host -- return SML_ERR_STATE; sml_res_set_members(c, 1) makes
 * them available again.
 * sml_res_member_tile: the members one update block serves (bounded by the device's
 * LDS where the region's state is staged there: update_lds 1) and the members one
 * W_out load of the readout serves; W_out is streamed ceil(members / readout_tile)
 * times per step. */
#define SML_RES_MAX_MEMBERS 32
int sml_res_set_members(sml_reservoirs *c, int members);
int sml_res_members(const sml_reservoirs *c, int *members);
int sml_res_set_state_member(sml_reservoirs *c, int member, int i, const double *x);
int sml_res_get_state_member(sml_reservoirs *c, int member, int i, double *x);
int sml_res_step_members(sml_reservoirs *c, const double *d_feedback, int64_t fb_stride,
                         const double *d_local_model, int64_t lm_stride, double *d_outvec, int64_t ov_stride,
                         void *stream);
int sml_res_synchronize_members(sml_reservoirs *c, const double *d_inputs, int length, int64_t stride,
                                int64_t member_stride, void *stream);
int sml_res_member_tile(const sml_reservoirs *c, int *update_tile, int *update_lds, int *readout_tile);
/* The split step for every member: sml_res_step_begin / _finish / _finish_grid /
 * _finish_assemble with a member dimension, so that an E-member hybrid forecast runs its
 * update and v_ml (about 98 % of the bytes) beside SPEEDY's windows and only the v_p finish
 * behind them.  Member e's data is at e * stride doubles of each array, as in
 * sml_res_step_members; every stride is checked against its packed size (SML_ERR_ARG naming
 * it): fb_stride, lm_stride, ov_stride as there, the forecast and grid strides >= 8*48*96*4
 * (fc4_stride, g4_stride) and >= 48*96 (fc2_stride, g2_stride: logp, and precip with it).
 * sml_res_step_begin_members: every member's update, then every member's v_ml into
 * context-owned partial sums (laid out by sml_res_set_members); two launches; the v_ml
 * launch honours sml_res_set_read_waves as a cap on its waves.  All members advance
 * together: one sml_res_step_cancel rolls all of them back, sml_res_step_begun reports
 * the step, sml_res_set_state_member discards it; sml_res_set_members, _step_members and
 * _synchronize_members inside it return SML_ERR_STATE.
 * sml_res_step_finish_members: per member v_p + v_ml from that member's local model,
 * unstandardized.  sml_res_step_finish_grid_members: each member's local model is first
 * tiled and standardized from that member's forecast grids (and written to d_local_model
 * when given), one block per (region, tile of members): sml_res_member_finish_tile
 * reports the tile (1 at more than one member: the single-member kernel once per member).
 * sml_res_step_finish_assemble_members also scatters each member's outputs into that
 * member's grids with the root's clips (every region on this rank, in global order).
 * None of them waits in-kernel for a forecast: order the stream behind the windows.
 * For every member, outvecs, local models, grids and state are bit for bit those of the
 * single-member calls on a context of its own.  At one member the four calls are the
 * single-member calls (the same kernels, the fused begin where the shape takes it) and
 * pair freely with them.  At more than one member sml_res_step_begin keeps refusing, and
 * the single-member finishes return SML_ERR_STATE and leave the step begun. */
int sml_res_step_begin_members(sml_reservoirs *c, const double *d_feedback, int64_t fb_stride, void *stream);
int sml_res_step_finish_members(sml_reservoirs *c, const double *d_local_model, int64_t lm_stride,
                                double *d_outvec, int64_t ov_stride, void *stream);
int sml_res_step_finish_grid_members(sml_reservoirs *c, const double *d_fc4d, int64_t fc4_stride,
                                     const double *d_fc2d, int64_t fc2_stride,
                                     double *d_local_model /* may be NULL */, int64_t lm_stride, double *d_outvec,
                                     int64_t ov_stride, void *stream);
int sml_res_step_finish_assemble_members(sml_reservoirs *c, const double *d_fc4d, int64_t fc4_stride,
                                         const double *d_fc2d, int64_t fc2_stride,
                                         double *d_local_model /* may be NULL */, int64_t lm_stride,
                                         double *d_outvec, int64_t ov_stride, double *d_grid4d, int64_t g4_stride,
                                         double *d_grid2d, double *d_precip, int64_t g2_stride, void *stream);
int sml_res_member_finish_tile(const sml_reservoirs *c, int *finish_tile);

/* ------------------------------------------------------------- exchange/tiling */
/* Global grids: d_grid4d[4*96*48*8], d_grid2d[96*48], d_precip[96*48].
 * assemble: scatter all numregions outvecs ([numregions][nout], region-major, as
 * produced by an all-gather of every rank's d_outvec) into the grids, then clip
 * q >= 1e-6 and precip < 1e-5 -> 0. */
int sml_exchange_assemble(sml_reservoirs *c, const double *d_outvec_all, double *d_grid4d, double *d_grid2d,
                          double *d_precip, void *stream);
/* tile: build the next step's inputs of every local region from the grids:
 *   feedback atmo/logp/precip entries from the overlap tile, standardized;
 *   feedback tisr entries copied from d_tisr (packed [nlocal][in2d], already
 *   standardized, may be NULL = keep); sst entries kept as they are;
 *   local_model from the SPEEDY forecast grids d_fc4d/d_fc2d, standardized
 *   (skipped when chunk_speedy == 0 or d_fc4d == NULL). */
int sml_res_tile_inputs(sml_reservoirs *c, const double *d_grid4d, const double *d_grid2d, const double *d_precip,
                        const double *d_fc4d, const double *d_fc2d, const double *d_tisr, double *d_feedback,
                        double *d_local_model, void *stream);
/* the two halves of sml_res_tile_inputs: feedback needs only the assembled grids
 * (ready before SPEEDY runs), local_model needs SPEEDY's forecast */
int sml_res_tile_feedback(sml_reservoirs *c, const double *d_grid4d, const double *d_grid2d, const double *d_precip,
                          const double *d_tisr, double *d_feedback, void *stream);
int sml_res_tile_local_model(sml_reservoirs *c, const double *d_fc4d, const double *d_fc2d, double *d_local_model,
                             void *stream);

/* --------------------------------------------------------- NetCDF weight files */
/* Reads worker_XXXX_level_1_<trial>.nc (NetCDF-3 classic / 64-bit offset) written
 * by the reference (write_trained_res).  Sizes come from the file's dimensions:
 * dims[0]=n (win_x), dims[1]=ninp (win_y), dims[2]=nout (wout_x),
 * dims[3]=ncs+n (wout_y), dims[4]=k (rows_x), dims[5]=36 (mean_x).
 * Call once with all array pointers NULL to get dims, then again with buffers.
 * Arrays are returned in the reference layouts (fp32 values as stored). */
int sml_nc_read_region(const char *path, int64_t *dims, float *win, float *wout, int *rows, int *cols, float *vals,
                       float *mean, float *std);
/* Writes the same layout (CDF-1, big-endian) -- for tests and tooling. */
int sml_nc_write_region(const char *path, int n, int ninp, int nout, int ncs_plus_n, int k, const float *win,
                        const float *wout, const int *rows, const int *cols, const float *vals, const float *mean,
                        const float *std);

/* ---------------------------------------------------------------- dynamics */
/* SPEEDY's spectral dynamical core on the device.  The context owns the
 * prognostic state in the reference's mod_dynvar layout (mod_dynvar.f90:15-27):
 *   vor, div, t, tr   complex(mx, nx, kx, 2) -> 2*8*1984 doubles each (level 1 first)
 *   ps                complex(mx, nx, 2)     -> 2*1984 doubles
 * and the forcing phis (mod_dynvar), tcorh, qcorh (mod_hdifcon), complex(mx, nx).
 * Physics grid tendencies, when given, are phys[4][kx][il][ix] = u, v, t, q
 * (the arrays phypar adds to, dyn_grtend.f90:225-226). */
typedef struct sml_dynamics sml_dynamics;

/* indyns (src/ini_indyns.f90:1-128) + parmtr/inifft; state and forcing zeroed */
int sml_dyn_create(double radius, sml_dynamics **out);
int sml_dyn_destroy(sml_dynamics *d);
/* impint(dt, alph) (src/ini_impint.f90:1-153): must precede sml_dyn_step and be
 * repeated whenever (dt, alph) changes, as stepone does (src/ini_stepone.f90:19-34) */
int sml_dyn_impint(sml_dynamics *d, double dt, double alph);
/* phis, tcorh, qcorh (host, any may be NULL = unchanged) */
int sml_dyn_set_forcing(sml_dynamics *d, const double *phis, const double *tcorh, const double *qcorh);
/* host copies in/out of the whole prognostic state (both time levels) */
int sml_dyn_set_state(sml_dynamics *d, const double *vor, const double *div, const double *t, const double *ps,
                      const double *tr);
int sml_dyn_get_state(sml_dynamics *d, double *vor, double *div, double *t, double *ps, double *tr);
/* phi(mx, nx, kx) = geop(j4) of the last step (src/dyn_geop.f90:1-33) */
int sml_dyn_get_phi(sml_dynamics *d, double *phi);
/* tendencies of the last step before time integration, 4*kx+1 spectral fields:
 * vordt | divdt | tdt | trdt | psdt (only meaningful after a dt <= 0 step: a step
 * with dt > 0 leaves the grid-point half of grtend's tendencies there) */
int sml_dyn_get_tendencies(sml_dynamics *d, double *tend);
/* device addresses of the state buffer ([vor|div|t|tr|ps] as above) and of a
 * scratch buffer sized for phys (4*kx*4608 doubles) */
int sml_dyn_state_device(sml_dynamics *d, double **d_state, double **d_phys);
/* step(j1, j2, dt, alph, rob, wil) (src/dyn_step.f90:1-128): grtend with the
 * physics tendencies d_phys (device, may be NULL = no physics), sptend, implic,
 * hordif, stratospheric drag, timint.  Asynchronous on `stream`. */
int sml_dyn_step(sml_dynamics *d, int j1, int j2, double dt, double alph, double rob, double wil,
                 const double *d_phys, void *stream);
/* nsteps x step(2, 2, dt, alph, rob, wil) -- the leapfrog loop of stloop
 * (src/dyn_stloop.f90:43) -- replayed from one captured hipGraph (re-captured
 * when (dt, alph, rob, wil, d_phys) change).  impint(dt, alph) must be current. */
int sml_dyn_leapfrog(sml_dynamics *d, int nsteps, double dt, double alph, double rob, double wil,
                     const double *d_phys, void *stream);
/* One SPEEDY window after iogrid(30), as run_model's agcm_main runs it
 * (src/mpires.f90:1605 -> at_gcm.f90): stepone (src/ini_stepone.f90:19-34:
 * step(1,1,delt/2), step(1,2,delt), with the lradsw the previous window left) and
 * nleap x step(2,2,2 delt) with stloop's clock restarted at istep = 1
 * (src/dyn_stloop.f90:37-56).  impint tables for delt/2, delt and 2 delt are built
 * (cached) first; the whole window is one hipGraph launch.  GPU physics as set by
 * sml_dyn_set_physics (no host tendencies).  Afterwards istep = 1 + nleap and
 * impint(2 delt, alph) is current. */
int sml_dyn_window(sml_dynamics *d, int nleap, double delt, double alph, double rob, double wil, void *stream);
/* iogrid(30) (src/ppo_iogrid.f90:497-571), the window entry: variables3d
 * grid4d(4, ix, il, kx) (T, u, v, q) and logp(ix, il), device, are rounded to
 * real(4), q < 0 set to 0, transformed (vdspec / spec + trunct) into time level 1;
 * the level is transformed back and d_minmax[8] (device, may be NULL) receives
 * min/max of u, v, t, q for the safety thresholds (see sml_dyn_is_safe). */
int sml_dyn_from_grid(sml_dynamics *d, const double *d_grid4d, const double *d_logp, double *d_minmax,
                      void *stream);
/* iogrid(31) (src/ppo_iogrid.f90:573-595), the window exit: level 1 -> grid4d, logp */
int sml_dyn_to_grid(sml_dynamics *d, double *d_grid4d, double *d_logp, void *stream);
/* is_safe_to_run_speedy from the 8 min/max values (src/ppo_iogrid.f90:563-577); a NaN
 * makes the state unsafe */
int sml_dyn_is_safe(const double *minmax);
/* run_model (src/mpires.f90:1516-1628) minus its file I/O: iogrid(30) of d_grid4d /
 * d_logp with the safety check, the window (as sml_dyn_window), iogrid(31) into
 * d_fc4d / d_fc2d, then q floored at 1e-6 (:1614-1616).  When the check fails,
 * agcm_main skips the integration (at_gcm.f90:37): the forecast is then the input
 * grid with q floored (run_model's copy, :1550-1553).  The check runs beside the
 * window; sml_dyn_last_safe reads its outcome.  The forecast buffers must not alias
 * the inputs.  The window runs as a replayed hipGraph with the exit captured in it,
 * keyed on d_grid4d / d_logp / d_fc4d / d_fc2d; up to four such graphs are kept, so a
 * caller alternating two or three buffer sets (ping-pong) replays one per set, and only
 * a fifth set evicts (re-captures) one. */
int sml_dyn_run_model(sml_dynamics *d, const double *d_grid4d, const double *d_logp, int nleap, double delt,
                      double alph, double rob, double wil, double *d_fc4d, double *d_fc2d, void *stream);
/* is_safe_to_run_speedy of the last sml_dyn_from_grid / sml_dyn_run_model, i.e. the
 * run_speedy flag the reference broadcasts (src/mpires.f90:721, :1623) and stops the
 * prediction loop on (src/parallelmain.f90:268-270).  Waits only for that check;
 * minmax (may be NULL) receives its 8 values. */
int sml_dyn_last_safe(sml_dynamics *d, int *safe, double *minmax);
/* CUs [first_cu, first_cu + num_cus) for the safety check that runs beside the
 * window (iogrid(30)'s re-grid + min/max on the context's check stream); num_cus = 0
 * lets it use any CU.  The hybrid loop puts it on CUs neither SPEEDY's nor the
 * reservoir's stream uses, so its kernels never share a CU with the window's. */
int sml_dyn_set_check_cus(sml_dynamics *d, int first_cu, int num_cus);
/* the give-up time (microseconds, default 1 s) of run_model's exit waiting in-kernel
 * for the check beside the window: an exit that gives up takes its window as unsafe
 * (the forecast is the input grid) and sml_dyn_last_safe reports that window -- and
 * only that window -- unsafe.  The hybrid loop sets it with its hop timeout. */
int sml_dyn_set_check_timeout(sml_dynamics *d, int64_t microseconds);
/* the step kernels' form: 1 (default) the fused step -- two launches per leapfrog step,
 * a*b + c contracted into FMAs, within 1e-13 of the reference's window; 0 the 8/9-launch
 * step whose Fourier transforms are FFTPACK's separate multiplies and adds, bit-exact
 * with the reference's rfftb / rfftf (the two agree to rounding, 1e-11 after 6 steps).
 * Takes effect at the next step / window. */
int sml_dyn_set_fused(sml_dynamics *d, int fused);
/* the check's stream (NULL before sml_dyn_set_check_cus or the first check): work a
 * host enqueues there runs before the next window's check */
int sml_dyn_check_stream(const sml_dynamics *d, void **stream);
/* synchronous host-buffer variants */
int sml_dyn_from_grid_host(sml_dynamics *d, const double *grid4d, const double *logp, double *minmax, int *safe);
int sml_dyn_to_grid_host(sml_dynamics *d, double *grid4d, double *logp);
/* synchronous variant taking host physics tendencies (may be NULL) */
int sml_dyn_step_host(sml_dynamics *d, int j1, int j2, double dt, double alph, double rob, double wil,
                      const double *phys);

/* ---------------------------------------------------------------- physics */
/* phypar on the GPU (src/phy_phypar.f90:1-228 with convmf, lscond, cloud, radsw,
 * radlw, suflux, vdifsc; icsea = 0, lrandf and sppt off as in the hybrid runs).
 * bc: host [15][ix*il] boundary fields in this order -- fmask1, phis0 (mod_surfcon),
 * stl_am, sst_am, soilw_am (mod_var_land/sea), alb_l, alb_s, albsfc, snowc, fsol,
 * ozone, ozupp, zenit, stratz (mod_radcon), forog (mod_sflcon).  Once set, every
 * step computes the physics of time level 1 on the GPU (dyn_grtend.f90:223-226)
 * and d_phys arguments must be NULL; bc = NULL switches it off.  Call again when the
 * fields change (the coupler / sol_oz run once a day, ini_fordate.f90). */
int sml_dyn_set_physics(sml_dynamics *d, const double *bc);
/* the slab ocean's SST in the window (run_model's sst_hybrid, src/mpires.f90:1576-1584,
 * applied by agcm_init's ini_sea, src/cpl_sea.f90:38-46): sst_am = the hybrid SST where
 * the coupler's sst_am (bc's, ice-blended as sea2atm leaves it) is < 6 K above it, +
 * sst_bias, then blended with the sea ice (sice, tice).  d_sst_grid(96, 48) device,
 * read on `stream`; NULL restores the coupler's field.  Kept in force across
 * sml_dyn_set_physics calls until replaced. */
int sml_dyn_set_hybrid_sst(sml_dynamics *d, const double *d_sst_grid, double sst_bias, void *stream);
/* sea-ice fraction / temperature sice_am, tice_am (host [ngp]; NULL = no ice) */
int sml_dyn_set_sea_ice(sml_dynamics *d, const double *sice, const double *tice);
int sml_dyn_get_sea_ice(sml_dynamics *d, double *sice, double *tice);
/* host copies of the boundary fields [15][ngp] (sml_dyn_set_physics order) and of the
 * forcing phis / tcorh / qcorh (any may be NULL) as the next window reads them */
int sml_dyn_get_physics(sml_dynamics *d, double *bc);
int sml_dyn_get_forcing(sml_dynamics *d, double *phis, double *tcorh, double *qcorh);
/* ---- the window's date-driven forcing.  run_model passes each window its calendar
 * date (src/mpires.f90:1545, :1595-1598) and agcm_init rebuilds the forcing before
 * stepone (src/ini_agcm_init.f90:57-89): newdate(0) (src/mod_date.f90:17-79),
 * ini_coupler(2) (src/cpl_main_interface.f90:1-25, cpl_land.f90:1-95, cpl_sea.f90:
 * 1-200 with icland 1, icsea 0, icice 1, isstan 0), ini_sea's hybrid SST, fordate(0)
 * (src/ini_fordate.f90:1-115); agcm_1day's fordate(1) (src/at_gcm.f90:84) repeats it
 * with the same inputs.
 * surface: host [3][ngp] = fmask_l (mod_cli_land), fmask_s (mod_cli_sea), alb0
 * (mod_surfcon) as inbcon leaves them (src/ini_inbcon.f90:38-70, 140-156). */
int sml_dyn_set_surface(sml_dynamics *d, const double *surface);
/* monthly climatologies, host [5][12][ngp] = stl12, snowd12, soilw12 (mod_cli_land),
 * sst12, sice12 (mod_cli_sea), January first (src/ini_inbcon.f90:71-230).  NULL: the
 * coupler's fields stay as sml_dyn_set_physics / sml_dyn_set_sea_ice set them. */
int sml_dyn_set_climatology(sml_dynamics *d, const double *clim);
/* the forcing of a window at (iyear, imonth, iday), on `stream` before the window:
 * with a climatology the coupler at that date (stl_am, soilw_am, snow depth, sst_am,
 * sice_am, tice_am), the hybrid SST if set (sml_dyn_set_hybrid_sst), then fordate:
 * sol_oz(tyear), snowc / alb_l / alb_s / albsfc, tcorh = spec(gamlat phis0), qcorh =
 * spec(refrh1 (qref - qsfc)) from the current stl_am / sst_am.  Skipped when neither
 * the date nor any input (the setters above, set_physics / set_sea_ice / set_forcing /
 * set_hybrid_sst) changed since the last call; _ex with force != 0 recomputes. */
int sml_dyn_fordate(sml_dynamics *d, int iyear, int imonth, int iday, void *stream);
int sml_dyn_fordate_ex(sml_dynamics *d, int iyear, int imonth, int iday, int force, void *stream);
/* fordate recomputations issued so far (skipped calls not counted) */
int sml_dyn_fordate_count(const sml_dynamics *d, int *count);
/* stloop's clock (dyn_stloop.f90:37-56): istep and mod_lflags' lradsw.  sml_dyn_step
 * uses lradsw as it stands; sml_dyn_leapfrog sets lradsw = (mod(istep, 3) == 1)
 * before each step and advances istep, as stloop does.  Initial: istep 1, lradsw 1. */
int sml_dyn_set_clock(sml_dynamics *d, int istep, int lradsw);
int sml_dyn_get_clock(const sml_dynamics *d, int *istep, int *lradsw);
/* radiation state kept between steps (mod_radcon tau2, stratc; mod_physvar tt_rsw,
 * ssrd), host [4*kx*ngp tau2 | 2*ngp stratc | kx*ngp tt_rsw | ngp ssrd], layouts
 * [band][k][ngp], [2][ngp], [k][ngp]; NULL to set = zero */
int sml_dyn_set_rad_state(sml_dynamics *d, const double *rad);
int sml_dyn_get_rad_state(sml_dynamics *d, double *rad);
/* phypar alone on grid inputs (the arrays phypar builds, phy_phypar.f90:54-66):
 * ug1, vg1, tg1, qg1, phig1 [kx][ngp] (k = 1 top), pslg1 [ngp]; tendencies
 * d_tend [4][kx][ngp] = u, v, t, q.  Uses and updates the radiation state. */
int sml_dyn_phypar(sml_dynamics *d, const double *d_ug1, const double *d_vg1, const double *d_tg1,
                   const double *d_qg1, const double *d_phig1, const double *d_pslg1, int lradsw, double *d_tend,
                   void *stream);
int sml_dyn_phypar_host(sml_dynamics *d, const double *ug1, const double *vg1, const double *tg1, const double *qg1,
                        const double *phig1, const double *pslg1, int lradsw, double *tend);
/* host forcing helpers: sol_oz(tyear) (src/phy_radiat.f90:1-121) -> fields5
 * [5][ngp] = fsol, ozone, ozupp, zenit, stratz; sflset (src/phy_suflux.f90:358-382)
 * phi0 [ngp] -> forog [ngp] */
int sml_dyn_sol_oz(const sml_dynamics *d, double tyear, double *fields5);
int sml_phys_sflset(const double *phi0, double *forog);

/* ---------------------------------------------------------------- training */
/* W_out ridge training for a batch of regions (one vertical level each).
 *   chunking_matmul  (src/mod_reservoir.f90:1643-1699): G += S S^T, B += T S^T
 *   fit_chunk_hybrid (src/mod_reservoir.f90:1233-1332) / fit_chunk_ml (:1175-1231):
 *                    regularisation + mldivide (src/mod_linalg.f90:109-151)
 * naug[i] = chunk_size_speedy + n (hybrid) or n (ML only); nout = 136.
 * sml_train_create takes 2 <= nout <= 144 and naug[i] >= 2, anything else is
 * SML_ERR_ARG: the Gram kernel loads operand rows in pairs and has no path for an
 * operand of one row (the model's naug = chunk_size_speedy + n is never near 1).
 * Device memory: nlocal x npad^2 doubles of Gram (npad = max naug rounded up to
 * 128), so batch the regions to fit HBM (e.g. 144 regions of 6300 = 47 GB). */
typedef struct sml_train sml_train;
int sml_train_create(int nlocal, const int *naug, int nout, sml_train **out);
int sml_train_destroy(sml_train *t);
/* zero the accumulators (a new training run; sml_train_solve consumes them) */
int sml_train_reset(sml_train *t, void *stream);
/* one chunking_matmul batch of m time steps for every region:
 *   d_states : per region augmented_states(naug_i, m), column-major, back to back
 *   d_targets: per region targetdata(nout, m), column-major, back to back
 * Stream-ordered on `stream` (blocking or not) with no host-side copy: m may change
 * from call to call while earlier launches are still running. */
int sml_train_accumulate(sml_train *t, const double *d_states, const double *d_targets, int m, void *stream);
/* regularise (diag += beta_model for i < ncs, beta_res otherwise; squared and with
 * prior(i,i) = prior_val*beta_model^2 on b_trans when using_prior), solve
 * G W^T = B^T, write W_out(nout, naug_i) column-major per region back to back into
 * d_wout.  info (host, nlocal ints, may be NULL): potrf status per region (0 = ok,
 * filled when the stream completes).  Destroys the accumulators.  Stream-ordered on
 * `stream`; the forward substitution runs on a stream of the context (forked from and
 * joined back to `stream` by events inside the call, graph-capturable), without a CU mask. */
int sml_train_solve(sml_train *t, int ncs, double beta_res, double beta_model, int using_prior, double prior_val,
                    double *d_wout, int *info, void *stream);
int sml_train_npad(const sml_train *t, int *npad);
/* block columns per Cholesky panel (default 8): the in-panel steps are left-looking,
 * the trailing update after each panel right-looking at depth 128 x panel */
int sml_train_set_panel(sml_train *t, int panel);
/* host copies for tests: G (npad x npad, column-major, lower triangle valid) and
 * B(j, o) (npad x nout) of local region i */
int sml_train_get_gram(sml_train *t, int i, double *G, double *B);

/* measurement: sustained fp64 MFMA rate of the current device (TFLOP/s), from
 * back-to-back v_mfma_f64_16x16x4_f64 chains on every SIMD */
int sml_probe_mfma_f64(int iters, double *tflops);
/* the same probe with the median in-kernel core clock of the timed run (GHz): the
 * clock the chip holds under back-to-back fp64 MFMA (DVFS), against the nominal 2.4 */
int sml_probe_mfma_f64_clock(int iters, double *tflops, double *ghz);

/* ------------------------------------------------------------------ streams */
/* A HIP stream whose kernels run only on the logical CUs [first_cu, first_cu +
 * num_cus) of the current device (hipExtStreamCreateWithCUMask).  The hybrid loop
 * (no reference counterpart: the reference runs SPEEDY after every predict, serially,
 * parallelmain.f90:225-260) gives SPEEDY's latency-bound window its own CUs beside
 * the reservoir's HBM-bound update/readout, so the window's blocks neither wait for
 * LDS behind update blocks nor share a CU's memory pipeline with readout waves. */
int sml_stream_create_cu_range(int first_cu, int num_cus, void **stream);
int sml_stream_destroy(void *stream);

/* ------------------------------------------------------------ communicator */
/* RCCL communicator of the ranks of one node (one process per GPU, xGMI): replaces
 * the MPI world of startmpi (src/mpires.f90:21-37) for the one collective of the hot
 * path.  The 128-byte unique id comes from rank 0 (sml_comm_unique_id) over the
 * host's own channel, or through a file (sml_comm_create_file: rank 0 publishes it,
 * the others wait up to timeout_s seconds). */
typedef struct sml_comm sml_comm;
int sml_comm_unique_id(unsigned char *id128);
int sml_comm_create(int world, int rank, const unsigned char *id128, sml_comm **out);
int sml_comm_create_file(int world, int rank, const char *path, int timeout_s, sml_comm **out);
/* a rank descriptor without a transport (no RCCL communicator): rank `rank` of
 * `world` for sml_hybrid_create when the host moves the outvec slabs itself and
 * advances with sml_hybrid_advance_slabs; sml_comm_allgather and sml_hybrid_step
 * refuse it (SML_ERR_STATE) */
int sml_comm_create_local(int world, int rank, sml_comm **out);
int sml_comm_destroy(sml_comm *c);
int sml_comm_rank(const sml_comm *c, int *world, int *rank);
/* the all-gather's layout for `world` ranks of processor_decomposition
 * (src/res_domain.f90:31-62): each rank's outvecs zero-padded to the largest share
 * *maxc, received as [world][maxc][nout]; *contiguous = 1 when that is already global
 * region order (even shares); perm[numregions] (may be NULL) = the slab row of each
 * region.  Host only. */
int sml_exchange_plan(int numregions, int world, int *maxc, int *contiguous, int32_t *perm);
/* all-gather of equal slabs of `count` doubles: d_recv[world][count] (ncclAllGather) --
 * the outvec exchange that replaces sendrecievegrid's point-to-point gather/scatter
 * (src/mpires.f90:338-716) */
int sml_comm_allgather(sml_comm *c, const double *d_send, double *d_recv, int64_t count, void *stream);

/* ------------------------------------------------------------ hybrid loop */
/* The prediction loop of one rank (src/parallelmain.f90:204-270): predict for the
 * rank's regions -> outvec exchange -> assemble -> run_model (SPEEDY's window on the
 * GPU) -> re-tile.  res must hold this rank's processor_decomposition
 * (res_domain.f90:31-62) of comm's world (comm NULL = one rank); dyn must have its
 * state, forcing and physics set.  overlap != 0: the reservoir's update and v_ml
 * readout run beside SPEEDY's window on a second stream (identical results), with
 * SPEEDY on CUs [0, speedy_cus) when 0 < speedy_cus < CUs. */
typedef struct sml_hybrid sml_hybrid;
int sml_hybrid_create(sml_reservoirs *res, sml_dynamics *dyn, sml_comm *comm, int nleap, double delt, double alph,
                      double rob, double wil, int overlap, int speedy_cus, sml_hybrid **out);
int sml_hybrid_destroy(sml_hybrid *h);
/* caller-owned device buffers: packed feedback, local model [nlocal][ncs], local
 * outvecs [nlocal][nout], the assembled grids grid4d(4,96,48,8) / grid2d / precip,
 * SPEEDY's forecast grids fc4d / fc2d, tisr [nlocal][16] (standardized, may be NULL =
 * feedback tisr entries left as they are) */
int sml_hybrid_set_buffers(sml_hybrid *h, double *d_feedback, double *d_local_model, double *d_outvec,
                           double *d_grid4d, double *d_grid2d, double *d_precip, double *d_fc4d, double *d_fc2d,
                           const double *d_tisr);
/* the loop's calendar (get_current_time_delta_hour as run_model and get_tisr_by_date
 * call it, src/mpires.f90:1545, :1661): startyear, hours_base = traininglength +
 * prediction marker + synclength, step_hours = timestep.  Turns on the window's
 * date-driven forcing: advance t (1-based) runs sml_dyn_fordate at the date of hour
 * hours_base + t step_hours before its window (needs sml_dyn_set_surface).  Shares its
 * fields and February latch with sml_hybrid_set_tisr_table; resets the step count. */
int sml_hybrid_set_calendar(sml_hybrid *h, int startyear, int64_t hours_base, int step_hours);
/* date[4] = year, month, day, hour of the next advance's window */
int sml_hybrid_window_date(sml_hybrid *h, int *date);
/* fixed tisr inputs of the next steps ([nlocal][16] standardized) */
int sml_hybrid_set_tisr(sml_hybrid *h, const double *d_tisr);
/* get_tisr_by_date (src/mpires.f90:1644-1676): hourly global tisr fields
 * d_table[nhours][48][96] (nhours >= 8760, unstandardized; the reference's
 * full_tisr is the same year read per region and standardized, get_full_tisr,
 * src/mod_reservoir.f90:888-906); after step t the next feedback's tisr entries
 * come from hour sml_tisr_date_index(startyear, hours_base + (t-1) step_hours) of
 * the table, tiled and standardized per region.  NULL switches back to set_tisr. */
int sml_hybrid_set_tisr_table(sml_hybrid *h, const double *d_table, int nhours, int startyear, int64_t hours_base,
                              int step_hours);
/* the reference calendar's hour-of-year index (1-based) after hours_elapsed hours from
 * Jan 1 00 of startyear (get_current_time_delta_hour + numof_hours_into_year,
 * src/mod_calendar.f90:24-175, wrapped past 8760 as get_tisr_by_date does); *feb29
 * carries the SAVEd February of the reference's month table (0 at the start) */
int sml_tisr_date_index(int startyear, int64_t hours_elapsed, int *feb29, int *index);
/* get_current_time_delta_hour (src/mod_calendar.f90:24-92): date[4] = current year,
 * month, day, hour after hours_elapsed hours from Jan 1 00 of startyear, with the same
 * SAVEd-February latch *feb29.  Host only. */
int sml_calendar_delta_hour(int startyear, int64_t hours_elapsed, int *feb29, int *date);
/* the loop's copy of that latch (set_tisr_table resets it to 0): a host whose own
 * calendar calls already met a leap year sets 1, as the reference's process-wide
 * SAVEd table would hold (mod_reservoir.f90:355/632/638, mpires.f90:108/489) */
int sml_hybrid_set_feb29(sml_hybrid *h, int feb29);
int sml_hybrid_get_feb29(const sml_hybrid *h, int *feb29);
/* the tisr entries of every local region's feedback from one hour's global tisr
 * field d_tisr_grid(96, 48): overlap tile, (x - mean(34)) / std(34) */
int sml_res_tile_tisr_field(sml_reservoirs *c, const double *d_tisr_grid, double *d_feedback, void *stream);
/* sml_res_tile_feedback / sml_res_tile_tisr_field for every member of the context
 * (sml_res_set_members), one launch each: member e's grids, precipitation and feedback
 * start e * g4_stride / g2_stride (d_grid2d and d_precip) / fb_stride doubles into their
 * arrays (each stride >= the packed size); d_tisr [nlocal][16] (or NULL: the tisr entries
 * stay) and d_tisr_grid(96, 48) are the members' common ones.  Per member bitwise the
 * single-member call; the feedback's sst entries are not written. */
int sml_res_tile_feedback_members(sml_reservoirs *c, const double *d_grid4d, int64_t g4_stride,
                                  const double *d_grid2d, const double *d_precip, int64_t g2_stride,
                                  const double *d_tisr, double *d_feedback, int64_t fb_stride, void *stream);
int sml_res_tile_tisr_field_members(sml_reservoirs *c, const double *d_tisr_grid, double *d_feedback,
                                    int64_t fb_stride, void *stream);
/* ---- the training front end: from a series of global grids to standardised blocks
 * (get_training_data's standardize_data_5d_logp_tisr / standardize_data_3d /
 * standardize_sst_data_3d, mod_utilities.f90:846-905, :1137-1186, and the tiling of the
 * truth and the SPEEDY forecasts).  Step t of a series starts t * stride doubles in:
 * d_g4 [T][8][48][96][4] with g4_stride; d_g2 (logp), d_pr (precipitation, in the form
 * sml_res_tile_feedback's d_precip has), d_sst, d_tisr [T][48][96] with g2_stride.
 *
 * sml_res_series_stats: for every local region i and slot l of the 36, over the grid
 * sources P of the region's feedback entries of that slot (slots 0..31 = v * 8 + z of the
 * 4-d grid, 32 logp, 34 precip, 33 tisr, 35 sst: the region's input tile) and N = T |P|,
 *     mean = (sum_t sum_p x_t[p]) / N,  std = sqrt(sum_t sum_p (x_t[p] - mean)^2 / N),
 * the population, two-pass form, for every slot: the reference's one-pass precipitation
 * statistic is deliberately not copied (ill-conditioned; equal mathematically).  No
 * guards: a constant field gives std 0 up to the sums' rounding.  d_meanstd [nlocal][72]
 * device doubles, mean then std, the context's own layout.  Slot 35 of a region without the
 * sst flag, and slot 33 when d_tisr is NULL, get mean 0 and std 1.  d_sst may be NULL iff
 * no local region has the sst flag.  d_sst_change [nlocal] device ints (may be NULL):
 * 1 iff sum (x - mean)^2 > 0 and std > 0.2 for the sst slot -- the reference's rule for
 * keeping the sst input, reported and not acted on (ninp is fixed at create); 0 for a
 * region without the flag.  Three launches on `stream` (two streaming passes over the
 * series per grid point, T split in chunks that depend on T alone, then a combine per
 * (region, slot)), no atomics, no host synchronisation: the same bits on any stream.  The
 * workspace (44 MB) is the context's, allocated at the first call.
 * SML_ERR_ARG with a message, before anything is enqueued: T < 1; g4_stride < 8*48*96*4
 * or g2_stride < 48*96; d_g4 or g4_stride off 16-byte alignment; a NULL context, d_g4,
 * d_g2, d_pr or d_meanstd; a sml_res_create_generic context. */
int sml_res_series_stats(sml_reservoirs *c, const double *d_g4, int64_t g4_stride, const double *d_g2,
                         const double *d_pr, const double *d_sst, const double *d_tisr, int64_t g2_stride, int T,
                         double *d_meanstd, int *d_sst_change, void *stream);
/* adopt a [nlocal][72] device table (sml_res_series_stats' layout) as the context's mean
 * / std: the device table every kernel standardises with and the host copy
 * sml_res_mean_std returns.  Copies on `stream` and synchronises it.  SML_ERR_ARG inside
 * a begun step (sml_res_step_begun) and on a context with members > 1. */
int sml_res_set_mean_std_device(sml_reservoirs *c, const double *d_meanstd, void *stream);
/* T input blocks and T model blocks in one launch each.  Input block t, at d_inputs +
 * t * in_stride (in_stride >= the total feedback: the layout sml_res_synchronize and
 * sml_res_train_drive read), is bit for bit sml_res_tile_feedback with d_tisr = NULL, then
 * sml_res_tile_tisr_field on step t's tisr field, on step t's grids; its sst entries, which
 * those calls leave alone, are (sst_t[p] - mean[35]) / std[35] at the tisr entries' points.
 * d_sst / d_tisr NULL: those entries are left untouched.  Model block t [nlocal][ncs], at
 * d_model + t * model_stride, is bit for bit sml_res_tile_local_model on d_fc4 + t *
 * fc4_stride, d_fc2 + t * fc2_stride.  d_fc4, d_fc2 and d_model are NULL together, and
 * must be NULL at chunk_speedy == 0.  Words between blocks are not written.  Checks as
 * sml_res_series_stats, and every stride against its packed size.  Stream-ordered. */
int sml_res_tile_series(sml_reservoirs *c, const double *d_g4, int64_t g4_stride, const double *d_g2,
                        const double *d_pr, const double *d_sst, const double *d_tisr, int64_t g2_stride,
                        const double *d_fc4, int64_t fc4_stride, const double *d_fc2, int64_t fc2_stride, int T,
                        double *d_inputs, int64_t in_stride, double *d_model, int64_t model_stride, void *stream);
/* The slab-ocean reservoirs' training inputs from the same series (train_slab_ocean_model's
 * get_training_data_from_atmo, mod_slab_ocean_reservoir.f90:272-376, with
 * rolling_average_over_a_period_2d, mod_utilities.f90:1766-1804).  `slab` is the generic
 * context of the local sst regions of `atmo` (the pair sml_hybrid_set_slab takes).  For slab
 * reservoir s and its feedback entry e (7 * in2d entries: the lowest level's 4 variables,
 * logp, sst, tisr over the input tile), z_t[e] is the value sml_res_tile_series writes for
 * the atmo feedback entry atmo_training_data_idx[e] of step t (t = x - mean; t / std with
 * atmo's adopted mean / std), and column t of the output is
 *     a_t[e] = (z_lo[e] + z_lo+1[e] + ... + z_t[e]) / d,   lo = max(0, t - window + 1),
 * summed from 0.0 in ascending step order, one fp64 add per term, no FMA; d = the number
 * of summed terms while t + 1 < window, `divisor` otherwise.  (window, divisor) = (P + 1, P)
 * is the reference's rolling average of period P, which sums P + 1 columns and divides by
 * P; (P, P) is the plain mean of P columns, the statistic the loop's ring feeds the slab at
 * prediction with P = timestep_slab / timestep - 1.  The caller chooses.
 * Columns t0 .. t0 + ncols - 1 are written, column t at d_out + (t - t0) * out_stride in
 * the slab's packed feedback layout (sml_res_feedback_offsets of `slab`); the series' steps
 * max(0, t0 - window + 1) .. t0 + ncols - 1 are read, straight from the grids.  d_tisr NULL:
 * the tisr entries are 0.  A column range is bit for bit the same columns of the whole
 * call; no atomics, no waits between blocks: the same bits on any stream, CU mask and
 * stride.  One launch per 65535 chunks of 64 columns (an LDS ring of the last values per
 * entry, re-summed in step order for every column).  The index table is built and uploaded at the first
 * call and is atmo's from then on.  ncols == 0 is a no-op.  Stream-ordered.  Not cheap on
 * the host: every call reads both contexts through their getters and re-runs the layout
 * unit's checks of the slab context (all the rank's regions: about the cost of building the
 * slab tables), so a caller that loops over column ranges should take large ranges.
 * SML_ERR_ARG with a message, before anything is enqueued: T < 1; window outside
 * [1, 1024]; divisor < 1; t0 < 0, ncols < 0 or t0 + ncols > T; the series' stride and
 * alignment rules of sml_res_tile_series; a NULL context, d_g4, d_g2, d_pr, d_sst or d_out;
 * out_stride below the slab's packed feedback size; an atmo context that is generic or has
 * members; a slab context that is not the ML-only generic context of atmo's local sst
 * regions in order with nout = resx * resy and 7 * in2d inputs each. */
int sml_slab_train_series(sml_reservoirs *atmo, const sml_reservoirs *slab, const double *d_g4, int64_t g4_stride,
                          const double *d_g2, const double *d_pr, const double *d_sst, const double *d_tisr,
                          int64_t g2_stride, int T, int window, int divisor, int t0, int ncols, double *d_out,
                          int64_t out_stride, void *stream);
/* the loop's main (reservoir + exchange) and side (SPEEDY) streams */
int sml_hybrid_streams(const sml_hybrid *h, void **main, void **side);
/* the CU split of the two streams: SPEEDY's CUs [0, speedy_cus) and the reservoir's
 * [speedy_cus, speedy_cus + res_cus) (one CU per 6 of the rank's regions, a multiple of
 * 8, 64..256 - speedy_cus; SML_RES_CUS overrides); both 0 without a split */
int sml_hybrid_cus(const sml_hybrid *h, int *speedy_cus, int *res_cus);
/* start_prediction's hand-over: inputs of the first step from an analysis grid and
 * a SPEEDY forecast of it (src/mod_reservoir.f90:938-959) */
int sml_hybrid_start(sml_hybrid *h, const double *d_grid4d, const double *d_grid2d, const double *d_precip,
                     const double *d_fc4d, const double *d_fc2d);
/* a step in two halves around a host-provided exchange: predict leaves the local
 * outvecs in d_outvec on the main stream; advance takes every region's outvecs in
 * global region order ([numregions][nout]) */
int sml_hybrid_predict(sml_hybrid *h);
int sml_hybrid_advance(sml_hybrid *h, const double *d_outvec_all);
/* advance from the all-gather's output d_recv[world][maxc][nout] (sml_exchange_plan;
 * rank q's rows zero-padded to maxc): permuted into global region order when the
 * shares are uneven, then sml_hybrid_advance.  Replaces the root's receive loop
 * and assembly of sendrecievegrid (src/mpires.f90:389-442). */
int sml_hybrid_advance_slabs(sml_hybrid *h, const double *d_recv);
/* predict + the loop's own exchange (identity on one rank, sml_comm_allgather
 * otherwise) + advance_slabs; asynchronous */
int sml_hybrid_step(sml_hybrid *h);
/* ---- slab ocean (src/parallelmain.f90:216-249; sendrecievegrid's sst half,
 * src/mpires.f90:288-478, 575-767; run_model's sst_hybrid, :1576-1584, applied by
 * ini_sea, src/cpl_sea.f90:38-46).  slab: a generic ML-only context
 * (sml_res_create_generic, chunk_speedy 0, nout = resx*resy, out_index 35, leakage 1)
 * over exactly this rank's regions with an sst input, in order, each with the 7*in2d
 * inputs of atmo_training_data_idx (src/mod_slab_ocean_reservoir.f90:1532-1563).
 * Every step the atmo feedback's lowest level, logp, sst and tisr enter a ring of
 * timestep_slab/timestep - 1 columns; when mod(t*timestep, timestep_slab) == 0 the slab
 * reservoirs predict from the ring's mean (predict_slab_ml, :1251-1296); their sst
 * travels in the exchange rows (nout + resx*resy doubles per region, so d_outvec and a
 * host exchange use sml_hybrid_exchange_width), is assembled into wholegrid_sst with
 * base_sst_grid on land (sea_mask > 0) and the 272 K floor, enters the window's sst_am
 * (sml_dyn_set_hybrid_sst) and, standardized with the slab's sst mean / std, the atmo
 * feedback's sst entries.  d_base_sst / d_sea_mask (96, 48) device, read every slab
 * step.  Call before sml_hybrid_set_buffers; train_on_sst_anomalies and
 * non_stationary_ocn_climo (both off by default, mod_reservoir.f90:42-44) are not
 * supported. */
int sml_hybrid_set_slab(sml_hybrid *h, sml_reservoirs *slab, const double *d_base_sst, const double *d_sea_mask,
                        int timestep, int timestep_slab, double sst_bias);
/* start_prediction_slab's hand-over, after sml_hybrid_start: the slab reservoirs' sst
 * d_slab_outvec[nslab][resx*resy] (unstandardized; their states synchronized by the
 * host with sml_res_start_prediction) */
int sml_hybrid_start_slab(sml_hybrid *h, const double *d_slab_outvec);
/* doubles per region in the exchange rows: nout, or nout + resx*resy with the slab */
int sml_hybrid_exchange_width(const sml_hybrid *h, int *width);
/* device views of the slab state: wholegrid_sst(96, 48), the ring
 * [timestep_slab/timestep - 1][*ring_len], the last slab feedback and slab outvecs */
int sml_hybrid_slab_buffers(const sml_hybrid *h, const double **d_sst_grid, const double **d_ring, int *ring_len,
                            const double **d_slab_feedback, const double **d_slab_outvec);
/* ---- the slab ocean of an E-member forecast on one rank (speedy_ml_amd.ensemble): the
 * stages above with a member dimension, one launch per stage for all members, per member
 * bitwise the single-member loop's.  atmo: the members' atmo context, every region in
 * global order; slab: the slab context as sml_hybrid_set_slab describes it, with the same
 * member count (sml_res_set_members on both first: E is the atmo context's).  Create
 * applies sml_hybrid_set_slab's checks and sets the atmo context's outvec row stride to
 * the exchange width (nout + resx*resy), so the members' outvecs are
 * [E][nlocal][exchange width].  The caller owns those and the members' feedbacks and
 * passes them with their member strides in doubles (>= the packed size); the slab
 * feedbacks, slab outvecs, rings and sst grids are the object's (sml_slab_buffers).  The
 * host calls, per step t + 1, in the single-member loop's order: sml_slab_predict(t + 1)
 * before the atmo finish, sml_slab_sst after it (then sml_dyn_set_hybrid_sst of each
 * member's grid when it wrote), and sml_slab_ring(t + 1) after the feedbacks' re-tiling. */
typedef struct sml_slab sml_slab;
int sml_slab_create(sml_reservoirs *atmo, sml_reservoirs *slab, const double *d_base_sst, const double *d_sea_mask,
                    int timestep, int timestep_slab, double sst_bias, sml_slab **out);
int sml_slab_destroy(sml_slab *s);
/* members, doubles per exchange row, slab reservoirs, the ring's columns
 * (timestep_slab/timestep - 1) and their length, current_sst_bias; any may be NULL */
int sml_slab_info(const sml_slab *s, int *members, int *exchange_width, int *nslab, int *ring_columns,
                  int *ring_len, double *sst_bias);
/* start_prediction_slab's hand-over of one member: 272 K in the sst columns of its
 * exchange rows, d_slab_outvec[nslab][resx*resy] (device, unstandardized) over them, its
 * ring cleared, its SST marked changed.  The slabs' sst mean / std are taken at the first
 * start.  d_outvec: the members' outvecs (member 0's).  Waits for `stream`. */
int sml_slab_start(sml_slab *s, int member, const double *d_slab_outvec, double *d_outvec, int64_t ov_stride,
                   void *stream);
/* on a slab step, mod(t_next * timestep, timestep_slab) == 0: every member's ring mean,
 * sml_res_step_members on the slab context, the new sst into the members' exchange rows,
 * every member marked changed, *predicted (may be NULL) = 1; nothing otherwise */
int sml_slab_predict(sml_slab *s, int64_t t_next, double *d_outvec, int64_t ov_stride, void *stream,
                     int *predicted);
/* if any member's sst changed: the E wholegrid_sst grids from the exchange rows and the sst
 * entries of the E feedbacks; *wrote (may be NULL) reports it */
int sml_slab_sst(sml_slab *s, const double *d_outvec, int64_t ov_stride, double *d_feedback, int64_t fb_stride,
                 void *stream, int *wrote);
/* column mod(t - 1, ring columns) of every member's ring from the E feedbacks */
int sml_slab_ring(sml_slab *s, int64_t t, const double *d_feedback, int64_t fb_stride, void *stream);
/* device views with their member strides in doubles: wholegrid_sst(96, 48), the ring
 * [ring columns][ring_len], the last slab feedback [ring_len], the slab outvecs
 * [nslab][resx*resy]; any may be NULL */
int sml_slab_buffers(const sml_slab *s, const double **d_sst_grid, int64_t *sst_stride, const double **d_ring,
                     int64_t *ring_stride, const double **d_slab_feedback, int64_t *fb_stride,
                     const double **d_slab_outvec, int64_t *ov_stride);
/* ---- the products of an E-member forecast: per-point mean and spread of the members'
 * assembled grids, and per step a row of area-weighted scores against a verifying analysis.
 * Fields: f = 4k + v is level k, variable v of a grid4d [8][48][96][4]; 32 is logp
 * [48][96], 33 precip [48][96].  Member e of d_g4 starts e * g4_stride doubles in, of d_g2
 * and d_pr e * g2_stride (>= the packed grids, else SML_ERR_ARG naming the stride).  d_pr
 * may be NULL: field 33 is then left untouched everywhere.  Per point, in member order:
 *   mean = (x_0 + x_1 + ...) / E;  var = sum_e (x_e - mean)^2 / (E - 1);  spread = sqrt(var)
 * (spread 0 at E = 1).  Point (j, i) weighs w_j = wt[min(j, 47 - j)] / (96 * sum_j wt[..]),
 * wt the Gaussian weights of sml_spectral_tables (sml_ens_weights; the 4608 weights sum to
 * 1).  Row t of scores [capacity][34][4] holds, summed over the field's points,
 *   rmse = sqrt(sum w (mean - y)^2), spread = sqrt(sum w var), bias = sum w (mean - y),
 *   crps = sum w [ 1/E sum_e |x_e - y| - 1/(2E(E-1)) sum_e sum_f |x_e - x_f| ]  (the fair CRPS)
 * and row t of ranks [capacity][34][33] counts the points by r = #{e : x_e < y} (ties and
 * NaN count as not below; bins above E stay 0).  The truth is three single-member grids:
 * all NULL (only `spread` of the row is written), or d_truth4 and d_truth2 with d_truthpr
 * or without (field 33 then as without truth).  The sums use no atomics and a fixed order:
 * for given inputs the tables are bit for bit the same across calls, streams, CU masks
 * and strides.  Launches are stream-ordered with no host synchronisation; the calls on one
 * context must be ordered among themselves. */
typedef struct sml_ens sml_ens;
/* members in 1..SML_RES_MAX_MEMBERS, capacity_steps >= 1 rows; the tables start reset */
int sml_ens_create(int members, int capacity_steps, sml_ens **out);
int sml_ens_destroy(sml_ens *e);
/* members, capacity, 34 fields, 4 scores per field, 33 rank bins; any may be NULL */
int sml_ens_info(const sml_ens *e, int *members, int *capacity_steps, int *fields, int *scores_per_field,
                 int *rank_bins);
/* quiet NaN into every score, 0 into every rank bin */
int sml_ens_reset(sml_ens *e, void *stream);
/* mean and spread in the packed single-member layouts; any output may be NULL */
int sml_ens_moments(sml_ens *e, const double *d_g4, int64_t g4_stride, const double *d_g2, const double *d_pr,
                    int64_t g2_stride, double *d_mean4, double *d_mean2, double *d_meanpr, double *d_spread4,
                    double *d_spread2, double *d_spreadpr, void *stream);
/* row t in [0, capacity) of both tables, else SML_ERR_ARG */
int sml_ens_scores(sml_ens *e, const double *d_g4, int64_t g4_stride, const double *d_g2, const double *d_pr,
                   int64_t g2_stride, const double *d_truth4, const double *d_truth2, const double *d_truthpr, int t,
                   void *stream);
/* rows [t0, t0 + count) to the host: scores [count][34][4], ranks [count][34][33] (either
 * may be NULL).  Waits for the device. */
int sml_ens_read(sml_ens *e, int t0, int count, double *scores, int32_t *ranks);
/* the 48 row weights w_j (host only, no context) */
int sml_ens_weights(double *w48);
/* the two cross-stream dependencies of the overlapped loop: SML_HOP_WAIT_VALUE (a
 * sequence number written by the producer's stream, waited for by the consumer's, as
 * CP stream memory operations), SML_HOP_EVENTS (event record + wait), SML_HOP_KERNEL
 * (the same sequence number, stored by a one-lane kernel behind the producer and
 * polled by a one-lane kernel ahead of the consumer; a wait that has not seen its
 * value after ~4 s gives up and sml_hybrid_sync returns SML_ERR_STATE), or
 * SML_HOP_AUTO (the default: kernel hops when the two streams run on disjoint CUs, i.e. speedy_cus > 0,
 * else wait-value hops; events when dispatch is serialised --
 * AMD_SERIALIZE_KERNEL or rocprofv3's counter collection -- where a waiting packet or
 * kernel could stall its queue ahead of its producer; SML_HYBRID_EVENTS=1 also
 * selects events).  In the kernel mode the v_p finish
 * and run_model's entry wait for their inputs inside their own kernels.  Drains both
 * streams before switching. */
#define SML_HOP_AUTO 0
#define SML_HOP_WAIT_VALUE 1
#define SML_HOP_EVENTS 2
#define SML_HOP_KERNEL 3
int sml_hybrid_set_hop_mode(sml_hybrid *h, int mode);
/* the give-up time of the loop's in-kernel waits (kernel hops; run_model's exit waiting
 * for its safety check, at most 1 s), microseconds; default 4 s.  A wait that gives up
 * hands its consumer NaN instead of the data it did not get (the finish's local model,
 * the entry's grid; the exit takes the window as unsafe) and marks a host-visible word:
 * the next sml_hybrid_step, sml_hybrid_run_speedy (which then also yields run = 0) or
 * sml_hybrid_sync returns SML_ERR_STATE once. */
int sml_hybrid_set_hop_timeout(sml_hybrid *h, int64_t microseconds);
int sml_hybrid_hop_mode(const sml_hybrid *h, int *requested, int *effective);
/* pipelined loop (default off): each advance also issues the NEXT step's reservoir
 * begin (update + v_ml readout of the feedback it has just tiled) on the main stream,
 * so a loop restarted after a sync does not pay one begin outside the overlap; every
 * step's outvecs, grids and forecast are bitwise those of the default loop, but after
 * a step (and a sync) the reservoir states are one update ahead (the next step's).
 * The next predict only finishes that begin. */
int sml_hybrid_set_pipelined(sml_hybrid *h, int on);
/* the exchange through the communicator's transport even at world 1 (default off): a
 * one-rank loop with an RCCL communicator (sml_comm_create at world 1) then runs
 * sml_hybrid_step's world > 1 path -- outvecs to the send slab, ncclAllGather on the
 * main stream, sml_hybrid_advance_slabs from the receive slab, separate assembly --
 * instead of the identity exchange fused into the finish.  Same results, bitwise;
 * for exercising the transport on one GPU.  Refused without a transport. */
int sml_hybrid_set_force_exchange(sml_hybrid *h, int on);
/* where a step's serial chain runs -- the v_p finish with the local-model tiling, the
 * exchange and the assembly: SML_CHAIN_TWO_STREAMS on the reservoir's (main) stream,
 * between a hop from SPEEDY's stream (the forecast) and one back (the assembled grid);
 * SML_CHAIN_SPEEDY on SPEEDY's stream right behind the window, so no hop sits on the
 * critical path (the main stream keeps the re-tiling and the reservoir begin, which
 * wait for the assembled grid and signal the finish); SML_CHAIN_AUTO (default) is the
 * two-stream form (measured faster at world 1 and in an 8-rank share).
 * Bitwise the same results.  Drains both streams. */
#define SML_CHAIN_AUTO 0
#define SML_CHAIN_TWO_STREAMS 1
#define SML_CHAIN_SPEEDY 2
int sml_hybrid_set_chain(sml_hybrid *h, int mode);
int sml_hybrid_chain(const sml_hybrid *h, int *requested, int *effective);
/* the stream the local outvecs are ready on after sml_hybrid_predict: a host-driven
 * exchange runs there before sml_hybrid_advance */
int sml_hybrid_exchange_stream(const sml_hybrid *h, void **stream);
/* the number of ncclAllGather calls sml_hybrid_step has issued on this loop */
int sml_hybrid_exchanges(const sml_hybrid *h, int64_t *allgathers);
/* run_speedy of the last step (0: the reference ends the prediction,
 * parallelmain.f90:268-270); waits only for that step's safety check */
int sml_hybrid_run_speedy(sml_hybrid *h, int *run);
/* wait for the issued steps; d_local_model then holds the last window's local model */
int sml_hybrid_sync(sml_hybrid *h);
/* ------------------------------------------------------------ host plumbing */
/* zeroed device allocation / free, synchronous copies (for hosts without a GPU
 * runtime binding of their own, e.g. the Fortran host) */
int sml_device_alloc(int64_t bytes, void **d_ptr);
int sml_device_free(void *d_ptr);
int sml_copy_to_device(void *d_dst, const void *src, int64_t bytes);
int sml_copy_to_host(void *dst, const void *d_src, int64_t bytes);
/* res_domain geometry of one region (getxyresextent / getoverlapindices,
 * src/res_domain.f90:123-204), 1-based: g[12] = res_xstart, res_xend, res_ystart,
 * res_yend, resx, resy, in_xstart, in_xend, in_ystart, in_yend, inx, iny */
int sml_region_geometry(int numregions, int region, int *g);
/* the 0-based positions of a region's training targets inside its feedback vector
 * [atmo(4,inx,iny,8) | logp(inx,iny) | precip(inx,iny) | sst? | tisr]
 * (tile_full_input_to_target_data2d, src/res_domain.f90:602-651): atmo (v, x, y, z) for
 * x, y in the tdata ranges of get_trainingdataindices (:547-574; the polar tiles
 * differ), z = 1..8, in Fortran order with v fastest, then logp (x, y), then precip
 * (x, y).  idx holds 34 * resx * resy entries (136 at 1152 regions); *count receives
 * that number.  sst (0 / 1) is the region's flag; its block follows the targets. */
int sml_region_target_index(int numregions, int region, int sst, int32_t *idx, int *count);
/* the 0-based positions of the slab-ocean reservoir's training targets inside the slab
 * feedback of a region [lowest level (4, inx, iny) | logp | sst | tisr]: entry 5 * inx * iny
 * + the input-tile position of resolved point o -- the sst section's inner tile
 * (tile_full_input_to_target_data2d_ocean_model, src/res_domain.f90:691-716), in the order
 * of the slab outvec (x fastest).  idx holds resx * resy entries (4 at 1152 regions);
 * *count receives that number.  Rows of sml_res_set_target_index's table. */
int sml_slab_target_index(int numregions, int region, int32_t *idx, int *count);
/* processor_decomposition (src/res_domain.f90:31-62): 0-based regions of rank irank */
int sml_processor_decomposition(int numregions, int numprocs, int irank, int *regions, int *count);
/* the mean / std (36 each) local region i was loaded with (host copies) */
int sml_res_mean_std(const sml_reservoirs *c, int i, double *mean, double *std);
/* row stride (>= nout) of the outvec arrays the context writes and
 * sml_exchange_assemble reads (the hybrid loop widens it for the slab ocean's sst) */
int sml_res_set_outvec_ld(sml_reservoirs *c, int ld);
/* numregions, nlocal, chunk_speedy, nout and the local region ids (any may be NULL) */
int sml_res_info(const sml_reservoirs *c, int *numregions, int *nlocal, int *chunk_speedy, int *nout,
                 int *region_ids);

#ifdef __cplusplus
}
#endif
#endif /* SPEEDY_ML_H */

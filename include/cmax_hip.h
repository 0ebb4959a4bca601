/*
 * cmax_hip.h -- C ABI of libcmax_hip.so: the MI355X (gfx950) contrast-maximization inner loop
 * (event warp -> image of warped events -> contrast objective + analytic gradient).
 *
 * The reference (tub-rip/event_based_optical_flow) is pure Python and has NO FFI; its "plugin API"
 * for this path is three Python classes.  Each entry point below names the
 * reference function it replaces (file:line relative to the reference root); the Python host
 * layer in event_based_optical_flow_amd/ mirrors those classes and calls this ABI through ctypes.
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *  - every function returns int: 0 ok, <0 bad argument (CMAX_E*), >0 a hipError_t.
 *    cmax_last_error() returns a thread-local description of the last failure.
 *  - all pointers are DEVICE pointers borrowed from the caller (PyTorch's allocator) unless the
 *    name ends in _host; nothing is retained after the call returns except by cmax_set_events.
 *  - work is enqueued on `stream` (a hipStream_t, e.g. torch.cuda.current_stream().cuda_stream);
 *    no entry point synchronises the device.
 *  - events are row-major [n,4] = (x, y, t, p); x is the ROW coordinate, y the COLUMN
 *    (src/event_image_converter.py:344-345); images are row-major [H, W].
 *  - dtype: CMAX_F32 or CMAX_F64 (leaf ops compute in the dtype of their inputs, like the reference,
 *    whose outputs follow the events' dtype, src/event_image_converter.py:338).
 */
#ifndef CMAX_HIP_H
#define CMAX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMAX_ABI_VERSION 4

/* dtypes */
#define CMAX_F32 0
#define CMAX_F64 1

/* motion models -- Warp.warp_event dispatcher, src/warp.py:156-199 */
#define CMAX_MODEL_2DOF 0  /* "2d-translation", "rigid-optical-flow"  src/warp.py:483-522 */
#define CMAX_MODEL_DENSE 1 /* "dense-flow"                            src/warp.py:263-313 */
#define CMAX_MODEL_VOXEL 2 /* "dense-flow-voxel"                      src/warp.py:315-396 */

/* reference-time modes -- Warp.calculate_reftime, src/warp.py:201-233 */
#define CMAX_REF_FIRST 0 /* t_min exactly */
#define CMAX_REF_LAST 1  /* t_max exactly */
#define CMAX_REF_FRAC 2  /* t_min + (t_max - t_min) * frac ("middle" = 0.5, "before" = -1, "after" = 2) */

/* contrast functions */
#define CMAX_COST_VARIANCE 0 /* ImageVariance      src/costs/image_variance.py:27-71 */
#define CMAX_COST_GRADMAG 1  /* GradientMagnitude  src/costs/gradient_magnitude.py:60-76 */
/* Focus losses (Gallego, Gehrig, Scaramuzza, "Focus is all you need", CVPR 2019): quadratic forms of the image I with 3 x 3
 * support, I read as zero outside the image; Omega = the image, without its one-pixel border when omit_boundary; n = |Omega|.
 * No further scale factors; `ddof` of cmax_contrast is ignored, as for the gradient magnitude. */
#define CMAX_COST_MEAN_SQUARE 2 /* (1/n) sum_Omega I^2 */
#define CMAX_COST_LAPLACIAN 3   /* (1/n) sum_Omega l^2,  l = I(r-1,c) + I(r+1,c) + I(r,c-1) + I(r,c+1) - 4 I(r,c) */
#define CMAX_COST_HESSIAN 4     /* (1/n) sum_Omega (h_rr^2 + 2 h_rc^2 + h_cc^2),  h_rr = I(r-1,c) - 2 I(r,c) + I(r+1,c), h_cc likewise
                                 * along columns, h_rc = (I(r+1,c+1) - I(r+1,c-1) - I(r-1,c+1) + I(r-1,c-1)) / 4 */

/* flow propagation schemes -- src/utils/flow_utils.py */
#define CMAX_SCHEME_BURGERS 0 /* inviscid_burger_flow_to_voxel_torch  567-639 */
#define CMAX_SCHEME_UPWIND 1  /* upwind_flow_to_voxel_torch           439-493 */

/* error codes */
#define CMAX_EINVAL -1   /* bad argument */
#define CMAX_ENOMEM -2   /* workspace allocation failed */
#define CMAX_ESTATE -3   /* call order (e.g. objective before set_events) */
#define CMAX_ENODEV -4   /* no usable gfx950 device / RCCL not loadable */
#define CMAX_ECOMM -5    /* an RCCL call failed (message in cmax_last_error) */
#define CMAX_EUNSUPPORTED -6 /* the call is not built for the state of the handle (e.g. per-event weights; message in cmax_last_error) */

typedef void *cmax_stream_t; /* hipStream_t */
typedef struct cmax_handle_s *cmax_handle_t;

const char *cmax_last_error(void);
int cmax_abi_version(void);

/* =============================================================================================
 * Leaf operators (stateless).  One per reference leaf function; dtype-generic.
 * ============================================================================================= */

/* min / max of the event timestamps -> tminmax[2] (device doubles).
 * Replaces nt_min / nt_max over events[..., 2] in Warp.calculate_reftime (src/warp.py:216-224). */
int cmax_tminmax(const void *events, int dtype, int64_t n, double *tminmax, cmax_stream_t stream);

/* Warp.warp_event (src/warp.py:156-199) incl. calculate_reftime (201-233) and calculate_dt
 * (235-259): warped[n,4] = (x', y', dt, p).
 *   ref_mode/ref_frac : reference time (CMAX_REF_*), evaluated on the device from tminmax[2]
 *   normalize_t       : dt /= (max(dt) - min(dt))            (src/warp.py:254-259)
 *   motion            : theta[2] | flow[2,H,W] | voxel[T,2,H,W], same dtype as events
 *   dt_out            : optional [n] copy of dt (saved for the backward pass)
 *   bin_out           : optional int32[n], voxel model only: time bin per event (-1 = none)  */
int cmax_warp_events(const void *events, int dtype, int64_t n, int model, const void *motion, int T,
                     int H, int W, const double *tminmax, int ref_mode, double ref_frac,
                     int normalize_t, void *warped, void *dt_out, int32_t *bin_out,
                     cmax_stream_t stream);

/* adjoint of cmax_warp_events w.r.t. the motion (what torch autograd derives for warp.py:304-307,
 * 357-362, 506-520): given gwarped[n,4] (only columns 0,1 are read)
 *   2DOF : gmotion[2]        = sum_e dt_e * (gx_e, gy_e)        (dtype, overwritten)
 *   DENSE: gmotion[2,H,W]   += -dt_e * g_e at the source pixel  (zeroed inside)
 *   VOXEL: gmotion[T,2,H,W] likewise into bin(e)                                            */
int cmax_warp_events_bwd(const void *events, int dtype, int64_t n, int model, int T, int H, int W,
                         const void *dt, const int32_t *bin, const void *gwarped, void *gmotion,
                         cmax_stream_t stream);

/* EventImageConverter.bilinear_vote_tensor / count_event_tensor
 * (src/event_image_converter.py:316-374, 209-255).
 *   xy      : pointer to x' of event 0; `stride` elements between events (4 for an [n,4] array)
 *   weight  : optional per-event weight [n]; else the scalar `wscalar`   (330-331)
 *   Hp, Wp  : PADDED image size; ph, pw: padding offsets                  (28, 344-345)
 *   eps     : 1e-6 (torch branch, 340) or 1e-8 (numpy branch, 282)
 *   count   : !=0 -> every in-bounds corner += 1                          (251-254)
 *   img     : [Hp,Wp], overwritten                                                          */
int cmax_vote(const void *xy, int dtype, int64_t stride, int64_t n, const void *weight,
              double wscalar, int Hp, int Wp, int ph, int pw, double eps, int count, void *img,
              cmax_stream_t stream);

/* adjoint of cmax_vote (autograd of scatter_add_ = gather; floor has zero derivative):
 *   gxy[n,2] = (dL/dx', dL/dy'),  gw[n] = dL/dweight (optional).  G is [Hp,Wp].             */
int cmax_vote_bwd(const void *xy, int dtype, int64_t stride, int64_t n, const void *weight,
                  double wscalar, int Hp, int Wp, int ph, int pw, double eps, const void *G,
                  void *gxy, void *gw, cmax_stream_t stream);

/* Gaussian blur of create_image_from_events_tensor (src/event_image_converter.py:153-159):
 * 3 taps exp(-0.5 (k/sigma)^2) normalised, reflect-101 padding, separable.  adjoint != 0 applies
 * the transposed operator (backward pass).  in != out.                                       */
int cmax_blur3(const void *in, int dtype, int H, int W, double sigma, int adjoint, void *out,
               cmax_stream_t stream);

/* numpy-branch blur of create_image_from_events_numpy (src/event_image_converter.py:122-124):
 * scipy.ndimage.gaussian_filter(image, sigma) -- radius int(4 sigma + 0.5), edge-duplicating 'reflect'
 * boundary, axis 0 then axis 1.  tmp: scratch image of the same size.                          */
int cmax_gaussian_filter(const void *in, int dtype, int H, int W, double sigma, void *tmp, void *out,
                         cmax_stream_t stream);

/* ImageVariance.calculate / GradientMagnitude.calculate (src/costs/image_variance.py:27-71,
 * src/costs/gradient_magnitude.py:60-76 + SobelTorch src/utils/stat_utils.py:50-83).
 *   value  : device double[4]: value[0] = the RAW contrast (no sign), value[1..3] = scratch
 *            accumulators (zeroed inside); ddof 1 = torch.var, 0 = np.var
 *   G      : optional [H,W] = gscale * d value / d img, gscale read from the device double
 *            `gscale` (NULL = 1) -- lets the caller chain the upstream gradient on the device */
int cmax_contrast(const void *img, int dtype, int H, int W, int cost, int omit_boundary, int ddof,
                  double *value, void *G, const double *gscale, cmax_stream_t stream);

/* TotalVariation.calculate_torch (src/costs/total_variation.py:60-75, 110-126): flow [2,h,w];
 * value is a device double[4] as for cmax_contrast.                                           */
int cmax_total_variation(const void *flow, int dtype, int h, int w, int omit_boundary,
                         double *value, void *G, const double *gscale, cmax_stream_t stream);

/* One propagation step (src/utils/flow_utils.py:567-639 / 439-493) on F[2,H,W] and its adjoint
 * (gF += J^T gout).                                                                          */
int cmax_flow_step(const void *F, int dtype, int H, int W, double dt, int scheme, void *out,
                   cmax_stream_t stream);
int cmax_flow_step_adj(const void *F, int dtype, int H, int W, double dt, int scheme,
                       const void *gout, void *gF, cmax_stream_t stream);

/* construct_dense_flow_voxel_torch (src/utils/flow_utils.py:99-161): V[T,2,H,W] from F at bin
 * t0 (0 = "first", T/2 = "middle"); and its adjoint (gV is clobbered: the sweep leaves dL/dF in
 * its bin t0; gF[2,H,W] receives a copy, NULL: no copy).                                        */
int cmax_voxel_construct(const void *F, int dtype, int T, int t0, int H, int W, int scheme, void *V,
                         cmax_stream_t stream);
int cmax_voxel_construct_adj(const void *V, int dtype, int T, int t0, int H, int W, int scheme,
                             void *gV, void *gF, cmax_stream_t stream);

/* Second order of the same chain, for exact Hessian-vector products of time-aware objectives (what
 * torch.autograd.functional.vhp differentiates, src/solver/scipy_autograd/torch_wrapper.py:51-73):
 *   _tan      V[T,2,H,W] and its directional derivative dV along dF, in one sweep
 *   _adj_tan  on entry gV = dL/dV, dgV = its tangent (both clobbered: the sweep leaves the results in their bins
 *             t0); gF[2,H,W] = copy of dL/dF, dgF[2,H,W] = copy of d/d(eps) [dL/dF](F + eps dF)
 *             = J^T dgV + (dJ[dV])^T gV   (either may be NULL: no copy)
 * sign(), the selectors of maximum / minimum and |.|' are piecewise constant (torch's convention).          */
int cmax_voxel_construct_tan(const void *F, const void *dF, int dtype, int T, int t0, int H, int W, int scheme,
                             void *V, void *dV, cmax_stream_t stream);
int cmax_voxel_construct_adj_tan(const void *V, const void *dV, int dtype, int T, int t0, int H, int W, int scheme,
                                 void *gV, void *dgV, void *gF, void *dgF, cmax_stream_t stream);

/* interpolate_dense_flow_from_patch_tensor (src/solver/patch_contrast_base.py:462-506): patch motion
 * [2,ph,pw] -> dense flow [2,H,W] = centre-crop(bilinear x(sw_h,sw_w), align_corners=False, of the
 * replicate-padded NEGATED grid).  adjoint != 0: `motion` is dL/dflow [2,H,W], out = dL/dmotion
 * [2,ph,pw] (overwritten).                                                                     */
int cmax_patch_to_dense(const void *motion, int dtype, int ph, int pw, int pad_h, int pad_w, int sw_h,
                        int sw_w, int H, int W, int adjoint, void *out, cmax_stream_t stream);

/* ... with the resize filter of `patch.filter_type` (src/solver/patch_contrast_base.py:49, 434-437, 492-495).
 * CMAX_FILTER_BILINEAR: cmax_patch_to_dense itself.  CMAX_FILTER_NEAREST: pixel (r, c) of the up-sampled padded
 * grid takes padded cell (r / sw_h, c / sw_w) -- nearest-neighbour resizing by an integer factor; the forward is a
 * negated copy, exact in both dtypes.  The adjoint sums each cell's one clipped rectangle of dL/dflow (a border
 * cell's includes the pixels of the replicate padding) in a fixed order without atomics: bit-identical from run
 * to run; a cell with no pixel on the sensor gets 0.  Any other filter: CMAX_EINVAL.                          */
#define CMAX_FILTER_BILINEAR 0
#define CMAX_FILTER_NEAREST 1
int cmax_patch_to_dense_filter(const void *motion, int dtype, int ph, int pw, int pad_h, int pad_w, int sw_h,
                               int sw_w, int H, int W, int filter, int adjoint, void *out, cmax_stream_t stream);

/* Flow basis -> dense flow: D = sum_k theta_k B_k, the map of every motion model that is linear in its parameters (similarity,
 * affine, the rotational motion field of a calibrated camera, a polynomial / PCA / learned basis).  The reference has no
 * counterpart; D is warped by its dense-flow rule x' = x - dt * D[src] (src/warp.py:263-313).
 *   basis_dev  device [K][2][H][W], fp32 or fp64 (`dtype`), 1 <= K <= CMAX_BASIS_MAX_K
 *   adjoint == 0: theta_dev = device DOUBLE [K] whatever `dtype` is; out = D [2][H][W] in `dtype`.  Accumulated in fp64 in the
 *                 order k = 0 .. K-1 and rounded once.
 *   adjoint != 0: theta_dev = dL/dD [2][H][W] in `dtype`; out = device DOUBLE [K], out[k] = sum_e B_k[e] g[e].  Workgroups own
 *                 chunks of CMAX_BASIS_ADJ_CHUNK consecutive elements of [2][H][W], reduce them in fp64 in a fixed tree and a
 *                 second launch adds the chunks in index order: no atomics, bit-identical from run to run.  The chunk sums use a
 *                 stream-ordered temporary of ceil(2 H W / CMAX_BASIS_ADJ_CHUNK) * K doubles (hipMallocAsync).
 * Asynchronous on `stream`.                                                                                              */
#define CMAX_BASIS_MAX_K 64
#define CMAX_BASIS_ADJ_CHUNK 2048
int cmax_basis_to_dense(const void *theta_dev, const void *basis_dev, int dtype, int K, int H, int W, int adjoint, void *out,
                        cmax_stream_t stream);

/* =============================================================================================
 * Fused objective (the hot path): events are packed + sorted once per batch, then every
 * evaluation runs  warp+vote -> contrast -> gather-gradient  without materialising warped events.
 * Replaces one pass of PatchContrastMaximization.get_arg_for_cost + cost.calculate +
 * torch.autograd.grad (src/solver/patch_contrast_base.py:273-352,
 * src/solver/scipy_autograd/torch_wrapper.py:30-49).  Arithmetic: fp32 per event, fp64 reductions.
 * ============================================================================================= */

/* H, W: un-padded sensor size; ph, pw: outer padding (image is [H+2ph, W+2pw]).               */
int cmax_create(int H, int W, int ph, int pw, cmax_handle_t *out);
int cmax_destroy(cmax_handle_t h);

/* Pack (12-bit row | 12-bit col | 8-bit time bin ; fp32 normalised time ; optional fractional
 * residuals) and sort the batch: source tile (16 x 16 pixels) major, inside a tile by pixel
 * (n_time_bin == 0) or by time bin.  events: [n,4] dtype; events whose source pixel is outside
 * the sensor (or NaN), and events whose time is not finite, are dropped (the latter take no part in the
 * time extremes either).  If have_tminmax, (tmin, tmax) are the GLOBAL batch extremes
 * (multi-GPU time slices); otherwise they are reduced from this call's events (all of them) on the
 * device.  n_time_bin > 0 precomputes the voxel bin of every event with the reference's fp64 edge
 * arithmetic (src/warp.py:342-345).  Blocks once (work list sized on the host); 0.10 ms per 1M events
 * (measured before every sort pass also carried the 4-byte source index; not re-measured since -- bench.py's once-per-batch preparation
 * of its 1M-event batch reads 0.21 ms with the index against 0.19 - 0.21 ms without, profiles/weights_cost.txt).
 * Device memory per event: 72 B (packed events, fp64 times, the source index cmax_set_event_weights gathers by, the sort's staging copy) + 4.5 B for the compact copy the hot kernels read
 * when the work list is cut into big segments (un-binned batches of >= 8M events, or by the work-list rule from ~4M). */
int cmax_set_events(cmax_handle_t h, const void *events, int dtype, int64_t n, int have_tminmax,
                    double tmin, double tmax, int n_time_bin, cmax_stream_t stream);
int cmax_set_time_bins(cmax_handle_t h, int n_time_bin, cmax_stream_t stream);
/* LARGE MOTIONS of a 2-DoF / dense objective (round 4): re-order the batch into n_slab time slabs, slab-major inside every source
 * tile row -- (tile row, slab, tile column) -- so that a segment's events span 1/n_slab of the batch's duration and its LDS window is
 * the tiles' extent plus 1/n_slab of the displacement range (a window that would overflow at 150 px over the batch fits again; see
 * DESIGN.md section 4 "large motions").  Results are those of the un-binned order (same events, same arithmetic; the sums are
 * associated differently).  Voxel objectives need cmax_set_time_bins order and refuse a slab handle (cmax_patch_search walks either
 * order since round 5); n_slab <= 1 returns to the un-binned order; the next cmax_set_events starts un-slabbed again.  Blocks once
 * like cmax_set_time_bins.                                                                                                        */
int cmax_set_time_slabs(cmax_handle_t h, int n_slab, cmax_stream_t stream);

/* Per-event weights of the current batch -- the `weight` argument of EventImageConverter.bilinear_vote_tensor / bilinear_vote_numpy and
 * of create_image_from_events_* (src/event_image_converter.py:316-372, 257-314): event e adds w_e times its bilinear footprint.
 *   weights : device pointer, fp32 or fp64 [n], in the CALLER's event order of the last cmax_set_events (n must equal that call's n);
 *             NULL returns the handle to the unweighted state (the kernels and numbers of a handle that never held weights).
 * Weights must be finite IN FP32, the format the library keeps them in (an fp64 weight above 3.4e38 counts as non-finite, one below
 * 1.4e-45 becomes 0): CMAX_EINVAL otherwise, and the handle is left unweighted; any sign and zero are allowed.  Votes are quantised to
 * wmax / 2^20, so results stay within the library's 1e-4 for min|w != 0| / wmax >= 0.01.  They apply to the
 * current batch only: the next cmax_set_events starts unweighted, the same rule as time slabs; cmax_set_time_bins /
 * cmax_set_time_slabs keep them (the library keeps the caller-order copy and every packed event's source index, and gathers again).
 * An event the packing dropped (cmax_set_keep_outside(h, 0)) drops its weight with it.  Device memory: + 8 B per event while weighted
 * (+ 8 B per event for the source index, always).
 * Weighted: cmax_objective, cmax_objective_host, cmax_objective_batch (candidate by candidate), cmax_iwe, cmax_copy_iwe and the
 * un-warped image of the normalised costs (the reference's orig_iwe built with the same weight) -- every model, cost, n_ref, sigma,
 * un-binned / binned / slab order and segment size.  2-DoF objectives take the general vote -> statistics -> gather path; the raw form
 * is not carried (cmax_objective_has_raw returns 0).
 * Numerics: the votes are normalised by wmax = max |w| over the packed events (reduced on the device, kept in device memory): an event
 * votes round(w / wmax * 2^20) (2^19 on big segments) split over its four cells so that the four integers add up to it exactly, and wmax
 * is folded back in where the fixed-point window is flushed to the fp32 image.  The gradient pass multiplies every event's
 * dL/d(x', y') by w.  All weights zero: the image is zero, loss and gradient are what the cost gives on a zero image.
 * REFUSED on a weighted handle with CMAX_EUNSUPPORTED: cmax_objective_hvp[_dist], cmax_objective_raw, cmax_objective_vote / _finish,
 * cmax_objective_dist, cmax_comm_init, cmax_patch_plan_create (and cmax_patch_plan_evaluate / _hvp of a plan made earlier), cmax_patch_search, cmax_set_deterministic(h, 1); and this call on a
 * deterministic handle or one with a communicator.  Blocks once (non-finite check, wmax read-back).                                  */
int cmax_set_event_weights(cmax_handle_t h, const void *weights, int dtype, int64_t n, cmax_stream_t stream);
/* Whether the current batch is weighted, and wmax = max |w| over its packed events (0 when unweighted).  Any pointer may be NULL.   */
int cmax_batch_weighted(cmax_handle_t h, int *weighted, double *wmax_host);

/* Image of warped events for one reference time (fp32 [Hp,Wp], blurred if sigma > 0).
 * motion: fp32 theta[2] | flow[2,H,W] | voxel[T,2,H,W] in pixel per (normalised) time.
 * model < 0 builds the un-warped image ("orig_iwe", patch_contrast_base.py:295-301).          */
int cmax_iwe(cmax_handle_t h, int model, const float *motion, int T, int ref_mode, double ref_frac,
             int normalize_t, double sigma, float *iwe_out, cmax_stream_t stream);

/* Objective descriptor.  loss = sum_k mult_k * term(v_k) over the listed reference times, with
 *   normalized == 0 : term = sign * v_k                      (ImageVariance / GradientMagnitude,
 *                                                              sign = -1 for "minimize")
 *   normalized == 1 : term = v_orig / v_k  ("minimize")       (normalized_*.py, multi_focal_*.py)
 *                     or v_k / v_orig      (otherwise)
 * v = raw contrast (cost, omit_boundary) of the (blurred) IWE; v_orig of the un-warped IWE
 * (NOT boundary-cropped for the variance, normalized_image_variance.py:40-41; cropped like the
 * warped one for every other cost).  The focus losses CMAX_COST_MEAN_SQUARE / _LAPLACIAN /
 * _HESSIAN take the place of the gradient magnitude in every form above; they have no raw form
 * (cmax_objective_has_raw = 0) and are evaluated candidate by candidate by the batched entries. */
typedef struct {
    int32_t model;        /* CMAX_MODEL_* */
    int32_t cost;         /* CMAX_COST_*: 0 .. 4, anything else is CMAX_EINVAL */
    int32_t normalized;   /* 0 / 1 */
    int32_t minimize;     /* 1 = direction "minimize", 0 = "natural"/"maximize" value */
    int32_t negate;       /* 1 = return -loss (multi_focal_* with direction "maximize") */
    int32_t omit_boundary;
    int32_t normalize_t;
    int32_t n_ref;        /* 1..4 reference times */
    int32_t ref_mode[4];  /* CMAX_REF_* */
    double ref_frac[4];
    double mult[4];       /* e.g. forward 1, backward 1, middle 2 */
    double sigma;         /* blur (0 = none) */
    int32_t T;            /* voxel time bins */
    int32_t motion_dtype; /* CMAX_F32 (0): `motion` is fp32.  CMAX_F64: `motion` points to doubles of the same layout -- double theta[2],
                             double flow[2,H,W] or double voxel[T,2,H,W], the optimiser's own fp64 parameters
                             (src/solver/patch_contrast_pyramid.py:186): the bulk arithmetic stays fp32, on (float)motion -- what an fp32
                             call on the rounded motion runs --, but the cell floor(x' + 1e-6) of an event that lies within fp32
                             rounding of a cell border is decided in fp64 from these doubles, like the reference does
                             (src/event_image_converter.py:340).  A flow / voxel is split once per call into (float)v and
                             (float)(v - (float)v) in scratch of the handle (one streaming launch; the scratch grows on the first such
                             call, with a stream synchronisation -- not inside a stream capture).  Accepted by every entry that takes a
                             descriptor with this field: cmax_objective, _host, _vote, _finish, _batch, _dist, _weight_grad,
                             _event_grad, _hvp, _hvp_dist and (cmax_iwes_t) cmax_iwes, _vjp, _jvp, _vjp_tan.  Outputs keep their
                             dtypes (the gradient and the product of a flow model are fp32), tangents stay fp32. */
} cmax_objective_t;

/* One evaluation.  result[0] = loss, result[1..n_ref] = v_k, result[5] = v_orig (device
 * doubles, result has 8 entries).  grad: fp64 [2] for 2DOF, fp32 [2,H,W] / [T,2,H,W] otherwise
 * (overwritten); NULL skips the gradient pass.  motion: fp32 theta[2] | flow[2,H,W] | voxel[T,2,H,W]
 * (or doubles of the same layout, see cmax_objective_t::motion_dtype).                         */
int cmax_objective(cmax_handle_t h, const cmax_objective_t *desc_host, const void *motion,
                   double *result, void *grad, cmax_stream_t stream);

/* The same evaluation plus dL/dw, the derivative of the loss with respect to the per-event weights -- what the reference leaves in
 * `weight.grad` when the image is built with a weight tensor on the autograd tape (src/event_image_converter.py:316-372) and the
 * loss is back-propagated; per event it is what cmax_vote_bwd returns as gw, summed over the images of the objective:
 *     dL/dw_e = sum_k bilin(G_k; x'_e,k)  (+ bilin(G_orig; x_e) for the normalised and multi-focal costs),
 *     bilin(G; x') = (1-a)(1-b) G00 + a(1-b) G10 + (1-a) b G01 + a b G11,   G_k = dL/dIWE_k,  G_orig = dL/dI_orig
 * (cell and fractions as the vote decided them; a corner outside the padded image, or outside the region the cost sums over, reads
 * 0).  The value is NOT multiplied by w: an event of weight 0 has a derivative.  An unweighted handle means w = 1.
 * result[8] and grad: exactly as cmax_objective (grad may be NULL).  grad_w: fp32 [n] in the CALLER'S event order, n = the n given to
 * cmax_set_events (CMAX_EINVAL otherwise); events that were not packed get 0; an empty handle returns zeros.  Asynchronous on `stream`.
 * Works on weighted and unweighted handles, after cmax_set_time_bins / cmax_set_time_slabs, on every segment layout, on the
 * clipped-window path and for 2-DoF batches with kept off-sensor events.  The evaluation takes the general vote -> statistics ->
 * gather path; a gather kernel of its own then interpolates a finished G image per reference time (and G_orig at the un-warped
 * positions) into one plane per image in packed order, and a scatter sums the planes in index order into grad_w.  Device memory
 * on first use: 20 B per event + 10 images.  CMAX_EUNSUPPORTED on a deterministic handle and on one that holds a communicator.   */
int cmax_objective_weight_grad(cmax_handle_t h, const cmax_objective_t *desc_host, const void *motion, double *result,
                               void *grad /* may be NULL */, float *grad_w, int64_t n, cmax_stream_t stream);

/* The same evaluation plus dL/d(event), the third leaf of the reference's autograd graph: its solvers mark the events themselves as a
 * leaf (`self.events = torch.from_numpy(events).double().requires_grad_()`, src/solver/patch_contrast_mixed.py:166, and the pyramid
 * solver likewise), so `events.grad` exists after `backward()` through the warp (src/warp.py:254-259, 303-307, 506-515) and the
 * bilinear vote (src/event_image_converter.py:316-372).  Row e of grad_events, fp32 [n][3] in the CALLER'S event order:
 *     [0], [1]  dL/dx_e, dL/dy_e (x = row) = sum_k w_e (dL/dx'_e,k, dL/dy'_e,k)  (+ the same pair from G_orig at the un-warped position for
 *               the normalised and multi-focal costs),  dL/dx' = (1-b)(G10-G00) + b(G11-G01),  dL/dy' = (1-a)(G01-G00) + a(G11-G10)
 *               -- what cmax_vote_bwd returns as (gx, gy) per image; cell and fractions as the vote decided them, a corner outside the
 *               padded image or outside the region the cost sums over reads 0; w_e = 1 on an unweighted handle;
 *     [2]       C_e = sum_k c_e,k,  c_e,k = dL/d(dt_e,k): the derivative with respect to the event's time offset AS THE WARP USES IT
 *               (normalised or raw, as normalize_t says): w_e (gx theta_x + gy theta_y) for 2-DoF, -w_e (gx f_x[src] + gy f_y[src]) for a
 *               dense flow, the same with the flow of the event's bin for a voxel flow; source pixel and bin are piecewise constant,
 *               as in the reference's autograd.
 * csum: device double[4], csum[k] = sum_e c_e,k per reference time in fp64 (entries k >= n_ref are zero) -- with C_e and the events'
 * times this is all the chain rule through t.min() / t.max() needs (CMaxHandle.events_grad composes the reference's [n,4]).
 * result[8] and grad: exactly as cmax_objective (grad may be NULL).  n = the n given to cmax_set_events (CMAX_EINVAL otherwise); events
 * that were not packed keep a row of zeros; an empty handle returns zeros.  Asynchronous on `stream`; the output is the same bits on
 * every run for the same images (no atomics behind the evaluation).  Works wherever cmax_objective_weight_grad works; the evaluation
 * takes the general path, `k_event_grad_gather` stores three packed-order planes per reference time (two for the un-warped image),
 * `k_event_grad_scatter` sums them into the caller's order.  Device memory on first use: 56 B per event + 10 images.
 * CMAX_EUNSUPPORTED on a deterministic handle and on one that holds a communicator.                                                  */
int cmax_objective_event_grad(cmax_handle_t h, const cmax_objective_t *desc_host, const void *motion, double *result,
                              void *grad /* may be NULL */, float *grad_events, int64_t n, double *csum, cmax_stream_t stream);

/* =============================================================================================
 * The image of warped events as a differentiable layer: the caller stands in for the image-side kernels (statistics, dL/dIWE) and
 * brings its own cost.  In the reference the IWE is an ordinary torch tensor, so any CostBase subclass -- or any torch expression on
 * arg["iwe"] -- is differentiable once and twice (src/costs/base.py, torch.autograd.functional.vhp in
 * src/solver/scipy_autograd/torch_wrapper.py:51-73); these four calls give the event side of that: the images, J^T G, J u and the
 * derivative of J^T G along a tangent, with the segment / window / exact-cell machinery of the fused objective.
 * I_k(m) below is the padded [Hp,Wp] image at reference time k, blurred when sigma > 0, weighted on a weighted handle: exactly what
 * cmax_iwe returns for that reference time.  J_k = dI_k/dm with the bilinear cells held fixed.
 * All four run on weighted and unweighted handles, in un-binned / binned / slab order and on every segment layout; CMAX_EUNSUPPORTED on a
 * deterministic handle and on one that holds a communicator; an empty handle gives exact zeros.
 * STATE: none of the four relies on anything an earlier call left on the handle -- not on the windows and cell offsets a vote published
 * (they belong to the last vote only), not on another cmax_iwes, cmax_objective, cmax_set_time_slabs / _bins or cmax_set_event_weights in
 * between.  Each call RE-DERIVES what it needs from the motion it is given: the second-order kernels (k_vote_tan, k_grad_hvp) warp
 * their segment and build their LDS window themselves, and the per-event interpolation behind grad_w runs behind a K1 launch that only
 * publishes windows (no votes).  The price: a backward call warps the events again (one warp per reference time in the gather; with
 * grad_w one windows-only K1 more) instead of re-using the forward's windows -- and the result is that of the handle's state (order,
 * weights) AT THE TIME OF THE CALL.  Scratch on first use: 28 images.
 * ============================================================================================= */
typedef struct {
    int32_t model;        /* CMAX_MODEL_* */
    int32_t normalize_t;
    int32_t n_ref;        /* 1..4 reference times */
    int32_t ref_mode[4];  /* CMAX_REF_* */
    double ref_frac[4];
    double sigma;         /* 3-tap blur of every image (0 = none) */
    int32_t T;            /* voxel time bins */
    int32_t motion_dtype; /* as cmax_objective_t::motion_dtype */
    int32_t with_orig;    /* 1: one more image behind the n_ref, the un-warped events (the reference's orig_iwe) */
} cmax_iwes_t;
int cmax_sizeof_iwes(void);
/* images: fp32 [n_ref (+1), Hp, Wp], overwritten: images[k] = I_k(m); images[n_ref] = the un-warped image when with_orig.  Votes go
 * straight into the caller's buffer (sigma > 0: into the library's scratch, the blur writes the caller's buffer); the handle's own
 * double-buffered vote images are not touched.                                                                                     */
int cmax_iwes(cmax_handle_t h, const cmax_iwes_t *desc_host, const void *motion, float *images, cmax_stream_t stream);
/* grad_motion = sum_k J_k^T gimages[k]: fp64 [2] for 2-DoF, fp32 [2,H,W] / [T,2,H,W] otherwise, overwritten (like cmax_objective's grad).
 * gimages: fp32, the shape of `images` -- the caller's dL/dI_k, the whole truth: no region mask, no chain factor; a corner outside the
 * padded image reads 0; the blur's transpose is applied when sigma > 0.  The un-warped image does not depend on the motion.
 * grad_w (NULL: skipped; else fp32 [n], n = the n given to cmax_set_events) = sum_k bilin(gimages[k]; x'_e,k) (+ bilin(gimages[n_ref]; x_e)
 * with with_orig), in the CALLER'S event order, NOT multiplied by w, zeros for events that were not packed: cmax_objective_weight_grad's
 * output with the caller's G.                                                                                                      */
int cmax_iwes_vjp(cmax_handle_t h, const cmax_iwes_t *desc_host, const void *motion, const float *gimages, void *grad_motion,
                  float *grad_w, int64_t n, cmax_stream_t stream);
/* dimages[k] = J_k u, fp32 [n_ref, Hp, Wp], overwritten (the un-warped image has no tangent: with_orig is ignored).  tangent: fp32, the
 * layout of the motion, SCALED TO UNIT MAX-NORM by the caller as for cmax_objective_hvp (fixed-point derivative votes, scale per
 * reference time; on a weighted handle the votes are normalised by wmax as in K1).                                                  */
int cmax_iwes_jvp(cmax_handle_t h, const cmax_iwes_t *desc_host, const void *motion, const float *tangent, float *dimages,
                  cmax_stream_t stream);
/* out = d/d(eps) [ J(m + eps u)^T (G + eps G') ] at eps = 0, summed over k; G = gimages, G' = gimages_tan (both the shape of `images`; the
 * plane of the un-warped image is not read).  out has the shape and dtype of grad_motion, overwritten.  With G' = (d2 l / dI2) J u this is
 * the exact Hessian-vector product of any loss l(I); with G' = 0 the mixed term alone.  tangent as for cmax_iwes_jvp.               */
int cmax_iwes_vjp_tan(cmax_handle_t h, const cmax_iwes_t *desc_host, const void *motion, const float *tangent, const float *gimages,
                      const float *gimages_tan, void *out, cmax_stream_t stream);

/* The same evaluation with its results delivered TO THE HOST -- what an optimiser written in C calls once per iteration
 * (the reference's TorchWrapper.get_value_and_grad ends in .cpu().numpy(), src/solver/scipy_autograd/torch_wrapper.py:46-49):
 * enqueues the evaluation and the copies on `stream` and returns when result_host[8] and grad_host (double[2] for 2DOF, else
 * fp32 [2,H,W] / [T,2,H,W]; NULL: value only) are filled.  Blocks (busy-waits).  For the 2-DoF image-variance objective
 * the one-wave finishing kernel writes loss and gradient straight into pinned host memory and a run counter behind them,
 * which this call polls: no copy engine and no driver call between the last kernel and the caller (23.7 us per sequential
 * evaluation of 1M events, profiles/r03_ablation.txt 10).  Other objectives: cmax_objective + copies through pinned staging. */
int cmax_objective_host(cmax_handle_t h, const cmax_objective_t *desc_host, const void *motion, double *result_host,
                        void *grad_host, cmax_stream_t stream);

/* K candidate motions in one call (the reference's gradient-free paths evaluate the objective for batches of sampled motions:
 * src/solver/base.py:738-758 run_optuna, src/solver/patch_contrast_pyramid.py:363-415; a line search asks for several steps along one
 * direction).  motions: K consecutive motions as cmax_objective takes one (fp32 theta[2] | flow[2,H,W] | voxel[T,2,H,W], or -- motion_dtype
 * CMAX_F64 -- doubles of the same layout); results: device double[K][8]; grads: device double[K][2] (2DOF) or fp32 [K][...] (NULL: values only).
 * For the 2-DoF image-variance objective (sigma 0, not normalised, default mode, no communicator) the K evaluations share ONE
 * launch of each kernel: blockIdx.z is the candidate -- its own vote image, sums and windows -- so the launch structure that is 40 %
 * of a single 1M-event evaluation is paid once per batch.  Every other objective is evaluated candidate by candidate inside the call
 * (same results).  1 <= K <= 64; the handle keeps 2 K vote images for it.                                                       */
int cmax_objective_batch(cmax_handle_t h, const cmax_objective_t *desc_host, const void *motions, int K, double *results,
                         void *grads, cmax_stream_t stream);

/* Raw form of the 2-DoF objectives (default mode, non-empty batch; cmax_objective_has_raw says whether a descriptor on the
 * current batch qualifies -- everything 2-DoF except a NORMALISED plain variance, whose fold needs device-side statistics).
 * cmax_objective ends such an evaluation with a one-wave kernel that only adds up what the gathering kernel left and divides a
 * few numbers -- a third of the headline evaluation, as a launch; here that kernel is not launched.  `raw` (device,
 * CMAX_RAW_DOUBLES doubles per reference time, cleared by the library inside the evaluation) receives CMAX_RAW_LINES partial
 * sums, one 128-byte line each, added with fp64 atomics by the gathering workgroups:
 *   image variance, sigma 0 ("deferred statistics": no image kernel runs at all): doubles 0..5 of a line =
 *     (S1x, S1y, S2x, S2y, sum I, sum I^2), S1 = sum_e dt * bilinear-difference(1_Omega IWE), S2 = the same of 1_Omega;
 *   every other objective: doubles 0, 1 = sum_e dt * dL/d(x', y') (chain factors applied), and doubles 8..15 of the FIRST
 *     line = result[8] as cmax_objective would deliver it (written by the gathering kernel's first workgroup).
 * The CONSUMER finishes: copy the buffer to the host whenever it needs the numbers and call cmax_finalize_raw_host (pure host
 * arithmetic: sums the lines; deferred form: loss = -/+ var, dL/dtheta = c (S1 - mu S2)).  Asynchronous like cmax_objective. */
#define CMAX_RAW_LINES 32
#define CMAX_RAW_DOUBLES (CMAX_RAW_LINES * 16)
int cmax_objective_has_raw(cmax_handle_t h, const cmax_objective_t *desc_host);
int cmax_objective_raw(cmax_handle_t h, const cmax_objective_t *desc_host, const void *motion, double *raw,
                       cmax_stream_t stream);
/* raw_host: host copy of `raw` ([n_ref][CMAX_RAW_DOUBLES]).  result_host[8] as for cmax_objective; grad_host double[2]
 * (NULL: value only).                                                                            */
int cmax_finalize_raw_host(cmax_handle_t h, const cmax_objective_t *desc_host, const double *raw_host,
                           double *result_host, double *grad_host);

/* Exact Hessian-vector product of the objective w.r.t. the motion, H u -- what
 * torch.autograd.functional.vhp returns in the reference (src/solver/scipy_autograd/torch_wrapper.py:
 * 51-73; the Hessian is symmetric): derivative of the analytic gradient along `tangent` with the
 * bilinear cells held fixed.  tangent: fp32, same layout as motion, SCALED TO UNIT MAX-NORM by the
 * caller (H is linear in u; the derivative votes are accumulated in fixed point).  hv: fp64 [2]
 * (2DOF) or fp32 [2,H,W] / [T,2,H,W], overwritten.  Costs as in cmax_objective.                 */
int cmax_objective_hvp(cmax_handle_t h, const cmax_objective_t *desc_host, const void *motion,
                       const float *tangent, void *hv, cmax_stream_t stream);

/* Phase-split form for time-sliced multi-GPU runs (one handle per GPU, each holding a contiguous
 * time slice of the batch and the GLOBAL tmin/tmax):
 *   cmax_objective_vote    raw votes of this slice: images[k] for k < n_ref, plus images[n_ref] =
 *                          the un-warped image when a normalised cost needs it and it is not cached;
 *                          *n_images_host = number of images written (n_ref or n_ref + 1)
 *   -- caller all-reduces (sum) images[0 .. n_images) across GPUs (RCCL) --
 *   cmax_objective_finish  blur, contrast statistics, loss (identical on every GPU), then the
 *                          gradient contribution of THIS slice's events
 *   -- caller all-reduces (sum) grad --
 * images: fp32 [5, Hp, Wp] caller-owned.  cmax_objective == vote + finish on internal images.
 * Without a blur the handle keeps POINTERS into `images` for cmax_copy_iwe (see there): keep the buffer until the image was read.
 * `motion` of the finish call must be the buffer AND the values of the preceding vote call: the gather re-uses
 * the LDS windows the vote derived for every segment.                                          */
int cmax_objective_vote(cmax_handle_t h, const cmax_objective_t *desc_host, const void *motion,
                        float *images, int *n_images_host, cmax_stream_t stream);
int cmax_objective_finish(cmax_handle_t h, const cmax_objective_t *desc_host, const void *motion,
                          const float *images, int n_images, double *result, void *grad,
                          cmax_stream_t stream);

/* =============================================================================================
 * Time-sliced multi-GPU evaluation (the reference has no distributed code).
 * One process per GPU; every rank owns a handle holding a contiguous TIME SLICE of the batch
 * (cmax_set_events with have_tminmax = 1 and the batch-wide extremes) and one RCCL communicator.
 * The collectives are enqueued by the library on the caller's stream, between its own kernels:
 *   K1 votes of this slice -> all-reduce(sum) of [n_images, Hp, Wp] fp32 (all reference times and the
 *   un-warped image in ONE call) -> contrast statistics + loss (redundantly, identical on every rank)
 *   + K3 gather of this slice's events -> all-reduce(sum) of the gradient (fp64 [2] | fp32 [2,H,W] |
 *   fp32 [T,2,H,W]).  No other exchange; no host synchronisation.
 *   2-DoF with the plain variance cost (BASELINE's headline) needs ONE exchange: K1 votes the image and its two
 *   tangent images dI/dtheta (two more votes per event), one all-reduce carries the three of them, and every rank
 *   finishes loss and gradient <dL/dI, dI/dtheta> in image space -- no pass over the events for the gradient and no
 *   16-byte all-reduce whose cost is pure latency.
 * RCCL is bound at run time (the librccl already in the process, i.e. torch's, else ROCm's); a handle
 * without a communicator -- or with nranks == 1 -- never touches it.
 * ============================================================================================= */
/* 0 if RCCL can be bound in this process (and binds it), CMAX_ENODEV otherwise -- a LOCAL call, no rank waits for another:
 * the ranks agree on it (by whatever transport carries the rendezvous id) BEFORE any of them enters cmax_comm_init, which
 * blocks in ncclCommInitRank until every rank has called it.  path_host (optional, path_capacity bytes): the shared
 * object the entry points were resolved from -- torch's bundled librccl when the process already holds one.       */
int cmax_comm_available(char *path_host, int path_capacity);
#define CMAX_COMM_ID_BYTES 128
/* rank 0: a fresh rendezvous id (ncclGetUniqueId) into id_host[128]; ship it to the other ranks
 * by any means (torch.distributed broadcast, a file, MPI).                                      */
int cmax_comm_unique_id(void *id_host);
/* Collective over the ranks (blocks until all nranks processes have called): binds the handle's
 * device (the current HIP device must be the one the handle was created on) to rank `rank`.
 * nranks == 1 with id_host == NULL: no communicator, RCCL is never loaded; with an id a real 1-rank
 * communicator is made (cmax_objective_dist then runs the N > 1 enqueue sequence, RCCL included). */
int cmax_comm_init(cmax_handle_t h, const void *id_host, int nranks, int rank);
int cmax_comm_destroy(cmax_handle_t h);
/* nranks / rank of the handle's communicator (1 / 0 without one); rccl_version: ncclGetVersion, 0
 * if RCCL was never loaded.                                                                      */
int cmax_comm_info(cmax_handle_t h, int *nranks, int *rank, int *rccl_version);
/* In-place all-reduce of a device buffer on the handle's communicator (dtype CMAX_F32 / CMAX_F64;
 * op 0 sum, 1 min, 2 max) -- e.g. (t_min, -t_max) with op min to agree on the batch extremes.   */
int cmax_comm_allreduce(cmax_handle_t h, void *buf, int64_t count, int dtype, int op, cmax_stream_t stream);
/* Overlap of the gradient exchange with the gather (dense objectives).  With bands > 1 cmax_objective_dist exchanges the gradient
 * as `bands` grouped all-reduces of source-tile-row bands on a second stream of the handle (events order the two streams; the
 * caller's stream continues after the last band is reduced).  EVERY RANK MUST SET THE SAME VALUE: the bands follow from the
 * sensor's tile rows and this setting alone, so all ranks issue the same collectives whatever their own slice looks like; a
 * rank whose work list is group-aligned (cmax_batch_info's owned_groups) launches its gathering kernel band by band, so that a
 * band's rows are exchanged while the next band is gathered -- the others (no owned groups, deterministic mode, no events)
 * finish their gradient first and issue the same exchanges behind it.  bands = 1 (default): one all-reduce.  Same results. */
int cmax_comm_set_c2_bands(cmax_handle_t h, int bands);
/* One evaluation of the whole (time-sliced) batch: same arguments and results as cmax_objective,
 * the same on every rank BIT FOR BIT -- the gradient because it is all-reduced, result[8] because
 * it leaves as rank 0's (every other rank zeroes its eight doubles and they ride in the gradient's
 * all-reduce as one grouped call; a value-only evaluation exchanges the 64 bytes alone): replicated
 * optimisers (src/solver/scipy_autograd/scipy_minimize.py:100-117 on every rank) take identical
 * decisions.  A rank may hold zero events.  Without a communicator: == cmax_objective.          */
int cmax_objective_dist(cmax_handle_t h, const cmax_objective_t *desc_host, const void *motion,
                        double *result, void *grad, cmax_stream_t stream);

/* The exact Hessian-vector product of the whole (time-sliced) batch: cmax_objective_hvp with one grouped all-reduce of the images
 * and the tangent images (both are sums over events) and one of the product.  Without a communicator: == cmax_objective_hvp.   */
int cmax_objective_hvp_dist(cmax_handle_t h, const cmax_objective_t *desc_host, const void *motion,
                            const float *tangent, void *hv, cmax_stream_t stream);

/* Deterministic mode ("race detection"): bit-identical IWE, loss and gradient from run
 * to run for cmax_iwe / cmax_objective / cmax_objective_vote + _finish / cmax_objective_hvp.  By default the vote flush, the flow
 * gradient and the contrast statistics use floating-point atomics, whose order -- like the order of events inside
 * a sorted group -- varies between runs, so results differ in their last bits (~1e-7 relative).  With enable != 0
 * everything that depends on such an order is accumulated in INTEGERS: votes as 2^-20 fixed point in a 64-bit image
 * (rounded to fp32 once), per-event gradient terms as 64-bit fixed point (scale from max |image|) added per thread,
 * per workgroup and with 64-bit global atomics, statistics with one workgroup per accumulator and the unfused image
 * kernels.  Same arithmetic per event, same parity (1e-4 of the reference); slower: no fused image kernels, one pair
 * of global atomics per event for the flow gradient (dense 5M events: ~10x an evaluation), 40 B per pixel more HBM.
 * cmax_objective_hvp is covered as well (round 3: integer tangent-vote images, integer accumulation of the second-order gather).
 * A patch plan on a deterministic handle (cmax_patch_plan_evaluate / _hvp) is covered too: the interpolation and its adjoint are
 * gathers, the adjoint sweeps of the voxel chain run order-free step kernels (every destination pixel evaluates the scatter of
 * its five sources itself instead of LDS atomics), the tail is one workgroup.  The stand-alone leaf entries
 * cmax_flow_step_adj / cmax_voxel_construct_adj[_tan] have no handle to read the mode from: cmax_set_leaf_deterministic (round 5, a
 * process-wide switch) makes them take the same order-free step kernels.  Across ranks (cmax_objective_dist) the result is as
 * repeatable as RCCL's reduction order.                                                                                          */
int cmax_set_deterministic(cmax_handle_t h, int enable);
int cmax_get_deterministic(cmax_handle_t h, int *enabled);
/* Process-wide: the adjoint leaf operators of the propagation step and of the voxel chain (cmax_flow_step_adj,
 * cmax_voxel_construct_adj, cmax_voxel_construct_adj_tan) accumulate without atomics, in a fixed order -- bit-identical results from
 * run to run (default 0: global / LDS atomics, last-bit differences).  Returns the previous setting.                              */
int cmax_set_leaf_deterministic(int enable);

/* Per-kernel-class timing for bench.py's roofline: when enabled every launch of the four hot kernels
 * is bracketed by HIP events ON THE LAUNCH STREAM.  enable = 1: one launch per bracket (results stay
 * valid; the bracket adds ~2.5 us of marker/dispatch latency to a ~8 us kernel).  enable = R in 2..64:
 * every hot launch is issued R times back to back inside its bracket, which amortises that latency;
 * TIMING ONLY -- votes and gradients are accumulated R times, so the evaluation's numbers are meaningless.  cmax_read_profile synchronises on them, returns
 * total milliseconds and launch counts for class 0 = K1 warp+vote, 1 = K2 contrast statistics,
 * 2 = K2b gradient image, 3 = K3 per-event gradient (host arrays of 4), and resets.           */
int cmax_set_profiling(cmax_handle_t h, int enable);
int cmax_read_profile(cmax_handle_t h, double *total_ms_host, int64_t *count_host);
/* The same with every class (host arrays of CMAX_PROF_CLASSES): 0..3 as above, 4 = finishing kernels
 * (k_finish*, k_finalize), 5 = RCCL collectives (never repeated inside a bracket).                 */
#define CMAX_PROF_CLASSES 6
int cmax_read_profile_all(cmax_handle_t h, double *total_ms_host, int64_t *count_host);

/* sizeof(cmax_objective_t) as compiled into the library (binding self-check).                 */
int cmax_sizeof_objective(void);

/* Copy the fp32 IWE [Hp,Wp] of reference time k of the last cmax_objective call (the image the
 * contrast was evaluated on, i.e. blurred when sigma > 0) into iwe_out, on `stream`.
 * After cmax_objective_finish WITHOUT a blur (sigma == 0) that image is the caller's own `images` buffer, which the library
 * does not copy: it has to stay allocated and unchanged until this call has run, or stale memory is copied with no error.      */
int cmax_copy_iwe(cmax_handle_t h, int k, float *iwe_out, cmax_stream_t stream);

/* What cmax_set_events made of the last batch: events packed; events DROPPED because their source pixel lies
 * outside the sensor or is NaN, or because their time is not finite (the fused path indexes the flow field and the source tiles with it; for 2-DoF
 * objectives cmax_set_keep_outside below keeps them, as the reference does -- the leaf operators cmax_warp_events +
 * cmax_vote have no such filter either way); whether
 * any source coordinate is fractional; whether the work list gives every group to one segment (owned groups:
 * single-reference dense / voxel gradients are then stored, not added).  Any pointer may be NULL.            */
int cmax_batch_info(cmax_handle_t h, int64_t *n_packed, int64_t *n_dropped, int *has_fractional, int *owned_groups);
/* Events OFF THE SENSOR (round 4).  The reference's 2-DoF warp has no bounds test on the source (src/warp.py:506-515): an event from
 * outside the sensor votes wherever it warps into the padded image.  With cmax_set_keep_outside(h, 1) the next cmax_set_events packs
 * such events (finite coordinates) instead of dropping them: at the NEAREST sensor pixel, the rest of the way in the fp32 residuals
 * that fractional source coordinates use -- the event kernels then see x = ix + rx exactly as for any fractional source (a residual of
 * r px carries ulp(r) / 2 of rounding: 4e-6 px at 100 px).  cmax_batch_outside reports how many the last batch held; they count as
 * packed, not as dropped.  Only the 2-DoF model (and the un-warped image) is defined for them: a dense / voxel objective, cmax_iwe of
 * those models and cmax_patch_search refuse a batch that holds any (CMAX_EINVAL) -- the reference indexes its flow with the source
 * pixel there (negative indices wrap around in torch; nothing a caller can mean).  Default since round 5: ON -- a handle follows the
 * function cited above; cmax_set_keep_outside(h, 0) asks for such events to be dropped (and counted: cmax_batch_info) while packing,
 * which is what a caller of a dense / voxel objective on such a batch has to say explicitly.                                     */
int cmax_set_keep_outside(cmax_handle_t h, int on);
int cmax_batch_outside(cmax_handle_t h, int64_t *n_outside);
/* The work list cmax_set_events / cmax_set_time_bins cut for the event kernels (one workgroup per segment): number of
 * segments; segment_events = the most events a segment holds (2040, 3064 for MID, or 4088 for BIG segments: batches of >= 8M events, and
 * smaller ones whose group sizes ask for it -- DESIGN.md section 2); small_accumulators = 1 when a binned list was cut at
 * three (tile, bin) groups per segment for the voxel gradient kernel with the small LDS accumulator array.  Any pointer may
 * be NULL.  (Introspection for tests and tuning: results do not depend on the cut.)                                       */
int cmax_work_list_info(cmax_handle_t h, int *n_segments, int *segment_events, int *small_accumulators);

/* Introspection for tests / bench: number of packed events, HBM bytes held by the handle.     */
int cmax_handle_info(cmax_handle_t h, int64_t *n_events, int64_t *workspace_bytes);
/* Measurement aid (bench.py's roofline.launch_floor_us): enqueues `pairs` times two dependent EMPTY kernels with the grids of
 * the warp + vote kernel and of the gather kernel of a single-reference objective on the current batch -- what the headline
 * evaluation's launch structure costs when its kernels do nothing.  The caller brackets the call with events on `stream`.   */
int cmax_debug_launch_floor(cmax_handle_t h, int pairs, cmax_stream_t stream);
/* Tuning aid (tools/timeline.py; libraries built with -DCMAX_TIMELINE only, CMAX_ESTATE otherwise): device buffer of 2 x 4096 x 8
 * uint64 into which thread 0 of the event kernels' workgroups stamps the wall clock at its phase boundaries (NULL: off).       */
int cmax_debug_timeline(void *device_buffer);
/* Test aid (tests/test_gpu_fused.py::test_packed_order): copies the packed, sorted events of the current batch -- n_events x 2 uint32:
 * [row | col << 12 | (time bin, or the time's residual beyond fp32) << 24,  bits of the fp32 normalised time] -- and the group starts
 * the work list was cut from ([n_groups + 1] int32; NULL skips them; *n_groups_host receives their number: source tiles, x time bins
 * / slabs on binned handles; all zero for an empty batch, which is not sorted) into device buffers, on `stream`.  The layout is what
 * DESIGN.md section 2 describes, not a stable ABI.                                                                                    */
int cmax_debug_packed_events(cmax_handle_t h, void *events_out, int *group_start_out, int *n_groups_host, cmax_stream_t stream);
/* Test aids (tests/test_gpu_work_list.py), in the style of cmax_debug_packed_events: not a stable ABI, nothing allocated that stays.
 * cmax_debug_work_list copies the work list of the last cut as the event kernels read it -- n_segments x int4 {first event, count, first
 * group, number of groups} -- into the device buffer segments_out on `stream` (NULL: the count only), and stores on the host the number
 * of segments, the CMAX_WL_* flags and the most events a segment may hold (2040 / 3064 / 4088), all as the handle holds them after the
 * last cut (an empty batch makes no cut: zero segments, the flags of the cut before).  Any host pointer may be NULL.
 * cmax_debug_compact_events copies the compact regions of that work list (cmax_event_kernels.inc, "COMPACT EVENTS": n_segments x 18496
 * bytes -- 4096 slot words | 512 words of tile nibbles | 16 header words) into the device buffer regions_out and stores the flag the
 * packing kernel raises when an event does not fit its segment's strip (0: never raised; the call waits for `stream`).  CMAX_ESTATE
 * on a handle whose current work list has no compact copy.                                                                         */
#define CMAX_WL_BIG 1u        /* segments of up to 4088 events                              */
#define CMAX_WL_MID 2u        /* segments of up to 3064 events                              */
#define CMAX_WL_OWNED 4u      /* every group belongs to exactly one segment of whole groups */
#define CMAX_WL_SMALL_ACC 8u  /* binned list cut at three groups per segment (five on mid)  */
#define CMAX_WL_SLAB_MAJOR 16u /* groups are (tile row, slab, tile column)                  */
#define CMAX_WL_COMPACT 32u   /* a compact copy of the events exists for this list          */
#define CMAX_WL_LONG_RUNS 64u /* >= 8 events per active source pixel                        */
int cmax_debug_work_list(cmax_handle_t h, void *segments_out, int *n_segments_host, unsigned *flags_host, int *seg_max_host, cmax_stream_t stream);
int cmax_debug_compact_events(cmax_handle_t h, void *regions_out, int *flag_host, cmax_stream_t stream);

/* =============================================================================================
 * The optimiser's objective for patch-based flow in one call: what
 * scipy.optimize calls through TorchWrapper.get_value_and_grad / get_hvp
 * (src/solver/scipy_autograd/torch_wrapper.py:30-73) on
 * PyramidalPatchContrastMaximization.objective_scipy + motion_to_dense_flow
 * (src/solver/patch_contrast_pyramid.py:430-516):
 *   x [2,ph,pw] patch motion (host fp64, pixel per time unit)
 *     -> dense flow (cmax_patch_to_dense) * t_scale  [-> voxel (cmax_voxel_construct)]  -> fp32
 *     -> loss = sum_i weight_i * cmax_objective(term_i)  + tv_weight * total_variation(x)
 *   and the gradient back through the adjoints, returned to host fp64.  One stream
 *   synchronisation per call; intermediates live in the plan.
 * Time-aware plans with scale_later != 0 (solver.scale_later, src/solver/base.py:219-224,
 * patch_contrast_pyramid.py:489-515) propagate the flow RESCALED BY ITS MAXIMUM: with D = dense flow of x,
 *   s = max D  (one signed scalar over both components),  voxel = s * cmax_voxel_construct(t_scale * D / s);
 *   the derivative of s goes evenly to the pixels equal to the maximum (torch.Tensor.max), and gradient and
 *   Hessian-vector product follow the whole map.  s lives in device memory: no host read-back inside a call.
 *   max D == 0 (x = 0) or not finite: loss, gradient and product are NaN, as the reference's 0/0 -- the event
 *   kernels are given a finite motion all the same.
 * Terms with motion_dtype == CMAX_F64 (all of them or none): the fused terms decide the cells of events on a cell border from the
 *   fp64 flow / voxel the plan holds, not from its fp32 rounding -- the conversion launches write both planes (see
 *   cmax_objective_t::motion_dtype), evaluate, product and graph replay alike.
 * ============================================================================================= */
typedef struct {
    int32_t n_terms;          /* 1..4 fused contrast terms of a hybrid cost (src/costs/hybrid.py:48-57) */
    int32_t time_aware;       /* 0: terms use CMAX_MODEL_DENSE; 1: CMAX_MODEL_VOXEL on the propagated flow */
    int32_t T, scheme, t0;    /* time bins, CMAX_SCHEME_*, bin that holds the patch flow (0 "first", T/2 "middle") */
    int32_t H, W;             /* sensor size of the handle */
    int32_t ph, pw;           /* patch grid */
    int32_t sw_h, sw_w;       /* sliding window = up-sampling factor */
    int32_t pad_h, pad_w;     /* replicate padding of the grid (patch_contrast_base.py:470-479) */
    int32_t tv_omit_boundary;
    int32_t scale_later;      /* time_aware only (ignored otherwise): propagate t_scale * D / max(D), multiply the voxel by max(D) */
    int32_t filter_type;      /* CMAX_FILTER_* of the patch grid -> dense flow map (0 = bilinear).  Sits in what was the padding in
                                 front of t_scale: sizeof and every other offset are unchanged */
    double t_scale;           /* pixel per time unit -> pixel per normalised batch period */
    double weight[4];
    double tv_weight;         /* 0 = no total_variation term; sign of the cost direction included */
    cmax_objective_t term[4];
} cmax_patch_objective_t;
typedef struct cmax_patch_plan_s *cmax_patch_plan_t;

int cmax_sizeof_patch_objective(void);
int cmax_patch_plan_create(cmax_handle_t h, const cmax_patch_objective_t *desc_host, cmax_patch_plan_t *out);
int cmax_patch_plan_destroy(cmax_patch_plan_t plan);
/* A plan outlives a batch: the next batch behind the same handle (cmax_set_events) usually has another duration.  */
int cmax_patch_plan_set_t_scale(cmax_patch_plan_t plan, double t_scale);
/* Introspection for tests.  Default: every evaluation is launched eagerly (*graph_replay_enabled = 0).  With
 * CMAX_PLAN_GRAPHS=1 in the environment at plan creation, evaluations after the first few are replayed from
 * captured hipGraphs (one per distinct launch sequence; 0 again if a capture failed).                        */
int cmax_patch_plan_info(cmax_patch_plan_t plan, int *n_graphs, int *graph_replay_enabled);
/* cmax_patch_plan_create on a handle that holds a communicator returns CMAX_EINVAL for a scale_later plan (not built for
 * time-sliced batches).
 * On a handle that holds a communicator (cmax_comm_init: a time slice of the batch per rank) both calls below evaluate the WHOLE
 * batch, the same numbers on every rank: the fused terms exchange their images like cmax_objective_dist (and the product its
 * tangent images), but the flow gradient is not exchanged -- each rank carries its share through the (linear) adjoints of the voxel
 * chain and of the patch interpolation, and the ranks all-reduce 2 ph pw numbers (4 KB for a 16 x 16 grid instead of 7.4 MB of flow
 * gradient at 720p).  Every rank must make the same calls in the same order.
 * x_host [2*ph*pw] -> *loss_host, grad_host [2*ph*pw] (NULL: value only).  with_tv = 0 leaves the
 * total_variation term out (the smooth part, differenced for time-aware Hessian-vector products).
 * Blocks until the result is on the host.                                                      */
int cmax_patch_plan_evaluate(cmax_patch_plan_t plan, const double *x_host, int with_tv, double *loss_host,
                             double *grad_host, cmax_stream_t stream);
/* Exact Hessian-vector product w.r.t. x: t^2 P^T H_flow P v (cmax_objective_hvp inside); time-aware plans add the
 * voxel chain, t P^T [J^T H_VV J + (dJ[.])^T g_V] t P v (cmax_voxel_construct_tan / _adj_tan).  The
 * total_variation term has zero Hessian almost everywhere.                                      */
int cmax_patch_plan_hvp(cmax_patch_plan_t plan, const double *x_host, const double *v_host, double *hv_host,
                        cmax_stream_t stream);

/* =============================================================================================
 * Device-resident first-order descent: n_iter iterations of SGD (with momentum) or Adam in ONE call.  What
 * SolverBase.run_torch runs (src/solver/base.py:840-881: torch.optim.__dict__[method]([poses], lr = 0.05),
 * StepLR(n_iter, 0.1), a loop that keeps the lowest loss) -- without a host decision between two evaluations: the
 * iterate, the optimiser's state, the loss history and the optional trace live in device memory, every iteration is
 * enqueued eagerly on the caller's stream (evaluation from the device-resident x -> loss and gradient left in device
 * memory -> one update launch), and the call waits ONCE, behind the last iteration.  All values of the descriptor are
 * explicit (the Python layer fills torch's defaults).  cmax_descent_t is a new struct: the ABI version is unchanged.
 *
 * The rules are torch's.  Iteration `it` (0-based) evaluates L_it, g_it at x_it, then steps:
 *   SGD      buf = g at the first step, afterwards buf = momentum * buf + g;  x <- x - lr_it * buf  (momentum = 0: x <- x - lr_it * g)
 *   Adam     t = it + 1;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;
 *            x <- x - (lr_it / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *   StepLR   lr_it = lr * lr_decay^floor(it / lr_step)
 *   best     if L_it < best_loss (strict; a NaN never wins): best_loss = L_it, best_iter = it, x_best = x_it.  No iteration won:
 *            best_loss = +inf, best_iter = -1, x_best = x0.
 *   x_last   the iterate after the last step taken; its loss is not evaluated, as in the reference.  The reference's
 *            `best_poses = poses` aliases the live tensor, so what it returns as "param" is x_last, not the iterate of
 *            best_iter: both are returned here.
 *   stop     the device-side form of the reference's `break`: if L_it or any entry of g_it is not finite, no step is taken at `it`
 *            or afterwards; n_done = it (n_iter when no iteration stopped); loss_history[it] = L_it and the entries of later
 *            iterations are NaN.  The remaining evaluations still run, at the unchanged, finite x: the host cannot know -- the
 *            price of not waiting.
 *   outputs  loss_history[it] = L_it;  x_trace (optional) row it = x_it, row n_iter = x_last;
 *            last_lr = lr_it of the last step taken (0: none was).
 * ============================================================================================= */
#define CMAX_OPT_SGD 0
#define CMAX_OPT_ADAM 1
#define CMAX_DESCENT_MAX_ITER 4096
typedef struct {
    int32_t method;   /* CMAX_OPT_* */
    int32_t n_iter;   /* 1 .. CMAX_DESCENT_MAX_ITER */
    double lr;        /* > 0 */
    int32_t lr_step;  /* >= 1 (four bytes of padding behind it) */
    double lr_decay;  /* > 0 */
    double momentum;  /* SGD: [0, 1) */
    double beta1;     /* Adam: [0, 1) */
    double beta2;     /* Adam: [0, 1) */
    double eps;       /* Adam: > 0 */
} cmax_descent_t;
typedef struct {
    double best_loss;
    int32_t best_iter; /* -1: no iteration had a loss below +inf */
    int32_t n_done;    /* steps taken */
    double last_lr;
} cmax_descent_result_t;
int cmax_sizeof_descent(void);
/* The descent on a patch plan's objective (src/solver/base.py:840-881 on objective_scipy).  x0_host [nx = 2*ph*pw];
 * res_host, x_last_host [nx], x_best_host [nx], loss_history_host [n_iter]: filled; x_trace_host [(n_iter + 1) * nx] or NULL.
 * Refused before any launch: CMAX_EINVAL for an unknown method, n_iter outside 1 .. 4096, a non-finite or non-positive lr,
 * lr_decay or eps, lr_step < 1, momentum / beta1 / beta2 outside [0, 1), null pointers; CMAX_EUNSUPPORTED for a handle with a
 * communicator and for a weighted handle (as cmax_patch_plan_evaluate).  Deterministic handles are allowed.  The handle's
 * host-side evaluation state advances as n_iter cmax_patch_plan_evaluate calls would advance it; never replayed from a graph.
 * Blocks until the results are on the host.                                                                            */
int cmax_patch_plan_descend(cmax_patch_plan_t plan, const double *x0_host, int with_tv, const cmax_descent_t *descent,
                            cmax_descent_result_t *res_host, double *x_last_host, double *x_best_host,
                            double *loss_history_host, double *x_trace_host, cmax_stream_t stream);
/* The descent on a 2-DoF fused objective (src/solver/base.py:840-881 on a "2d-translation" warp): what cmax_objective runs per
 * iteration, theta in fp64 in device memory -- desc->motion_dtype must be CMAX_F64 and desc->model CMAX_MODEL_2DOF (CMAX_EINVAL
 * with the reason otherwise).  nx = 2.  The plain variance without a blur on the deferred path ends every iteration in ONE
 * one-wave launch that folds the raw sums AND applies the step (k_finish_raw_step); every other objective runs its normal
 * sequence and the update launch behind it.  Weighted and deterministic handles are allowed; a handle with a communicator is
 * CMAX_EUNSUPPORTED.  Same descriptor checks, outputs and blocking as cmax_patch_plan_descend.                          */
int cmax_objective_descend(cmax_handle_t h, const cmax_objective_t *desc_host, const double *theta0_host,
                           const cmax_descent_t *descent, cmax_descent_result_t *res_host, double *x_last_host,
                           double *x_best_host, double *loss_history_host, double *x_trace_host, cmax_stream_t stream);
/* Multi-start: K independent trajectories of cmax_objective_descend in ONE call (src/solver/base.py:840-881 from K starting points; the
 * 2-DoF objective is not convex and the grid of patch.initialize "global-best", src/solver/patch_contrast_base.py:164-187, is correct
 * only to its spacing).  theta0_host [K][2]; res_host [K], x_last_host [K][2], x_best_host [K][2], loss_history_host [K][n_iter]:
 * filled; x_trace_host [K][n_iter + 1][2] or NULL.  The rules above hold PER CANDIDATE: every candidate has its own control block,
 * optimiser state, history and trace, and a candidate that stops freezes alone -- the others go on.
 * Where cmax_objective_batch shares its launches (K > 1; plain variance without a blur, not normalised, on an unweighted,
 * non-deterministic handle without profiling), an iteration of all K candidates is three launches: the vote and the gather with one
 * grid layer per candidate, and a finishing launch of K waves, each of which folds its candidate's sums and applies its step
 * (k_finish_raw_step_batch).  Every other objective, weighted and deterministic handles, and K = 1 run candidate by candidate
 * inside the call exactly as cmax_objective_descend runs (same results, no speed-up).
 * Checked in this order, before any launch: the descent descriptor (CMAX_EINVAL as above, needs neither handle nor device); null
 * pointers and 1 <= K <= CMAX_DESCENT_MAX_STARTS (CMAX_EINVAL); desc->model / desc->motion_dtype as for cmax_objective_descend
 * (CMAX_EINVAL with the reason); a handle with a communicator (CMAX_EUNSUPPORTED).
 * State: one handle-owned device buffer of 8 * K * (32 + n_iter + (x_trace_host ? 2 * (n_iter + 1) : 0)) bytes, counted in
 * cmax_handle_info, kept while it is large enough (a later call with a smaller K or n_iter allocates nothing); on the shared-launch
 * path also the workspace of cmax_objective_batch for K candidates.  Iteration 0 reads none of the state: a call never sees what
 * an earlier call left, whatever K was.  The handle's evaluation state advances as n_iter cmax_objective_batch calls (or K * n_iter
 * cmax_objective calls) would advance it.  One wait: the states are copied to pinned memory behind the last launch and the stream
 * is synchronised once.  Never replayed from a graph.  Blocks until the results are on the host.                         */
#define CMAX_DESCENT_MAX_STARTS 64
int cmax_objective_descend_batch(cmax_handle_t h, const cmax_objective_t *desc_host, const double *theta0_host, int K,
                                 const cmax_descent_t *descent, cmax_descent_result_t *res_host, double *x_last_host,
                                 double *x_best_host, double *loss_history_host, double *x_trace_host, cmax_stream_t stream);

/* =============================================================================================
 * Device-resident L-BFGS with a backtracking (Armijo) line search: a quasi-Newton solve in ONE call.  The reference has no
 * counterpart (its second-order methods are SciPy's, driven from the host through TorchWrapper): the formulas below ARE the
 * contract.  A call consumes exactly n_eval evaluations e = 0 .. n_eval-1 of the objective, enqueued eagerly on the caller's
 * stream (evaluation from the device-resident x -> loss and gradient left in device memory -> one k_lbfgs_step launch, which
 * takes every decision and writes the next point), and waits ONCE, behind the last step.  All state is fp64 in device memory.
 * cmax_lbfgs_t / cmax_lbfgs_result_t are new structs: the ABI version is unchanged.
 *
 * Notation: (x_a, L_a, g_a) the accepted point, d the direction, alpha the trial step, x_t the trial point, gd = g_a^T d;
 * lo = x0 - max_move, hi = x0 + max_move (entrywise, rounded once); up to m = history pairs (s_i, y_i) in a ring, newest last.
 *   trial     x_t[p] = min(max(x_a[p] + alpha * d[p], lo[p]), hi[p])      (the clamp only absorbs the rounding of the clipped alpha)
 *   e = 0     evaluate at x0.  L or any entry of g not finite: status NONFINITE_START, terminate, x = x0 (final_loss = L as
 *             evaluated, gnorm_inf = NaN).  Otherwise (x_a, L_a, g_a) <- (x0, L, g) (code start; no pair, n_iter stays 0); if
 *             |g|inf <= gtol: status CONVERGED, terminate; otherwise CHOOSE.
 *   e > 0     (not terminated)  ok = finite(L) and all finite(g) and L <= L_a + c1 * alpha * gd  -- ONE boolean.
 *     not ok  n_ls += 1.  n_ls > max_ls and the history is empty: status LINESEARCH, terminate (code rejected).
 *             n_ls > max_ls and the history is not empty: clear the history, n_ls = 0, CHOOSE from g_a (code reset).
 *             Otherwise alpha <- shrink * alpha (code rejected) and the next trial is formed from the same x_a and d.
 *     ok      (code accepted)  s = x_t - x_a (as actually stepped), y = g - g_a.  If y^T y > 0 and s^T y > curv_eps * y^T y: push
 *             (s, y), dropping the oldest pair when m are held; otherwise the pair is skipped (Armijo alone does not guarantee
 *             curvature).  (x_a, L_a, g_a) <- (x_t, L, g), n_iter += 1, n_ls = 0, last_alpha = alpha.  If |g|inf <= gtol: status
 *             CONVERGED, terminate; otherwise CHOOSE.
 *   CHOOSE    empty history: d = -g_a, alpha = min(1, step0 / |g_a|_1).  Otherwise d = -H g_a by the L-BFGS two-loop recursion
 *             over the held pairs, oldest i = 0 .. newest i = k-1, rho_i = 1 / (s_i^T y_i):
 *                 q = g_a;   for i = k-1 .. 0:  a_i = rho_i s_i^T q,  q -= a_i y_i;
 *                 r = (s_{k-1}^T y_{k-1} / y_{k-1}^T y_{k-1}) q;   for i = 0 .. k-1:  b = rho_i y_i^T r,  r += (a_i - b) s_i;   d = -r
 *             and alpha = 1.  If not g_a^T d < 0: clear the history and take the empty-history direction.
 *             (The shipped kernel is the Gram form: it evaluates this recursion on the coefficients of d in the basis {s_i, y_i, g_a},
 *             with every inner product taken from the Gram matrix of that basis, which it keeps between steps.  Equal in exact
 *             arithmetic, not bit for bit: products read from the Gram matrix round differently from products of the vectors, by
 *             an amount that grows with the conditioning of the pairs.  The tests hold the trial points of both forms to
 *             1e-9 max(1, |x|inf) of the recursion above.)
 *   BOX       then alpha <- min(alpha, the largest value with lo <= x_a + alpha * d <= hi): over the entries with d[p] > 0 the
 *             minimum of (hi[p] - x_a[p]) / d[p], with d[p] < 0 of (lo[p] - x_a[p]) / d[p].  This alpha is the one the Armijo test
 *             and the trial use.  Not alpha > 0: status BOX, terminate.  The box is what lets a caller decide anything that depends
 *             on the size of x (time slabs) ONCE, from max|x0| + max_move.
 *   after     termination: the device-resident x is x_a and stays there; the remaining evaluations still run at that finite point
 *             (code idle, loss_history NaN, alpha 0) -- the host cannot know: the price of not waiting.  The budget exhausted while
 *             still running: status BUDGET; the result is x_a -- a trial that was never accepted is never returned.
 *   outputs   x [nx] = x_a;  loss_history[e] = L evaluated at e (NaN for idle evaluations);  alpha[e] = the alpha of the point evaluated
 *             at e (0 for e = 0 and idle);  code[e];  x_trace (optional) row e = the point evaluated at e, row n_eval = the final x_a;
 *             final_loss = L_a, gnorm_inf = |g_a|inf, n_iter = accepted steps, n_eval_used = evaluations up to and including the
 *             terminating one (n_eval: none terminated), last_alpha = alpha of the last accepted step (0: none).
 * The accepted losses are non-increasing by construction.  Every reduction runs through one fixed tree, without atomics: on a
 * deterministic handle a solve is bit-repeatable.
 * ============================================================================================= */
#define CMAX_LBFGS_MAX_HISTORY 16
#define CMAX_LBFGS_BUDGET 0          /* status: the budget ran out (also: still running) */
#define CMAX_LBFGS_CONVERGED 1
#define CMAX_LBFGS_LINESEARCH 2
#define CMAX_LBFGS_BOX 3
#define CMAX_LBFGS_NONFINITE_START 4
#define CMAX_LBFGS_CODE_START 0      /* code[e] */
#define CMAX_LBFGS_CODE_ACCEPTED 1
#define CMAX_LBFGS_CODE_REJECTED 2
#define CMAX_LBFGS_CODE_RESET 3
#define CMAX_LBFGS_CODE_IDLE 4
typedef struct {
    int32_t n_eval;   /* 1 .. CMAX_DESCENT_MAX_ITER: evaluations per call */
    int32_t history;  /* m: 1 .. CMAX_LBFGS_MAX_HISTORY */
    int32_t max_ls;   /* >= 1: rejected trials in a row before a reset / LINESEARCH (four bytes of padding behind it) */
    double c1;        /* Armijo constant, in (0, 0.5) */
    double shrink;    /* backtracking factor, in (0, 1) */
    double curv_eps;  /* >= 0 */
    double gtol;      /* >= 0 */
    double step0;     /* > 0: length (1-norm) of the first trial step along -g */
    double max_move;  /* > 0: the box |x - x0|inf <= max_move */
} cmax_lbfgs_t;
typedef struct {
    double final_loss;
    double gnorm_inf;
    double last_alpha;
    int32_t n_iter;
    int32_t n_eval_used;
    int32_t status;   /* CMAX_LBFGS_* (four bytes of padding behind it) */
} cmax_lbfgs_result_t;
int cmax_sizeof_lbfgs(void);
/* L-BFGS on a patch plan's objective (every plan cmax_patch_plan_descend takes: time-aware, scale_later, basis plans, plans with a
 * flow regulariser).  x0_host [nx]; res_host, x_host [nx], loss_history_host [n_eval], alpha_host [n_eval], code_host [n_eval]:
 * filled; x_trace_host [(n_eval + 1) * nx] or NULL.
 * Checked in this order, before any launch: the descriptor (CMAX_EINVAL naming the field: n_eval, history, max_ls, c1, shrink,
 * curv_eps, gtol, step0, max_move, all finite; needs neither plan nor device); null pointers (CMAX_EINVAL); a handle with a
 * communicator (CMAX_EUNSUPPORTED); a weighted handle (CMAX_EUNSUPPORTED, as cmax_patch_plan_descend).  Deterministic handles are
 * allowed.  State: one plan-owned device buffer of 8 * (1112 + (4 + 2 m) nx + 2 n_eval + ceil(n_eval / 2) + (x_trace_host ? (n_eval + 1) nx : 0))
 * bytes, kept while it is large enough; evaluation 0 reads none of it: a call never sees what an earlier call left.  The
 * handle's host-side evaluation state advances as n_eval cmax_patch_plan_evaluate calls would advance it; never replayed from a
 * graph.  Blocks until the results are on the host.                                                                      */
int cmax_patch_plan_lbfgs(cmax_patch_plan_t plan, const double *x0_host, int with_tv, const cmax_lbfgs_t *lbfgs,
                          cmax_lbfgs_result_t *res_host, double *x_host, double *loss_history_host, double *alpha_host,
                          int32_t *code_host, double *x_trace_host, cmax_stream_t stream);
/* L-BFGS on a 2-DoF fused objective: what cmax_objective runs per evaluation (the general sequence), theta in fp64 in device
 * memory -- desc->motion_dtype must be CMAX_F64 and desc->model CMAX_MODEL_2DOF (CMAX_EINVAL with the reason otherwise), then the
 * step launch.  nx = 2.  Weighted and deterministic handles are allowed; a handle with a communicator is CMAX_EUNSUPPORTED.  The
 * state is handle-owned (16 doubles of theta | gradient | result in front of it) and counted in cmax_handle_info.  Same
 * descriptor checks, outputs and blocking as cmax_patch_plan_lbfgs.                                                          */
int cmax_objective_lbfgs(cmax_handle_t h, const cmax_objective_t *desc_host, const double *theta0_host, const cmax_lbfgs_t *lbfgs,
                         cmax_lbfgs_result_t *res_host, double *x_host, double *loss_history_host, double *alpha_host,
                         int32_t *code_host, double *x_trace_host, cmax_stream_t stream);

/* =============================================================================================
 * Flow-basis plan: the optimiser's objective for a motion model that is LINEAR in its parameters, in one call.
 *   theta [K] (host fp64)  ->  dense flow D = sum_k theta_k B_k (cmax_basis_to_dense) * t_scale
 *     [-> voxel (cmax_voxel_construct)] -> fp32 -> loss = sum_i weight_i * cmax_objective(term_i)
 * and back: the gradient B^T dL/dD, the exact product H_theta = t^2 B^T H_flow B (time-aware plans add the voxel chain's
 * second-order adjoint), and the device-resident descent.  The reference has no counterpart (its models: 2-DoF translation,
 * per-pixel flow, patch grid); D is warped by its dense-flow rule x' = x - dt * D[src] (src/warp.py:263-313).  The map
 * theta -> D is linear exactly as the patch interpolation is, and the plan IS a patch plan with that map exchanged:
 * cmax_basis_plan_create returns a cmax_patch_plan_t with nx = K on which cmax_patch_plan_evaluate / _hvp / _descend /
 * _set_t_scale / _info / _destroy work unchanged (with_tv is ignored: there is no patch grid).
 * cmax_basis_objective_t is a new struct: the ABI version is unchanged.
 * ============================================================================================= */
typedef struct {
    int32_t n_terms;          /* 1..4 fused contrast terms */
    int32_t time_aware;       /* 0: terms use CMAX_MODEL_DENSE; 1: CMAX_MODEL_VOXEL on the propagated flow */
    int32_t T, scheme, t0;    /* as cmax_patch_objective_t */
    int32_t H, W;             /* sensor size of the handle */
    int32_t K;                /* 1 .. CMAX_BASIS_MAX_K basis fields */
    int32_t basis_dtype;      /* CMAX_F32 or CMAX_F64: what basis_dev points to, and what the plan keeps */
    int32_t scale_later;      /* must be 0: the rescaled propagation is not built for these plans (CMAX_EINVAL) */
    double t_scale;           /* pixel per time unit -> pixel per normalised batch period */
    double weight[4];
    cmax_objective_t term[4]; /* motion_dtype == CMAX_F64 on all of them or on none (an exact plan, as for the patch plan) */
} cmax_basis_objective_t;
int cmax_sizeof_basis_objective(void);
/* basis_dev: device [K][2][H][W] in desc->basis_dtype; the plan keeps ITS OWN COPY in that dtype (copied on `stream`).  The call
 * reduces max |B_k| per field on the device and reads the K numbers back: it synchronises `stream`.  A product's tangent v is
 * handed to cmax_objective_hvp as B v / sum_k |v_k| max|B_k| (max-norm <= 1; unlike the patch interpolation a basis can amplify)
 * and the product is scaled back; time-aware plans keep their device-side maximum behind the voxel chain.
 * Refused: K outside 1 .. CMAX_BASIS_MAX_K, an unknown basis_dtype, scale_later != 0 and everything cmax_patch_plan_create
 * checks about the terms (CMAX_EINVAL); a handle that holds a communicator and a handle that holds per-event weights
 * (CMAX_EUNSUPPORTED).  A plan on a deterministic handle is bit-repeatable: the basis kernels use no atomics.            */
int cmax_basis_plan_create(cmax_handle_t h, const cmax_basis_objective_t *desc_host, const void *basis_dev, cmax_stream_t stream,
                           cmax_patch_plan_t *out);

/* =============================================================================================
 * Depth and ego-motion: the motion field of a static scene over a grid of inverse depth.
 *   x = [a_0 .. a_{Ka-1} | b_0 .. b_{Kb-1} | s]   s: a scalar patch grid [ph][pw], row-major;  nx = Ka + Kb + ph pw
 *   rho = Q s          Q: the bilinear interpolation of cmax_patch_to_dense (replicate pad, align_corners = False, centre crop) on ONE
 *                      plane and WITHOUT the negation the patch map carries
 *   U = sum_k a_k A_k,  R = sum_j b_j B_j,   D[c][e] = rho[e] U[c][e] + R[c][e]
 * A [Ka][2][H][W]: the translational field per unit inverse depth; B [Kb][2][H][W]: what does not depend on depth (the rotational
 * field of a calibrated camera).  1 <= Ka, 0 <= Kb, Ka + Kb <= CMAX_BASIS_MAX_K.  D is a PRODUCT of unknowns: neither the patch
 * plan nor the basis plan expresses it.  Gallego, Rebecq, Scaramuzza (CVPR 2018) name depth among the applications of contrast
 * maximisation; Shiba, Klose, Aoki, Gallego (TPAMI 2024) put inverse depth on a patch grid.  The reference has no counterpart; D is
 * warped by its dense-flow rule x' = x - dt * D[src] (src/warp.py:263-313).
 * GAUGE: (a, s) -> (lambda a, s / lambda) leaves D unchanged, so the Hessian is singular along that line.  That is a property of the
 * model; nothing here works around it.
 * Leaf operators (a, b, s, da, db, ds: device fp64; A, B, g, dg, out of the forward and the tangent: `dtype`; every adjoint output:
 * device fp64).  fp64 arithmetic, one rounding at the store, no atomics (fixed trees: two runs agree bit for bit).  b, B, db, g_b
 * may be NULL when Kb = 0.  The adjoints cut the image into chunks of CMAX_DEPTH_ADJ_CHUNK consecutive pixels and use a
 * stream-ordered temporary (hipMallocAsync) of ceil(H W / CMAX_DEPTH_ADJ_CHUNK) (Ka + Kb) + Ka + Kb + H W doubles.
 *   cmax_depth_to_dense        out = D
 *   cmax_depth_to_dense_tan    out = dD = (Q ds) U + rho (A da) + B db
 *   cmax_depth_to_dense_adj    g_a[k] = sum rho A_k . g,  g_b[j] = sum B_j . g,  g_s = Q^T q with q[e] = sum_c U[c][e] g[c][e]
 *   cmax_depth_to_dense_adj2   J(x)^T dg + (dJ[u])^T g for u = (da, db, ds):  out_a[k] = sum rho A_k . dg + sum (Q ds) A_k . g,
 *                              out_b[j] = sum B_j . dg,  out_s = Q^T [U . dg + (A da) . g]     (db does not enter)
 * Only the bilinear filter is built.                                                                                          */
#define CMAX_DEPTH_ADJ_CHUNK 1024
int cmax_depth_to_dense(const void *a, const void *b, const void *s, const void *A, const void *B, int dtype, int Ka, int Kb, int ph,
                        int pw, int pad_h, int pad_w, int sw_h, int sw_w, int H, int W, void *out, cmax_stream_t stream);
int cmax_depth_to_dense_tan(const void *a, const void *s, const void *da, const void *db, const void *ds, const void *A, const void *B,
                            int dtype, int Ka, int Kb, int ph, int pw, int pad_h, int pad_w, int sw_h, int sw_w, int H, int W,
                            void *out, cmax_stream_t stream);
int cmax_depth_to_dense_adj(const void *a, const void *s, const void *g, const void *A, const void *B, int dtype, int Ka, int Kb,
                            int ph, int pw, int pad_h, int pad_w, int sw_h, int sw_w, int H, int W, double *g_a, double *g_b,
                            double *g_s, cmax_stream_t stream);
int cmax_depth_to_dense_adj2(const void *a, const void *s, const void *da, const void *ds, const void *g, const void *dg,
                             const void *A, const void *B, int dtype, int Ka, int Kb, int ph, int pw, int pad_h, int pad_w, int sw_h,
                             int sw_w, int H, int W, double *out_a, double *out_b, double *out_s, cmax_stream_t stream);

/* Depth plan: the optimiser's objective for that model in one call.
 *   x (host fp64) -> D * t_scale [-> voxel (cmax_voxel_construct)] -> fp32 -> loss = sum_i weight_i * cmax_objective(term_i)
 * and back: the gradient t J^T dL/dF, the exact product (the map is not linear: t [J^T (H_FF t dD) + (dJ[v])^T g_F], with the tangent of
 * the flow scaled to unit max-norm by a maximum taken ON THE DEVICE -- a host bound does not hold for a product of unknowns), the
 * device-resident descent and L-BFGS.  cmax_depth_plan_create returns a cmax_patch_plan_t with nx = Ka + Kb + ph pw on which
 * cmax_patch_plan_evaluate / _hvp / _descend / _lbfgs / _set_t_scale / _set_flow_regularizer / _info / _destroy work unchanged
 * (with_tv is ignored).  cmax_depth_objective_t is a new struct: the ABI version is unchanged.                                   */
typedef struct {
    int32_t n_terms;          /* 1..4 fused contrast terms */
    int32_t time_aware;       /* 0: terms use CMAX_MODEL_DENSE; 1: CMAX_MODEL_VOXEL on the propagated flow */
    int32_t T, scheme, t0;    /* as cmax_patch_objective_t */
    int32_t H, W;             /* sensor size of the handle */
    int32_t Ka, Kb;           /* fields of A (>= 1) and of B (>= 0); Ka + Kb <= CMAX_BASIS_MAX_K */
    int32_t ph, pw;           /* the grid of inverse depth */
    int32_t pad_h, pad_w;     /* as cmax_patch_objective_t */
    int32_t sw_h, sw_w;
    int32_t basis_dtype;      /* CMAX_F32 or CMAX_F64: what A_dev and B_dev point to, and what the plan keeps */
    int32_t scale_later;      /* must be 0 (CMAX_EINVAL) */
    int32_t filter_type;      /* must be CMAX_FILTER_BILINEAR: the nearest filter is not built for this map (CMAX_EINVAL) */
    double t_scale;           /* pixel per time unit -> pixel per normalised batch period */
    double weight[4];
    double tv_weight;         /* must be 0: total variation of the depth grid is not built (CMAX_EINVAL) */
    cmax_objective_t term[4]; /* motion_dtype == CMAX_F64 on all of them or on none (an exact plan, as for the patch plan) */
} cmax_depth_objective_t;
int cmax_sizeof_depth_objective(void);
/* A_dev [Ka][2][H][W], B_dev [Kb][2][H][W] (NULL when Kb = 0) in desc->basis_dtype; the plan keeps ITS OWN COPY (copied on `stream`,
 * which the call synchronises).  Refused: Ka < 1, Kb < 0, Ka + Kb > CMAX_BASIS_MAX_K, an unknown basis_dtype, scale_later != 0,
 * filter_type != CMAX_FILTER_BILINEAR, tv_weight != 0 and everything cmax_patch_plan_create checks about sizes and terms
 * (CMAX_EINVAL); a handle that holds a communicator and a handle that holds per-event weights (CMAX_EUNSUPPORTED).  A plan on a
 * deterministic handle is bit-repeatable: the depth kernels use no atomics.                                                     */
int cmax_depth_plan_create(cmax_handle_t h, const cmax_depth_objective_t *desc_host, const void *A_dev, const void *B_dev,
                           cmax_stream_t stream, cmax_patch_plan_t *out);

/* The reduction of the scale_later map as a leaf operator (the autograd-chained path chains it with cmax_patch_to_dense and
 * cmax_voxel_construct).  x: device fp32 / fp64 [n].  out: device double[4] -- out[0] = max x (signed), out[1] = number of
 * elements EQUAL to it (exact comparison of the values the device holds), out[2..3] scratch.  Asynchronous.                 */
int cmax_field_max(const void *x, int dtype, int64_t n, double *out, cmax_stream_t stream);
/* Its adjoint, as torch.Tensor.max() back-propagates: gx[i] = gout[0] / out[1] where x[i] == out[0], 0 elsewhere.  `out` as
 * cmax_field_max left it; gout: device double[1]; gx: like x.                                                                */
int cmax_field_max_adj(const void *x, int dtype, int64_t n, const double *out, const double *gout, void *gx, cmax_stream_t stream);

/* =============================================================================================
 * Event-collapse regularisers on the dense flow.  A contrast objective on a motion model that contains a zoom (similarity, affine,
 * a free basis, a patch grid) has a global optimum that is not the motion: shrinking every event onto a line or a point maximises
 * every focus measure (Shiba, Aoki, Gallego, "Event Collapse in Contrast Maximization Frameworks", Sensors 2022).  Their remedy is a
 * penalty on the deformation of the warp; this is its form on the flow FIELD (the per-event, IWE-weighted form is not built).  The
 * reference has no counterpart: these formulas are the contract.
 *   F [2,H,W]: displacement field in pixel over the batch, F[0] along rows, F[1] along columns.  The warp is x' = x - dt F[src]; its
 *   Jacobian for a time offset s is I - s grad F.
 *   Omega: 1 <= r <= H-2, 1 <= c <= W-2;  n = (H-2)(W-2);  H, W >= 3 (CMAX_EINVAL otherwise).
 *   On Omega, central differences:  a = (F0(r+1,c) - F0(r-1,c))/2   b = (F0(r,c+1) - F0(r,c-1))/2
 *                                   c = (F1(r+1,c) - F1(r-1,c))/2   d = (F1(r,c+1) - F1(r,c-1))/2
 *   psi_eps(u) = sqrt(u^2 + eps^2) - eps, eps >= 0.  eps = 0: |u| with psi'(0) = 0 and psi'' = 0; otherwise
 *   psi' = u / sqrt(u^2 + eps^2), psi'' = eps^2 / (u^2 + eps^2)^(3/2).
 *   CMAX_FLOWREG_DIVERGENCE  R = (1/n)  sum_Omega psi(a + d)
 *   CMAX_FLOWREG_AREA        R = (1/2n) sum_Omega [psi(A(+s) - 1) + psi(A(-s) - 1)],
 *                            A(sigma) = det(I - sigma grad F) = 1 - sigma (a + d) + sigma^2 (a d - b c);  s > 0 is the caller's (1: the
 *                            area ratio of a pixel cell warped across the whole batch, in both directions)
 *   Gradient w.r.t. F: the transposed central difference of dR/d(a,b,c,d), which are zero outside Omega -- non-zero on the whole image.
 *   Product (grad^2 R)[dF]: psi'' acts on the directional derivative of u, psi' on the constant Hessian of A (d2A/da dd = sigma^2,
 *   d2A/db dc = -sigma^2): the area product is non-zero even at eps = 0, the divergence product at eps = 0 is exactly zero.
 * All arithmetic is fp64 whatever the field's dtype is; the value is a fixed-order sum without atomics (the same field gives the same
 * bits).  cmax_flow_regularizer_t is a new struct: the ABI version is unchanged.
 * ============================================================================================= */
#define CMAX_FLOWREG_NONE 0
#define CMAX_FLOWREG_DIVERGENCE 1
#define CMAX_FLOWREG_AREA 2
typedef struct {
    int32_t kind;      /* CMAX_FLOWREG_* */
    int32_t reserved;  /* 0 */
    double weight;     /* the plan's weight of the term (sign of the cost direction included); ignored by the leaf operators */
    double eps;        /* >= 0 */
    double s;          /* > 0 (area; checked for both kinds) */
} cmax_flow_regularizer_t;
int cmax_sizeof_flow_regularizer(void);
/* Leaf operators.  F, dF: device fp32 / fp64 [2,H,W] (`dtype`); value_dev: device double[1]; grad / hv: device [2,H,W] in `dtype`
 * (grad may be NULL: value only).  CMAX_EINVAL for H or W < 3, eps < 0, s <= 0, a non-finite parameter or an unknown kind.
 * Asynchronous on `stream`.                                                                                                    */
int cmax_flow_regularizer(const void *F, int dtype, int H, int W, const cmax_flow_regularizer_t *desc_host, double *value_dev,
                          void *grad_or_null, cmax_stream_t stream);
int cmax_flow_regularizer_tan(const void *F, const void *dF, int dtype, int H, int W, const cmax_flow_regularizer_t *desc_host, void *hv,
                              cmax_stream_t stream);
/* One more term of a patch plan or a basis plan: loss += weight * R(F) with F = t_scale * (map x), the field the fused terms warp by
 * (the t0 field of a time-aware plan), evaluated in fp64 on the plan's fp64 field before it is rounded for the event kernels.
 * cmax_patch_plan_evaluate, _hvp (the exact second-order term) and _descend carry it.  desc_host NULL or kind CMAX_FLOWREG_NONE removes
 * the term: such a plan enqueues exactly the launches of a plan on which this was never called.  Captured launch sequences are dropped.
 * Refused: bad parameters as above, a non-finite weight, a sensor smaller than 3 x 3, a scale_later plan -- its map is rescaled by a
 * maximum -- (CMAX_EINVAL); a handle that holds a communicator, where the term would be counted once per rank (CMAX_EUNSUPPORTED;
 * evaluate, hvp and descend refuse likewise if the communicator arrives later).                                                  */
int cmax_patch_plan_set_flow_regularizer(cmax_patch_plan_t plan, const cmax_flow_regularizer_t *desc_host_or_null);

/* =============================================================================================
 * Per-patch translation search: the re-initialisation the pyramid solver runs at every scale above
 * the coarsest.  Replaces the trial loop of initialize_guess_from_optuna_sampling / objective_initial /
 * calculate_cost_for_small_patch (src/solver/patch_contrast_pyramid.py:320-414): per patch, the events
 * with x_min <= x < x_max, y_min <= y < y_max (utils.crop_event) are shifted to the patch origin, warped
 * by a candidate translation to the MIDDLE of the patch's own time span, voted (bilinear) into an
 * img_h x img_w image, blurred with scipy.ndimage.gaussian_filter(sigma) and scored with the numpy
 * branch of GradientMagnitude: mean of (Sobel/8)^2 over the whole image, reflect-101 border
 * (src/costs/gradient_magnitude.py:78-95).  One workgroup per (patch, candidate); every pair of a scale
 * in one launch.
 *   boxes     device int32 [n_patch][4] = x_min, x_max, y_min, y_max (rows first), sensor coordinates
 *   cand      device fp32  [n_patch][n_cand][2] translations, pixel per unit of the RAW timestamps
 *   gm_out    device fp32  [n_patch][n_cand + 1]: gradient magnitude per candidate; the last column is
 *             the un-warped patch, so the reference's NormalizedGradientMagnitude loss of candidate c is
 *             gm_out[p][n_cand] / gm_out[p][c]   (normalized_gradient_magnitude.py:81-94)
 *   count_out device int32 [n_patch] events inside the box (the reference keeps the incoming motion
 *             when a patch holds <= 10 events, patch_contrast_pyramid.py:336)
 * Needs events set on the handle; 2 * img_h * img_w floats must fit 64 KB of LDS.  Asynchronous.  */
int cmax_patch_search(cmax_handle_t h, int n_patch, const int *boxes, int img_h, int img_w, int n_cand,
                      const float *cand, double sigma, float *gm_out, int *count_out, cmax_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CMAX_HIP_H */

/* halo_hip.h -- C ABI of libhalo_hip.so: HALO's per-pixel hyperbolic acquisition-scoring
 * path as hand-written HIP kernels for gfx950 (MI355X / CDNA4).
 *
 * The reference (paolomandica/HALO) is pure Python on stock PyTorch + geoopt; it has no FFI.
 * Each entry point below replaces the reference call named in its comment (paths relative to
 * the reference repository).  The Python classes in halo_amd/core/ bind these through ctypes
 * (halo_amd/_lib.py); INTEGRATION.md shows the binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (tensor.data_ptr()); tensors are dense row-major,
 *     exactly the reference's layouts: logit (B,O,H,W) f32, decoder_out (B,C,H,W) f64|f32,
 *     maps (B,H,W); batch strides are passed in ELEMENTS so a caller may hand in views
 *   - stream is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     one call = asynchronous enqueue on that stream, no allocation, no host sync, no global
 *     state => re-entrant and hipGraph-capturable
 *   - scratch comes from the caller: size it with the matching *_workspace_bytes()
 *   - return 0 on success, <0 on error (HALO_E_*); halo_last_error() gives the message of the
 *     calling thread's last failure
 *   - dtype codes: HALO_F32 = 0, HALO_F64 = 1; integer maps (labels, predictions): HALO_I64 = 2, HALO_I32 = 3, HALO_U8 = 4;
 *     half operands of the autocast passes: HALO_F16 = 5, HALO_BF16 = 6
 */
#ifndef HALO_HIP_H
#define HALO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HALO_ABI_VERSION 13

enum { HALO_F32 = 0, HALO_F64 = 1, HALO_I64 = 2, HALO_I32 = 3, HALO_U8 = 4, HALO_F16 = 5, HALO_BF16 = 6 };

enum { HALO_OK = 0, HALO_E_ARG = -1, HALO_E_UNSUPPORTED = -2, HALO_E_WORKSPACE = -3, HALO_E_LAUNCH = -4 };

/* unc_type of FloatingRegionScore.forward (core/active/floating_region.py:158-163, 70-92).
 * Every other string the reference accepts ('none', 'hyperbolic', 'certainty', ...) yields a
 * zero map (floating_region.py:84-90) => HALO_UNC_ZEROS. */
enum { HALO_UNC_ENTROPY = 0, HALO_UNC_PIXEL_ENTROPY = 1, HALO_UNC_ORACLE_ACC = 2, HALO_UNC_ZEROS = 3 };

/* pur_type of FloatingRegionScore.forward (floating_region.py:165-202); anything else is the
 * reference's NotImplementedError and must be rejected by the caller. */
/* padding_mode of FloatingRegionScore's two box windows (floating_region.py:49,63: forwarded to nn.Conv2d): what a window tap
 * outside the image reads.  ZEROS (every caller in the reference's tree): nothing, and the purity window counts its in-image
 * taps only; REFLECT / REPLICATE / CIRCULAR: the image pixel torch's F.pad(mode) puts there, so every tap counts. */
enum { HALO_PAD_ZEROS = 0, HALO_PAD_REFLECT = 1, HALO_PAD_REPLICATE = 2, HALO_PAD_CIRCULAR = 3 };
/* halo_score_args.flags: bit 0 = normalise both maps (the reference's `normalize`), bits 8-9 = HALO_PAD_* << 8.  0 / 1 mean
 * zero padding. */
enum { HALO_FLAG_NORMALIZE = 1 };
#define HALO_FLAG_PAD(mode) ((mode) << 8)

enum { HALO_PUR_RIPU = 0, HALO_PUR_ORACLE_RIPU = 1, HALO_PUR_HYPER = 2, HALO_PUR_NONE = 3,
       HALO_PUR_RADIUS = 4, HALO_PUR_EUC_NORM = 5 };

int halo_version(void);
const char *halo_last_error(void);

/* ---- hyperbolic ops: core/utils/hyperbolic.py (arithmetic = geoopt.manifolds.stereographic.math) ---- */

/* HyperMapper.expmap(x, dim) (hyperbolic.py:28-39): project(expmap0(x.double())).
 * x viewed as (outer, C, inner), reduced over C; x_dtype F32|F64; y is f64. */
int halo_expmap0_project(const void *x, int x_dtype, double *y, int64_t outer, int64_t C, int64_t inner,
                         double c, void *stream);

/* HyperMapper.logmap(x) (hyperbolic.py:51-60): project(logmap0(x.double())), f64 in/out. */
int halo_logmap0_project(const double *x, double *y, int64_t outer, int64_t C, int64_t inner, double c,
                         void *stream);

/* HyperMapper.poincare_distance_origin(x, dim) (hyperbolic.py:74-83): geoopt dist0; out dtype = dtype. */
int halo_dist0(const void *x, int dtype, void *out, int64_t outer, int64_t C, int64_t inner, double c,
               void *stream);

/* HyperMapper.poincare_distance(x, y) (hyperbolic.py:62-72): geoopt dist over the last dim, f64. */
int halo_pdist(const double *x, const double *y, double *out, int64_t n, int64_t d, double c, void *stream);

/* HyperMLR.forward / _hyper_logits (hyperbolic.py:120-188): x (B,C,hw) f64, P_MLR/A_MLR (O,C) f64,
 * out (B,O,hw) in out_dtype (F32 fuses the head's .float(), core/models/classifier.py:373,554).
 * workspace: halo_hypermlr_workspace_bytes(O, C). */
size_t halo_hypermlr_workspace_bytes(int64_t O, int64_t C);
int halo_hypermlr_logits(const double *x, const double *P, const double *A, void *out, int out_dtype,
                         int64_t B, int64_t C, int64_t O, int64_t hw, double c, void *workspace,
                         size_t workspace_bytes, void *stream);

/* The inference tail of both hyperbolic heads in one call (classifier.py:364-379: ASPP_Classifier_V2_Hyper.forward, :552-558:
 * DepthwiseSeparableASPP_Hyper.forward):  embed = mapper.expmap(feat, dim=1)  (B,C,hw) f64;  out = conv_seg(embed)[.float()]
 * (B,O,hw) in out_dtype.  feat (B,C,hw) f32.  Returns 1 and enqueues NOTHING when the shape is not served by the fused kernel
 * (C != 64, O > 32, odd hw, unaligned bases): the caller then makes the two calls above, whose results this call reproduces bit
 * for bit.  workspace: halo_hypermlr_workspace_bytes(O, C). */
int halo_head_tail(const float *feat, const double *P, const double *A, double *embed, void *out, int out_dtype, int64_t B,
                   int64_t C, int64_t O, int64_t hw, double c, void *workspace, size_t workspace_bytes, void *stream);

/* Backward of the head tail for training (classifier.py:553-554 under autograd).
 *  - halo_expmap0_project_bwd: gx = J^T gy for y = HyperMapper.expmap(x, dim); gy f64, gx in x's dtype.
 *  - halo_hypermlr_bwd_terms: reverse sweep through _hyper_logits' scalar algebra (hyperbolic.py:146-183):
 *    from gout = dL/dlogit (B,O,hw) f64 it writes dL/dpx, dL/dxa, and the per-element contributions to
 *    dL/dpp, dL/dpa, dL/d||A|| (B,O,hw each) plus dL/dxx summed over classes (B,hw).  The two remaining
 *    contractions (d x = W^T D + 2 x dxx, d W = D x^T) are plain GEMMs done by the caller's BLAS.
 *    workspace: halo_hypermlr_workspace_bytes(O, C). */
int halo_expmap0_project_bwd(const void *x, int x_dtype, const double *gy, void *gx, int64_t outer, int64_t C,
                             int64_t inner, double c, void *stream);
int halo_hypermlr_bwd_terms(const double *x, const double *P, const double *A, const double *gout, int64_t B, int64_t C,
                            int64_t O, int64_t hw, double c, double *dpx, double *dxa, double *dxx, double *dpp,
                            double *dpa, double *dan, void *workspace, size_t workspace_bytes, void *stream);

/* The whole backward of HyperMLR._hyper_logits in one call (ABI 7): from gout = dL/dlogit (B,O,hw), HALO_F64 or HALO_F32 (the head's
 * `.float()` under autograd hands a float32 gradient back: classifier.py:554), it writes
 * gx = dL/dx (B,C,hw), gP = dL/dP_MLR and gA = dL/dA_MLR (O,C), all f64 -- the reverse sweep above, d x = W^T D + 2 x dxx,
 * d W = D x^T and the parameter algebra (||P||^2, <-P,A^>, F.normalize, ||A||; hyperbolic.py:137-174) on the device, every sum
 * in a fixed order (run-to-run identical).  Serves O <= 20 classes and C a multiple of 64 up to 256 (the heads' 19 x 64):
 * halo_hypermlr_backward_workspace_bytes returns 0 for any other shape, and the caller then composes the backward from
 * halo_hypermlr_bwd_terms and its own GEMMs (halo_amd/core/utils/hyperbolic.py does). */
size_t halo_hypermlr_backward_workspace_bytes(int64_t B, int64_t C, int64_t O, int64_t hw);
int halo_hypermlr_backward(const double *x, const double *P, const double *A, const void *gout, int gout_dtype, int64_t B, int64_t C,
                           int64_t O, int64_t hw, double c, double *gx, double *gP, double *gA, void *workspace,
                           size_t workspace_bytes, void *stream);

/* F.interpolate(mode="bilinear", align_corners=True) (core/active/build.py:123-125,133-135;
 * classifier.py:375-377,556-557): planes x (h,w) -> planes x (H,W), dtype F32|F64.  ATen's order (columns first, rows second,
 * every p*q + r*s as fma(p, q, r*s)): the bits torch's CPU kernel returns at the path's shapes. */
int halo_bilinear_upsample(const void *src, void *dst, int dtype, int64_t planes, int64_t h, int64_t w,
                           int64_t H, int64_t W, void *stream);

/* The adjoint of that resize (its backward under autograd): grad_out planes x (H,W) -> WRITES grad_in planes x (h,w), both dense,
 * dtype F32|F64, H >= h and W >= w (anything else: HALO_E_ARG, nothing launched).
 *   grad_in[p,i,j] = sum_Y sum_X wy(Y,i) wx(X,j) grad_out[p,Y,X],  wy(Y,i) = [i0(Y) == i] l0(Y) + [i1(Y) == i] l1(Y)
 * with the forward's taps and weights in the operand dtype.  A gather: no atomics, every grad_in element summed by one thread in
 * a fixed order (ascending X inside a row, rows in ascending Y), so repeated calls give identical bits.  No workspace. */
int halo_bilinear_upsample_bwd(const void *grad_out, void *grad_in, int dtype, int64_t planes, int64_t h, int64_t w,
                               int64_t H, int64_t W, void *stream);

/* ---- scoring: FloatingRegionScore.forward (core/active/floating_region.py:129-217) ----
 *
 * ONE call, halo_score(&args, stream), described by a halo_score_args.  The descriptor is plain data that is read only
 * during the call (build it on the stack; nothing keeps a pointer to it, so a captured graph does not depend on it either).
 * (ABI 11 collapsed six positional entry points and two of their three workspace queries into this one; no kernel changed.)
 *
 * route: where the two sources live.
 *   HALO_SCORE_FULL     logit (B,O,H,W) f32 and feat = decoder_out (B,C,H,W) at the maps' resolution; hl, wl, hf, wf are ignored.
 *   HALO_SCORE_LR       LOW-RESOLUTION sources, fusing RegionSelection's two F.interpolate calls (core/active/build.py:122-135)
 *                       into the scorer: logit (B,O,hl,wl) f32 and feat (B,C,hf,wf) f64|f32 are interpolated on the fly (bilinear,
 *                       align_corners=True) to (H,W); the C x H x W tensor is never materialised.  Results are bit-identical to
 *                       halo_bilinear_upsample + HALO_SCORE_FULL.  Returns HALO_E_UNSUPPORTED when a source window does not
 *                       fit LDS (strong downsampling): the caller then upsamples explicitly.
 *   HALO_SCORE_LR_GRAM  HALO_SCORE_LR with the embedding's radius / norm evaluated through the Gram form SURVEY 8f N1 describes:
 *                       ||sum_i w_i v_i||^2 = sum_{i<=j} (2 - [i==j]) w_i w_j <v_i, v_j> over the four corner vectors of an output
 *                       pixel's low-res cell -- the inner products are computed once (one pass over feat; 5 maps over the low-res
 *                       grid hold them), each output pixel then costs 10 terms instead of C.  Same mathematics, different rounding
 *                       (|difference| of the sum of squares: a few 1e-16 of the largest corner norm^2), so this route is NOT
 *                       bit-identical to upsample + HALO_SCORE_FULL; float64 feat only (HALO_E_UNSUPPORTED otherwise).  Everything
 *                       else (logits, normalisation, -inf masking) as HALO_SCORE_LR; a purity type that does not read feat makes
 *                       the two routes the same.  hf * wf above 2^31 - 1 is HALO_E_UNSUPPORTED and a workspace below
 *                       halo_score_args_workspace_bytes is HALO_E_WORKSPACE on EVERY call of this route (before ABI 11 the
 *                       timed variant of the call skipped the first check: the one intended tightening of the collapse).
 *   On the two low-res routes hl, wl <= 0, or hf, wf <= 0 with a purity type that reads feat, are HALO_E_ARG.
 *
 * sources
 *   logit, logit_bstride   f32, image b at logit + b * logit_bstride (ELEMENTS; planes dense)
 *   hl, wl                 size of the low-res logit planes (low-res routes)
 *   feat, feat_dtype, feat_bstride   HALO_F64 | HALO_F32, needed for pur HYPER / RADIUS / EUC_NORM (may be NULL otherwise)
 *   hf, wf                 size of the low-res embedding planes (low-res routes)
 *   gt                     (B,H,W) i64, needed for UNC_ORACLE_ACC / PUR_ORACLE_RIPU
 *   active                 (B,H,W) u8, optional: where non-zero the score is written as -inf, fusing `score[active] = -inf`
 *                          (core/active/build.py:146); NULL for the plain forward
 * geometry + parameters
 *   B, O, C, H, W          images, classes, embedding channels, size of the maps
 *   unc_type, pur_type     HALO_UNC_* / HALO_PUR_*; a pur_type outside the enum is the reference's NotImplementedError
 *                          (HALO_E_UNSUPPORTED, "... not implemented")
 *   flags                  bit 0 = HALO_FLAG_NORMALIZE: normalise both maps (the reference's `normalize`); bits 8-9 =
 *                          HALO_FLAG_PAD(HALO_PAD_*): padding mode of the two box windows.  0 / 1 mean zero padding; any other
 *                          bit is HALO_E_ARG
 *   ksize, pksize          entropy_conv size (constructor `size`) and purity_conv size (3 if the module was built with
 *                          purity_type=='hyper', floating_region.py:54-55); both odd
 *   K, c                   histogram bins for HYPER; curvature
 * outputs, (B,H,W)
 *   score, impurity        f64 when pur is RADIUS | EUC_NORM and feat is f64, otherwise f32 (the reference's type promotion,
 *                          floating_region.py:210)
 *   uncertainty            f32.  impurity / uncertainty may be NULL when only the score is wanted
 * scratch
 *   workspace, workspace_bytes   at least halo_score_args_workspace_bytes(&args): right for every route (FULL: what
 *                          halo_score_workspace_bytes(B, H, W) returns; the low-res routes add an upsampled logit tensor for class
 *                          counts other than 19 / 16, the Gram route its 5 maps); 0 for a NULL descriptor, another struct_bytes, an
 *                          empty shape or an unknown route
 * optional, NULL = none, honoured on every route
 *   tail_stream            a second stream of the caller: the passes over logit and feat run on `stream`, ev_feat_stop (then
 *                          required) is recorded behind them, tail_stream waits for it and receives every launch after that (min /
 *                          max, normalize_map, the product, score[active] = -inf: floating_region.py:204-217 + build.py:146).  The
 *                          small tail kernels of one call then overlap the feature pass of the NEXT call on `stream` instead of
 *                          standing between two of them.  The outputs are complete on tail_stream; `workspace` belongs to the call
 *                          until then (one workspace per call in flight).  Needs a purity type that reads decoder_out.
 *                          tail_stream == stream: the same as NULL
 *   score_range            a buffer of halo_score_range_bytes(B) bytes for these B maps: receives the value range of each score map
 *                          -- and, for normalised maps, the selector's coarse histogram of it -- in the form halo_greedy_select
 *                          accepts, so that the selector need not read the map once or twice more to find them.  Free when the
 *                          maps are normalised (a product of two values in [0, 1]); otherwise the range is reduced exactly and no
 *                          histogram is handed over
 *   ev_*                   hipEvent_t (as void*, from halo_event_create) recorded on `stream`: ev_logit_start / ev_logit_stop around
 *                          the logit pass, ev_feat_start / ev_feat_stop immediately before and after the embedding pass (k_feat_reduce,
 *                          the HBM-roofline kernel; only recorded when the purity type reads feat), ev_feat_mid between the Gram pass
 *                          and the radius pass of the Gram route, ev_tail_stop behind the tail kernels (on tail_stream when there is
 *                          one) -- bench.py times the kernels live inside the pipelined run with them
 */
enum { HALO_SCORE_FULL = 0, HALO_SCORE_LR = 1, HALO_SCORE_LR_GRAM = 2 };
typedef struct halo_score_args {
    size_t struct_bytes;            /* sizeof(halo_score_args) as the caller compiled it; anything else: HALO_E_ARG */
    int route;                      /* HALO_SCORE_* */
    const float *logit;
    int64_t logit_bstride;
    int64_t hl, wl;
    const void *feat;
    int feat_dtype;
    int64_t feat_bstride;
    int64_t hf, wf;
    const int64_t *gt;
    const uint8_t *active;
    int64_t B, O, C, H, W;
    int unc_type, pur_type, flags, ksize, pksize;
    int64_t K;
    double c;
    void *score;
    void *impurity;
    float *uncertainty;
    void *workspace;
    size_t workspace_bytes;
    void *tail_stream;
    void *score_range;
    void *ev_logit_start, *ev_logit_stop, *ev_feat_start, *ev_feat_mid, *ev_feat_stop, *ev_tail_stop;
} halo_score_args;
size_t halo_score_workspace_bytes(int64_t B, int64_t H, int64_t W);     /* route FULL; also halo_quantize_radius's scratch */
size_t halo_score_args_workspace_bytes(const halo_score_args *a);
int halo_score(const halo_score_args *a, void *stream);

/* Helper methods of FloatingRegionScore that are public by convention:
 *  - compute_region_uncertainty(unc_type, logit, p, ground_truth) / compute_pixel_entropy(p)
 *    (floating_region.py:70-92,123-127): x (B,O,H,W) f32 holds logits (is_prob=0) or softmax
 *    probabilities (is_prob=1); do_box bit 0 applies the k x k box sum, its bits 8-9 carry the padding mode
 *    (HALO_FLAG_PAD(HALO_PAD_*)); out (B,H,W) f32.  workspace: B*H*W*4 + 256 bytes.
 *  - compute_region_impurity(predict, K) (floating_region.py:112-121): pred (B,H,W) i64 ->
 *    impurity, count (B,H,W) f32 (count may be NULL); pad_mode = HALO_PAD_*.
 *  - quantize_uncert_map(decoder_out) (floating_region.py:94-110): -> pred (B,H,W) i64 in [0,K-1].
 *    workspace: halo_score_workspace_bytes(B,H,W). */
int halo_region_uncertainty(const float *x, int64_t bstride, int is_prob, const int64_t *gt, int64_t B, int64_t O,
                            int64_t H, int64_t W, int unc_type, int ksize, int do_box, float *out, void *workspace,
                            size_t workspace_bytes, void *stream);
int halo_region_impurity(const int64_t *pred, int64_t B, int64_t H, int64_t W, int ksize, int64_t K, float *impurity,
                         float *count, int pad_mode, void *stream);
/* Which kernels serve a k x k window pass -- the box sum of the uncertainty (HALO_WINDOW_BOX) or the class histogram of the purity
 * window (HALO_WINDOW_HIST; bins = classes, or K for 'hyper') -- on an H x W map: 0 the generic one-thread-per-pixel kernels, 1 the
 * 3 x 3 zero-padding tile kernels of the scorer, 2 the LDS-tiled wide-window kernels (odd k from 5 to 33, every padding mode,
 * at most 32 bins).  A pure host function: the launchers branch on it.  Every route computes the same bits.  <0: HALO_E_ARG. */
#define HALO_WINDOW_BOX 0
#define HALO_WINDOW_HIST 1
int halo_window_route(int what, int ksize, int pad_mode, int64_t bins, int64_t H, int64_t W);
int halo_quantize_radius(const void *feat, int feat_dtype, int64_t feat_bstride, int64_t B, int64_t C, int64_t H,
                         int64_t W, int64_t K, double c, int64_t *pred, void *workspace, size_t workspace_bytes,
                         void *stream);

/* ---- selection: select_pixels_to_label (core/active/build.py:27-64) ----
 *
 * score (B,H,W) f32|f64 is mutated (windows -> -inf) exactly like the reference; active, selected
 * (B,H,W) u8 (torch.bool storage) and active_mask (B,H,W) i64 are updated in place; gt (B,H,W) i64.
 * Up to n_regions picks per image: repeat { argmax with ties -> smallest w, then smallest h
 * (the reference's two-stage torch.max, build.py:38-43); stop when the max is -inf }.
 * picks (B,n_regions,3) f64 receives (h, w, value) in selection order (may be NULL);
 * n_picked (B) i32 receives the count (may be NULL).
 */
/* method: HALO_SELECT_AUTO runs the value-binned sweep (visit pixels in descending value order, test each
 * against the picks so far -- no per-pick pass over the map) and leaves what it cannot finish (NaN / +inf
 * in the map, large plateaus of exact ties, pick grid larger than LDS, mask radius 0 or above 14) to the serial
 * tile-table kernel on the same stream; HALO_SELECT_SERIAL runs only the latter; HALO_SELECT_BINNED
 * fails with HALO_E_UNSUPPORTED where the sweep does not serve the geometry.  All three give identical results.
 * workspace: halo_select_workspace_bytes(B, H, W, n_regions, mask_radius). */
enum { HALO_SELECT_AUTO = 0, HALO_SELECT_SERIAL = 1, HALO_SELECT_BINNED = 2 };
size_t halo_select_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t n_regions, int64_t mask_radius);
/* `score_range`: the value range of each score map, a buffer of halo_score_range_bytes(B) bytes filled by halo_score
 * (halo_score_args.score_range) or halo_score_range for the same B maps; NULL = find it here.  The range
 * only has to BOUND the finite values: the binning is monotone, so the picks do not depend on it.  The buffer also holds room
 * for the selector's coarse histogram of each map (2048 counters): for normalised maps the scorer counts it while it writes the
 * score and marks the record; the selector then skips its pass over the map and CLEARS the mark (the buffer is written through
 * the const pointer's storage: the counts describe the map as it was scored and are used once; should the caller have changed
 * the map in between, the sweep hands an exhausted image over to the serial kernel instead of trusting them -- results never
 * depend on the histogram).  halo_score_range computes the exact range records of existing maps (no histogram).
 * `handover` (B,2) i32, NULL = do not report: what the value-binned sweep did with each image; row b = {reason, picks the sweep
 * made before it stopped}.  Reason 0 = the sweep finished the image; anything else = the serial kernel continued it from that
 * pick on (results are identical either way -- this is a cost counter: a handed-over image costs milliseconds instead of tens
 * of microseconds). */
enum { HALO_SWEEP_DONE = 0,
       HALO_SWEEP_BAD_VALUES = 1,     /* NaN / +inf in the map, a constant map, or nothing pickable: no value range to bin */
       HALO_SWEEP_BIN_OVERFLOW = 2,   /* a run of candidates too dense for its value bins (a plateau of ties) */
       HALO_SWEEP_SURVIVORS = 3,      /* more unsuppressed candidates in one step than the resolve stage holds */
       HALO_SWEEP_EXHAUSTED = 4,      /* candidates ran out behind a dropped threshold bin / a stale histogram */
       HALO_SWEEP_NOT_RUN = 5 };      /* serial method, or a geometry the sweep does not serve */
size_t halo_score_range_bytes(int64_t B);
int halo_score_range(const void *score, int dtype, int64_t B, int64_t H, int64_t W, void *score_range, void *stream);
int halo_greedy_select(void *score, int dtype, int64_t B, int64_t H, int64_t W, int64_t n_regions,
                       int64_t active_radius, int64_t mask_radius, uint8_t *active, uint8_t *selected,
                       int64_t *active_mask, const int64_t *gt, double *picks, int32_t *n_picked,
                       void *workspace, size_t workspace_bytes, int method, const void *score_range,
                       int32_t *handover, void *stream);
/* The sweep places and walks its candidates in two tranches: the top halo_select_first_tranche(...) values of a map first, the
 * rest of the proven bound n_regions x (2 mask_radius + 1)^2 only for an image whose first tranche ran out before n_regions picks
 * (a second round inside the same call; results never depend on it).  halo_select_first_tranche: a host query, no device work.
 * halo_select_stats: the counters of the LAST halo_greedy_select that used `workspace` with the same geometry, copied on `stream`
 * into stats (B,3) i32: row b = {candidates placed, candidates in the chunks the sweep processed, sweep rounds run (0: the sweep
 * did not run, 1, or 2)}.  Zeros where the sweep does not serve the geometry. */
int64_t halo_select_first_tranche(int64_t H, int64_t W, int64_t n_regions, int64_t mask_radius);
int halo_select_stats(const void *workspace, size_t workspace_bytes, int64_t B, int64_t H, int64_t W, int64_t n_regions,
                      int64_t mask_radius, int32_t *stats, void *stream);

/* ---- pool side of the round: image-wise sharding, ONE all-gather of pick tables (the reference runs the
 * round on rank 0 only, core/train_learners.py:307-326) ----
 *  - halo_pack_pick_tables: picks (B,n_regions,3) f64 + n_picked (B) i32 (as halo_greedy_select writes them) -> B rows of
 *    the int32 wire block of halo_amd/pool.py: per pick (h << 16) | w and the two words of the float64 score, then the
 *    pick count at word 3*n_regions; wire_row_stride >= 3*n_regions + 1, in int32 elements.
 *  - halo_reset_round_state: the loader's round-1 state for n_pixels pixels (core/datasets/cityscapes.py:245-251):
 *    active = selected = False, active_mask = 255.
 *  - halo_undo_picks: the same state restored after a selection whose state WAS the round-1 state, from its pick
 *    table: only the windows select_pixels_to_label wrote (build.py:52-62) are rewritten.
 *  - halo_device_identity: "pci=<bus id> uuid=<32 hex digits>" of a HIP device ordinal, NUL-terminated, len >= 64
 *    (the ranks of a node must hold distinct devices).
 *  (Round 3 also exported HBM probes and a contiguous-range allocator here; ABI 5 moved those measurement aids to
 *  tools/halo_probe.hip -- this header keeps only entry points that replace a reference call, plus halo_event_*.) */
int halo_pack_pick_tables(const double *picks, const int32_t *n_picked, int64_t B, int64_t n_regions, int32_t *wire,
                          int64_t wire_row_stride, void *stream);
int halo_reset_round_state(uint8_t *active, uint8_t *selected, int64_t *active_mask, int64_t n_pixels, void *stream);
int halo_undo_picks(const double *picks, const int32_t *n_picked, int64_t B, int64_t H, int64_t W, int64_t n_regions,
                    int64_t active_radius, int64_t mask_radius, uint8_t *active, uint8_t *selected, int64_t *active_mask,
                    void *stream);
int halo_device_identity(int device, char *buf, size_t len);

/* ---- training-side window losses, float32 tensors, float64 sums on the device ----
 *  - NegativeLearningLoss (core/loss/negative_learning_loss.py:6-16): sums = {sum -mask*log(1-p+1e-6), sum mask},
 *    mask = p < threshold; loss = sums[0]/sums[1].  bwd: gp = gloss * mask / ((1-p+1e-6) * sums[1]).
 *  - LocalConsistentLoss (core/loss/local_consistent_loss.py:5-17 = LocalDiscrepancy + DetectSPBoundary,
 *    core/loss/boundary.py): x (B,O,h,w) logits, label (B,h,w) i64; writes p = softmax(x) and sums =
 *    {sum of the per-pixel discrepancy over boundary pixels with a valid label, their count}; kl: 0 'l1', 1 'kl'.
 *    coef_a/coef_b (B,O,h,w) and mask (B,h,w) bytes are for the backward call (all three NULL when no gradient is needed):
 *    mask = 1 at the selected pixels, and d l/d p, d l/d mean are written AT THOSE PIXELS ONLY (ABI 7: the rest of the two
 *    coefficient maps is left untouched -- allocate, do not clear).  bwd: gx = d (sums[0]/sums[1]) / d x * gloss  (zero when
 *    the selection is empty).
 *  workspace: halo_loss_workspace_bytes(number of pixels or elements). */
size_t halo_loss_workspace_bytes(int64_t n);
int halo_negative_learning_fwd(const float *p, int64_t n, double threshold, double *sums, void *workspace,
                               size_t workspace_bytes, void *stream);
int halo_negative_learning_bwd(const float *p, int64_t n, double threshold, const double *sums, const float *gloss,
                               float *gp, void *stream);
int halo_local_consistent_fwd(const float *x, const int64_t *label, int64_t B, int64_t O, int64_t h, int64_t w, int kl,
                              float *p, double *sums, float *coef_a, float *coef_b, uint8_t *mask, void *workspace,
                              size_t workspace_bytes, void *stream);
int halo_local_consistent_bwd(const float *p, const float *coef_a, const float *coef_b, const uint8_t *mask, int64_t B, int64_t O,
                              int64_t h, int64_t w, const double *sums, const float *gloss, float *gx, void *stream);

/* ---- validation metric (ABI 9): BaseLearner.inference + validation_step + intersectionAndUnionGPU
 *  (core/train_learners.py:57-128, core/utils/misc.py:35-47) ----
 *  halo_eval_confusion: logit holds `views` (1 or 2) low-resolution maps (K, h, w) f32 per image, view v of image i at
 *    logit + (views*i + v) * logit_bstride (a head output of [x, flip(x)] for views = 2); label (B, H, W) of label_dtype
 *    HALO_I64 / HALO_I32 / HALO_U8.  Per output pixel: bilinear upsampling to H x W (align_corners=True), softmax, view 1 read at
 *    column W-1-x, (a + b) / 2, the first maximal class (a NaN counts as maximal) -- torch's CPU kernels bit for bit.
 *    pred (B, H, W) i64 receives that arg-max when not NULL.
 *  halo_confusion_from_pred: the same counting for a prediction map (B, H, W) of pred_dtype HALO_I64 / HALO_I32 / HALO_U8.
 *  Both ADD the image's counts into counts (B, 3, K) i64, rows [intersection, union, target], with the reference's integer
 *  semantics: o = (t == ignore_index) ? ignore_index : pred; output counts o, target counts t, intersection counts o where
 *  o == t; each only where the value lies in [0, K) (torch.histc(bins=K, min=0, max=K-1)); union = output + target -
 *  intersection.  K <= 1024; other K, views or dtypes return HALO_E_UNSUPPORTED.
 *  workspace: halo_eval_workspace_bytes(B, K, H, W) (one u32 histogram of 3 x K per 1024 pixels). */
size_t halo_eval_workspace_bytes(int64_t B, int64_t K, int64_t H, int64_t W);
int halo_eval_confusion(const float *logit, int64_t logit_bstride, int views, int64_t K, int64_t h, int64_t w, const void *label,
                        int label_dtype, int64_t H, int64_t W, int64_t B, int64_t ignore_index, int64_t *counts, int64_t *pred,
                        void *workspace, size_t workspace_bytes, void *stream);
int halo_confusion_from_pred(const void *pred, int pred_dtype, const void *label, int label_dtype, int64_t K, int64_t H, int64_t W,
                             int64_t B, int64_t ignore_index, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);

/* ---- training criterion from low-resolution logits (ABI 10): BaseLearner.forward(size=input_size) -> torch.softmax ->
 *  nn.CrossEntropyLoss(ignore_index) + NegativeLearningLoss(threshold), and their backward to the logits
 *  (core/train_learners.py:224-243, 328-368, 404-463, 505-563; core/loss/negative_learning_loss.py:6-16) ----
 *  logit (B, K, h, w) f32, image i at logit + i * logit_bstride; label (B, H, W) of label_dtype HALO_I64 / HALO_I32 / HALO_U8.
 *  Per output pixel: bilinear upsampling to H x W (align_corners=True) and softmax, torch's CPU kernels bit for bit (as
 *  halo_eval_confusion); the full-resolution maps are never written.  terms: HALO_LOSS_CE | HALO_LOSS_NL.
 *  halo_upsampled_loss_fwd OVERWRITES sums[5] (f64, device) = {ce_sum, ce_count, nl_sum, nl_count, bad_label_count}:
 *    ce over the labels y with 0 <= y < K and y != ignore_index, -log_softmax[y]; nl over the (pixel, class) pairs with
 *    p < (float)threshold, -log((1 - p) + 1e-6); bad_label_count = labels neither ignore_index nor in [0, K) (never used as an
 *    index).  The counts are computed whatever `terms` says; a term that is off leaves its sum 0.  The caller forms
 *    ce = ce_sum / ce_count (NaN over no label, as torch) and nl = nl_sum / nl_count.
 *  halo_upsampled_loss_bwd WRITES grad_logit (B, K, h, w) f32 dense: the adjoint of the resize applied to
 *    d_k = g_ce/ce_count (p_k - [k = y]) [labelled] + g_nl/nl_count p_k (q_k - sum_c q_c p_c),  q_c = [p_c < thr] / ((1 - p_c) + 1e-6),
 *    with sums from the forward of the same inputs and g_ce / g_nl device scalars f32 (NULL = no upstream gradient); a term
 *    whose count is 0 contributes 0.  Gather order fixed, no atomics: repeated calls give identical bits.
 *  Both reduce in a fixed order without atomics.  HALO_E_UNSUPPORTED: K > 1024, H < h or W < w (torch also interpolates
 *  down; this path upsamples only), other label dtypes; HALO_E_ARG: an empty shape; HALO_E_WORKSPACE: a short workspace.
 *  workspace (fwd only): halo_upsampled_loss_workspace_bytes(B, K, H, W) (five f64 partials per 1024 output pixels). */
enum { HALO_LOSS_CE = 1, HALO_LOSS_NL = 2 };
size_t halo_upsampled_loss_workspace_bytes(int64_t B, int64_t K, int64_t H, int64_t W);
int halo_upsampled_loss_fwd(const float *logit, int64_t logit_bstride, int64_t B, int64_t K, int64_t h, int64_t w, const void *label,
                            int label_dtype, int64_t H, int64_t W, int64_t ignore_index, double threshold, int terms, double *sums,
                            void *workspace, size_t workspace_bytes, void *stream);
int halo_upsampled_loss_bwd(const float *logit, int64_t logit_bstride, int64_t B, int64_t K, int64_t h, int64_t w, const void *label,
                            int label_dtype, int64_t H, int64_t W, int64_t ignore_index, double threshold, int terms,
                            const double *sums, const float *g_ce, const float *g_nl, float *grad_logit, void *stream);

/* ---- HFR weighted normalisation of the DeepLab-v3+ hyperbolic head, forward and backward (core/models/classifier.py:529-550) ----
 *  x (B, C, P) f32 dense (the conv_reduce output, P = h * w); wn_mlp = Linear(C, C) [W1 (C, C), b1] -> BatchNorm1d(C) [gamma, beta,
 *  NULL = not affine] -> ReLU -> Linear(C, C) [W2, b2]; every parameter f32 dense on the device.  C <= 256 (C = 64 templated).
 *    h_p = W1 x_p + b1, z = BN(h), w_b = W2 mean_p relu(z_p) + b2, wc = clamp(w, min=1e-5), y = (x / max(||x_bc||_2, 1e-12)) * wc.
 *  One workspace of halo_hfr_workspace_bytes(B, C, P) serves a forward and the backward of the same inputs: it carries the
 *  forward's state to the backward, so the caller keeps it between the two.
 *  halo_hfr_fwd_stats WRITES stats (C, 3) f64 = (count, mean, M2) of h per channel over the B * P rows.  Rows of several ranks
 *    may be merged (Chan's formula) by the caller before:
 *  halo_hfr_fwd_apply WRITES y (B, C, P) f32.  stats = the batch statistics (training), then running_mean / running_var (f32,
 *    NULL = not tracked) take F.batch_norm's update with factor `momentum` and the unbiased variance; stats = NULL: the running
 *    statistics normalise (evaluation) and are not changed.
 *  halo_hfr_bwd_reduce (g = dL/dy) WRITES g_W2, g_b2, g_gamma, g_beta (NULL when not affine; this call's rows only) and
 *    gsums (C, 2) f64 = (sum g_z, sum g_z zhat) per channel.  Ranks may all-reduce gsums before:
 *  halo_hfr_bwd_apply WRITES g_x (B, C, P), g_W1 (C, C), g_b1 (C).
 *  Every reduction runs in a fixed order without atomics: repeated calls give identical bits.  HALO_E_UNSUPPORTED: C > 256,
 *  B > 65535 or P > 65535 * 1024; HALO_E_ARG: an empty shape or a missing pointer; HALO_E_WORKSPACE: a short workspace. */
size_t halo_hfr_workspace_bytes(int64_t B, int64_t C, int64_t P);
int halo_hfr_fwd_stats(const float *x, int64_t B, int64_t C, int64_t P, const float *W1, const float *b1, double *stats, void *workspace,
                       size_t workspace_bytes, void *stream);
int halo_hfr_fwd_apply(const float *x, int64_t B, int64_t C, int64_t P, const float *W1, const float *b1, const double *stats,
                       float *running_mean, float *running_var, double momentum, double eps, const float *gamma, const float *beta,
                       const float *W2, const float *b2, float *y, void *workspace, size_t workspace_bytes, void *stream);
int halo_hfr_bwd_reduce(const float *x, int64_t B, int64_t C, int64_t P, const float *W2, const float *g, float *g_W2, float *g_b2,
                        float *g_gamma, float *g_beta, double *gsums, void *workspace, size_t workspace_bytes, void *stream);
int halo_hfr_bwd_apply(const float *x, int64_t B, int64_t C, int64_t P, const float *W1, const float *b1, const float *gamma,
                       const float *g, const double *gsums, float *g_x, float *g_W1, float *g_b1, void *workspace,
                       size_t workspace_bytes, void *stream);

/* ---- depthwise 3x3 conv + frozen norm + ReLU: the first half of DepthwiseSeparableConv2d (core/models/classifier.py:78-81) ----
 *  x, y, g, g_x (B, C, H, W) f32 dense NCHW; w (C, 1, 3, 3) f32; scale, shift (C) f32; dilation d >= 1 = padding, stride 1, zeros.
 *    pre = (sum_{ky,kx} w[c,ky,kx] x[b,c,i+(ky-1)d,j+(kx-1)d]) * scale[c] + shift[c]   (two roundings), y = max(pre, 0)
 *    gp = g [y > 0] scale[c];  g_x[p] = sum_k w[c,k] gp[p - k d];  g_w[c,k] = sum_{b,p} gp[b,c,p] x[b,c,p + k d]
 *  The 9-term sums run over the input positions in ascending (row, column) order, the first product rounded and every further
 *  term one fma, whatever the route; g_w is summed in float64 (per-block rows in the workspace, added in ascending (image,
 *  block) order) and rounded once.  No atomics: repeated calls give identical bits.  Only bwd_weight needs the workspace
 *  (8-byte aligned).  HALO_E_UNSUPPORTED: H, W or d above 2^24, H * W above 2^31 - 1; HALO_E_ARG: an empty shape, d < 1 or a
 *  missing pointer; HALO_E_WORKSPACE: a short workspace. */
size_t halo_dwconv_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int64_t d);
int halo_dwconv3x3_affine_relu_fwd(const float *x, const float *w, const float *scale, const float *shift, float *y, int64_t B, int64_t C,
                                   int64_t H, int64_t W, int64_t d, void *stream);
int halo_dwconv3x3_affine_relu_bwd_data(const float *g, const float *y, const float *w, const float *scale, float *g_x, int64_t B,
                                        int64_t C, int64_t H, int64_t W, int64_t d, void *stream);
int halo_dwconv3x3_affine_relu_bwd_weight(const float *g, const float *y, const float *x, const float *scale, float *g_w, int64_t B,
                                          int64_t C, int64_t H, int64_t W, int64_t d, void *workspace, size_t workspace_bytes,
                                          void *stream);

/* ---- the ASPP pyramid: n dilated depthwise 3x3 conv + frozen norm + ReLU over one input, one pass each way ----
 *  x, g_x, every g[i] (B, C, H, W) f32 dense NCHW; y (n, B, C, H, W) f32 dense, y[i] the output of dilation d[i]; w (n, C, 9),
 *  scale, shift (n, C) f32; d a HOST array of n dilations, 2 <= n <= 4, in any order, repeats allowed; g a HOST array of n device
 *  pointers (they travel in the kernel's arguments), NULL for an output that has no gradient, at least one not NULL.
 *    y[i] = the forward above over (x, w[i], scale[i], shift[i], d[i]): its bits.
 *    g_x  = ((gx_0 + gx_1) + gx_2) ..., gx_i the bwd_data above over (g[i], y[i], w[i], scale[i], d[i]), float32 adds in list order,
 *           the NULL entries left out: the bits of that composition.
 *  A workgroup keeps one plane in LDS (forward: x, read from memory once; backward: gp_i and the running sum, g_x written once),
 *  so H * W <= halo_multi_dwconv_max_plane() (a host-only query: no device call).  No atomics.  16-byte accesses when W % 4 == 0
 *  and x, y (fwd) or every g[i], y, g_x (bwd) are 16-byte aligned, one element per lane otherwise: the same bits.  The weight
 *  gradients are n calls of halo_dwconv3x3_affine_relu_bwd_weight.  HALO_E_ARG: n outside 2..4, a missing pointer, every g[i]
 *  NULL, an empty shape, a d[i] < 1; HALO_E_UNSUPPORTED: the size limits above, a plane above the query's; HALO_E_LAUNCH: the device
 *  refused the LDS size.  Every check comes before any launch. */
int64_t halo_multi_dwconv_max_plane(void);
int halo_multi_dwconv3x3_affine_relu_fwd(const float *x, const float *w, const float *scale, const float *shift, float *y, int64_t B,
                                         int64_t C, int64_t H, int64_t W, int64_t n, const int64_t *d, void *stream);
int halo_multi_dwconv3x3_affine_relu_bwd_data(const float *const *g, const float *y, const float *w, const float *scale, float *g_x,
                                              int64_t B, int64_t C, int64_t H, int64_t W, int64_t n, const int64_t *d, void *stream);

/* ---- the ASPP fan-out: the pyramid's backward with the gradients of x's other readers added in the same pass ----
 *  The arguments of the multi bwd_data entry above, plus m extra addends, 0 <= m <= 4: e a HOST array of m device pointers (NULL: left
 *  out), e_plane a HOST array of m flags -- 0: e[j] is (B, C, H, W) f32 dense NCHW; 1: e[j] is (B, C) f32, one value per plane that
 *  enters as e[j][b C + c] at every pixel.
 *    g_x = ((((gx_0 + gx_1) + gx_2) + e_0) + e_1) ...   float32 adds in list order, NULL g[i] and NULL e[j] left out: the bits of
 *          the entry above followed by torch float32 adds of the addends.  m = 0 gives that entry's bits.
 *  The addends join where the running sum leaves LDS, so the plane limit is halo_multi_dwconv_max_plane().  The 16-byte route also
 *  needs every dense e[j] 16-byte aligned; otherwise one element per lane, the same bits.  At least one g[i] is not NULL.
 *  HALO_E_ARG: the entry above's, m outside 0..4, e or e_plane NULL with m > 0; the other codes as above.  Every check comes
 *  before any launch. */
int halo_fan_dwconv3x3_affine_relu_bwd_data(const float *const *g, const float *y, const float *w, const float *scale, float *g_x,
                                            int64_t B, int64_t C, int64_t H, int64_t W, int64_t n, const int64_t *d, int64_t m,
                                            const float *const *e, const int32_t *e_plane, void *stream);

/* ---- the front of the v3+ decoder: resize + concat + depthwise 3x3 conv + frozen norm + ReLU in one pass ----
 *  a (B, Ca, h, w), s (B, Cs, H, W) with H >= h, W >= w, y and g (B, Ca + Cs, H, W), g_up (B, Ca, H, W), g_s (B, Cs, H, W): f32 dense
 *  NCHW; w (Ca + Cs, 1, 3, 3), scale, shift (Ca + Cs) f32; dilation = padding = 1.
 *    x[b,c] = c < Ca ? bilinear_align_corners(a[b,c], (H, W)) : s[b,c-Ca]      (never stored: halo_bilinear_upsample's bits)
 *    y = the forward above over x;  gp = g [y > 0] scale;  g_up | g_s = the planes below | from Ca of sum_k w[c,k] gp[p - k];
 *    g_w[c,k] = sum_{b,p} gp x[p + k]  (x recomputed from a / s)
 *  Same summation orders and the same work split as the calls above for C = Ca + Cs, d = 1, so y, g_up | g_s and g_w carry the
 *  bits those calls return for the stored concatenation.  g_a is halo_bilinear_upsample_bwd(g_up).  bwd_data: either output may
 *  be NULL, its planes are then skipped; with both NULL nothing is launched.  a may be NULL when Ca = 0, s when Cs = 0.  16-byte
 *  loads and stores when W % 4 == 0 and s, y, g, g_up, g_s are 16-byte aligned, one column per thread otherwise: the same bits.
 *  bwd_weight's workspace: halo_dwconv_workspace_bytes(B, Ca + Cs, H, W, 1).  HALO_E_ARG: a missing pointer, an empty shape
 *  (Ca + Cs = 0 included), H < h or W < w; HALO_E_UNSUPPORTED: the limits above; HALO_E_WORKSPACE: a short workspace. */
int halo_upcat_dwconv3x3_affine_relu_fwd(const float *a, const float *s, const float *w, const float *scale, const float *shift, float *y,
                                         int64_t B, int64_t Ca, int64_t Cs, int64_t h, int64_t w_in, int64_t H, int64_t W, void *stream);
int halo_upcat_dwconv3x3_affine_relu_bwd_data(const float *g, const float *y, const float *w, const float *scale, float *g_up, float *g_s,
                                              int64_t B, int64_t Ca, int64_t Cs, int64_t H, int64_t W, void *stream);
int halo_upcat_dwconv3x3_affine_relu_bwd_weight(const float *g, const float *y, const float *a, const float *s, const float *scale,
                                                float *g_w, int64_t B, int64_t Ca, int64_t Cs, int64_t h, int64_t w_in, int64_t H, int64_t W,
                                                void *workspace, size_t workspace_bytes, void *stream);

/* ---- both gradients of a depthwise block from one pass: g, y and x are read once, g_x is written once ----
 *  The operands of the bwd_data and bwd_weight calls above (plain, and the decoder front's); a thread keeps the window of gp and the
 *  window of x and runs the statements of both calls per output row, in their order.  All outputs are required (the front's g_up
 *  when Ca > 0, g_s when Cs > 0).  The workspace is bwd_weight's: halo_dwconv_workspace_bytes(B, C, H, W, d), for the front
 *  (B, Ca + Cs, H, W, 1).  16-byte loads and stores only when W % 4 == 0 and ALL of g, y, x, g_x (the front: g, y, s, g_up, g_s)
 *  are 16-byte aligned; one column per thread otherwise.
 *    g_x (g_up | g_s) carries the bits of ..._bwd_data on either route: its sums do not depend on the route.
 *    g_w carries the bits of ..._bwd_weight whenever that call takes the same route on g, y, x (the front: g, y, s).  In the one
 *        remaining case -- those aligned, W % 4 == 0, and only g_x (g_up, g_s) misaligned -- g_w equals ..._bwd_weight on the
 *        one-column route (what it returns for the same values at a misaligned x).
 *  Checks in the parents' order, before any launch: the shape (HALO_E_ARG / HALO_E_UNSUPPORTED as above), a missing pointer
 *  (HALO_E_ARG), the workspace (HALO_E_WORKSPACE: short, NULL or not 8-byte aligned).  No atomics: repeated calls give identical bits. */
int halo_joint_dwconv3x3_affine_relu_bwd(const float *g, const float *y, const float *x, const float *w, const float *scale, float *g_x,
                                         float *g_w, int64_t B, int64_t C, int64_t H, int64_t W, int64_t d, void *workspace,
                                         size_t workspace_bytes, void *stream);
int halo_joint_upcat_dwconv3x3_affine_relu_bwd(const float *g, const float *y, const float *a, const float *s, const float *w,
                                               const float *scale, float *g_up, float *g_s, float *g_w, int64_t B, int64_t Ca, int64_t Cs,
                                               int64_t h, int64_t w_in, int64_t H, int64_t W, void *workspace, size_t workspace_bytes,
                                               void *stream);

/* ---- the same block half under torch.autocast: half in, half out (halo_amd/dwconv.py: depthwise_bn_relu_autocast) ----
 *  half_dtype = HALO_F16 | HALO_BF16 is the element type of y16 and g16; x (x_dtype) and g_x (gx_dtype) are HALO_F32 or half_dtype;
 *  w, scale, shift and g_w are float32.  All activations (B, C, H, W) dense NCHW.  h() rounds to nearest even to half_dtype
 *  (overflow to +-inf, a NaN stays a NaN), half -> float is exact:
 *    xh = h(x) (the identity for a half x);  wh = h(w[c,k]);  c16 = h(sum_k wh[k] xh[tap k])
 *    pre = fl(fl(float(c16) scale[c]) + shift[c]);  y32 = pre <= 0 ? 0 : pre (a NaN stays a NaN);  y16 = h(y32), the only output
 *    gp = y16 > 0 ? fl(float(g16) scale[c]) : 0;  gc16 = h(gp);  g_x = h(sum_k wh[k] gc16[p - k d]), widened for gx_dtype HALO_F32
 *    g_w[c,k] = float(h(fl32(sum_{b,p} float(gc16) float(xh[p + k d]))))
 *  the stages and roundings of `conv(x); x * scale + bias; relu_; .to(half)` under autocast and of its autograd backward, with one
 *  deviation: the gate is read off y16, so where 0 < y32 rounds to a half zero the gradient is 0 and autograd's passes.  The sums
 *  are the float32 passes': nine terms in ascending input position, the first product rounded, one fma each (a product of two
 *  halves is exact in float32); g_w in float64 partials and halo_dwconv_workspace_bytes(B, C, H, W, d) of workspace, no atomics.
 *  The bits depend on the operands and the shape alone.  They are not the library convolution's: a sum within the float32
 *  accumulation error of a half rounding boundary may land on the other neighbour.  W % 4 == 0 with every float32 activation
 *  16-byte and every half activation 8-byte aligned runs four columns per thread, anything else one.  Checks before any launch:
 *  HALO_E_ARG for a missing pointer, a half_dtype outside {HALO_F16, HALO_BF16}, an x_dtype / gx_dtype outside {HALO_F32,
 *  half_dtype}, an empty shape or d < 1; HALO_E_UNSUPPORTED for the limits above; HALO_E_WORKSPACE for a short workspace. */
int halo_half_dwconv3x3_affine_relu_fwd(const void *x, int x_dtype, const float *w, const float *scale, const float *shift, void *y16,
                                        int half_dtype, int64_t B, int64_t C, int64_t H, int64_t W, int64_t d, void *stream);
int halo_half_dwconv3x3_affine_relu_bwd_data(const void *g16, const void *y16, const float *w, const float *scale, void *g_x, int gx_dtype,
                                             int half_dtype, int64_t B, int64_t C, int64_t H, int64_t W, int64_t d, void *stream);
int halo_half_dwconv3x3_affine_relu_bwd_weight(const void *g16, const void *y16, const void *x, int x_dtype, const float *scale, float *g_w,
                                               int half_dtype, int64_t B, int64_t C, int64_t H, int64_t W, int64_t d, void *workspace,
                                               size_t workspace_bytes, void *stream);

/* ---- frozen norm + residual add + ReLU of a ResNet block(core/models/resnet.py:53-69, 92-112; core/models/layers.py) ----
 *  x, r, y, g, g_x, g_r (B, C, HW) f32 dense NCHW planes; scale, shift, r_scale, r_shift (C) f32.
 *    pre = fl(fl(x scale[c]) + shift[c]);  id = r  or  fl(fl(r r_scale[c]) + r_shift[c]);  y = relu(pre)  or  relu(fl(pre + id))
 *    gp = y <= 0 ? 0 : g;  g_x = fl(gp scale[c]);  g_r = gp  or  fl(gp r_scale[c])
 *  relu(s) = s <= 0 ? 0 : s keeps a NaN; a NaN y lets g through.  Every product and sum is rounded on its own (no fma): the bits
 *  are those of the torch statements `x * scale + bias; out += identity; relu_(out)` and of their autograd backward.
 *  fwd: r == NULL: no residual; r_scale == NULL: r is added as it stands; r_scale and r_shift come together.  bwd: a NULL g_x or
 *  g_r is neither computed nor written; r_scale == NULL: g_r = gp.  y must not overlap x or r; g_x and g_r must not overlap g, y.
 *  HW % 4 == 0 with every operand 16-byte aligned runs 16-byte accesses, anything else one element per lane: same statements,
 *  same bits.  HALO_E_ARG: an empty shape, a missing pointer, r_scale without r_shift or without r, bwd with neither output;
 *  HALO_E_UNSUPPORTED: HW above 2^31 - 1025 or more than 2^31 - 1 workgroups. */
int halo_affine_relu_fwd(const float *x, const float *scale, const float *shift, const float *r, const float *r_scale, const float *r_shift,
                         float *y, int64_t B, int64_t C, int64_t HW, void *stream);
int halo_affine_relu_bwd(const float *g, const float *y, const float *scale, const float *r_scale, float *g_x, float *g_r, int64_t B,
                         int64_t C, int64_t HW, void *stream);
/*  The same backward for a y that two consumers read (a block output: the next block's conv1 and its identity), so that two
 *  gradients g_a, g_b (B, C, HW) arrive at it:  g = fl(g_a + g_b), the one float32 add of autograd's accumulation, then the
 *  statements above on that g.  g_x and g_r must not overlap g_a, g_b or y; the 16-byte route needs g_b aligned as well.  Checks
 *  and limits are those of the single-gradient entry; a NULL g_a or g_b is HALO_E_ARG. */
int halo_fork_affine_relu_bwd(const float *g_a, const float *g_b, const float *y, const float *scale, const float *r_scale, float *g_x,
                              float *g_r, int64_t B, int64_t C, int64_t HW, void *stream);

/* ---- the same chain under torch.autocast (halo_norm_autocast.hip, halo_amd/norm.py: norm_relu_autocast) ----
 *  The convolution in front returns half, the stock statements promote to float32, autocast rounds the result back to half for
 *  the next convolution.  half_dtype = HALO_F16 | HALO_BF16 is the element type of every half operand of a call: x, y16, g16, g_x
 *  always; r and g_r when r_scale is given (the downsample convolution's output, its norm folded in).  Without r_scale r and g_r are
 *  float32 (the block's identity).  y32, g32 float32; all (B, C, HW) dense NCHW planes; scale, shift, r_scale, r_shift (C) f32.
 *    pre = fl(fl(float(x) scale[c]) + shift[c]);  id = r32  or  fl(fl(float(r16) r_scale[c]) + r_shift[c])
 *    s = pre  or  fl(pre + id);  y32 = s <= 0 ? 0 : s (a NaN stays a NaN);  y16 = rne_half(y32)
 *    g = g32,  float(g16)  or  fl(g32 + float(g16));  gp = s <= 0 ? 0 : g (a NaN s lets g through)
 *    g_x = rne_half(fl(gp scale[c]));  g_r = gp  or  rne_half(fl(gp r_scale[c]))
 *  half -> float is exact; float -> half rounds to nearest even, overflows to +-inf, keeps a NaN a NaN (payload not specified).
 *  fwd: a NULL y32 or y16 is not written, one of them must be given.  bwd: a NULL g32 or g16 is not read, one of them must be
 *  given; the gate s <= 0 is read off y32, or off pre recomputed from x, scale and shift -- exactly one of y32 and x is given, and
 *  x only for a pass without a residual (g_r NULL): y16 cannot stand in for it, a small positive y32 rounds to a half zero.  A
 *  NULL g_x or g_r is neither computed nor written.  Outputs must not overlap inputs.  HW % 8 == 0 with every operand 16-byte
 *  aligned runs 16-byte accesses, anything else one element per lane: same statements, same bits.  HALO_E_ARG: an empty shape, a
 *  missing or contradictory pointer, another half_dtype; HALO_E_UNSUPPORTED: HW above 2^31 - 1025 or more than 2^31 - 1 workgroups. */
int halo_autocast_norm_relu_fwd(const void *x, const float *scale, const float *shift, const void *r, const float *r_scale,
                                const float *r_shift, float *y32, void *y16, int half_dtype, int64_t B, int64_t C, int64_t HW, void *stream);
int halo_autocast_norm_relu_bwd(const float *g32, const void *g16, const float *y32, const void *x, const float *scale, const float *shift,
                                const float *r_scale, void *g_x, void *g_r, int half_dtype, int64_t B, int64_t C, int64_t HW, void *stream);

/* ---- frozen norm + ReLU + Dropout2d: the pointwise tail of a separable block and the dropout behind it (halo_amd/norm.py) ----
 *  x, y, g, g_x (B, C, HW) f32 dense NCHW planes; scale, shift (C) f32; mask (B, C) f32: the multiplier of plane (b, c), 0 or
 *  fl32(1 / (1 - p)), drawn by the caller (nn.Dropout2d's noise tensor).
 *    y   = fl(relu(fl(fl(x scale[c]) + shift[c])) mask[b,c])        every product and sum rounded on its own, a NaN stays a NaN
 *    g_x = y <= 0 ? 0 : fl(fl(g mask[b,c]) scale[c])                a NaN y lets g through
 *  The bits of `dropout2d(relu_(x * scale + bias))` and, for a finite g, of its autograd backward.  The forward reads x in dropped
 *  planes too (inf * 0 is a NaN there, as in the stock chain).  The backward writes zeros for a plane whose mask is 0 without
 *  reading g or y: a non-finite g in a dropped plane gives 0 where autograd gives a NaN.  y must not overlap x; g_x must not
 *  overlap g or y.  Routes, alignment rule and limits are those of the pair above.  HALO_E_ARG: an empty shape or a missing
 *  pointer; HALO_E_UNSUPPORTED: HW above 2^31 - 1025 or more than 2^31 - 1 workgroups. */
int halo_masked_affine_relu_fwd(const float *x, const float *scale, const float *shift, const float *mask, float *y, int64_t B, int64_t C,
                                int64_t HW, void *stream);
int halo_masked_affine_relu_bwd(const float *g, const float *y, const float *scale, const float *mask, float *g_x, int64_t B, int64_t C,
                                int64_t HW, void *stream);

/* ---- frozen norm + ReLU + Dropout2d, both tensors kept: the Euclidean v3+ head's decoder[1], decoder[2] (halo_amd/norm.py) ----
 *  The old decoder layout of DepthwiseSeparableASPP returns the tensor in front of its nn.Dropout2d and feeds the one behind it to
 *  the classifier conv.  x, y, z, g_y, g_z, g_x (B, C, HW) f32 dense NCHW planes; scale, shift (C) f32; mask (B, C) f32 as above.
 *    y   = relu(fl(fl(x scale[c]) + shift[c]))                       the first pair's statements, a NaN stays a NaN
 *    z   = fl(y mask[b,c])                                           inf * 0 is the stock chain's NaN
 *    g   = g_y,  fl(g_z mask[b,c])  or  fl(g_y + fl(g_z mask[b,c]))  the product first, then autograd's accumulation
 *    g_x = fl((y <= 0 ? 0 : g) scale[c])                             a NaN y lets g through
 *  bwd: g_y or g_z may be NULL (an output nobody used), not both; a NULL one is not read.  In a plane whose mask is 0 g_z is not
 *  read and its term is taken as 0: with g_y NULL such a plane is written as zeros without reading y either.  A non-finite g_z in
 *  a dropped plane therefore gives g_y's share alone where autograd gives a NaN; for finite gradients the bits are autograd's.
 *  y and z must not overlap x or each other; g_x must not overlap g_y, g_z or y.  Routes, alignment rule and limits are those of
 *  the pairs above.  HALO_E_ARG: an empty shape or a missing pointer; HALO_E_UNSUPPORTED: HW above 2^31 - 1025 or more than
 *  2^31 - 1 workgroups. */
int halo_dropout_pair_fwd(const float *x, const float *scale, const float *shift, const float *mask, float *y, float *z, int64_t B, int64_t C,
                          int64_t HW, void *stream);
int halo_dropout_pair_bwd(const float *g_y, const float *g_z, const float *y, const float *scale, const float *mask, float *g_x, int64_t B,
                          int64_t C, int64_t HW, void *stream);

/* ---- the image-pooling branch of the v3+ bottleneck folded into a border-aware bias (halo_amd/aspp.py) ----
 *  The bottleneck's 3x3 zero-padded conv reads Cx pyramid channels and Cg channels that are constant planes v[b,c] (the pooled branch,
 *  broadcast).  The constant planes' share of its output takes 9 values per (image, output channel): 3 row classes (0 top row, 1
 *  interior, 2 bottom row) x 3 column classes, by which taps fall inside the map.
 *  w: the conv's (Co, Cx + Cg, 3, 3) f32 weight, read in place: Wg[o,c,k] = w[o row_stride + (c_off + c) 9 + k] with c_off = Cx and
 *  row_stride = (Cx + Cg) 9 elements; v (B, Cg) f32; T (B, Co, 3, 3) f32; z, y, g, g_z (B, Co, H, W) f32 dense NCHW; scale, shift (Co)
 *  f32; g_T (B, Co, 3, 3) f64.
 *    S[b,o,ky,kx] = sum_c Wg[o,c,ky,kx] v[b,c]                       float64 products and sums, channel c on lane c % 256, a fixed tree
 *    T[b,o,rc,cc] = fl32(sum_{ky in R(rc)} sum_{kx in C(cc)} S)      float64, ky then kx ascending; R(0) = {1,2}, R(1) = {0,1,2},
 *                                                                    R(2) = {0,1}, C likewise
 *    y   = relu(fl(fl(fl(z + T[b,o,rc(i),cc(j)]) scale[o]) + shift[o]))       three roundings, never an fma; a NaN stays a NaN
 *    gp  = y <= 0 ? 0 : g;   g_z = fl(gp scale[o]);   g_T[b,o,rc,cc] = sum over the class's pixels of g_z in float64
 *  g_T is summed without atomics: a workgroup adds its elements in a fixed order into its own row of the workspace, a second kernel adds
 *  a plane's rows in ascending order -- the same bits on every call and every stream.  bwd: g_z or g_T may be NULL (g_T NULL needs no
 *  workspace); with both NULL nothing is launched.  16-byte accesses when W % 4 == 0 and z, y, g, g_z are 16-byte aligned, one element
 *  per lane otherwise: the same bits.  HALO_E_ARG: a missing pointer, an empty shape, H < 2 or W < 2, a channel range outside the weight
 *  row; HALO_E_UNSUPPORTED: H W above 2^31 - 1025 or more than 2^31 - 1 workgroups; HALO_E_WORKSPACE: a short workspace.
 *  halo_pool_fold_workspace_bytes sizes the slab for the route with the most workgroups (B Co ceil(H W / 1024) rows of 72 bytes) and
 *  returns 0 for a shape the calls refuse, B Co ceil(H W / 1024) above 2^31 - 1 included. */
size_t halo_pool_fold_workspace_bytes(int64_t B, int64_t Co, int64_t H, int64_t W);
int halo_pool_fold_table(const float *w, const float *v, float *T, int64_t B, int64_t Co, int64_t Cg, int64_t c_off, int64_t row_stride,
                         void *stream);
int halo_pool_fold_affine_relu_fwd(const float *z, const float *T, const float *scale, const float *shift, float *y, int64_t B, int64_t Co,
                                   int64_t H, int64_t W, void *stream);
int halo_pool_fold_affine_relu_bwd(const float *g, const float *y, const float *scale, float *g_z, double *g_T, int64_t B, int64_t Co,
                                   int64_t H, int64_t W, void *workspace, size_t workspace_bytes, void *stream);

/* ---- frozen norm + ReLU + 3x3 / stride 2 / padding 1 max-pool: the stem behind its convolution (halo_amd/norm.py) ----
 *  x, g_x (B, C, H, W) f32 dense NCHW; out, g (B, C, OH, OW) f32 and tap (B, C, OH, OW) u8 dense, OH = (H - 1) / 2 + 1,
 *  OW = (W - 1) / 2 + 1; scale, shift (C) f32.
 *    z          = relu(fl(fl(x scale[c]) + shift[c]))               halo_affine_relu_fwd's statements and bits; never stored
 *    out[oh,ow] = the recorded tap's z of the window of rows 2oh-1 .. 2oh+1 and columns 2ow-1 .. 2ow+1, taps inside the map only,
 *                 scanned row-major from -inf, a tap taken if (v > max || isnan(v)): the first of equal values, the last NaN
 *    tap[oh,ow] = 3 kh + kw of the recorded tap (its place in the window, 0..8), or 9 when its z <= 0 (no gradient passes)
 *    g_x[h,w]   = fl(S scale[c]),  S = the f32 sum of g[oh,ow] over the windows whose tap names (h, w), ascending oh, then
 *                 ascending ow, from +0: one to four terms, no atomics, the same bits on every call and every stream
 *  The bits of `max_pool2d(relu_(x * scale + bias), 3, 2, 1)` and of the gather form of its autograd backward; a NaN z lets the
 *  gradient through.  fwd: tap == NULL: the codes are not kept (no backward follows).  The backward reads g, tap and scale only.
 *  out and tap must not overlap x; g_x must not overlap g or tap.  W % 4 == 0 with x and g_x 16-byte, out 8-byte and tap 2-byte
 *  aligned runs 16-byte accesses of x and g_x, anything else one element per lane: same statements, same bits.  HALO_E_ARG: an
 *  empty shape or a missing pointer; HALO_E_UNSUPPORTED: H W above 2^31 - 1025 or more than 2^31 - 1 workgroups. */
int halo_maxpool_affine_relu_fwd(const float *x, const float *scale, const float *shift, float *out, uint8_t *tap, int64_t B, int64_t C,
                                 int64_t H, int64_t W, void *stream);
int halo_maxpool_affine_relu_bwd(const float *g, const uint8_t *tap, const float *scale, float *g_x, int64_t B, int64_t C, int64_t H,
                                 int64_t W, void *stream);

/* ---- the optimiser step of one param group: RiemannianSGD on the Euclidean manifold and torch.optim.SGD (halo_amd/optim.py) ----
 *  One call covers a list of tensors that share their hyper-parameters.  Per tensor: p, g, buf dense arrays of n elements of dtype
 *  HALO_F32 | HALO_F64 (both may occur in one list), and `first`: this parameter has no momentum buffer yet.  In T = the tensor's
 *  dtype, every scalar cast to T once:
 *    HALO_SGD_GEOOPT  g1 = fma(wd, p, g), always (wd = 0 with p = +-inf gives NaN), stored to g;
 *                     momentum > 0: b0 = first ? g : buf (the raw gradient, no clone pass), b1 = fma(1 - dampening, g1, fl(b0 momentum))
 *                     stored to buf; nesterov: g2 = fma(momentum, b1, g1) stored to g, d = g2; else d = b1;  momentum <= 0: d = g1;
 *                     p = fl(p + fl(-lr d))                            two roundings
 *    HALO_SGD_TORCH   g1 = wd != 0 ? fma(wd, p, g) : g, g is not written;
 *                     momentum != 0: b1 = first ? g1 : fma(1 - dampening, g1, fl(buf momentum)) stored to buf;
 *                     d = nesterov ? fma(momentum, b1, g1) : b1;  momentum == 0: d = g1;
 *                     p = fma(-lr, d, p)                               one rounding
 *  The bits of geoopt.optim.RiemannianSGD.step for plain parameters and of torch.optim.SGD.step (maximize = False), denormals kept.
 *  buf is neither read nor written without momentum (it may be NULL) and not read on a first use.  p, g and buf must not overlap.
 *  A workgroup owns one chunk of one tensor; the table of a launch travels in the kernel arguments, `cap` tensors per launch, so
 *  the call launches ceil(tensors of n > 0 / cap) kernels, allocates nothing, reads nothing back, never synchronises and keeps no
 *  pointer: a host many steps ahead is fine.  A tensor whose three pointers are 16-byte aligned moves 16 bytes per lane, any
 *  other one element per lane: same statements, same bits.  Plain stores, no atomics, no LDS.  Every check comes before the first
 *  launch.  HALO_E_ARG: a descriptor of another size, an unknown mode, n < 0, a missing pointer of a tensor with n > 0, nesterov
 *  without momentum; HALO_E_UNSUPPORTED: n >= 2^31, another dtype.
 *  halo_sgd_plan_limits: the chunk's elements and cap.  halo_sgd_plan: the launch each tensor of a size list falls in (-1: n = 0,
 *  in none) and its first block there; its blocks follow one another, block c of a tensor covers elements c chunk ..
 *  min(n, (c + 1) chunk) - 1, and a launch's tensors fill its grid in list order.  Both are pure host functions. */
#define HALO_SGD_GEOOPT 0
#define HALO_SGD_TORCH 1
typedef struct halo_sgd_tensor {
    void *p;
    void *g;
    void *buf;
    int64_t n;
    int dtype;
    int first;
} halo_sgd_tensor;
typedef struct halo_sgd_args {
    size_t struct_bytes;            /* sizeof(halo_sgd_args) as the caller compiled it; anything else: HALO_E_ARG */
    int mode;
    int nesterov;
    double lr;
    double momentum;
    double dampening;
    double weight_decay;
    int64_t count;
    const halo_sgd_tensor *tensors; /* host array of `count` entries, read during the call only */
} halo_sgd_args;
int halo_sgd_plan_limits(int64_t *chunk, int64_t *cap);
int halo_sgd_plan(const int64_t *n, int64_t count, int64_t *launch_of, int64_t *first_block, int64_t *launches);
int halo_sgd_step(const halo_sgd_args *a, void *stream);

/* ---- measurement helpers (HIP events in the same runtime the kernels are launched through) ---- */
void *halo_event_create(void);
int halo_event_record(void *event, void *stream);
int halo_event_elapsed_ms(void *start, void *stop, float *ms);   /* synchronises on `stop` */
int halo_event_destroy(void *event);

#ifdef __cplusplus
}
#endif
#endif /* HALO_HIP_H */

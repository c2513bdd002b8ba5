/* gsrast.h -- C ABI of libgsrast.so, the MI355X-native differentiable 3D Gaussian splatting rasterizer.
 *
 * This is the boundary a binding of the reference would target. The reference (DreamScene) reaches its
 * rasterizer through the Python package `diff_gaussian_rasterization` (scene_gaussian.py:11-12), whose
 * native half is `diff_gaussian_rasterization._C` (un-vendored CUDA, README.md:47-51). The entry points below
 * replace that native half one for one:
 *
 *   gsr_forward_project + gsr_forward_render   <->  _C.rasterize_gaussians            (the forward the
 *        autograd.Function behind GaussianRasterizer.forward calls; call sites scene_gaussian.py:637-646,
 *        861-870, 1012-1021; outputs image / radii / depth_alpha [/ important_score], :637, :1012)
 *   gsr_backward                               <->  _C.rasterize_gaussians_backward   (invoked by
 *        loss.backward(), training/object_trainer.py:382, training/scene_trainer.py:881)
 *   GsrView                                    <->  GaussianRasterizationSettings     (12 fields,
 *        scene_gaussian.py:951-964)
 *
 * Rules of the boundary:
 *   - plain C: POD structs of raw DEVICE pointers and sizes, no torch / C++ types;
 *   - the caller owns every buffer (inputs, outputs, state saved for backward, scratch); the library
 *     allocates nothing that outlives a call and keeps no mutable global state: re-entrant, any thread;
 *   - all work is enqueued on the caller's stream (a hipStream_t passed as void*); the only host
 *     synchronisation is inside gsr_forward_project (it returns the data-dependent pair count N);
 *   - every entry point returns 0 or a negative GSR_E* code, never throws; gsr_strerror() explains;
 *   - fp32 contiguous tensors only; layouts are those of the reference call sites, quoted per field.
 */
#ifndef GSRAST_H
#define GSRAST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_VERSION 1
#define GSR_TILE 16 /* 16x16 pixel tiles */

enum {
  GSR_OK = 0,
  GSR_EINVAL = -1,    /* bad shape / null pointer / unsupported SH degree            */
  GSR_ECAPACITY = -2, /* pair count N does not fit the 32-bit list positions         */
  GSR_EHIP = -3,      /* a HIP call failed; gsr_last_hip_error() has the hipError_t  */
  GSR_ESCRATCH = -4   /* scratch buffer too small for this (P, N)                    */
};

/* Per-view configuration == GaussianRasterizationSettings (scene_gaussian.py:951-964). The four tensors
 * stay on the device exactly as RCamera holds them (utils/cam_utils.py:196-210): row-vector convention,
 * i.e. viewmatrix is the TRANSPOSED world-to-camera matrix, projmatrix = viewmatrix @ projection^T. */
typedef struct GsrView {
  int32_t P;            /* number of Gaussians                                                        */
  int32_t sh_stride;    /* K: SH coefficients stored per Gaussian = (max_sh_degree+1)^2; 0 if no SHs   */
  int32_t sh_degree;    /* D: active degree 0..3 (raster_settings.sh_degree)                           */
  int32_t image_height, image_width;
  float tanfovx, tanfovy, scale_modifier;
  int32_t prefiltered;  /* accepted for API parity; no effect (frustum test always runs)               */
  int32_t score_mode;   /* important_score weight: 0 = opacity per contributing (pixel,splat), 1 = alpha*T, 2 = RAW COUNTS:
                           the number of contributing pixels as uint32 in the (zero-initialised) score buffer, no opacity
                           factor -- for callers that add many views into one buffer and weight once at the end (mode 0
                           counts the same way internally, integer atomics, and multiplies by the opacity itself) */
  const float* bg;         /* device f32[3]  */
  const float* viewmatrix; /* device f32[16] */
  const float* projmatrix; /* device f32[16] */
  const float* campos;     /* device f32[3]  */
  const float* dynamic;    /* NULL, or device f32[4] = (tanfovx, tanfovy, sh_degree, reserved): when set, the kernels take
                              these three from HERE at the time they run instead of the by-value fields above -- with bg /
                              viewmatrix / projmatrix / campos already being device tensors, every per-camera quantity then
                              lives in device memory and a captured graph of a step (hipGraph) can be replayed with new
                              cameras by rewriting that memory (gsr_pack_views). The by-value fields must still be valid
                              (they are what the host-side checks see) */
} GsrView;

/* ---- gather-free multi-model input with the activations fused into K1 / K8 -------
 * `scene_render` (scene_gaussian.py:673-893) concatenates the leaf tensors of every visible GaussianModel with
 * torch.cat on every call (:753-843), after running their activations (gs_renderer.py:464-488: exp, normalize,
 * sigmoid, cat(features_dc, features_rest)) and, when training, the noise augmentations (:844-852). A GsrScene hands
 * the RAW leaf tensors of up to GSR_MAX_MODELS models to K1 / K8 instead: Gaussian i of the concatenated index space
 * is row i - first(m) of model m, nothing is copied, and culled Gaussians never touch their SH rows. */
#define GSR_MAX_MODELS 16
typedef struct GsrModel {      /* leaf tensors of one GaussianModel (gs_renderer.py:185-203), all on the device */
  int32_t count;               /* Gaussians in this model                                                   */
  int32_t reserved_;
  const float* xyz;            /* [count,3]      _xyz                                                      */
  const float* scaling;        /* [count,3]      _scaling  (log scale;   activation exp,       :465-466)    */
  const float* rotation;       /* [count,4]      _rotation (raw w,x,y,z; activation normalize, :469-470)    */
  const float* opacity;        /* [count,1]      _opacity  (logit;       activation sigmoid,   :487-488)    */
  const float* features_dc;    /* [count,1,3]    _features_dc                                               */
  const float* features_rest;  /* [count,K-1,3]  _features_rest (NULL if K == 1)                            */
} GsrModel;
typedef struct GsrScene {
  int32_t n_models;            /* 1..GSR_MAX_MODELS; GsrView.P must equal the sum of the counts, sh_stride = K */
  int32_t reserved_;
  GsrModel models[GSR_MAX_MODELS];
  const float* scale_noise;    /* NULL or [P,3]   N(0,1) samples: scales <- max(0, s + n * (sqrt(0.2) * s / 4)) (:849-852) */
  const float* sh_noise;       /* NULL or [P,K,3] N(0,1) samples: shs <- shs + n * (sqrt(0.2) * shs)           (:844-847) */
  float* scales_out;           /* NULL or [P,3]: the activated (and augmented) scales scene_render returns (:892) */
  float* rotations_out;        /* NULL or [P,4]: normalised quaternions (parity tests)                        */
  float* opacities_out;        /* NULL or [P]:   sigmoid(opacity)        (parity tests)                        */
  /* Seeded noise (SEMANTICS.md "Seeded noise"): the samples a tensor above would hold are computed inside K1 and again inside
   * K8 as a pure function of (noise_seed, stream, concatenated Gaussian index, element) -- no tensor exists. All zero: today's
   * meaning. A flag together with ITS tensor pointer, or an unknown flag bit, is GSR_EINVAL before any launch; one flag
   * together with the other noise's tensor is legal. The views of a batched call share one K1 / K8 pass when the scenes that
   * set flags agree on noise_seed and their noise_stream_dev, if given, are consecutive words (view k + 1 reads the word after
   * view k's); otherwise K1 / K8 run view by view, with the same results. */
  uint64_t noise_seed;
  const uint32_t* noise_stream_dev; /* NULL, or device u32[1] read when the kernels run (forward AND backward) */
  uint32_t noise_stream;            /* used when noise_stream_dev is NULL */
  uint32_t noise_flags;             /* GSR_NOISE_*: that noise comes from the generator */
} GsrScene;
#define GSR_NOISE_SCALES 1u
#define GSR_NOISE_SHS    2u
/* Gradients w.r.t. the RAW leaf tensors of each model (same shapes). NULL entries are skipped. */
typedef struct GsrModelGrads {
  float *xyz, *scaling, *rotation, *opacity, *features_dc, *features_rest;
} GsrModelGrads;
typedef struct GsrSceneGrads {
  GsrModelGrads models[GSR_MAX_MODELS];
  const float* dL_dscales_out; /* NULL or [P,3]: gradient arriving through GsrScene.scales_out (the trainers put a loss
                                  on the returned scales, object_trainer.py:378-379); chained into `scaling` */
} GsrSceneGrads;

/* Inputs of GaussianRasterizer.forward (scene_gaussian.py:1012-1021). Exactly one of shs / colors_precomp and
 * exactly one of (scales, rotations) / cov3D_precomp is non-NULL -- or `scene` is set and all of them are NULL. */
typedef struct GsrGaussians {
  const float* means3D;        /* [P,3]                                            */
  const float* opacities;      /* [P] (the reference passes [P,1])                  */
  const float* shs;            /* [P,K,3] coefficient-major (gs_renderer.py:480-484) */
  const float* colors_precomp; /* [P,3]                                            */
  const float* scales;         /* [P,3] post-activation                            */
  const float* rotations;      /* [P,4] (w,x,y,z), already normalised              */
  const float* cov3D_precomp;  /* [P,6] [xx,xy,xz,yy,yz,zz] (gs_renderer.py:79-88)  */
  const GsrScene* scene;       /* host pointer or NULL: raw multi-model input (see GsrScene) */
} GsrGaussians;

/* Projected per-Gaussian state: written by gsr_forward_project, read by render and backward (save it).
 * splat holds 12 floats per Gaussian as three float4 rows q0,q1,q2 (row-major [P][12]):
 *   q0 = (x_pix, y_pix, conic_a, conic_b)   q1 = (conic_c, opacity, view_depth, r)   q2 = (g, b, tau, 0)
 * (tau = 2 ln(255 opacity), slightly inflated: the level of the conic form inside which alpha can reach 1/255;
 *  < 0 if nowhere; used only to skip work)
 * Rows of culled Gaussians (radii == 0) are left unwritten. */
typedef struct GsrGeom {
  float* splat;            /* [P,12], 16-byte aligned */
  int32_t* radii;          /* [P]  screen radius in pixels, 0 = culled (output `radii`)            */
  uint32_t* tiles_touched; /* [P]  number of 16x16 tiles overlapped                               */
  uint32_t* block_offsets; /* [gsr_num_blocks(P)+8], 8-byte aligned; grids of more than 256 x 256 tiles only: exclusive
                              scan of the tile counts of each run of 256 Gaussians IN DEPTH ORDER, [nb] = N (low 32 bits) */
  void* scratch;           /* gsr_project_scratch_bytes(P) bytes, 256-byte aligned: depth-sort buffers, column counts
                              and the device-side counts (N, visible Gaussians). Must stay alive until
                              gsr_forward_render has been enqueued; not needed for backward                       */
  size_t scratch_bytes;
  uint32_t* sorted_idx;    /* OUT (set by gsr_forward_project*), OPAQUE: one of the depth sort's two value buffers inside
                              `scratch`, handed from gsr_forward_project* to gsr_forward_render*. It holds the Gaussian
                              indices in (depth bits, index) order ONLY when the sort's last pass moved keys; a last pass
                              that is the identity (the top byte of one object's depths) is skipped, the order then lives
                              in the OTHER buffer and a flag word in `scratch` says so -- the library's consumers read the
                              flag, a caller must not read this pointer (the depth order is observable through
                              GsrBinning.point_list, whose entries are in (tile, depth bits, index) order)           */
} GsrGeom;

/* Tile binning. point_list / ranges are saved for backward; the rest is scratch for the forward only. */
typedef struct GsrBinning {
  uint32_t* point_list; /* [N] Gaussian index per (tile, depth)-sorted pair                         */
  uint32_t* ranges;     /* [tiles,2] (start,end) into point_list; (0,0) for an empty tile            */
  uint32_t* tile_work;  /* [tiles + 2 + 2*bwd_items_cap] u32: forward work list (tile ids, heaviest first) followed by
                           the number of non-empty tiles, then the backward's (tile, segment) item list; written by
                           the forward and by the backward: keep it with the saved state                          */
  uint32_t bwd_items_cap; /* capacity of the backward item list: >= n_pairs / seg_len + tiles                     */
  uint32_t seg_len;       /* list entries per checkpoint of the forward = per work item of the backward: 256 (also: 0), 128
                             or 64. A backward item is a serial recurrence over its entries, so a launch cannot end before its
                             longest item has (256 entries: 65-90 us on MI355X); a launch with little total work (one view, a
                             small scene) finishes sooner with shorter items, a large one pays for the extra checkpoints and
                             prologues. Same value for the forward and the backward of a view; views of one batched
                             call that differ in it are composited by one launch each instead of one for all; fwd_mode 1
                             requires 256. Sizes: bwd_items_cap (above), GsrImages.ckpt */
  uint64_t* keys_sorted;/* [N] optional: receives the sorted 64-bit keys (tile<<32 | depth bits); may be NULL */
  void* scratch;        /* gsr_sort_scratch_bytes(N, tiles) bytes, 256-byte aligned                   */
  size_t scratch_bytes;
  int32_t count_on_device; /* 0: n_pairs passed to gsr_forward_render is the exact N (after the synchronous
                              gsr_forward_project). 1: capacity mode -- n_pairs is the CAPACITY of point_list /
                              scratch; the kernels take the true N from the device (GsrGeom.block_offsets tail)
                              and clamp it to the capacity; the caller compares N with the capacity afterwards
                              and re-runs gsr_forward_render with larger buffers if it did not fit            */
  int32_t fwd_mode;        /* forward compositing variant: 0 = four 8x8-quarter work items per tile, 4 lanes per pixel
                              (few / deep tiles); 1 = one work item per tile, one pixel per lane (thousands of
                              shallow tiles). Same semantics; a performance choice                 */
  uint32_t* stats_host;    /* optional page-locked (device-visible, e.g. hipHostMalloc / torch pinned) host word: a
                              kernel stores the number of non-empty tiles of this view there, the statistic a caller
                              can base the next call's fwd_mode on                                                */
} GsrBinning;

/* Per-pixel outputs (scene_gaussian.py:1012,1023) and the per-pixel state backward needs. */
typedef struct GsrImages {
  float* color;           /* [3,H,W]                                                         */
  float* depth_alpha;     /* [2,H,W]: plane 0 = sum z_i a_i T_i, plane 1 = sum a_i T_i        */
  float* final_T;         /* [H,W] transmittance after the last contributor                  */
  uint32_t* n_contrib;    /* [H,W] 1-based list position of the last contributor             */
  uint32_t* tile_depth;   /* [tiles] max of n_contrib over the tile (written by forward, read by backward) */
  float* ckpt;            /* [n_pairs/seg_len + 1][6][256] per-pixel prefix state (T, C rgb, depth, alpha) at the
                             seg_len-entry boundaries of the tile lists (slot = absolute list position / seg_len;
                             GsrBinning.seg_len), written by the forward as far as it composites, read by the backward.
                             NULL = FORWARD ONLY: the forward writes no checkpoints (inference renders, importance
                             scores: ~5 % of K6 and the largest region of the saved state); gsr_backward* then refuses
                             the view with GSR_EINVAL */
  float* important_score; /* [P], or NULL (score_flag False). MUST BE ALL ZERO ON ENTRY: K6 adds to it. score_mode 1: float
                             sums (several views may add into one buffer); score_mode 2: u32 pixel counts (bit patterns; several
                             views may add into one buffer, the caller converts); score_mode 0: u32 counts converted IN PLACE
                             to opacity x count at the end of the call -- one buffer per view (views of one batched call that
                             share a buffer are refused with GSR_EINVAL: the second conversion would read the first one's
                             floats as counts)                                                                             */
} GsrImages;

typedef struct GsrImageGrads {
  const float* dL_dcolor;       /* [3,H,W] */
  const float* dL_ddepth_alpha; /* [2,H,W] */
} GsrImageGrads;

/* Gradients w.r.t. the forward inputs. NULL = not wanted (must be NULL where the input was NULL).
 * Every non-NULL output is fully overwritten (zeros for culled Gaussians) unless `accumulate`. dL_dview / dL_dproj /
 * dL_dcampos treat viewmatrix, projmatrix and campos as three independent inputs. */
typedef struct GsrGrads {
  float* dL_dmeans3D;   /* [P,3]                                                                     */
  float* dL_dmeans2D;   /* [P,3] (d/d ndc_x, d/d ndc_y, 0): what lands in viewspace_points.grad     */
  float* dL_dopacities; /* [P]                                                                       */
  float* dL_dshs;       /* [P,K,3]                                                                   */
  float* dL_dcolors;    /* [P,3]                                                                     */
  float* dL_dscales;    /* [P,3]                                                                     */
  float* dL_drotations; /* [P,4]                                                                     */
  float* dL_dcov3D;     /* [P,6]                                                                     */
  float* dL_dview;      /* [16] or NULL; zero-initialised by the caller                              */
  float* dL_dproj;      /* [16] or NULL; zero-initialised by the caller                              */
  float* dL_dcampos;    /* [3]  or NULL; zero-initialised by the caller                              */
  float* partials;      /* scratch [P,32] 32-bit words (128 B / Gaussian, 16-byte aligned) = 16 f64 per Gaussian, 12 used:
                           sum q u, sum q v, sum q u^2, sum q u v, sum q v^2, dL/dopacity, dL/dr, dL/dg, dL/db, dL/ddepth
                           (the last two as two half-wave sums each: doubles 8-11). K7 reduces a splat's sums over the 64
                           pixels of a wave in fp32 in a fixed order and adds the wave's result ACROSS waves in double
                           (one global_atomic_add_f64 instruction, 12 lanes, one 128-byte line). A double holds the sum of
                           fp32 addends exactly while their exponents span less than 2^29: within that span the order in
                           which K7's workgroups arrive does not show in the gradients (bit-reproducible backward); an
                           addend more than 2^29 below the running sum can move the double by one unit of its last place,
                           which reaches the fp32 result only on a rounding tie (about one value in 10^9)            */
  int32_t accumulate;   /* 0: overwrite the parameter gradients; 1: ADD this view's gradients to what the buffers
                           hold (device-side sum over the views of one optimizer step). dL_dmeans2D is per view
                           and always overwritten; dL_dview/proj/campos always accumulate                     */
  int32_t reserved_;
  /* SURVEY.md section 8(f) rank 3, densification statistics fused into K8 (all three NULL or all three set, [P] fp32):
   * what the trainers do after backward with the view's radii / visibility_filter / viewspace_points.grad
   * (object_trainer.py:386-390, gs_renderer.py:1061-1065), for the visible Gaussians (radii > 0) of THIS view:
   *   max_radii2D = max(max_radii2D, radii); xyz_gradient_accum += ||dL_dmeans2D[:2]||; denom += 1              */
  float* stat_max_radii2D;
  float* stat_xyz_gradient_accum;
  float* stat_denom;
  const GsrSceneGrads* scene; /* host pointer; required iff GsrGaussians.scene was given: the parameter gradients go
                                 to the models' raw leaves and dL_dmeans3D/scales/rotations/opacities/shs must be NULL */
  uint64_t* reached_mask;     /* NULL or device u64[(P + 63) / 64]: bit i % 64 of word i / 64 is set when Gaussian i MAY have
                                 received a non-zero parameter gradient from this call -- the rows a multi-GPU gradient
                                 exchange has to send (everything behind the opaque front layers of
                                 an object is exactly zero). K8 classifies the Gaussians K7 reached anyway (its sparse form);
                                 forms of K8 that do not classify set every bit. accumulate = 0: the words are overwritten;
                                 accumulate = 1: OR-ed into (the union over the views added to the gradient buffers) */
  uint64_t* reach;            /* NULL or device scratch u64[(P + 63) / 64] next to `partials`: K7 sets bit i % 64 of word
                                 i / 64 for the Gaussians it composited into this view, so that K8 finds them without
                                 reading the [P,12] sums of every visible Gaussian (96 MB of the 4-view step at 500 k
                                 Gaussians, of which 15 MB are non-zero): one word per 64 Gaussians and view */
  int32_t scratch_clean;      /* 0: `partials` (and `reach`) hold anything on entry -- the library clears them first -- and
                                 anything on return. 1 (needs `reach`): the caller keeps both buffers between calls and
                                 guarantees they are ALL ZERO on entry; the library leaves them all zero on return, and
                                 launches no clear before K7: K8's views forms without a scene zero the rows and marks they
                                 consume, after its other forms the library clears the scratch. A call that returns an
                                 error leaves them undefined.                                                          */
  int32_t zero_outside;       /* What the caller KNOWS about the outputs as they are on entry (accumulate = 0 only; needs reached_mask,
                                 which must then hold the mask the previous writer of these buffers left):
                                 bit 0: every row of the summed-gradient outputs (dL_dmeans3D / dL_dopacities / dL_dshs / dL_dscales
                                        / dL_drotations) OUTSIDE reached_mask is zero -- i.e. the buffers hold what the previous
                                        gsr_backward* call with these same buffers and this same reached_mask wrote, untouched;
                                 bit 1: the same for the per-view outputs of every view of the call (dL_dmeans2D, per-view dL_dscales).
                                 The sparse form of K8 then writes only the rows this call reaches and zeros over the rows the mask
                                 names but this call does not reach, instead of zeros over everything nothing reached (84 % of
                                 the rows at 500 k Gaussians @1024^2: 118 + 24 MB per 4-view step). Results identical. The other
                                 forms of K8 ignore it (they write every row and set every bit of reached_mask). 0: nothing known. */
} GsrGrads;

/* Optional per-stage timing with HIP events on the caller's stream (bench.py uses it for `roofline`). */
enum {
  GSR_STAGE_PREPROCESS = 0, GSR_STAGE_SCAN, GSR_STAGE_DUPLICATE, GSR_STAGE_SORT, GSR_STAGE_RANGES,
  GSR_STAGE_RENDER_FWD, GSR_STAGE_RENDER_BWD, GSR_STAGE_PREPROCESS_BWD, GSR_STAGE_COUNT
};
typedef struct GsrProfile GsrProfile;
GsrProfile* gsr_profile_create(void);
void gsr_profile_destroy(GsrProfile*);
/* Record only the stages whose bit (1u << GSR_STAGE_*) is set; default all. */
void gsr_profile_set_stage_mask(GsrProfile*, uint32_t mask);
/* Record only one of every `every` occurrences of each stage (bounds the cost of the two event records per occurrence
 * inside a timed region); counts[] of gsr_profile_collect reports how many were recorded. */
void gsr_profile_set_sampling(GsrProfile*, uint32_t every);
/* Synchronises the recorded events and ADDS each stage's elapsed ms into ms[GSR_STAGE_COUNT] and the
 * number of recordings into counts[]; then clears the recordings. */
int gsr_profile_collect(GsrProfile*, double* ms, int64_t* counts);

int gsr_version(void);
const char* gsr_strerror(int code);
int gsr_last_hip_error(void); /* thread-local hipError_t of the last GSR_EHIP on this thread */

size_t gsr_project_scratch_bytes(int32_t P);
size_t gsr_sort_scratch_bytes(uint64_t n_pairs, uint32_t n_tiles);
uint32_t gsr_num_tiles(int32_t image_height, int32_t image_width);
uint32_t gsr_num_blocks(int32_t P); /* entries of GsrGeom.block_offsets minus one */

/* K1 projection (cull, cov3D, EWA cov2D, conic, radius, tile rect, SH colour), stable depth sort of the P
 * Gaussians, scan of the depth-ordered tile counts.
 * Synchronises `stream` once and stores the pair count N in *n_pairs_host (ordinary host memory). */
int gsr_forward_project(const GsrView*, const GsrGaussians*, GsrGeom*, uint64_t* n_pairs_host, void* stream,
                        GsrProfile* prof);
/* Same work, no host synchronisation: N lands in *n_pairs_pinned (must be page-locked, device-visible host memory:
 * hipHostMalloc / torch pinned; a kernel stores it there) and is valid once the caller has waited for the work enqueued
 * so far. Used with capacity mode
 * (GsrBinning.count_on_device) so that a whole forward is enqueued without draining the GPU.
 * The word holds GSR_N_PENDING from the call until a kernel has stored N (P == 0: 0 at once). On grids of at most 256 x 256
 * tiles with P < 2^24 the count is stored EARLY -- by the first workgroup of the depth sort's first pass, i.e. after K1 and
 * one histogram launch, long before the sort and the column counts are over (stored once per call: a caller that has
 * read it may re-arm the word for its next call at once): a caller may poll the word (relaxed loads of page-locked memory)
 * instead of waiting for the stream, and fall back to the stream when it still reads GSR_N_PENDING after the enqueued work
 * has finished. */
#define GSR_N_PENDING UINT64_MAX
int gsr_forward_project_async(const GsrView*, const GsrGaussians*, GsrGeom*, uint64_t* n_pairs_pinned, void* stream,
                              GsrProfile* prof);

/* The same for n_views views of the SAME Gaussians (the C_batch_size views of one optimizer step,
 * object_trainer.py:302-382): the launch-latency-bound depth sorts and column counts of all views go through each
 * launch together. Requirements: equal P / image size / sh_stride, and the views' GsrGeom.scratch buffers equally
 * spaced (geoms[k].scratch == geoms[0].scratch + k * stride, stride a multiple of 256). n_views > 1 also requires a grid
 * of at most 256 x 256 tiles (image at most 4096 x 4096) and P < 2^24: anything else is GSR_EINVAL from the argument
 * checks, with nothing enqueued and n_pairs_pinned untouched (render such views one by one). n_views == 1 accepts any
 * size; beyond those limits its count arrives by a device-to-host copy enqueued behind the projection.
 * gaussians[k] are the inputs of view k: identical pointers for every view except `scales`, which may be a different
 * tensor per view (the trainers add fresh noise to the activated scales of every view, scene_gaussian.py:1004-1008);
 * with a `scene`, every view has its own GsrScene holding the SAME models and its own noise samples / scales_out.
 * K1 runs once over all views (parameter rows read once) for shs or scene input with K in {1,4,9,16}.
 * No host synchronisation: n_pairs_pinned[n_views] (page-locked, device-visible) receives the counts straight from a
 * kernel and is valid once the work enqueued so far has finished (GSR_N_PENDING until then; pollable as described at
 * gsr_forward_project_async, but stored at the END of the projection here -- the early store costs the batched launches
 * more than their GPU-bound callers gain).
 * The views then continue with gsr_forward_render_batch (or each with its own gsr_forward_render). */
#define GSR_MAX_BATCH_VIEWS 16
#define GSR_PARTIAL_WORDS 32   /* 32-bit words per Gaussian of GsrGrads.partials (16 doubles) */
int gsr_forward_project_batch(int32_t n_views, const GsrView* views, const GsrGaussians* gaussians /* [n_views] */,
                              GsrGeom* geoms, uint64_t* n_pairs_pinned, void* stream, GsrProfile* prof);

/* Camera block of n_views views in one launch: packed[k] = (bg[3], 0, viewmatrix[16], projmatrix[16], campos[3], 0,
 * tanfovx, tanfovy, sh_degree, 0) = GSR_PACKED_VIEW_FLOATS floats (every tensor 16-byte aligned), gathered from the
 * views' device tensors and by-value fields. A caller that replays a captured step points the GsrView tensors of the
 * CAPTURED views into such a block (bg = row, viewmatrix = row + 4, projmatrix = row + 20, campos = row + 36,
 * dynamic = row + 40) and refreshes it with this call from the settings of the step at hand. packed must be 16-byte
 * aligned; no host synchronisation. */
#define GSR_PACKED_VIEW_FLOATS 44
int gsr_pack_views(int32_t n_views, const GsrView* views, float* packed, void* stream);
/* The same launch also stores the views' noise stream ids: streams_dev[k] = streams[k] (streams: n_views HOST words, taken by
 * value with the call; streams_dev: n_views device words, 4-byte aligned -- what the GsrScene.noise_stream_dev of a captured
 * step's views point at, view k at word k). A caller that replays a captured scene step refreshes cameras and ids with this
 * one call, at the forward only: K8 reads the words again. streams or streams_dev NULL: exactly gsr_pack_views. */
int gsr_pack_views_streams(int32_t n_views, const GsrView* views, const uint32_t* streams, float* packed,
                           uint32_t* streams_dev, void* stream);

/* K3 pair emission in depth order, K4 stable tile sort, K5 tile ranges, K6 front-to-back compositing. */
int gsr_forward_render(const GsrView*, const GsrGeom*, uint64_t n_pairs, GsrBinning*, GsrImages*, void* stream,
                       GsrProfile* prof);

/* The same for n_views views projected together (gsr_forward_project_batch), all with buffers for n_pairs pairs:
 * binning per view, the heaviest-first work lists of all views in one launch, then K6 per view. */
int gsr_forward_render_batch(int32_t n_views, const GsrView* views, const GsrGeom* geoms, uint64_t n_pairs,
                             GsrBinning* binnings, GsrImages* images, void* stream, GsrProfile* prof);

/* K7 reverse traversal of every pixel's blend list + K8 chain rule to the inputs. */
int gsr_backward(const GsrView*, const GsrGaussians*, const GsrGeom*, const GsrBinning*, const GsrImages*,
                 const GsrImageGrads*, GsrGrads*, void* stream, GsrProfile* prof);

/* Backward of n_views views of the SAME Gaussians (forwarded together or not): K7 per view, then ONE K8 pass that reads
 * every parameter row once, loops over the views and writes the summed parameter gradients once (supported for shs with
 * K in {1,4,9,16} + scales/rotations without camera gradients; other combinations run K8 view by view with the same
 * result). All arrays have n_views entries. Per view: outs[k].partials and outs[k].dL_dmeans2D (and dL_dview / dL_dproj /
 * dL_dcampos, stat_*); the parameter gradient pointers and `accumulate` are taken from outs[0] (give every
 * entry the same ones): the SUM over the views is written (accumulate = 0) or added (accumulate = 1) there. The
 * densification statistics are updated for the views whose entry sets the stat_* pointers (all such entries must name
 * the same three tensors) -- the reference's trainers count the LAST view of a step only (object_trainer.py:386-390) --
 * once per such view that saw the Gaussian. With per-view `scales` (see gsr_forward_project_batch)
 * every outs[k].dL_dscales is its own [P,3] buffer and receives view k's scale gradient (never accumulated). With a
 * scene every outs[k].scene names the SAME model gradient tensors (summed over the views) and its own dL_dscales_out. */
int gsr_backward_views(int32_t n_views, const GsrView* views, const GsrGaussians* gaussians /* [n_views] */,
                       const GsrGeom* geoms,
                       const GsrBinning* binnings, const GsrImages* images, const GsrImageGrads* image_grads,
                       GsrGrads* outs, void* stream, GsrProfile* prof);

/* ---- replacement of `simple_knn._C.distCUDA2` (gs_renderer.py:9, 590-593) --------
 * out[i] = mean of the squared distances from points[i] to its 3 nearest other points (exact; FLT_MAX stands in
 * for neighbours that do not exist when n < 4). points [n,3] fp32, out [n] fp32, both on the device; scratch:
 * gsr_knn_scratch_bytes(n) bytes, 256-byte aligned. Enqueued on `stream`, no host synchronisation. */
size_t gsr_knn_scratch_bytes(int32_t n);
int gsr_knn_mean_dist2(const float* points, int32_t n, float* out, void* scratch, size_t scratch_bytes, void* stream);

/* ---- the optimizer of the post-raster epilogue ----------------------------------
 * One launch of torch.optim.Adam's update (no amsgrad / weight decay) over all parameter groups of a model
 * (gs_renderer.py:615-653: Adam(l, lr=0.0, eps=1e-15), six groups with their own lr). All pointers are device fp32,
 * 16-byte aligned; `step` is the 1-based step count (bias correction); zero_grad != 0 clears the gradients in the same
 * pass. The densification statistics of that epilogue are fused into K8 (GsrGrads.stat_*). */
#define GSR_MAX_ADAM_GROUPS 32
typedef struct GsrAdamGroup {
  float* param;        /* [numel] updated in place        */
  float* grad;         /* [numel] (cleared if zero_grad)   */
  float* exp_avg;      /* [numel] first moment             */
  float* exp_avg_sq;   /* [numel] second moment            */
  int64_t numel;
  float lr;
  float reserved_;
} GsrAdamGroup;
int gsr_adam_step(const GsrAdamGroup* groups, int32_t n_groups, int32_t step, double beta1, double beta2, double eps,
                  int32_t zero_grad, void* stream);

/* ---- device side of the sparse gradient-exchange formats -------------------------------------
 * One view per GPU, the only exchange of a step is the sum of the ranks' parameter gradients (the reference sums the
 * C_batch_size views of a step in one process, training/object_trainer.py:302-382). K8 leaves the rows that can be non-zero
 * as a bitmap (GsrGrads.reached_mask: 16 % of the rows at 500 k Gaussians @1024^2); the row formats of the exchange move
 * (row index, row) messages. A ROW SET is a table whose logical row i is the concatenation of slices of up to
 * GSR_ROWSET_MAX_REGIONS strided regions -- element f of row i, in region k, lives at regions[k].ptr[i * stride + (f - first_k)]:
 * the planar gradient arena (means3D [P,3] | scales [P,3] | rotations [P,4] | opacities [P,1] | the active SH columns of shs
 * [P,K,3]: width 3 (D+1)^2, stride 3 K) as well as a plain row-major buffer (one region). All device pointers, fp32. */
#define GSR_ROWSET_MAX_REGIONS 8
typedef struct GsrRowRegion {
  float* ptr;
  int32_t width;    /* floats of a logical row that live in this region          */
  int32_t stride;   /* floats between consecutive rows of this region (>= width) */
} GsrRowRegion;
typedef struct GsrRowSet {
  int32_t rows;       /* logical rows */
  int32_t n_regions;  /* 1..GSR_ROWSET_MAX_REGIONS */
  GsrRowRegion regions[GSR_ROWSET_MAX_REGIONS];
} GsrRowSet;
size_t gsr_rows_scratch_bytes(int32_t rows);
/* The rows whose bit is set in mask (u64[(rows + 63) / 64], bit i % 64 of word i / 64; bits beyond `rows` ignored) as a message:
 * idx[n] = their indices in ascending order, rows_out[n][F] = the rows (F = sum of the region widths), *count = n (device u32;
 * the caller reads it to size its wire buffers). At most `cap` rows are written; n may exceed cap (then re-run with more room).
 * scratch: gsr_rows_scratch_bytes(rows) bytes, 256-byte aligned. Two launches, no host synchronisation. */
int gsr_rows_pack(const GsrRowSet* set, const uint64_t* mask, uint32_t* idx, float* rows_out, uint32_t cap, uint32_t* count,
                  void* scratch, size_t scratch_bytes, void* stream);
/* The reverse: row idx[j] - row_base of the set receives rows_in[j] (mode 1: stored, mode 0: ADDED -- one message per launch
 * and the indices of a message distinct, so messages applied in rank order give every rank the same sums); touched (NULL or
 * u64[(rows + 63) / 64]): the bits of the rows written are OR-ed in (the owner side of a sparse reduce-scatter). Entries whose
 * idx[j] - row_base falls outside [0, set->rows) are skipped. */
int gsr_rows_unpack(const GsrRowSet* set, const uint32_t* idx, const float* rows_in, uint32_t n, int64_t row_base, int32_t mode,
                    uint64_t* touched, void* stream);
/* The local sum of the `direct` exchange (multiview.GradExchange: one all-to-all, THIS, one all-gather): out[i] =
 * ((s_0[i] + s_1[i]) + s_2[i]) + ... over n_slices slices of slice_floats floats, slice w at slices + w * stride_floats -- rank
 * order, the association every rank applies to the slice it owns. out may be slice 0 (in place). One launch. */
int gsr_sum_slices(const float* slices, int32_t n_slices, uint64_t slice_floats, uint64_t stride_floats, float* out, void* stream);
/* Self-describing row messages: the host-read-free forms of the sparse exchanges (multiview.GradExchange `rows` / `sparse_rs`; they
 * stand in for the count reads gsr_rows_pack needs -- the sequential accumulation all of it implements: training/object_trainer.py:
 * 302-382). A message of `rows` rows of `row_floats` floats with a fixed capacity of `cap` rows is gsr_rowmsg_bytes() bytes (a multiple
 * of 256): [header u32[64]: count, cap, rows, F, largest count its sender received | bitmap u64[(rows+63)/64] | rows in front of each
 * 64-row word u32[...] | rows f32[cap][F]]. Messages are 256-byte aligned; message q of an array sits at msgs + q * msg_stride.
 *   gsr_rowmsg_pack          ONE launch: the rows whose bit is set in `mask` (as gsr_rows_pack) -> msg. A count above cap is recorded
 *                            in the header (the rows beyond cap are not written).
 *   gsr_rowmsg_pack_slices   ONE launch: the set cut into n_slices slices of slice_rows rows (a multiple of 64; n_slices * slice_rows
 *                            >= rows): message y = slice y with slice-local row numbers -- what a rank sends to owner y.
 *   gsr_rowmsg_reduce        ONE launch, messages -> message: n_msgs (<= 16) messages describing the SAME rows (one per rank, rank
 *                            order) -> the message of their union, every row = ((g_0 + g_1) + ...) over the messages that hold it. If
 *                            an input does not fit cap_in (or has another shape) the output's count is 0xFFFFFFFF. layout_rows (0 =
 *                            rows): the row count the messages' layout was sized for (slice_rows of a slice message; >= rows).
 *   gsr_rowmsg_apply         ONE launch over n_msgs messages of the whole set (rank order): every row ANY message holds receives the
 *                            rank-ordered sum over the messages that hold it, STORED (rows nobody holds are left as they are); touched
 *                            (NULL or u64[(rows+63)/64]) receives the union bitmap (every word of it, if the messages are applied).
 *   gsr_rowmsg_apply_slices  ONE launch: message y (an owner's reduced slice) stored into rows [y * slice_rows, ...) of the set;
 *                            touched as above (the bitmaps of the slices side by side: slice_rows is a multiple of 64).
 * Both apply forms write NOTHING if any header's count exceeds cap (or its cap / rows / F differ from the call's). *status (NULL, or
 * one u64, device or page-locked host memory), stored when the kernel STARTS: bits 1:0 = 1 applied / 2 nothing applied, bits 32:2 the
 * largest count among the messages, bits 63:33 the largest count their senders received (owners' messages; 0 otherwise). */
size_t gsr_rowmsg_bytes(int32_t rows, int32_t row_floats, uint32_t cap);
int gsr_rowmsg_pack(const GsrRowSet* set, const uint64_t* mask, void* msg, uint32_t cap, void* stream);
int gsr_rowmsg_pack_slices(const GsrRowSet* set, const uint64_t* mask, void* msgs, uint64_t msg_stride, int32_t n_slices,
                           int32_t slice_rows, uint32_t cap, void* stream);
int gsr_rowmsg_reduce(int32_t rows, int32_t layout_rows, int32_t row_floats, const void* msgs, uint64_t msg_stride, int32_t n_msgs,
                      uint32_t cap_in, void* msg_out, uint32_t cap_out, void* stream);
int gsr_rowmsg_apply(const GsrRowSet* set, const void* msgs, uint64_t msg_stride, int32_t n_msgs, uint32_t cap, uint64_t* status,
                     uint64_t* touched, void* stream);
int gsr_rowmsg_apply_slices(const GsrRowSet* set, const void* msgs, uint64_t msg_stride, int32_t n_slices, int32_t slice_rows,
                            uint32_t cap, uint64_t* status, uint64_t* touched, void* stream);

/* ---- per-pixel glue between the rasterizer and the loss (dreamscene_amd/glue.py; SEMANTICS.md "disp post-processing and
 * tv_loss") --------------------------------------------------------------------------------------------------------------------
 * disp post-processing, scene_gaussian.py:651-658, :874-881, :1023-1032, for up to GSR_MAX_DISP_VIEWS views of one size per call:
 *   d = (1 / ((depth + alpha * 10) + 1e-5)) * focal;  m = min of d over alpha <= 0.1 (fp32 compare), or over every pixel when no
 *   pixel qualifies;  M = max of d;  disp = clamp((d - m) / (M - m), 0, 1)  (a flat view gives NaN, as torch does).
 * gsr_disp_forward   two launches: disp [V,1,H,W], alpha [V,1,H,W] (a copy of the alpha planes), stats [V][4] floats
 *                    (m, M, masked flag, M - m; 16-byte aligned) which the backward reads. No host read.
 * gsr_disp_backward  two launches: dL/d depth_alpha per view (dL_ddepth_alpha[k], [2,H,W]) from dL_ddisp [V,1,H,W] and
 *                    dL_dalpha ([V,1,H,W] or NULL); d is recomputed. The gradients of m and M are shared evenly among the pixels
 *                    that equal them (torch's min() / max()); their sums are formed in double in a fixed order.
 * scratch: gsr_disp_scratch_bytes(V, H, W) bytes, 16-byte aligned, for either call (0: the shape is not accepted).
 * tv_loss, utils/system_utils.py:39-47, x [B,C,H,W] fp32 contiguous, H >= 2 and W >= 2:
 * gsr_tv_forward     two launches: *out (device fp32) = 2 (h_tv / (C (H-1) W) + w_tv / (C H (W-1))) / B, the squared differences
 *                    in fp32 and their sums in double (fixed order). scratch: gsr_tv_scratch_bytes(B, C, H, W) bytes, 16-aligned.
 * gsr_tv_backward    one launch: dL_dx [B,C,H,W] (stored) from the scalar *dL_dout in device memory.
 * All of them: enqueued on `stream`, no allocation, no host synchronisation (capturable into a hipGraph). */
#define GSR_MAX_DISP_VIEWS 16
#define GSR_DISP_STATS_FLOATS 4
typedef struct GsrDispViews {
  int32_t n_views;                                   /* 1..GSR_MAX_DISP_VIEWS                                 */
  int32_t height, width;
  int32_t reserved_;
  const float* depth_alpha[GSR_MAX_DISP_VIEWS];      /* view k: [2,H,W], the depth plane then the alpha plane  */
  float* dL_ddepth_alpha[GSR_MAX_DISP_VIEWS];        /* view k: [2,H,W], written by the backward (unused by the forward) */
  float focal[GSR_MAX_DISP_VIEWS];                   /* 1 / (2 tan(FoVx / 2)) rounded to fp32                  */
} GsrDispViews;
size_t gsr_disp_scratch_bytes(int32_t n_views, int32_t height, int32_t width);
int gsr_disp_forward(const GsrDispViews* views, float* disp, float* alpha, float* stats, void* scratch, size_t scratch_bytes,
                     void* stream);
int gsr_disp_backward(const GsrDispViews* views, const float* stats, const float* dL_ddisp, const float* dL_dalpha, void* scratch,
                      size_t scratch_bytes, void* stream);
size_t gsr_tv_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int gsr_tv_forward(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, float* out, void* scratch, size_t scratch_bytes,
                   void* stream);
int gsr_tv_backward(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, const float* dL_dout, float* dL_dx, void* stream);

/* ---- the densification itself: GaussianModel.densify_and_prune / prune / prune_points with their optimizer surgery
 * (gs_renderer.py:889-1059; dreamscene_amd/densify.py; SEMANTICS.md "densify_and_prune") ------------------------------------------
 * The reference clones, splits and prunes through boolean-mask gathers and torch.cat over six parameters and their twelve Adam
 * moments: every row moves about four times. Here: a PLAN over the P original rows, ONE host read of the new sizes (output sizes
 * depend on the data and the caller owns all memory), then ONE gather pass.
 * gsr_densify_plan       two launches. Row i: g = accum / denom (NaN -> 0), smax = max_c exp(scaling[i][c]);
 *                          clone <=> densify and g >= max_grad and smax <= dense_threshold; split <=> ... smax > dense_threshold;
 *                          pruned <=> sigmoid(opacity) < min_opacity or (use_screen_size and (radius > max_screen_size or smax >
 *                          world_size_threshold)), radius = max_radii2D[i], or 0 when max_radii2D is NULL (densify_and_prune tests
 *                          after its statistics were reset); children are tested with exp(log(exp(scaling) / child_divisor)) and
 *                          radius 0. All comparisons in fp32 against thresholds the caller rounded once from double.
 *                        sizes (GSR_DENSIFY_SIZE_WORDS int32, to sizes_dev and, if not NULL, to page-locked sizes_host):
 *                          [0] surviving non-split originals, [1] surviving clones, [2 .. 2+N) surviving children per copy (all
 *                          equal), [GSR_DENSIFY_SIZE_WORDS-1] P_out. densify requires max_grad > 0 (clones are never split).
 * gsr_densify_plan_mask  the same from a caller's mask (uint8 / bool [P], non-zero = remove): prune_points.
 * gsr_densify_apply      two launches with the sizes the host read: src[j] (int32 [P_out]) = the original row of output row j --
 *                          survivors in index order | clones in source order | children of copy 0 in parent order | copy 1 | ... --
 *                          then every output tensor: parameters copied from src[j] (children: xyz = R(q / |q|) (n * exp(scaling))
 *                          + xyz, scaling = log(exp(scaling) / child_divisor)), moments of survivors copied and of new rows zero,
 *                          statistics gathered or (zero_stats) zero. n = noise[copy][i][0..3) if noise is not NULL, else three
 *                          standard normals from Philox-4x32-10 + Box-Muller keyed by (seed, i, copy): independent of the launch
 *                          geometry and of every other row. Moments and statistics may be NULL (src and dst together).
 * P = 0 and P_out = 0 are valid. max(2, N) * P rows must keep the 32-bit element offsets in range (else GSR_ECAPACITY;
 * gsr_densify_scratch_bytes returns 0). scratch: gsr_densify_scratch_bytes(P, N) bytes, 256-byte aligned, the SAME buffer for the
 * plan and its apply. dst pointers 16-byte aligned. Enqueued on `stream`; the library does not synchronise. */
#define GSR_DENSIFY_TENSORS 6
#define GSR_DENSIFY_MAX_SPLIT 8
#define GSR_DENSIFY_SIZE_WORDS 16
enum { GSR_DENSIFY_XYZ = 0, GSR_DENSIFY_F_DC = 1, GSR_DENSIFY_F_REST = 2, GSR_DENSIFY_OPACITY = 3, GSR_DENSIFY_SCALING = 4,
       GSR_DENSIFY_ROTATION = 5 };
typedef struct GsrDensifyPlan {
  int32_t P;                       /* original rows                                             */
  int32_t N;                       /* children per split row, 1..GSR_DENSIFY_MAX_SPLIT          */
  int32_t densify;                 /* 0: prune only                                             */
  int32_t use_screen_size;         /* the reference's `if max_screen_size:`                     */
  const float* scaling;            /* [P,3] log                                                 */
  const float* opacity;            /* [P,1] logit                                               */
  const float* xyz_gradient_accum; /* [P] (densify)                                             */
  const float* denom;              /* [P] (densify)                                             */
  const float* max_radii2D;        /* [P] or NULL = all zero                                    */
  float max_grad, dense_threshold, min_opacity, world_size_threshold, max_screen_size, child_divisor;
} GsrDensifyPlan;
typedef struct GsrDensifyTensor {
  const float* src;    float* dst;      /* [P,width] -> [P_out,width]                           */
  const float* m1_src; float* m1_dst;   /* exp_avg (both NULL: no optimizer state)              */
  const float* m2_src; float* m2_dst;   /* exp_avg_sq                                           */
  int32_t width;                        /* floats per row (0: nothing to move, f_rest at K = 1) */
  int32_t reserved_;
} GsrDensifyTensor;
typedef struct GsrDensifyTable {
  GsrDensifyTensor t[GSR_DENSIFY_TENSORS];   /* indexed by GSR_DENSIFY_XYZ ...                   */
  const float* stat_src[3];                  /* xyz_gradient_accum, denom, max_radii2D ([P])     */
  float* stat_dst[3];                        /* [P_out]                                          */
  const float* noise;                        /* [N,P,3] standard normals or NULL (generator)     */
  uint64_t seed;
  int32_t P, N;
  int32_t n_survivors, n_clones, n_children, P_out;   /* sizes[0], [1], [2], [last] of the plan */
  int32_t zero_stats;                        /* statistics written as zeros (densify_and_prune)  */
  float child_divisor;                       /* 0.8 N rounded to fp32                            */
} GsrDensifyTable;
size_t gsr_densify_scratch_bytes(int32_t P, int32_t N);
int gsr_densify_plan(const GsrDensifyPlan* plan, void* scratch, size_t scratch_bytes, int32_t* sizes_dev, int32_t* sizes_host,
                     void* stream);
int gsr_densify_plan_mask(const uint8_t* mask, int32_t P, void* scratch, size_t scratch_bytes, int32_t* sizes_dev,
                          int32_t* sizes_host, void* stream);
int gsr_densify_apply(const GsrDensifyTable* table, const void* scratch, size_t scratch_bytes, int32_t* src, void* stream);

/* ---- seeded noise as tensors (SEMANTICS.md "Seeded noise") -----------------------------------------------------------------------
 * Writes the N(0,1) samples that GsrScene.noise_seed / noise_stream(_dev) / noise_flags stand for: scale_noise [P,3] and / or
 * sh_noise [P,K,3] (either may be NULL) of the Gaussians 0..P-1 of the concatenated index space. A scene given these tensors
 * renders, and differentiates, bit for bit like the same scene with the flags set. stream_dev: NULL, or a device u32[1] read
 * when the kernel runs (then `stream` is ignored). One launch on `hip_stream`, no synchronisation, no allocation.
 * Checked in this order, before any HIP call: P < 0, K outside 1..16, both outputs NULL -> GSR_EINVAL; P == 0 -> 0, no launch. */
int gsr_noise_fill(uint64_t seed, uint32_t stream, const uint32_t* stream_dev, int32_t P, int32_t K, float* scale_noise,
                   float* sh_noise, void* hip_stream);

/* ---- object placement: SceneGaussian.add_objects_to_scene (scene_gaussian.py:318-427; dreamscene_amd/compose.py; SEMANTICS.md
 * "Object placement") ---------------------------------------------------------------------------------------------------------------
 * One trained object moved into the scene frame by a rotation R, a per-axis scale S and a translation, for K = 1, 4, 9 or 16 SH
 * coefficients per colour:
 *   xyz'      = fl32(R S x) + T       rs = R S rounded once to fp32; ((rs0 x0 + rs1 x1) + rs2 x2) + T, one rounding per operator;
 *                                     T = t, or with ground != 0 T.z = t.z - min over the rows of fl32(R S x).z (the object stands
 *                                     on z = t.z; one fp32 subtraction on the device, no host read);
 *   scaling'  = scaling + log_scale   one fp32 add per entry;
 *   rotation' = q (x) rotation        the raw Hamilton product, real part first, not normalised;
 *   f_rest'   [P,K-1,3]: band l = 1, 2, 3 (coefficients [0,3), [3,8), [8,15)) multiplied on the COEFFICIENT axis,
 *                                     k'[j][c] = sum_i k[i][c] m_l[i][j] (row-major m1 [3][3], m2 [5][5], m3 [7][7], the same for
 *                                     the three colours c), summed in index order; only the bands K holds are touched.
 * features_dc and opacity are not read (NULL is accepted); they are listed so that an output overlapping them is refused.
 * gsr_place  two launches on `stream`, no host synchronisation, no allocation (capturable): the box of fl32(R S x) per block into
 *            scratch, then every row. bounds[6] = (min xyz', max xyz') of the rows written; t_effective (NULL or 3 floats) = the T
 *            that was added. NaN coordinates do not enter the box. An output may be its own input (in place); an output that
 *            overlaps anything else the call touches, K outside {1, 4, 9, 16}, a NULL or not 16-byte aligned pointer and a
 *            scratch smaller than gsr_place_scratch_bytes(P) (16-byte aligned; 0: P is not accepted) return GSR_EINVAL before
 *            any HIP call. P = 0 is valid and launches nothing. */
typedef struct GsrPlacement {
  int32_t P;                       /* rows                                                       */
  int32_t K;                       /* SH coefficients per colour: 1, 4, 9 or 16                  */
  const float* xyz;                /* [P,3]                                                      */
  const float* scaling;            /* [P,3] log                                                  */
  const float* rotation;           /* [P,4] (w, x, y, z)                                         */
  const float* opacity;            /* [P,1] not read                                             */
  const float* features_dc;        /* [P,1,3] not read                                           */
  const float* features_rest;      /* [P,K-1,3] (unused at K = 1)                                */
  float* xyz_out;
  float* scaling_out;
  float* rotation_out;
  float* features_rest_out;
  float rs[9];                     /* R S, row-major                                             */
  float t[3];                      /* the centre                                                 */
  float log_scale[3];              /* log of the per-axis scale, formed in double, rounded once  */
  float q[4];                      /* the quaternion of R (w, x, y, z)                           */
  float m1[9], m2[25], m3[49];     /* the band matrices, Y_i(R^T d) = sum_j m_l[i][j] Y_j(d)     */
  int32_t ground;                  /* != 0: T.z = t.z - min z                                    */
  float* bounds;                   /* [6] out                                                    */
  float* t_effective;              /* [3] out, or NULL                                           */
} GsrPlacement;
size_t gsr_place_scratch_bytes(int32_t P);
int gsr_place(const GsrPlacement* placement, void* scratch, size_t scratch_bytes, void* stream);

/* ---- frame export: the uint8 tail of video_inference / scene_video_inference / scene_cams_record (training/object_trainer.py:
 * 81-118, training/scene_trainer.py:261-340; dreamscene_amd/frames.py; SEMANTICS.md "Frame export") -----------------------------
 * Up to GSR_MAX_FRAME_VIEWS rendered views of one size, each its own image [3,H,W] and (optionally) depth_alpha [2,H,W] as the
 * forward returns them (no stacking), to interleaved bytes:
 *   rgb   [F,H,W,3] uint8 = rint(fl32(clamp(x, 0, 1) * 255)), round half to even (numpy's round);
 *   depth [F,H,W,1] uint8 = the same chain on fl32(d / M), d = plane 0 of depth_alpha, M = that frame's own maximum of the plane,
 *                           a correctly rounded fp32 division; NULL: not wanted.
 * Inputs are finite (precondition). A NaN of the chain -- only 0 / 0 of an all-zero depth frame -- gives byte 0.
 * gsr_frames_quantize  depth != NULL: two launches (the per-block maxima into scratch, then every block reduces its frame's
 *                      maxima and writes the bytes); depth == NULL: one launch, depth_alpha and scratch are not read. Enqueued on
 *                      `stream`, no allocation, no host synchronisation, no atomics (capturable; the same bytes on every run).
 *                      Plane pointers 4-byte aligned (16-byte aligned planes with H*W % 4 == 0 are read 16 bytes at a time); rgb
 *                      and depth need no alignment. scratch: gsr_frames_scratch_bytes(F, H, W) bytes, 16-byte aligned (0: the
 *                      shape is not accepted); too small: GSR_ESCRATCH. Bad shapes and NULL pointers: GSR_EINVAL before any HIP
 *                      call. */
#define GSR_MAX_FRAME_VIEWS 16
typedef struct GsrFrameViews {
  int32_t n_views;                                   /* 1..GSR_MAX_FRAME_VIEWS                                  */
  int32_t height, width;
  int32_t reserved_;
  const float* image[GSR_MAX_FRAME_VIEWS];           /* view k: [3,H,W]                                         */
  const float* depth_alpha[GSR_MAX_FRAME_VIEWS];     /* view k: [2,H,W]; only plane 0 is read; unused without depth */
} GsrFrameViews;
size_t gsr_frames_scratch_bytes(int32_t n_views, int32_t height, int32_t width);
int gsr_frames_quantize(const GsrFrameViews* views, uint8_t* rgb, uint8_t* depth, void* scratch, size_t scratch_bytes,
                        void* stream);

/* ---- photometric loss: l2_loss, l1_loss and ssim of the reconstructive refine steps (utils/system_utils.py:59-126; training/
 * object_trainer.py:626-653, training/scene_trainer.py:1269-1293, :1737-1770; dreamscene_amd/photometric.py; SEMANTICS.md
 * "Photometric loss") ---------------------------------------------------------------------------------------------------------------
 * Up to GSR_MAX_PHOTO_VIEWS views of one size, each its own image x [C,H,W] fp32 (as the forward returns it: no stacking) and
 * target y [C,H,W] fp32 or fp16 (widened exactly), C in 1..GSR_MAX_PHOTO_CHANNELS, any H, W >= 1:
 *   loss[v] = l2 mean((x-y)^2) + l1 mean|x-y| + dssim (1 - mean(ssim_map(x, y)))        means over the view's C H W entries
 *   ssim_map: window 11x11 Gaussian, sigma 1.5 (gsr_photo_window), zero padding 5, per channel, applied separably;
 *             s = E[ab] - mu_a mu_b, C1 = 0.01^2, C2 = 0.03^2. round_image_to_half: x is rounded to fp16 (nearest even) on load
 *             -- the refine steps' .to(torch.float16) -- and its gradient passes straight through.
 * All per-pixel arithmetic is fp32 (NOT the reference's fp16 L2: SEMANTICS.md), every sum over pixels is in double in a fixed
 * order: no atomics, the same bits on every run.
 * gsr_photo_window    the 11 taps: exp(-(i-5)^2 / 4.5) in double, rounded to fp32, divided in fp32 by their fp32 sum. Host only.
 * gsr_photo_forward   dssim != 0: one launch over (32x32 tile, channel, view) with the halo of x and y in LDS, then one small
 *                     launch that adds the per-block partials. saved != NULL: also the planes dm/dmu_x, dm/ds_x, dm/ds_xy,
 *                     [3][V,C,H,W] fp32, which the backward needs; NULL (no gradient wanted) skips the store.
 *                     dssim == 0: the point-wise form, no halo and no saved planes (saved is not touched).
 *                     loss [V]; terms [V,3] or NULL: the unweighted (L2, L1, D-SSIM) of every view (D-SSIM is NaN in the
 *                     point-wise form, which does not evaluate it). scratch: gsr_photo_scratch_bytes(V, C, H, W) bytes, 16-byte
 *                     aligned (0: the shape is not accepted); too small: GSR_ESCRATCH.
 * gsr_photo_backward  one launch: dL_dimage[k] [C,H,W] (stored, not accumulated) = dL_dloss[k] (device memory, [V]) times the
 *                     exact d loss[k] / dx; d|x-y|/dx at x == y is 0. No gradient goes to the targets. With dssim != 0 it reads
 *                     the `saved` planes of the forward on the same views and weights.
 * Both: enqueued on `stream`, no allocation, no host synchronisation (capturable into a hipGraph). Bad shapes and counts, NULL
 * or misaligned (4 bytes; fp16 targets 2) pointers, all-zero or NaN weights and a missing `saved` with dssim != 0 in the backward:
 * GSR_EINVAL before any HIP call. */
#define GSR_MAX_PHOTO_VIEWS 16
#define GSR_MAX_PHOTO_CHANNELS 4
#define GSR_PHOTO_WINDOW 11
typedef struct GsrPhotoViews {
  int32_t n_views;                                   /* 1..GSR_MAX_PHOTO_VIEWS                                  */
  int32_t channels;                                  /* 1..GSR_MAX_PHOTO_CHANNELS                               */
  int32_t height, width;
  int32_t target_is_half;                            /* != 0: the targets are fp16                              */
  int32_t round_image_to_half;                       /* != 0: x is rounded to fp16 on load                      */
  const float* image[GSR_MAX_PHOTO_VIEWS];           /* view k: [C,H,W]                                         */
  const void* target[GSR_MAX_PHOTO_VIEWS];           /* view k: [C,H,W] fp32 or fp16                            */
  float* dL_dimage[GSR_MAX_PHOTO_VIEWS];             /* view k: [C,H,W], written by the backward (unused by the forward) */
} GsrPhotoViews;
typedef struct GsrPhotoWeights {
  float l2, l1, dssim;
} GsrPhotoWeights;
void gsr_photo_window(float* taps);
size_t gsr_photo_scratch_bytes(int32_t n_views, int32_t channels, int32_t height, int32_t width);
int gsr_photo_forward(const GsrPhotoViews* views, const GsrPhotoWeights* weights, float* loss, float* terms, float* saved,
                      void* scratch, size_t scratch_bytes, void* stream);
int gsr_photo_backward(const GsrPhotoViews* views, const GsrPhotoWeights* weights, const float* saved, const float* dL_dloss,
                       void* stream);

/* ---- model lifecycle: GaussianModel.create_from_pcd, reset_opacity and add_densification_stats(_div) (gs_renderer.py:582-608,
 * :746-749 with :854-868, :1061-1080; dreamscene_amd/model.py; SEMANTICS.md section 15) -------------------------------------------
 * Three element-wise kernels, one launch each on `stream`, no allocation, no host synchronisation, no memset (capturable).
 * Every pointer is 4-byte aligned device memory; one rounding per operator, full-precision expf / logf / sqrtf and IEEE division.
 * gsr_model_init     the six leaves of a new model of P rows with K = 1, 4, 9 or 16 SH coefficients per colour:
 *                      xyz [P,3] = points;  f_dc [P,1,3] = (colors - 0.5f) / C0, C0 = fl32(0.28209479177387814);
 *                      f_rest [P,K-1,3] = 0 (K == 1: not touched, NULL accepted);  scaling [P,3] = logf(sqrtf(fmaxf(dist2, 1e-7f)))
 *                      in its three columns;  rotation [P,4] = (1,0,0,0);  opacity [P,1] = opacity_logit.
 * gsr_opacity_reset  opacity_out[i] = logf(m / (1 - m)), m = min(s, cap) with a NaN s kept (torch.min), s = 1 / (1 + expf(-x));
 *                    exp_avg and exp_avg_sq ([P], either may be NULL) are cleared. opacity_out is a tensor of its own: one that
 *                    overlaps the input, or moments that overlap anything else of the call, are GSR_EINVAL.
 * gsr_densify_stats  where filter[i] != 0 (uint8 / bool [n]): accum[i] += sqrtf(gx*gx + gy*gy) with (gx, gy) the first two
 *                    entries of row start + i of grad [P_total,3], and denom[i] += 1 -- the expression the rasterizer backward
 *                    uses for GsrGrads.stat_*, so both routes leave equal bits. 0 <= start, start + n <= P_total.
 * Bad counts, NULL and misaligned pointers: GSR_EINVAL before any HIP call. P == 0 (n == 0) is valid and launches nothing. */
int gsr_model_init(const float* points, const float* colors, const float* dist2, int32_t P, int32_t K, float opacity_logit,
                   float* xyz, float* f_dc, float* f_rest, float* scaling, float* rotation, float* opacity, void* stream);
int gsr_opacity_reset(const float* opacity, int32_t P, float cap, float* opacity_out, float* exp_avg, float* exp_avg_sq,
                      void* stream);
int gsr_densify_stats(const float* grad, int32_t P_total, const uint8_t* filter, int32_t start, int32_t n, float* accum,
                      float* denom, void* stream);

/* ---- k-th value select and 3D Gaussian filtering: calculate_v_imp_score and the mask of GaussianModel.prune_gaussians
 * (scene_gaussian.py:1046-1061, gs_renderer.py:1082-1087; dreamscene_amd/filtering.py; SEMANTICS.md section 16) ------------------
 * The k-th order statistic is EXACT: the value torch.sort(x)[0][k] has (k 0-based, ascending). -0 and +0 are equal (either may
 * come back); every NaN, whatever its sign bit, sorts after +inf and comes back as the quiet NaN 0x7FC00000. An MSD radix select
 * on the order-preserving key of the float, four passes of 8 bits, one launch a pass; the launch boundary is the only hand-off
 * between workgroups and every count is an integer, so the result has the same bits on every run. Nothing is allocated, nothing
 * is read by the host, no memset (capturable into a hipGraph).
 * scratch: gsr_select_scratch_bytes(n) bytes (0: n is not accepted), 16-byte aligned, the caller's; its contents on entry do
 * not matter (each call clears what it counts in, on `stream`); too small: GSR_ESCRATCH.
 * gsr_kth_value          out[0] = the k-th smallest of x [n]. Six launches.
 * gsr_importance_filter  volume[i] = (s0 * s1) * s2 of row i of scaling [n,3] (activated == 0: of expf of each entry);
 *                        kth = the k_volume-th smallest volume; v[i] = powf(volume[i] / kth, v_pow) * imp[i];
 *                        thr = the k_threshold-th smallest v; mask[i] = v[i] <= thr (uint8 1 / 0; a NaN v is never 1, every tie
 *                        of thr is). IEEE results for a zero kth, a zero volume and inf are what the formulas give. Ten launches;
 *                        kth and thr never leave device memory. v_list [n] (NULL: v lives in the scratch) and n_pruned (NULL: not
 *                        wanted), a device int32 that receives the number of ones.
 *                        Two partial forms: mask == NULL stops after v (v_list required, k_threshold and n_pruned unused, six
 *                        launches); scaling == NULL starts from v_list as INPUT (imp, v_pow, k_volume unused, six launches).
 *                        The reference's ranks: k_volume = n - 1 - (int)(n * 0.9), k_threshold = (int)(percent * (n - 1)).
 * n <= 0, a rank outside [0, n), NULL or misaligned (4 bytes) pointers, buffers that overlap each other or the scratch:
 * GSR_EINVAL before any HIP call. */
size_t gsr_select_scratch_bytes(int32_t n);
int gsr_kth_value(const float* x, int32_t n, int32_t k, float* out, void* scratch, size_t scratch_bytes, void* stream);
int gsr_importance_filter(const float* scaling, int32_t activated, const float* imp, int32_t n, float v_pow, int32_t k_volume,
                          int32_t k_threshold, uint8_t* mask, float* v_list, int32_t* n_pruned, void* scratch,
                          size_t scratch_bytes, void* stream);

/* ---- seeded point clouds: what GaussianModel.init_env_pcd, init_floor_pcd and init_pcd draw on the host (gs_renderer.py:218-408;
 * dreamscene_amd/pointcloud.py; SEMANTICS.md section 17) ----------------------------------------------------------------------------
 * points and colors are fp32 [rows,3] device memory, written from (seed, cloud id, index) alone: Philox-4x32-10 keyed by the seed,
 * counter (index, block, cloud id, 3), uniforms of 24 bits in the open interval (0,1), uniform e of a row = slot e % 4 of block
 * e / 4. The same seed gives the same bits on every device and for every launch geometry, and the first m rows of an n-row draw
 * are the m-row draw (per sheet for the indoor env). fp32 arithmetic in the written order, IEEE division, full-precision sqrtf /
 * cbrtf / sinf / cosf. One launch each on `stream`, nothing allocated, no host synchronisation (capturable).
 * gsr_sample_env_indoor    5n rows in sheet order around box [6] (x0 y0 z0 x1 y1 z1), which is read from DEVICE memory
 * gsr_sample_floor_indoor  n rows under box [6] (device memory) of colour (r, g, b)
 * gsr_sample_shell         n rows of the shell radius * cbrt(0.95 .. 1.05), the upper half with zero_ground != 0
 * gsr_sample_disc          n rows of the disc of `radius`, z in z0 - 0.1 .. z0
 * gsr_sample_ball          n rows of the ball of `radius`, colours u / 255 * C0 + 0.5
 * gsr_sample_jitter        n_seeds * copies rows: row (i, copy) = (x, -y, z + 0.15) of seed point i + the copy's offset (shared
 *                          by every seed point, |offset| <= radius); colours seed_colors[i] + 1e-4 u, or the ball's with
 *                          seed_colors == NULL
 * gsr_mesh_areas           area [n_faces] (double): the fp32 area of each triangle of faces [n_faces,3] (int32) over vertices
 *                          [n_vertices,3]; 0 for a face that names a vertex outside the table
 * gsr_sample_mesh          n rows on the triangles chosen by cdf [n_faces] (double, non-decreasing, last entry 1: the first t with
 *                          u < cdf[t]), axes swapped to (x, z, y); triangle [n] (int32, NULL accepted) receives each row's choice
 * gsr_mesh_center          points[i] = (points[i] - fl32(mean)) / 80 with mean [3] doubles in device memory
 * A row count outside 1 .. 2^31 - 1, a non-finite radius, NULL or misaligned pointers: GSR_EINVAL before any HIP call. */
enum {
  GSR_CLOUD_ENV = 0,
  GSR_CLOUD_FLOOR = 1,
  GSR_CLOUD_BALL = 2,
  GSR_CLOUD_JITTER_OFFSETS = 3,
  GSR_CLOUD_JITTER_COLORS = 4,
  GSR_CLOUD_MESH = 5
};
int gsr_sample_env_indoor(uint64_t seed, const float* box, int32_t n, float* points, float* colors, void* stream);
int gsr_sample_floor_indoor(uint64_t seed, const float* box, float r, float g, float b, int32_t n, float* points, float* colors,
                            void* stream);
int gsr_sample_shell(uint64_t seed, float radius, int32_t zero_ground, float r, float g, float b, int32_t n, float* points,
                     float* colors, void* stream);
int gsr_sample_disc(uint64_t seed, float radius, float z0, float r, float g, float b, int32_t n, float* points, float* colors,
                    void* stream);
int gsr_sample_ball(uint64_t seed, float radius, int32_t n, float* points, float* colors, void* stream);
int gsr_sample_jitter(uint64_t seed, const float* seed_points, const float* seed_colors, int32_t n_seeds, int32_t copies,
                      float radius, float* points, float* colors, void* stream);
int gsr_mesh_areas(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces, double* area, void* stream);
int gsr_sample_mesh(uint64_t seed, const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces,
                    const double* cdf, int32_t n, float* points, float* colors, int32_t* triangle, void* stream);
int gsr_mesh_center(const double* mean, int32_t n, float* points, void* stream);

/* ---- occupancy field: GaussianModel.extract_fields (gs_renderer.py:490-573 with gaussian_3d_coeff, :95-121; dreamscene_amd/
 * fields.py; SEMANTICS.md section 18) -----------------------------------------------------------------------------------------------
 * The opacity-weighted density of P Gaussians on a resolution^3 grid, fp32, from the raw leaves xyz [P,3], opacity_raw [P] (logits),
 * scaling_raw [P,3] (log-scales) and rotation_raw [P,4] (any length, real part first). A row takes part iff sigmoid(opacity_raw) >
 * 0.005. The axis is cut into n_chunks = ceil(resolution / split_size) chunks of split_size coordinates (the last may be shorter);
 * a row belongs to chunk triple (cx, cy, cz) iff gate_lo[c] < its normalised centre < gate_hi[c], strictly, on every axis, and
 * occ[x][y][z] = the sum over the members of the voxel's triple, in index order, of opacity * expf(power) (0 where power > 0).
 * scratch: gsr_fields_scratch_bytes(P) bytes (0: P is not accepted), 16-byte aligned, the caller's; its contents on entry do not
 * matter; too small: GSR_ESCRATCH. Nothing is allocated, no memset, no atomics on floats: the same bits on every run.
 * gsr_fields_bounds    three launches. Writes the first 8 words of the scratch: the per-axis minimum [3] and maximum [3] of xyz over
 *                      the rows that take part (fp32, exact; NaN where none does or an entry is NaN), their number (int32), 0.
 *                      Reading them is the caller's one host read; center and scale follow from them on the host.
 * gsr_extract_fields   two launches, nothing read by the host. center [3] is HOST memory; a row's normalised centre is (xyz -
 *                      center) * scale and its standard deviations expf(scaling_raw) * scale. coords [resolution], gate_lo
 *                      [n_chunks] and gate_hi [n_chunks] are device tables the kernels never recompute (the reference forms them on
 *                      the host: torch.linspace(-1, 1, resolution), and a chunk's first / last coordinate -/+ the relaxed block
 *                      size), both gates ascending. Every element of occ [resolution]^3 is written exactly once; occ needs no
 *                      clearing. It does not read the head gsr_fields_bounds wrote.
 * P <= 0, resolution outside 1 .. 1024, split_size outside 1 .. resolution, n_chunks != ceil(resolution / split_size) or > 255, a
 * non-finite center or scale, NULL or misaligned (4 bytes; scratch 16) pointers, buffers that overlap occ or the scratch: GSR_EINVAL
 * before any HIP call. */
size_t gsr_fields_scratch_bytes(int32_t P);
int gsr_fields_bounds(const float* xyz, const float* opacity_raw, int32_t P, void* scratch, size_t scratch_bytes, void* stream);
int gsr_extract_fields(const float* xyz, const float* opacity_raw, const float* scaling_raw, const float* rotation_raw, int32_t P,
                       const float* center, float scale, const float* coords, const float* gate_lo, const float* gate_hi,
                       int32_t resolution, int32_t split_size, int32_t n_chunks, float* occ, void* scratch, size_t scratch_bytes,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSRAST_H */

// gsr_launch.h -- the stage launchers api.hip calls, declared once, with their parameter names. Included by api.hip and
// by every file that defines one of them: caller and definition read the same text. (These are C++ functions, so a
// definition whose parameter types drift is a new overload, not an error -- change the declaration here first and both
// sides stop compiling until they follow.) Declarations only.
#pragma once
#include "gsr_common.h"

// preprocess.hip (K1)
int gsr_launch_preprocess(const GsrView& v, const GsrGaussians& g, GsrGeom& geom, hipStream_t stream);
bool gsr_preprocess_views_supported(const GsrView& v, const GsrGaussians& g);
bool gsr_batch_noise_fits(int n_views, const GsrGaussians* gs);   // seeded noise of a batch: what the views kernels can carry
int gsr_launch_preprocess_views(int n_views, const GsrView* views, const GsrGaussians* gs, GsrGeom* geoms,
                                hipStream_t stream);
int gsr_launch_noise_fill(uint64_t seed, uint32_t stream, const uint32_t* stream_dev, int32_t P, int32_t K,
                          float* scale_noise, float* sh_noise, hipStream_t hip_stream);

// preprocess_bwd.hip (K8)
bool gsr_preprocess_bwd_views_supported(const GsrView& v, const GsrGaussians& g, const GsrGrads& out);
int gsr_launch_preprocess_bwd(int n_views, const GsrView* views, const GsrGaussians* gs, const GsrGeom* geoms,
                              const GsrGrads* outs, hipStream_t stream, bool* restored);

// binning.hip
bool gsr_uses_columns(const GsrView& v);
uint64_t* gsr_pair_counts(const GsrGeom& geom, int32_t P);
int gsr_launch_depth_order(GsrGeom& geom, const GsrView& v, hipStream_t stream, GsrProfile* prof, int batch,
                           size_t bstride, uint64_t* n_pairs_all, bool early);
int gsr_launch_binning_batch(int n, const GsrView* views, const GsrGeom* geoms, uint64_t cap, GsrBinning* bs,
                             hipStream_t stream, GsrProfile* prof);
int gsr_launch_binning(const GsrView& v, const GsrGeom& geom, uint64_t cap, const uint64_t* n_dev,
                       const uint64_t* n_dev_vis, GsrBinning& b, hipStream_t stream, GsrProfile* prof);

// render_fwd.hip (K6)
int gsr_launch_work_order_fwd(int n, const GsrView* views, const GsrBinning* bs, const GsrImages* imgs,
                              hipStream_t stream);
int gsr_launch_render_fwd_views(int n, const GsrView* views, const GsrGeom* geoms, const GsrBinning* bs, GsrImages* imgs,
                                hipStream_t stream, GsrProfile* prof);

// render_bwd.hip (K7)
int gsr_launch_work_order_bwd(int n, const GsrView* views, const GsrBinning* bs, const GsrImages* imgs,
                              hipStream_t stream);
int gsr_launch_render_bwd_views(int n, const GsrView* views, const GsrGeom* geoms, const GsrBinning* bs,
                                const GsrImages* imgs, const GsrImageGrads* igs, GsrGrads* outs, hipStream_t stream,
                                GsrProfile* prof);

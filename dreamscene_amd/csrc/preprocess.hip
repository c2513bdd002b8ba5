// preprocess.hip -- K1 (per-Gaussian EWA projection + SH colour), gfx950. K8, its backward: preprocess_bwd.hip; what the
// two share: gsr_project.h.
//
// Replaces the preprocess stage of the rasterizer DreamScene imports (scene_gaussian.py:11-12); the math
// follows SEMANTICS.md / SURVEY.md Appendix A.1, A.3 and the Python statements the reference does hold:
// cov3D gs_renderer.py:124-172, SH utils/sh_utils.py:25-102, projection utils/graphics_utils.py:29-36.
//
// Both kernels are HBM-streaming (44 + 12K bytes in per Gaussian for K1; 276 in / 248 out for K8 at K=16).
// One thread per Gaussian. K1: every lane pulls its own 12K-byte SH row with 16-byte loads straight into registers (the
// SH stride is a template parameter; the rows of a wave are contiguous, so L1/TA serve the pieces of a line to successive
// loads -- measured faster than the LDS transpose of round 1, which cost 50 KB of LDS per block). K8: the SH rows are
// read the same way; dL/dSH is written back coalesced through an LDS transpose (direct row stores measured 25 % slower).
//
// Both translation units are built with -ffp-contract=off: every fp32 operator that feeds an integer artefact
// (depth bits, radius, tile rectangle) rounds exactly once, in the order written -- the same order as
// oracle/gsr_oracle.c -- which is what makes radii / tile counts / sort keys bit-exact against the oracle.
#include "gsr_project.h"
#include "gsr_launch.h"

namespace {

// ---- the per-view projection of one Gaussian (K1), shared by the single-view and the multi-view kernel
struct Proj {
  bool vis;
  int32_t radius;
  uint32_t ntiles, rect;   // rect: x0 | y0 << 8 | (w-1) << 16 | (h-1) << 24 (grids up to 256 x 256 tiles)
  float q0x, q0y, ca, cb, cc, depth;
};
// near-plane cull (view depth > 0.2) and the NDC position with the reference's 1/(w + 1e-7) (graphics_utils.py:29-36)
__device__ __forceinline__ bool proj_in_front(const ViewConst& vc, float px, float py, float pz, float& ndcx, float& ndcy) {
  const float tzq = ((vc.V[2] * px + vc.V[6] * py) + vc.V[10] * pz) + vc.V[14];
  if (!(tzq > GSR_NEAR_Z)) return false;
  const float* PV = vc.PV;
  const float hx = ((PV[0] * px + PV[4] * py) + PV[8] * pz) + PV[12];
  const float hy = ((PV[1] * px + PV[5] * py) + PV[9] * pz) + PV[13];
  const float hw = ((PV[3] * px + PV[7] * py) + PV[11] * pz) + PV[15];
  const float pw = 1.0f / (hw + 0.0000001f);
  ndcx = hx * pw; ndcy = hy * pw;
  return true;
}
__device__ __forceinline__ void proj_footprint(const ViewConst& vc, float px, float py, float pz, const float c6[6],
                                               float fx, float fy, float limx, float limy, int W, int H, int gx, int gy,
                                               float ndcx, float ndcy, Proj& o) {
  o.vis = false; o.radius = 0; o.ntiles = 0; o.rect = 0;
  Ewa e;
  ewa_forward(vc, px, py, pz, c6, fx, fy, limx, limy, e);
  if ((fabsf(e.det) > 0.0f) && (fabsf(e.det) < INFINITY)) {
    const float inv = 1.0f / e.det;
    const float mid = 0.5f * (e.ca + e.cc);
    const float lam = mid + sqrtf(fmaxf(0.1f, mid * mid - e.det));
    const int32_t radius = gsr_f2i_sat(ceilf(3.0f * sqrtf(lam)));
    const float pxl = ((ndcx + 1.0f) * (float)W - 1.0f) * 0.5f;
    const float pyl = ((ndcy + 1.0f) * (float)H - 1.0f) * 0.5f;
    const float rf = (float)radius;
    const int32_t x0 = min(gx, max(0, gsr_f2i_sat((pxl - rf) * 0.0625f)));
    const int32_t y0 = min(gy, max(0, gsr_f2i_sat((pyl - rf) * 0.0625f)));
    const int32_t x1 = min(gx, max(0, gsr_f2i_sat(((pxl + rf) + 15.0f) * 0.0625f)));
    const int32_t y1 = min(gy, max(0, gsr_f2i_sat(((pyl + rf) + 15.0f) * 0.0625f)));
    o.ntiles = (uint32_t)((x1 - x0) * (y1 - y0));
    o.rect = (uint32_t)x0 | ((uint32_t)y0 << 8) | ((uint32_t)(x1 - x0 - 1) << 16) | ((uint32_t)(y1 - y0 - 1) << 24);
    if (o.ntiles != 0) {
      o.vis = true;
      o.radius = radius;
      o.q0x = pxl; o.q0y = pyl;
      o.ca = e.cc * inv; o.cb = -e.cb * inv; o.cc = e.ca * inv;
      o.depth = e.tz;
    }
  }
}
// Level of the conic form below which a splat can pass the alpha >= 1/255 gate: sigma exp(-q/2) >= 1/255 <=>
// q = d^T Conic d <= 2 ln(255 sigma) =: tau (slightly inflated). Used only to skip (pixel block, splat) pairs that
// cannot contribute (gsr_render.h, block_mask_t); negative = the splat contributes nowhere. Not part of any parity artefact.
__device__ __forceinline__ float splat_tau(float opac) {
  return (opac * 255.0f > 1.0f) ? 2.0f * logf(opac * 255.0f) * 1.0001f + 0.001f : -1.f;
}

// The integer outputs K1 writes for every Gaussian and view (culled: zeros, and the depth key that the depth sort drops).
__device__ __forceinline__ void store_view_ints(int32_t* radii, uint32_t* tiles_touched, uint32_t* depth_keys, uint32_t* rects,
                                                int64_t i, int32_t radius, uint32_t ntiles, bool vis, float depth, uint32_t rect) {
  radii[i] = radius;
  tiles_touched[i] = ntiles;
  depth_keys[i] = vis ? __float_as_uint(depth) : 0xFFFFFFFFu;
  rects[i] = rect;
}

// --------------------------------------------------------------------------------------------------------- K1
// The loads of a Gaussian are issued as early as their addresses are known instead of behind the test that makes them
// necessary (EARLY below, and k_preprocess_views): rotation / scales / opacity (32 B) with the position, the SH row as soon as
// the Gaussian is in front of a camera -- two memory round trips per wave instead of three, the second one under the footprint
// arithmetic. Measured (round 4, one call, same box): k_preprocess_views<16> 65.8 -> 64.7 us at C3, k_preprocess<16> 30.9 ->
// 29.9 us per view: the kernel is not bound by its round trips (VALU 50 % busy, 4 TB/s of mixed read / write traffic).
// GEN (scene only): the augmentation noise may come from the generator (NoiseSrc, gsr_project.h) instead of a tensor.
template <int KT, bool SCENE = false, typename TAB = NoScene, bool GEN = false>
__global__ void __launch_bounds__(256)
k_preprocess(const GsrView v, const GsrGaussians g, const TAB sc, float* __restrict__ splat,
             int32_t* __restrict__ radii, uint32_t* __restrict__ tiles_touched, uint32_t* __restrict__ depth_keys,
             uint32_t* __restrict__ rects, uint32_t* __restrict__ sort_state, const uint32_t sort_state_words) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  // the depth sort that follows starts from a zeroed state (digit histograms, tickets, look-back words; radix_sort.h): cleared
  // here, a few words per workgroup, instead of by a launch of its own in front of the sort
  for (uint32_t w = blockIdx.x * 256u + threadIdx.x; w < sort_state_words; w += gridDim.x * 256u) sort_state[w] = 0u;
  const int P = v.P, W = v.image_width, H = v.image_height, K = KT > 0 ? KT : v.sh_stride;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const Rows rw = resolve_rows<SCENE>(sc, P);
  const int64_t i = rw.i, row = rw.row, wave_first = rw.wave_row;
  const int n_valid = rw.n_valid;
  const float *p_xyz = g.means3D, *p_scale = g.scales, *p_rot = g.rotations, *p_opac = g.opacities;
  [[maybe_unused]] uint32_t nstream = 0u;
  if constexpr (SCENE) {
    p_xyz = sc.xyz[rw.m]; p_scale = sc.scaling[rw.m]; p_rot = sc.rotation[rw.m]; p_opac = sc.opacity[rw.m];
    nstream = noise_stream<GEN>(sc.noise);
  }
  const int gx = (W + GSR_TILE - 1) / GSR_TILE, gy = (H + GSR_TILE - 1) / GSR_TILE;
  const ViewDyn vd = view_dyn(v.dynamic, v.tanfovx, v.tanfovy, v.sh_degree);
  const float fx = (float)W / (2.0f * vd.tanfovx), fy = (float)H / (2.0f * vd.tanfovy);
  const float limx = 1.3f * vd.tanfovx, limy = 1.3f * vd.tanfovy;

  ViewConst vc;
  load_view(v, vc);

  bool vis = false;
  float px = 0, py = 0, pz = 0;
  float q0x = 0, q0y = 0, ca_ = 0, cb_ = 0, cc_ = 0, depth = 0, opac = 0, tau_ = -1.f;
  int32_t radius = 0;
  uint32_t ntiles = 0;
  uint32_t rect = 0;   // x0 | y0 << 8 | (w-1) << 16 | (h-1) << 24 of the tile rectangle (grids up to 256 x 256 tiles)
  constexpr bool EARLY = !SCENE;
  constexpr int FH = (EARLY && KT > 0) ? 3 * KT : 1;
  float shr_h[FH];
  if (rw.ok) {
    px = p_xyz[3 * row]; py = p_xyz[3 * row + 1]; pz = p_xyz[3 * row + 2];
    float sa_e[3] = {0.f, 0.f, 0.f}, opac_e = 0.f;
    float4 q_e = make_float4(0.f, 0.f, 0.f, 0.f);
    float c6_e[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (EARLY) {
      if (!g.cov3D_precomp) {
        sa_e[0] = p_scale[3 * row]; sa_e[1] = p_scale[3 * row + 1]; sa_e[2] = p_scale[3 * row + 2];
        q_e = *reinterpret_cast<const float4*>(p_rot + 4 * row);
      } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) c6_e[k] = g.cov3D_precomp[6 * i + k];
      }
      opac_e = p_opac[row];
    }
    if constexpr (SCENE) {
      // activated values the caller gets back (scene_render returns the augmented scales, scene_gaussian.py:892)
      if (sc.scales_out) {
        float n[3];
        noise_scale3<GEN>(sc.noise, nstream, i, n);
#pragma unroll
        for (int k = 0; k < 3; ++k)
          sc.scales_out[3 * i + k] = act_scale(p_scale[3 * row + k], noise_has_scale<GEN>(sc.noise), n[k]).out;
      }
      if (sc.rotations_out) {
        const float4 q = *reinterpret_cast<const float4*>(p_rot + 4 * row);
        const float nrm = act_quat_norm(q);
        *reinterpret_cast<float4*>(sc.rotations_out + 4 * i) = make_float4(q.x / nrm, q.y / nrm, q.z / nrm, q.w / nrm);
      }
      if (sc.opacities_out) sc.opacities_out[i] = act_sigmoid(p_opac[row]);
    }
    float ndcx, ndcy;
    if (proj_in_front(vc, px, py, pz, ndcx, ndcy)) {
      if constexpr (EARLY && KT > 0) {
        if (g.shs) load_row<FH>(g.shs + (size_t)i * FH, shr_h);     // in flight during the footprint arithmetic
      }
      float c6[6];
      if (g.cov3D_precomp) {
#pragma unroll
        for (int k = 0; k < 6; ++k) c6[k] = EARLY ? c6_e[k] : g.cov3D_precomp[6 * i + k];
      } else {
        const float mod = v.scale_modifier;
        float sa[3];
        float4 q;
        if constexpr (EARLY) {
          sa[0] = sa_e[0]; sa[1] = sa_e[1]; sa[2] = sa_e[2]; q = q_e;
        } else {
          sa[0] = p_scale[3 * row]; sa[1] = p_scale[3 * row + 1]; sa[2] = p_scale[3 * row + 2];
          q = *reinterpret_cast<const float4*>(p_rot + 4 * row);
        }
        if constexpr (SCENE) {
          float n[3];
          noise_scale3<GEN>(sc.noise, nstream, i, n);
#pragma unroll
          for (int k = 0; k < 3; ++k) sa[k] = act_scale(sa[k], noise_has_scale<GEN>(sc.noise), n[k]).out;
          const float nrm = act_quat_norm(q);
          q = make_float4(q.x / nrm, q.y / nrm, q.z / nrm, q.w / nrm);
        }
        const float s0 = mod * sa[0], s1 = mod * sa[1], s2 = mod * sa[2];
        float R[9];
        quat_to_R(q, R);
        cov3d_from(s0, s1, s2, R, c6);
      }
      Proj pr;
      proj_footprint(vc, px, py, pz, c6, fx, fy, limx, limy, W, H, gx, gy, ndcx, ndcy, pr);
      radius = pr.radius; ntiles = pr.ntiles; rect = pr.rect;
      if (pr.vis) {
        vis = true;
        q0x = pr.q0x; q0y = pr.q0y; ca_ = pr.ca; cb_ = pr.cb; cc_ = pr.cc; depth = pr.depth;
        if constexpr (EARLY) opac = opac_e;
        else opac = SCENE ? act_sigmoid(p_opac[row]) : p_opac[row];
        tau_ = splat_tau(opac);
      }
    }
  }

  // ---- colour
  float rgb[3] = {0.f, 0.f, 0.f};
  if constexpr (SCENE && KT > 0) {
    // raw leaves, compile-time K: each lane pulls its features_dc / features_rest rows straight into registers
    if (vis) {
      constexpr int F = 3 * KT;
      float shr[F];
      load_row<3>(sc.dc[rw.m] + row * 3, shr);
      if constexpr (KT > 1) load_row<F - 3>(sc.rest[rw.m] + row * (F - 3), shr + 3);
      if constexpr (GEN) {
        if (noise_has_sh<GEN>(sc.noise)) sh_noise_apply<GEN, F>(sc.noise, nstream, i, shr);
      } else if (sc.noise.sh) {
        float nz[F];
        load_row<F>(sc.noise.sh + (size_t)i * F, nz);
#pragma unroll
        for (int k = 0; k < F; ++k) shr[k] = shr[k] + nz[k] * (kSqrtPoint2 * shr[k]);
      }
      const ViewDir d = view_dir(vc, px, py, pz);
      float b[16];
      sh_basis(vd.sh_degree, d.x, d.y, d.z, b);
      float acc[3];
      sh_colour_n<KT>(vd.sh_degree, shr, b, acc);
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[c] = fmaxf(acc[c] + 0.5f, 0.0f);
    }
  } else if (!SCENE && g.shs && KT > 0) {
    // compile-time SH stride: every lane pulls its own 12*KT-byte row straight into registers (measured faster
    // than the coalesced-load + LDS-transpose path K8 uses for its read-modify-write of the same block: the rows
    // of a wave are contiguous, so L1/TA serve the 16-byte pieces of one line to successive loads)
    // (the row was requested in front of the footprint arithmetic: shr_h; this arm is never taken with KT == 0)
    if constexpr (KT > 0) {
      if (vis) {
        float shr[3 * KT];
#pragma unroll
        for (int q = 0; q < 3 * KT; ++q) shr[q] = shr_h[q];
        const ViewDir d = view_dir(vc, px, py, pz);
        float b[16];
        sh_basis(vd.sh_degree, d.x, d.y, d.z, b);
        float acc[3];
        sh_colour_n<KT>(vd.sh_degree, shr, b, acc);
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = fmaxf(acc[c] + 0.5f, 0.0f);
      }
    }
  } else if (SCENE || g.shs) {
    const unsigned long long vmask = __ballot(vis);
    float* lw = lds + wave * (64 * sh_lds_stride(K));
    if constexpr (SCENE) {
      // features_dc / features_rest rows of the wave, side by side in the lanes' LDS rows; then the SH noise
      if (vmask) {
        stage_rows_in(sc.dc[rw.m] + wave_first * 3, 3, 0, sh_lds_stride(K), n_valid, vmask, lw);
        if (K > 1) stage_rows_in(sc.rest[rw.m] + wave_first * (3 * K - 3), 3 * K - 3, 3, sh_lds_stride(K), n_valid, vmask, lw);
      }
      if (noise_has_sh<GEN>(sc.noise) && vis) {
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        float* shw = lw + lane * sh_lds_stride(K);
        if constexpr (GEN) {
          sh_noise_apply_n<GEN>(sc.noise, nstream, i, 3 * K, shw);
        } else {
          const float* nz = sc.noise.sh + (size_t)i * (3 * K);
          for (int k = 0; k < 3 * K; ++k) shw[k] = shw[k] + nz[k] * (kSqrtPoint2 * shw[k]);
        }
      }
    } else if (vmask) stage_sh_in<KT>(g.shs, wave_first, n_valid, K, vmask, lw);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (vis) {
      const ViewDir d = view_dir(vc, px, py, pz);
      float b[16];
      sh_basis(vd.sh_degree, d.x, d.y, d.z, b);
      float acc[3];
      sh_colour(vd.sh_degree, lw + lane * sh_lds_stride(K), b, acc);
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[c] = fmaxf(acc[c] + 0.5f, 0.0f);
    }
  } else if (vis) {
    rgb[0] = g.colors_precomp[3 * i]; rgb[1] = g.colors_precomp[3 * i + 1]; rgb[2] = g.colors_precomp[3 * i + 2];
  }

  if (rw.ok) {
    radii[i] = radius;
    tiles_touched[i] = ntiles;
    depth_keys[i] = vis ? __float_as_uint(depth) : 0xFFFFFFFFu;   // culled Gaussians are dropped by the depth sort
    rects[i] = rect;
    if (vis) {
      float4* o = reinterpret_cast<float4*>(splat + 12 * i);
      o[0] = make_float4(q0x, q0y, ca_, cb_);
      o[1] = make_float4(cc_, opac, depth, rgb[0]);
      o[2] = make_float4(rgb[1], rgb[2], tau_, 0.f);
    }
  }
}

// ------------------------------------------------------------------------------------------- K1 over several views
// The parameter rows (44 + 12K bytes per Gaussian) are read once for all views of a step; per view only the 48-byte
// splat record, radius, tile count, depth key and tile rectangle are written. cov3D is view independent.
struct K1Views {
  int32_t nv;
  const float* viewmatrix[GSR_MAX_BATCH_VIEWS];
  const float* projmatrix[GSR_MAX_BATCH_VIEWS];
  const float* campos[GSR_MAX_BATCH_VIEWS];
  float tanfovx[GSR_MAX_BATCH_VIEWS];
  float tanfovy[GSR_MAX_BATCH_VIEWS];
  int32_t sh_degree[GSR_MAX_BATCH_VIEWS];
  const float* dyn[GSR_MAX_BATCH_VIEWS];    // GsrView.dynamic of every view (NULL: the by-value entries above)
  int32_t per_view_scales;
  const float* scales[GSR_MAX_BATCH_VIEWS];
  // scene input (raw leaves): per-view noise samples and the per-view activated scales handed back to the caller
  NoiseViews noise;
  float* scales_out[GSR_MAX_BATCH_VIEWS];
  float* splat[GSR_MAX_BATCH_VIEWS];
  int32_t* radii[GSR_MAX_BATCH_VIEWS];
  uint32_t* tiles_touched[GSR_MAX_BATCH_VIEWS];
  uint32_t* depth_keys[GSR_MAX_BATCH_VIEWS];
  uint32_t* rects[GSR_MAX_BATCH_VIEWS];
  uint32_t* sort_state[GSR_MAX_BATCH_VIEWS];   // state of the depth sort that follows, cleared here (see k_preprocess)
  uint32_t sort_state_words;
};

__device__ __forceinline__ void k1_clear_sort_state(const K1Views& vb) {
  for (int vv = 0; vv < vb.nv; ++vv)
    for (uint32_t w = blockIdx.x * 256u + threadIdx.x; w < vb.sort_state_words; w += gridDim.x * 256u) vb.sort_state[vv][w] = 0u;
}

template <int KT>
// (4 waves per SIMD: 128 VGPRs instead of 131 at K = 16, no spills -- the kernel is latency-bound on its division chains.
//  Round 6 probe, one call: the SAME kernel without its colour -- no SH row loaded or held, ~60 VGPRs -- takes 11.7 us per view at 4
//  AND at 6 waves per SIMD, 10.0 at 8, against 16.1-17.3 with the colour: the geometry alone is 40-47 us per 4-view step at 3.2 TB/s
//  of its own traffic, whatever the occupancy; the colour adds ~20 us for 96 MB of SH rows, i.e. it already runs at a stream's
//  rate. A geometry pass + a separate colour pass would cost 47 + >= 22 us: the split round 4's review asked for does not pay.)
#ifndef GSR_K1_WAVES
#define GSR_K1_WAVES 4
#endif
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(GSR_K1_WAVES, GSR_K1_WAVES)))
k_preprocess_views(const GsrView v, const GsrGaussians g, const K1Views vb) {
  constexpr int F = 3 * KT;
  const int P = v.P, W = v.image_width, H = v.image_height;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  k1_clear_sort_state(vb);
  if (i >= P) return;
  const int gx = (W + GSR_TILE - 1) / GSR_TILE, gy = (H + GSR_TILE - 1) / GSR_TILE;
  const float px = g.means3D[3 * i], py = g.means3D[3 * i + 1], pz = g.means3D[3 * i + 2];
  // ONE memory round trip in front of the arithmetic instead of three (position -> scales / rotation -> SH row, each
  // issued only after the test that needs the one before): rotation, scales and opacity (32 B) are fetched with the
  // position whatever the tests will say; the SH row (12K B) as soon as the position shows the Gaussian in front of ANY of the
  // views (3 FMAs per view) -- it is in flight while cov3D and the first footprint are computed.
  const float4 q_l = *reinterpret_cast<const float4*>(g.rotations + 4 * i);
  const float opac = g.opacities[i];
  float sl[3] = {0.f, 0.f, 0.f};
  if (!vb.per_view_scales) { const float* sc = vb.scales[0]; sl[0] = sc[3 * i]; sl[1] = sc[3 * i + 1]; sl[2] = sc[3 * i + 2]; }
  bool front_any = false;
  for (int vv = 0; vv < vb.nv; ++vv) {
    gsr_cfloat* V = gsr_const(vb.viewmatrix[vv]);
    front_any |= (((V[2] * px + V[6] * py) + V[10] * pz) + V[14]) > GSR_NEAR_Z;
  }
  if (!front_any) {        // behind every camera: the culled record of every view, and out (no join in front of the loop below:
    for (int vv = 0; vv < vb.nv; ++vv)     // the wait counts of the loads stay exact)
      store_view_ints(vb.radii[vv], vb.tiles_touched[vv], vb.depth_keys[vv], vb.rects[vv], i, 0, 0u, false, 0.f, 0u);
    return;
  }
  float c6[6], shr[F];
  load_row<F>(g.shs + (size_t)i * F, shr);
  if (!vb.per_view_scales) {
    const float mod = v.scale_modifier;
    float R[9];
    quat_to_R(q_l, R);
    cov3d_from(mod * sl[0], mod * sl[1], mod * sl[2], R, c6);
  }
  const float tau = splat_tau(opac);
  // View 0 is peeled: the wait for the SH row stands behind its footprint arithmetic and in front of its stores, so the
  // loop over the other views has no load of the prologue pending -- a wait INSIDE the loop would also wait for the
  // previous view's stores (on gfx9 loads and stores share vmcnt and complete in order).
  auto one_view = [&](const int vv, auto first) {
    ViewConst vc;
    load_view_const(vb.viewmatrix[vv], vb.projmatrix[vv], vb.campos[vv], vc);
    const ViewDyn vd = view_dyn(vb.dyn[vv], vb.tanfovx[vv], vb.tanfovy[vv], vb.sh_degree[vv]);
    const float tfx = vd.tanfovx, tfy = vd.tanfovy;
    const float fx = (float)W / (2.0f * tfx), fy = (float)H / (2.0f * tfy);
    Proj pr;
    pr.vis = false; pr.radius = 0; pr.ntiles = 0; pr.rect = 0;
    float ndcx, ndcy;
    if (proj_in_front(vc, px, py, pz, ndcx, ndcy)) {
      if (vb.per_view_scales) {
        const float mod = v.scale_modifier;
        const float* sc = vb.scales[vv];
        const float s0 = mod * sc[3 * i], s1 = mod * sc[3 * i + 1], s2 = mod * sc[3 * i + 2];
        float R[9];
        quat_to_R(q_l, R);
        cov3d_from(s0, s1, s2, R, c6);
      }
      proj_footprint(vc, px, py, pz, c6, fx, fy, 1.3f * tfx, 1.3f * tfy, W, H, gx, gy, ndcx, ndcy, pr);
    }
    if constexpr (decltype(first)::value) {
#pragma unroll
      for (int k = 0; k < F; ++k) asm volatile("" : "+v"(shr[k]));
    }
    float rgb[3] = {0.f, 0.f, 0.f};
    if (pr.vis) {
      const ViewDir d = view_dir(vc, px, py, pz);
      float b[16];
      sh_basis(vd.sh_degree, d.x, d.y, d.z, b);
      float acc[3];
      sh_colour_n<KT>(vd.sh_degree, shr, b, acc);
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[c] = fmaxf(acc[c] + 0.5f, 0.0f);
    }
    store_view_ints(vb.radii[vv], vb.tiles_touched[vv], vb.depth_keys[vv], vb.rects[vv], i, pr.radius, pr.ntiles, pr.vis,
                    pr.depth, pr.rect);
    if (pr.vis) {
      float4* o = reinterpret_cast<float4*>(vb.splat[vv] + 12 * i);
      o[0] = make_float4(pr.q0x, pr.q0y, pr.ca, pr.cb);
      o[1] = make_float4(pr.cc, opac, pr.depth, rgb[0]);
      o[2] = make_float4(rgb[1], rgb[2], tau, 0.f);
    }
  };
  one_view(0, std::true_type{});
  for (int vv = 1; vv < vb.nv; ++vv) one_view(vv, std::false_type{});
}

// K1 over several views of a SCENE (raw leaves of several models, activations fused; see k_preprocess<K, true>): the
// raw rows are read once, exp / normalize / sigmoid are applied once, the per-view scale noise (and SH noise) per view.
template <int KT, bool GEN = false>
__global__ void __launch_bounds__(256)
k_preprocess_views_scene(const GsrView v, const SceneTab sc, const K1Views vb) {
  constexpr int F = 3 * KT;
  const int W = v.image_width, H = v.image_height;
  k1_clear_sort_state(vb);
  const Rows rw = resolve_rows<true>(sc, v.P);
  if (!rw.ok) return;
  const int64_t i = rw.i, row = rw.row;
  const int m = rw.m;
  const int gx = (W + GSR_TILE - 1) / GSR_TILE, gy = (H + GSR_TILE - 1) / GSR_TILE;
  const float* xyz = sc.xyz[m];
  const float px = xyz[3 * row], py = xyz[3 * row + 1], pz = xyz[3 * row + 2];
  float aact[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) aact[k] = expf(sc.scaling[m][3 * row + k]);
  bool have_R = false, have_cov = false, have_sh = false;
  float R[9], c6[6], shr[F];
  float opac = 0.f, tau = -1.f;
  for (int vv = 0; vv < vb.nv; ++vv) {
    const NoiseSrc nz = vb.noise.view(vv);
    const uint32_t nstream = noise_stream<GEN>(nz);
    const bool sn = noise_has_scale<GEN>(nz);
    float sa[3], nsc[3];
    noise_scale3<GEN>(nz, nstream, i, nsc);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      sa[k] = sn ? fmaxf(aact[k] + nsc[k] * ((kSqrtPoint2 * aact[k]) / 4.0f), 0.0f) : aact[k];
    if (vb.scales_out[vv]) {
      float* so = vb.scales_out[vv];
      so[3 * i] = sa[0]; so[3 * i + 1] = sa[1]; so[3 * i + 2] = sa[2];
    }
    ViewConst vc;
    load_view_const(vb.viewmatrix[vv], vb.projmatrix[vv], vb.campos[vv], vc);
    const ViewDyn vd = view_dyn(vb.dyn[vv], vb.tanfovx[vv], vb.tanfovy[vv], vb.sh_degree[vv]);
    const float tfx = vd.tanfovx, tfy = vd.tanfovy;
    const float fx = (float)W / (2.0f * tfx), fy = (float)H / (2.0f * tfy);
    Proj pr;
    pr.vis = false; pr.radius = 0; pr.ntiles = 0; pr.rect = 0;
    float ndcx, ndcy;
    if (proj_in_front(vc, px, py, pz, ndcx, ndcy)) {
      if (!have_R) {
        have_R = true;
        float4 q = *reinterpret_cast<const float4*>(sc.rotation[m] + 4 * row);
        const float nrm = act_quat_norm(q);
        q = make_float4(q.x / nrm, q.y / nrm, q.z / nrm, q.w / nrm);
        quat_to_R(q, R);
      }
      if (!have_cov || sn) {
        have_cov = true;
        const float mod = v.scale_modifier;
        cov3d_from(mod * sa[0], mod * sa[1], mod * sa[2], R, c6);
      }
      proj_footprint(vc, px, py, pz, c6, fx, fy, 1.3f * tfx, 1.3f * tfy, W, H, gx, gy, ndcx, ndcy, pr);
    }
    float rgb[3] = {0.f, 0.f, 0.f};
    if (pr.vis) {
      if (!have_sh) {
        have_sh = true;
        load_row<3>(sc.dc[m] + row * 3, shr);
        if constexpr (KT > 1) load_row<F - 3>(sc.rest[m] + row * (F - 3), shr + 3);
        opac = act_sigmoid(sc.opacity[m][row]);
        tau = splat_tau(opac);
      }
      const ViewDir d = view_dir(vc, px, py, pz);
      float b[16];
      sh_basis(vd.sh_degree, d.x, d.y, d.z, b);
      float acc[3];
      if (noise_has_sh<GEN>(nz)) {
        float shv[F];
        if constexpr (GEN) {
#pragma unroll
          for (int k = 0; k < F; ++k) shv[k] = shr[k];
          sh_noise_apply<GEN, F>(nz, nstream, i, shv);
        } else {
          const float* nr = nz.sh + (size_t)i * F;
#pragma unroll
          for (int k = 0; k < F; ++k) shv[k] = shr[k] + nr[k] * (kSqrtPoint2 * shr[k]);
        }
        sh_colour_n<KT>(vd.sh_degree, shv, b, acc);
      } else {
        sh_colour_n<KT>(vd.sh_degree, shr, b, acc);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[c] = fmaxf(acc[c] + 0.5f, 0.0f);
    }
    vb.radii[vv][i] = pr.radius;
    vb.tiles_touched[vv][i] = pr.ntiles;
    vb.depth_keys[vv][i] = pr.vis ? __float_as_uint(pr.depth) : 0xFFFFFFFFu;
    vb.rects[vv][i] = pr.rect;
    if (pr.vis) {
      float4* o = reinterpret_cast<float4*>(vb.splat[vv] + 12 * i);
      o[0] = make_float4(pr.q0x, pr.q0y, pr.ca, pr.cb);
      o[1] = make_float4(pr.cc, opac, pr.depth, rgb[0]);
      o[2] = make_float4(rgb[1], rgb[2], tau, 0.f);
    }
  }
}

// The tensors the generator stands for (gsr_noise_fill): one thread per Philox block -- block 0 of a Gaussian is its scale
// noise, block 1 + j is block j of its SH noise. The values are formed by the function K1 and K8 call (noise_block), under
// the same -ffp-contract=off: a scene fed with these tensors sees the same bits.
__global__ void __launch_bounds__(256)
k_noise_fill(const NoiseSrc z, const int64_t P, const int F, float* __restrict__ scale_noise, float* __restrict__ sh_noise) {
  const int nb = 1 + (F + 3) / 4;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i = t / nb;
  const int b = (int)(t - i * nb);
  if (i >= P) return;
  const uint32_t stream = noise_stream<true>(z);
  float n[4];
  if (b == 0) {
    if (!scale_noise) return;
    noise_block(z.seed_lo, z.seed_hi, stream, kNoiseTagScale, (uint32_t)i, 0u, n);
#pragma unroll
    for (int k = 0; k < 3; ++k) scale_noise[3 * i + k] = n[k];
  } else {
    if (!sh_noise) return;
    const int j = b - 1;
    noise_block(z.seed_lo, z.seed_hi, stream, kNoiseTagSh, (uint32_t)i, (uint32_t)j, n);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * j + e < F) sh_noise[i * F + 4 * j + e] = n[e];
  }
}

}  // namespace

int gsr_launch_noise_fill(uint64_t seed, uint32_t stream, const uint32_t* stream_dev, int32_t P, int32_t K,
                          float* scale_noise, float* sh_noise, hipStream_t hip_stream) {
  NoiseSrc z = NoiseSrc{};
  z.stream_dev = stream_dev; z.stream = stream;
  z.seed_lo = (uint32_t)seed; z.seed_hi = (uint32_t)(seed >> 32);
  const int F = 3 * K;
  const int64_t threads = (int64_t)P * (1 + (F + 3) / 4);
  hipLaunchKernelGGL(k_noise_fill, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, hip_stream, z, (int64_t)P, F,
                     scale_noise, sh_noise);
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

uint32_t* gsr_depth_keys(const GsrGeom& geom, int32_t P);   // binning.hip: first key buffer of the depth sort
uint32_t* gsr_depth_sort_state(const GsrGeom& geom, int32_t P, uint32_t* words);   // binning.hip: state K1 clears for the sort
uint32_t* gsr_tile_rects(const GsrGeom& geom, int32_t P);   // binning.hip: packed tile rectangles, one per Gaussian

int gsr_launch_preprocess(const GsrView& v, const GsrGaussians& g, GsrGeom& geom, hipStream_t stream) {
  uint32_t ss_words = 0;
  uint32_t* ss = gsr_depth_sort_state(geom, v.P, &ss_words);
  if (g.scene) {
    SceneTab t; SceneGradTab gt;
    const uint32_t nbs = scene_tables(*g.scene, nullptr, t, gt);
    const size_t lds = gsr_preprocess_lds_bytes(v.sh_stride);
    return launch_sh<16, 9, 4, 1, 0>(fixed_sh(v.sh_stride), [&](auto kt) {
      with_flag(scene_noise_generated(1, &g), [&](auto gen) {
        hipLaunchKernelGGL((k_preprocess<kt, true, SceneTab, gen>), dim3(nbs), dim3(256), kt > 0 ? 0 : lds, stream, v, g, t,
                           geom.splat, geom.radii, geom.tiles_touched, gsr_depth_keys(geom, v.P),
                           gsr_tile_rects(geom, v.P), ss, ss_words);
      });
    });
  }
  const uint32_t nb = gsr_num_blocks(v.P);
  const size_t lds = g.shs ? gsr_preprocess_lds_bytes(v.sh_stride) : 0;
  return launch_sh<16, 9, 4, 1, 0>(fixed_sh(g.shs ? v.sh_stride : 0), [&](auto kt) {
    hipLaunchKernelGGL(k_preprocess<kt>, dim3(nb), dim3(256), kt > 0 ? 0 : lds, stream, v, g, NoScene{}, geom.splat,
                       geom.radii, geom.tiles_touched, gsr_depth_keys(geom, v.P), gsr_tile_rects(geom, v.P), ss, ss_words);
  });
}

// K1 for n_views views of the same Gaussians in one pass (shs with K in {1,4,9,16}, scales + rotations, no scene table).
bool gsr_preprocess_views_supported(const GsrView& v, const GsrGaussians& g) {
  const int K = v.sh_stride;
  if (g.scene) return K == 1 || K == 4 || K == 9 || K == 16;
  return g.shs && !g.scene && g.scales && g.rotations && !g.cov3D_precomp && !g.colors_precomp &&
         (K == 1 || K == 4 || K == 9 || K == 16);
}

// The generator parameters of a batch travel compactly (NoiseViews): one seed, and device stream words that are consecutive.
bool gsr_batch_noise_fits(int n_views, const GsrGaussians* gs) {
  const GsrScene* first = nullptr;
  int kf = 0;
  for (int k = 0; k < n_views; ++k) {
    const GsrScene* sc = gs[k].scene;
    if (!sc || !sc->noise_flags) continue;
    if (!first) { first = sc; kf = k; continue; }
    if (sc->noise_seed != first->noise_seed || (sc->noise_stream_dev != nullptr) != (first->noise_stream_dev != nullptr)) return false;
    if (sc->noise_stream_dev && sc->noise_stream_dev != first->noise_stream_dev + (k - kf)) return false;
  }
  return true;
}

int gsr_launch_preprocess_views(int n_views, const GsrView* views, const GsrGaussians* gs, GsrGeom* geoms,
                                hipStream_t stream) {
  const GsrGaussians& g = gs[0];
  K1Views vb = K1Views{};
  vb.nv = n_views;
  fill_view_fields(vb, n_views, views, gs);
  for (int k = 0; k < n_views; ++k) {
    if (g.scene) vb.scales_out[k] = gs[k].scene->scales_out;
    vb.splat[k] = geoms[k].splat; vb.radii[k] = geoms[k].radii; vb.tiles_touched[k] = geoms[k].tiles_touched;
    vb.depth_keys[k] = gsr_depth_keys(geoms[k], views[k].P); vb.rects[k] = gsr_tile_rects(geoms[k], views[k].P);
    vb.sort_state[k] = gsr_depth_sort_state(geoms[k], views[k].P, &vb.sort_state_words);
  }
  const GsrView& v = views[0];
  if (g.scene) {
    SceneTab t; SceneGradTab gt;
    const uint32_t nbs = scene_tables(*g.scene, nullptr, t, gt);
    return launch_sh<16, 9, 4, 1>(v.sh_stride, [&](auto kt) {
      with_flag(scene_noise_generated(n_views, gs), [&](auto gen) {
        hipLaunchKernelGGL((k_preprocess_views_scene<kt, gen>), dim3(nbs), dim3(256), 0, stream, v, t, vb);
      });
    });
  }
  const uint32_t nb = gsr_num_blocks(v.P);
  return launch_sh<16, 9, 4, 1>(v.sh_stride, [&](auto kt) {
    hipLaunchKernelGGL(k_preprocess_views<kt>, dim3(nb), dim3(256), 0, stream, v, g, vb);
  });
}

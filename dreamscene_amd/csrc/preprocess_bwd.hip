// preprocess_bwd.hip -- K8, the backward of K1 (preprocess.hip; kernel forms, traffic and the -ffp-contract=off build: see
// there), gfx950. K8 recomputes K1's projection with the statements of gsr_project.h: same order, same values.
#include "gsr_project.h"
#include "gsr_launch.h"
#include <cstdlib>

namespace {

// LDS rows (float offset o0, F floats each) -> the wave's contiguous [n_valid, F] block in global memory, 16 bytes
// per lane and step. F == 0: runtime row length Fr. Rows of culled Gaussians hold zeros (the caller cleared them), so
// accumulating adds nothing there; 16-byte pieces that only cover culled rows are skipped when accumulating.
template <int F>
__device__ __forceinline__ void stage_rows_out(float* __restrict__ dst, int Fr, int o0, int lds_stride, int n_valid,
                                               const float* lds_wave, bool accumulate, unsigned long long vis) {
  const int FF = F > 0 ? F : Fr;
  const int total = n_valid * FF;
  const int lane = gsr_lane();
  for (int q = lane * 4; q < total; q += 64 * 4) {
    const int g0 = q / FF, g1 = min(n_valid - 1, (q + 3) / FF);
    if (accumulate && !(((vis >> g0) | (vis >> g1)) & 1ull)) continue;
    float e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int f = q + k;
      const int g = f / FF, o = f - g * FF;
      e[k] = (f < total) ? lds_wave[g * lds_stride + o0 + o] : 0.f;
    }
    if (q + 3 < total) {
      float4 o = make_float4(e[0], e[1], e[2], e[3]);
      if (accumulate) {
        const float4 old = *reinterpret_cast<const float4*>(dst + q);
        o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w;
      }
      *reinterpret_cast<float4*>(dst + q) = o;
    } else {
      for (int k = 0; k < 4; ++k)
        if (q + k < total) dst[q + k] = accumulate ? dst[q + k] + e[k] : e[k];
    }
  }
}

// LDS -> global coalesced store of the wave's [n_valid, 3K] block.
template <int KT>
__device__ __forceinline__ void stage_sh_out(float* __restrict__ dst_base, int64_t wave_first, int n_valid, int K,
                                             const float* lds_wave, bool accumulate) {
  const int F = KT > 0 ? 3 * KT : 3 * K;
  const int stride = F | 1;
  const int total = n_valid * F;
  float* dst = dst_base + wave_first * (int64_t)F;
  const int lane = gsr_lane();
  for (int q = lane * 4; q < total; q += 64 * 4) {
    float e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int f = q + k;
      const int g = f / F, o = f - g * F;
      e[k] = (f < total) ? lds_wave[g * stride + o] : 0.f;
    }
    if (q + 3 < total) {
      float4 o = make_float4(e[0], e[1], e[2], e[3]);
      if (accumulate) {
        const float4 old = *reinterpret_cast<const float4*>(dst + q);
        o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w;
      }
      *reinterpret_cast<float4*>(dst + q) = o;
    } else {
      for (int k = 0; k < 4; ++k)
        if (q + k < total) dst[q + k] = accumulate ? dst[q + k] + e[k] : e[k];
    }
  }
}

// d colour / d (unit view direction), contracted with s_k = <sh_k, dL/dcolour>: the derivative of the SH basis
__device__ __forceinline__ void sh_ddir(int D, float x, float y, float z, const float s[16], float& ddx, float& ddy,
                                        float& ddz) {
  ddx = 0.f; ddy = 0.f; ddz = 0.f;
  if (D > 0) {
    ddy += -GSR_SH_C1 * s[1]; ddz += GSR_SH_C1 * s[2]; ddx += -GSR_SH_C1 * s[3];
    if (D > 1) {
      const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
      ddx += GSR_SH_C2_0 * y * s[4] + GSR_SH_C2_2 * (-2.0f * x) * s[6] + GSR_SH_C2_3 * z * s[7] + GSR_SH_C2_4 * 2.0f * x * s[8];
      ddy += GSR_SH_C2_0 * x * s[4] + GSR_SH_C2_1 * z * s[5] + GSR_SH_C2_2 * (-2.0f * y) * s[6] + GSR_SH_C2_4 * (-2.0f * y) * s[8];
      ddz += GSR_SH_C2_1 * y * s[5] + GSR_SH_C2_2 * 4.0f * z * s[6] + GSR_SH_C2_3 * x * s[7];
      if (D > 2) {
        ddx += GSR_SH_C3_0 * 6.0f * xy * s[9] + GSR_SH_C3_1 * yz * s[10] + GSR_SH_C3_2 * (-2.0f * xy) * s[11] +
               GSR_SH_C3_3 * (-6.0f * xz) * s[12] + GSR_SH_C3_4 * (4.0f * zz - 3.0f * xx - yy) * s[13] +
               GSR_SH_C3_5 * 2.0f * xz * s[14] + GSR_SH_C3_6 * 3.0f * (xx - yy) * s[15];
        ddy += GSR_SH_C3_0 * 3.0f * (xx - yy) * s[9] + GSR_SH_C3_1 * xz * s[10] +
               GSR_SH_C3_2 * (4.0f * zz - xx - 3.0f * yy) * s[11] + GSR_SH_C3_3 * (-6.0f * yz) * s[12] +
               GSR_SH_C3_4 * (-2.0f * xy) * s[13] + GSR_SH_C3_5 * (-2.0f * yz) * s[14] + GSR_SH_C3_6 * (-6.0f * xy) * s[15];
        ddz += GSR_SH_C3_1 * xy * s[10] + GSR_SH_C3_2 * 8.0f * yz * s[11] +
               GSR_SH_C3_3 * (6.0f * zz - 3.0f * xx - 3.0f * yy) * s[12] + GSR_SH_C3_4 * 8.0f * xz * s[13] +
               GSR_SH_C3_5 * (xx - yy) * s[14];
      }
    }
  }
}

// Steps (2a)-(5) of K8 for one view: K7's moments -> dL/d(ndc xy), dL/dconic -> cov2D -> dL/dSigma (dS, assigned) and
// the position terms (added to dp); camera gradients (assigned) when want_cam.
__device__ __forceinline__ void geom_backward(const ViewConst& vc, const Ewa& e, float fx, float fy, int W, int H,
                                              float px, float py, float pz, float S1, float S2, float S3, float S4,
                                              float S5, float gdep, bool want_cam, float& gndx, float& gndy,
                                              float dS[9], float dp[3], float dview[12], float dproj[12]) {
  const float* V = vc.V;
  const float* PV = vc.PV;
  // (2) K7's sums -> dL/d(ndc xy) and dL/dcov2D. With d = centre - pixel, (u, v) = -conic d and q = dL/dG G per pixel:
  // S1 = sum q u, S2 = sum q v are dL/d(pixel centre); dL/dSigma = 1/2 sum q (conic d)(conic d)^T, i.e. S3 = sum q u^2,
  // S4 = sum q u v, S5 = sum q v^2 are the covariance gradient up to the factors below -- K7 forms them per pixel
  // (render_bwd.hip). The lineage goes through dL/dconic and divides by det^2 + 1e-7 instead of det^2: the factor
  // det^2 / (det^2 + 1e-7) keeps that regulariser (SEMANTICS.md section 5).
  gndx = S1 * (0.5f * (float)W);
  gndy = S2 * (0.5f * (float)H);
  const float det2 = e.det * e.det;
  const float reg = det2 * (1.0f / (det2 + 0.0000001f));
  const float dca = (0.5f * S3) * reg, dcb = S4 * reg, dcc = (0.5f * S5) * reg;
  // (3) cov2D = M Sigma M^T
  const float h = 0.5f * dcb;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      dS[3 * r + c] = (e.M0[r] * (dca * e.M0[c] + h * e.M1[c])) + (e.M1[r] * (h * e.M0[c] + dcc * e.M1[c]));
  float dM0[3], dM1[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    dM0[j] = 2.0f * (dca * e.U0[j] + h * e.U1[j]);
    dM1[j] = 2.0f * (h * e.U0[j] + dcc * e.U1[j]);
  }
  const float dJ00 = (dM0[0] * V[0] + dM0[1] * V[4]) + dM0[2] * V[8];
  const float dJ02 = (dM0[0] * V[2] + dM0[1] * V[6]) + dM0[2] * V[10];
  const float dJ11 = (dM1[0] * V[1] + dM1[1] * V[5]) + dM1[2] * V[9];
  const float dJ12 = (dM1[0] * V[2] + dM1[1] * V[6]) + dM1[2] * V[10];
  const float tzi = 1.0f / e.tz, tz2 = tzi * tzi, tz3 = tz2 * tzi;
  float dt[3];
  dt[0] = e.clx ? 0.0f : (-fx * tz2 * dJ02);
  dt[1] = e.cly ? 0.0f : (-fy * tz2 * dJ12);
  dt[2] = ((-fx * tz2 * dJ00 - fy * tz2 * dJ11) + (2.0f * fx * e.txc) * tz3 * dJ02) + (2.0f * fy * e.tyc) * tz3 * dJ12;
  dt[2] += gdep;                                                               // (5) depth
#pragma unroll
  for (int r = 0; r < 3; ++r) dp[r] += (V[4 * r] * dt[0] + V[4 * r + 1] * dt[1]) + V[4 * r + 2] * dt[2];
  // (4) ndc -> p
  const float hx = ((PV[0] * px + PV[4] * py) + PV[8] * pz) + PV[12];
  const float hy = ((PV[1] * px + PV[5] * py) + PV[9] * pz) + PV[13];
  const float hw = ((PV[3] * px + PV[7] * py) + PV[11] * pz) + PV[15];
  const float pw = 1.0f / (hw + 0.0000001f);
  const float dh[3] = {pw * gndx, pw * gndy, -(pw * pw) * (hx * gndx + hy * gndy)};
#pragma unroll
  for (int r = 0; r < 3; ++r) dp[r] += (PV[4 * r] * dh[0] + PV[4 * r + 1] * dh[1]) + PV[4 * r + 3] * dh[2];

  if (want_cam) {
    const float p4[4] = {px, py, pz, 1.0f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) dview[3 * r + c] = p4[r] * dt[c];
      dproj[3 * r + 0] = p4[r] * dh[0];
      dproj[3 * r + 1] = p4[r] * dh[1];
      dproj[3 * r + 2] = p4[r] * dh[2];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      dview[3 * r + 0] += e.J00 * dM0[r];
      dview[3 * r + 1] += e.J11 * dM1[r];
      dview[3 * r + 2] += e.J02 * dM0[r] + e.J12 * dM1[r];
    }
  }
}

// Step (6) of K8: dL/dSigma -> dL/dscale (of the scales as given) and dL/dquaternion (of the quaternion as given).
__device__ __forceinline__ void sigma_backward(const float dS[9], const float R[9], const float s3[3], float mod,
                                               const float4 q, float dscale[3], float drot[4]) {
  float L[9], dL[9], dR[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b2 = 0; b2 < 3; ++b2) L[3 * a + b2] = R[3 * a + b2] * s3[b2];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b2 = 0; b2 < 3; ++b2) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) acc += (dS[3 * a + k] + dS[3 * k + a]) * L[3 * k + b2];
      dL[3 * a + b2] = acc;
    }
#pragma unroll
  for (int b2 = 0; b2 < 3; ++b2) {
    const float ds = (dL[b2] * R[b2] + dL[3 + b2] * R[3 + b2]) + dL[6 + b2] * R[6 + b2];
    dscale[b2] = mod * ds;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b2 = 0; b2 < 3; ++b2) dR[3 * a + b2] = dL[3 * a + b2] * s3[b2];
  const float r = q.x, x = q.y, y = q.z, z = q.w;
  drot[0] = 2.0f * (-z * dR[1] + y * dR[2] + z * dR[3] - x * dR[5] - y * dR[6] + x * dR[7]);
  drot[1] = 2.0f * (y * dR[1] + z * dR[2] + y * dR[3] - 2.0f * x * dR[4] - r * dR[5] + z * dR[6] + r * dR[7] - 2.0f * x * dR[8]);
  drot[2] = 2.0f * (-2.0f * y * dR[0] + x * dR[1] + r * dR[2] + x * dR[3] + z * dR[5] - r * dR[6] + z * dR[7] - 2.0f * y * dR[8]);
  drot[3] = 2.0f * (-2.0f * z * dR[0] - r * dR[1] + x * dR[2] + r * dR[3] - 2.0f * z * dR[4] + y * dR[5] + x * dR[6] + y * dR[7]);
}
// Scene input: d(returned scale)/d(raw scaling) = exp(raw) * (1 + n sqrt(0.2)/4) where the clamp passes (torch.clamp:
// pre >= 0). act = exp(raw), pre = the noisy scale in front of the clamp (ActScale).
__device__ __forceinline__ float scale_draw(float act, float pre, bool noisy, float n) {
  return noisy ? (pre >= 0.0f ? act * (1.0f + n * (kSqrtPoint2 / 4.0f)) : 0.0f) : act;
}
// ---- K7's per-Gaussian sums: a row of 16 doubles, 12 used (render_bwd.hip, render_bwd_body) -- wave results added across
// waves in double, rounded to fp32 HERE, once. partial_rows() hands them out as the chain rule below was written:
// a = (S1, S2, S3, S4), b = (S5, dL/dopacity, r, g), c = (b, depth, b', depth').
struct PartialRaw { float4 w[6]; };     // as loaded: 12 doubles, still raw bits (conversions wait for the loads: do them late)
__device__ __forceinline__ PartialRaw partial_load(const float* __restrict__ partials, int64_t i) {
  const float4* pp = reinterpret_cast<const float4*>(partials + GSR_PARTIAL_WORDS * i);
  PartialRaw r;
#pragma unroll
  for (int k = 0; k < 6; ++k) r.w[k] = pp[k];
  return r;
}
__device__ __forceinline__ PartialRaw partial_none() {
  PartialRaw r;
#pragma unroll
  for (int k = 0; k < 6; ++k) r.w[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  return r;
}
__device__ __forceinline__ float f64_words(float lo, float hi) {
  return (float)__hiloint2double(__float_as_int(hi), __float_as_int(lo));
}
__device__ __forceinline__ void partial_rows(const PartialRaw& r, float4& a, float4& b, float4& c) {
  a = make_float4(f64_words(r.w[0].x, r.w[0].y), f64_words(r.w[0].z, r.w[0].w), f64_words(r.w[1].x, r.w[1].y), f64_words(r.w[1].z, r.w[1].w));
  b = make_float4(f64_words(r.w[2].x, r.w[2].y), f64_words(r.w[2].z, r.w[2].w), f64_words(r.w[3].x, r.w[3].y), f64_words(r.w[3].z, r.w[3].w));
  c = make_float4(f64_words(r.w[4].x, r.w[4].y), f64_words(r.w[4].z, r.w[4].w), f64_words(r.w[5].x, r.w[5].y), f64_words(r.w[5].z, r.w[5].w));
}
__device__ __forceinline__ void partial_zero(float* __restrict__ partials, int64_t i) {
  float4* pp = reinterpret_cast<float4*>(partials + GSR_PARTIAL_WORDS * i);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < 6; ++k) pp[k] = z;
}

// --------------------------------------------------------------------------------------------------------- K8
// partials [P,16 doubles] from K7 (see above): S1 = sum q u, S2 = sum q v, S3 = sum q u^2, S4 = sum q u v, S5 = sum q v^2
// [(u, v) = -conic d], dL/dopacity, dL/dr, dL/dg, dL/db, dL/ddepth; q = dL/dG * G
// GEN (scene only): the noise K1 drew from the generator is regenerated here (NoiseSrc, gsr_project.h).
template <int KT, bool SCENE = false, typename TAB = NoScene, typename GTAB = NoScene, bool GEN = false>
__global__ void __launch_bounds__(256)
k_preprocess_bwd(const GsrView v, const GsrGaussians g, const TAB sc, const GTAB sg,
                 const int32_t* __restrict__ radii, const float* __restrict__ partials, const GsrGrads out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float cam_red[4][32];
  const ViewDyn vd = view_dyn(v.dynamic, v.tanfovx, v.tanfovy, v.sh_degree);
  const int P = v.P, W = v.image_width, H = v.image_height, K = KT > 0 ? KT : v.sh_stride, D = vd.sh_degree;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const Rows rw = resolve_rows<SCENE>(sc, P);
  const int64_t i = rw.i, row = rw.row, wave_first = rw.wave_row;
  const int n_valid = rw.n_valid;
  const float *p_xyz = g.means3D, *p_scale = g.scales, *p_rot = g.rotations;
  [[maybe_unused]] uint32_t nstream = 0u;
  if constexpr (SCENE) {
    p_xyz = sc.xyz[rw.m]; p_scale = sc.scaling[rw.m]; p_rot = sc.rotation[rw.m];
    nstream = noise_stream<GEN>(sc.noise);
  }
  const float fx = (float)W / (2.0f * vd.tanfovx), fy = (float)H / (2.0f * vd.tanfovy);
  const float limx = 1.3f * vd.tanfovx, limy = 1.3f * vd.tanfovy;
  const float mod = v.scale_modifier;
  const bool want_cam = (out.dL_dview != nullptr) || (out.dL_dproj != nullptr) || (out.dL_dcampos != nullptr);

  ViewConst vc;
  load_view(v, vc);

  const bool vis = rw.ok && (radii[i] > 0);
  float px = 0, py = 0, pz = 0;
  float4 pa = make_float4(0, 0, 0, 0), pb = pa, pc = pa;
  if (vis) {
    px = p_xyz[3 * row]; py = p_xyz[3 * row + 1]; pz = p_xyz[3 * row + 2];
    partial_rows(partial_load(partials, i), pa, pb, pc);
    pc.x += pc.z; pc.y += pc.w;      // (K7 commits the last two sums from the two halves of a wave: render_bwd.hip, reduce10)
  }
  const float S1 = pa.x, S2 = pa.y, S3 = pa.z, S4 = pa.w, S5 = pb.x, gop = pb.y;
  float gndx = 0.f, gndy = 0.f;
  const float grgb[3] = {pb.z, pb.w, pc.x};
  const float gdep = pc.y;

  float dp[3] = {0.f, 0.f, 0.f};
  float dview[12];   // rows 0..3 x cols 0..2 of dL/dviewmatrix
  float dproj[12];   // rows 0..3 x cols {0,1,3} of dL/dprojmatrix
  float dcam[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 12; ++k) { dview[k] = 0.f; dproj[k] = 0.f; }

  // ---- (1) colour -> SH coefficients, view direction
  if (SCENE || g.shs) {
    const unsigned long long vmask = __ballot(vis);
    const int stride = sh_lds_stride(K);
    float* lw = lds + wave * (64 * stride);
    float* sh = lw + lane * stride;
    if constexpr (SCENE) {
      if constexpr (KT > 0) {
        if (vis) {   // each lane parks its own rows in its LDS row
          load_row<3>(sc.dc[rw.m] + row * 3, sh);
          if constexpr (KT > 1) load_row<3 * KT - 3>(sc.rest[rw.m] + row * (3 * KT - 3), sh + 3);
        }
      } else {
        if (vmask) {
          stage_rows_in(sc.dc[rw.m] + wave_first * 3, 3, 0, stride, n_valid, vmask, lw);
          if (K > 1) stage_rows_in(sc.rest[rw.m] + wave_first * (3 * K - 3), 3 * K - 3, 3, stride, n_valid, vmask, lw);
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      }
      if (noise_has_sh<GEN>(sc.noise) && vis) {   // the augmented coefficients K1 saw
        if constexpr (GEN) {
          sh_noise_apply_n<GEN>(sc.noise, nstream, i, 3 * K, sh);
        } else {
          const float* nz = sc.noise.sh + (size_t)i * (3 * K);
          for (int k = 0; k < 3 * K; ++k) sh[k] = sh[k] + nz[k] * (kSqrtPoint2 * sh[k]);
        }
      }
    } else if constexpr (KT > 0 && (3 * KT) % 4 == 0) {
      // compile-time stride: each lane pulls its own row (as K1 does) and parks it in its LDS row; LDS is still
      // needed for the coalesced write-back of dL/dSH
      if (vis) {
        const float4* r = reinterpret_cast<const float4*>(g.shs + (size_t)i * (3 * KT));
#pragma unroll
        for (int q = 0; q < (3 * KT) / 4; ++q) {
          const float4 t = r[q];
          sh[4 * q] = t.x; sh[4 * q + 1] = t.y; sh[4 * q + 2] = t.z; sh[4 * q + 3] = t.w;
        }
      }
    } else {
      if (vmask) stage_sh_in<KT>(g.shs, wave_first, n_valid, K, vmask, lw);
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    if (vis) {
      const ViewDir d = view_dir(vc, px, py, pz);
      const float x = d.x, y = d.y, z = d.z, len = d.len;
      float b[16];
      sh_basis(D, x, y, z, b);
      const int nb = (D + 1) * (D + 1);
      float gch[3];
      {
        float acc[3];
        sh_colour(D, sh, b, acc);
#pragma unroll
        for (int c = 0; c < 3; ++c) gch[c] = (acc[c] + 0.5f < 0.0f) ? 0.0f : grgb[c];   // K1's clamp decision (same operator order)
      }
      float s[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) s[k] = 0.f;
      // s_k = <sh_k, g>, and the row is overwritten in place by dL/dsh_k = b_k g (constant register indices per band)
#define GSR_SH_BWD_BAND(K0, K1)                                                                        \
  _Pragma("unroll") for (int k = K0; k <= K1; ++k) {                                                   \
    s[k] = (sh[3 * k] * gch[0] + sh[3 * k + 1] * gch[1]) + sh[3 * k + 2] * gch[2];                     \
    sh[3 * k] = b[k] * gch[0]; sh[3 * k + 1] = b[k] * gch[1]; sh[3 * k + 2] = b[k] * gch[2];           \
  }
      GSR_SH_BWD_BAND(0, 0)
      if (D > 0) {
        GSR_SH_BWD_BAND(1, 3)
        if (D > 1) {
          GSR_SH_BWD_BAND(4, 8)
          if (D > 2) { GSR_SH_BWD_BAND(9, 15) }
        }
      }
#undef GSR_SH_BWD_BAND
      for (int k = 3 * nb; k < 3 * K; ++k) sh[k] = 0.f;
      if constexpr (SCENE) {
        if (noise_has_sh<GEN>(sc.noise)) {   // d(sh + n c sh)/dsh = 1 + c n
          if constexpr (GEN) {
            sh_noise_chain_n<GEN>(sc.noise, nstream, i, 3 * K, 3 * nb, sh);
          } else {
            const float* nz = sc.noise.sh + (size_t)i * (3 * K);
            for (int k = 0; k < 3 * nb; ++k) sh[k] = sh[k] * (1.0f + kSqrtPoint2 * nz[k]);
          }
        }
      }
      float ddx, ddy, ddz;
      sh_ddir(D, x, y, z, s, ddx, ddy, ddz);
      const float dot = (x * ddx + y * ddy) + z * ddz;
      const float dvx = (ddx - x * dot) / len, dvy = (ddy - y * dot) / len, dvz = (ddz - z * dot) / len;
      dp[0] += dvx; dp[1] += dvy; dp[2] += dvz;
      dcam[0] = -dvx; dcam[1] = -dvy; dcam[2] = -dvz;
    } else if (lane < n_valid) {
      for (int k = 0; k < 3 * K; ++k) sh[k] = 0.f;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // accumulating: a wave without a visible Gaussian adds nothing to its rows
    if constexpr (SCENE) {
      if (!(out.accumulate && vmask == 0ull)) {
        if (sg.dc[rw.m])
          stage_rows_out<3>(sg.dc[rw.m] + wave_first * 3, 3, 0, stride, n_valid, lw, out.accumulate != 0, vmask);
        if (K > 1 && sg.rest[rw.m])
          stage_rows_out<(KT > 1 ? 3 * KT - 3 : 0)>(sg.rest[rw.m] + wave_first * (3 * K - 3), 3 * K - 3, 3, stride, n_valid,
                                                   lw, out.accumulate != 0, vmask);
      }
    } else if (out.dL_dshs && !(out.accumulate && vmask == 0ull))
      stage_sh_out<KT>(out.dL_dshs, wave_first, n_valid, K, lw, out.accumulate != 0);
  }

  float dscale[3] = {0.f, 0.f, 0.f};
  float drot[4] = {0.f, 0.f, 0.f, 0.f};
  float dc6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  [[maybe_unused]] float dsc_draw[3] = {1.f, 1.f, 1.f};   // scene: d(returned scale)/d(raw scaling)
  if (vis) {
    float c6[6];
    float R[9];
    float s3[3] = {0.f, 0.f, 0.f};
    float4 q = make_float4(1, 0, 0, 0);
    [[maybe_unused]] float4 qraw = q;
    [[maybe_unused]] float qnorm = 1.0f;
    if (g.cov3D_precomp) {
#pragma unroll
      for (int k = 0; k < 6; ++k) c6[k] = g.cov3D_precomp[6 * i + k];
    } else {
      float sa[3] = {p_scale[3 * row], p_scale[3 * row + 1], p_scale[3 * row + 2]};
      q = *reinterpret_cast<const float4*>(p_rot + 4 * row);
      if constexpr (SCENE) {
        qraw = q;
        float n[3];
        noise_scale3<GEN>(sc.noise, nstream, i, n);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const ActScale a = act_scale(sa[k], noise_has_scale<GEN>(sc.noise), n[k]);
          sa[k] = a.out;
          dsc_draw[k] = scale_draw(a.act, a.pre, noise_has_scale<GEN>(sc.noise), n[k]);
        }
        qnorm = act_quat_norm(q);
        q = make_float4(q.x / qnorm, q.y / qnorm, q.z / qnorm, q.w / qnorm);
      }
      s3[0] = mod * sa[0]; s3[1] = mod * sa[1]; s3[2] = mod * sa[2];
      quat_to_R(q, R);
      cov3d_from(s3[0], s3[1], s3[2], R, c6);
    }
    Ewa e;
    ewa_forward(vc, px, py, pz, c6, fx, fy, limx, limy, e);

    float dS[9];
    geom_backward(vc, e, fx, fy, W, H, px, py, pz, S1, S2, S3, S4, S5, gdep, want_cam, gndx, gndy, dS, dp, dview, dproj);

    // (6) Sigma -> its parameters
    if (g.cov3D_precomp) {
      dc6[0] = dS[0]; dc6[1] = dS[1] + dS[3]; dc6[2] = dS[2] + dS[6];
      dc6[3] = dS[4]; dc6[4] = dS[5] + dS[7]; dc6[5] = dS[8];
    } else {
      sigma_backward(dS, R, s3, mod, q, dscale, drot);
      if constexpr (SCENE) {
        // through exp (+ noise, clamp) and through q = raw / |raw|:  d raw = (dq - q <q, dq>) / |raw|
#pragma unroll
        for (int k = 0; k < 3; ++k) dscale[k] = dscale[k] * dsc_draw[k];
        const float qd = ((q.x * drot[0] + q.y * drot[1]) + q.z * drot[2]) + q.w * drot[3];
        drot[0] = (drot[0] - q.x * qd) / qnorm; drot[1] = (drot[1] - q.y * qd) / qnorm;
        drot[2] = (drot[2] - q.z * qd) / qnorm; drot[3] = (drot[3] - q.w * qd) / qnorm;
      }
    }
  }

  if (vis && out.stat_denom) {   // densification statistics of this view (gs_renderer.py:1061-1065)
    out.stat_xyz_gradient_accum[i] += sqrtf(gndx * gndx + gndy * gndy);
    out.stat_denom[i] += 1.0f;
    out.stat_max_radii2D[i] = fmaxf(out.stat_max_radii2D[i], (float)radii[i]);
  }
  if constexpr (SCENE) {
    if (rw.ok) {
      out.dL_dmeans2D[3 * i] = gndx; out.dL_dmeans2D[3 * i + 1] = gndy; out.dL_dmeans2D[3 * i + 2] = 0.f;
      // gradient arriving through the RETURNED scales (the trainers' loss_scale, object_trainer.py:378-379): it
      // reaches every Gaussian, visible or not
      const bool has_gs = sg.dL_dscales_out != nullptr;
      if (has_gs) {
        float n[3] = {0.f, 0.f, 0.f};
        if (!vis) noise_scale3<GEN>(sc.noise, nstream, i, n);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (!vis) {
            const ActScale a = act_scale(p_scale[3 * row + k], noise_has_scale<GEN>(sc.noise), n[k]);
            dsc_draw[k] = scale_draw(a.act, a.pre, noise_has_scale<GEN>(sc.noise), n[k]);
          }
          dscale[k] += sg.dL_dscales_out[3 * i + k] * dsc_draw[k];
        }
      }
      if (out.accumulate && !vis) {
        float* o = sg.scaling[rw.m];
        if (has_gs && o) {
#pragma unroll
          for (int k = 0; k < 3; ++k) o[3 * row + k] += dscale[k];
        }
      } else {
        const bool acc = out.accumulate != 0;
        float gop_raw = 0.f;
        if (vis) {
          const float sg_ = act_sigmoid(sc.opacity[rw.m][row]);
          gop_raw = gop * (sg_ * (1.0f - sg_));
        }
        float* o;
        if ((o = sg.xyz[rw.m])) {
#pragma unroll
          for (int k = 0; k < 3; ++k) o[3 * row + k] = acc ? o[3 * row + k] + dp[k] : dp[k];
        }
        if ((o = sg.scaling[rw.m])) {
#pragma unroll
          for (int k = 0; k < 3; ++k) o[3 * row + k] = acc ? o[3 * row + k] + dscale[k] : dscale[k];
        }
        if ((o = sg.rotation[rw.m])) {
          float4 t = make_float4(drot[0], drot[1], drot[2], drot[3]);
          if (acc) {
            const float4 old = *reinterpret_cast<const float4*>(o + 4 * row);
            t.x += old.x; t.y += old.y; t.z += old.z; t.w += old.w;
          }
          *reinterpret_cast<float4*>(o + 4 * row) = t;
        }
        if ((o = sg.opacity[rw.m])) o[row] = acc ? o[row] + gop_raw : gop_raw;
      }
    }
  } else if (i < P && out.accumulate && !vis) {
    // accumulating: a culled Gaussian adds nothing; only the per-view means2D gradient is (re)written
    out.dL_dmeans2D[3 * i] = 0.f; out.dL_dmeans2D[3 * i + 1] = 0.f; out.dL_dmeans2D[3 * i + 2] = 0.f;
  } else if (i < P) {
    float gop_o = gop;
    if (out.accumulate) {
      // sum over views on the device (the reference accumulates C_batch_size views per optimizer step,
      // training/object_trainer.py:302-382); means2D is per view and is never accumulated
      dp[0] += out.dL_dmeans3D[3 * i]; dp[1] += out.dL_dmeans3D[3 * i + 1]; dp[2] += out.dL_dmeans3D[3 * i + 2];
      gop_o += out.dL_dopacities[i];
      if (out.dL_dscales) { dscale[0] += out.dL_dscales[3 * i]; dscale[1] += out.dL_dscales[3 * i + 1]; dscale[2] += out.dL_dscales[3 * i + 2]; }
      if (out.dL_drotations) {
        const float4 o = *reinterpret_cast<const float4*>(out.dL_drotations + 4 * i);
        drot[0] += o.x; drot[1] += o.y; drot[2] += o.z; drot[3] += o.w;
      }
      if (out.dL_dcov3D) {
#pragma unroll
        for (int k = 0; k < 6; ++k) dc6[k] += out.dL_dcov3D[6 * i + k];
      }
    }
    out.dL_dmeans3D[3 * i] = dp[0]; out.dL_dmeans3D[3 * i + 1] = dp[1]; out.dL_dmeans3D[3 * i + 2] = dp[2];
    out.dL_dmeans2D[3 * i] = gndx; out.dL_dmeans2D[3 * i + 1] = gndy; out.dL_dmeans2D[3 * i + 2] = 0.f;
    out.dL_dopacities[i] = gop_o;
    if (out.dL_dcolors) {
      float c0 = grgb[0], c1 = grgb[1], c2 = grgb[2];
      if (out.accumulate) { c0 += out.dL_dcolors[3 * i]; c1 += out.dL_dcolors[3 * i + 1]; c2 += out.dL_dcolors[3 * i + 2]; }
      out.dL_dcolors[3 * i] = c0; out.dL_dcolors[3 * i + 1] = c1; out.dL_dcolors[3 * i + 2] = c2;
    }
    if (out.dL_dscales) { out.dL_dscales[3 * i] = dscale[0]; out.dL_dscales[3 * i + 1] = dscale[1]; out.dL_dscales[3 * i + 2] = dscale[2]; }
    if (out.dL_drotations) *reinterpret_cast<float4*>(out.dL_drotations + 4 * i) = make_float4(drot[0], drot[1], drot[2], drot[3]);
    if (out.dL_dcov3D) {
#pragma unroll
      for (int k = 0; k < 6; ++k) out.dL_dcov3D[6 * i + k] = dc6[k];
    }
  }

  // ---- camera gradients: block reduction, one atomic per value per block
  if (want_cam) {
    float vals[27];
#pragma unroll
    for (int k = 0; k < 12; ++k) { vals[k] = dview[k]; vals[12 + k] = dproj[k]; }
    vals[24] = dcam[0]; vals[25] = dcam[1]; vals[26] = dcam[2];
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      const float s = gsr_wave_sum_to_lane63(vals[k]);
      if (lane == 63) cam_red[wave][k] = s;
    }
    __syncthreads();
    if (tid < 27) {
      const float s = (cam_red[0][tid] + cam_red[1][tid]) + (cam_red[2][tid] + cam_red[3][tid]);
      if (tid < 12) {
        if (out.dL_dview) unsafeAtomicAdd(out.dL_dview + 4 * (tid / 3) + (tid % 3), s);
      } else if (tid < 24) {
        const int k = tid - 12, r = k / 3, c = k % 3;
        if (out.dL_dproj) unsafeAtomicAdd(out.dL_dproj + 4 * r + (c == 2 ? 3 : c), s);
      } else {
        if (out.dL_dcampos) unsafeAtomicAdd(out.dL_dcampos + (tid - 24), s);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------- K8 over several views
// The views of one optimizer step share their Gaussians (object_trainer.py:302-382): one pass reads every
// parameter row once, loops over the views' cameras / K7 partials, sums the gradients in registers and writes them
// once -- 4 views: ~185 B per Gaussian and view instead of ~700 (the SH rows dominate both the reads and the writes).
// dL/dSigma is summed over the views before the (view-independent) step to scales / quaternion.
struct K8Views {
  int32_t nv;
  const float* viewmatrix[GSR_MAX_BATCH_VIEWS];
  const float* projmatrix[GSR_MAX_BATCH_VIEWS];
  const float* campos[GSR_MAX_BATCH_VIEWS];
  float tanfovx[GSR_MAX_BATCH_VIEWS];
  float tanfovy[GSR_MAX_BATCH_VIEWS];
  int32_t sh_degree[GSR_MAX_BATCH_VIEWS];   // the active degree may differ per view (scene_render's sh_deg_aug)
  const float* dyn[GSR_MAX_BATCH_VIEWS];    // GsrView.dynamic of every view (NULL: the by-value entries above)
  const int32_t* radii[GSR_MAX_BATCH_VIEWS];
  float* partials[GSR_MAX_BATCH_VIEWS];
  // GsrGrads.reach of every view (all set or all NULL) and its contract: restore = zero the consumed sums and marks again
  unsigned long long* reach[GSR_MAX_BATCH_VIEWS];
  int32_t restore;
  float* dL_dmeans2D[GSR_MAX_BATCH_VIEWS];
  // per-view scales (the trainers add fresh noise to the activated scales of every view, scene_gaussian.py:1004-1008):
  // then every view has its own scales tensor and its own scale gradient; the other parameters are shared
  int32_t per_view_scales;
  const float* scales[GSR_MAX_BATCH_VIEWS];
  float* dL_dscales[GSR_MAX_BATCH_VIEWS];
  // scene input (raw leaves): per-view noise samples, per-view gradient arriving through the returned scales
  NoiseViews noise;
  const float* dL_dscales_out[GSR_MAX_BATCH_VIEWS];
  // bit k set: view k's densification statistics count (the reference's trainers use the LAST view of a step only,
  // object_trainer.py:386-390; a caller sets the stat_* pointers on the GsrGrads entries of the views that count)
  uint32_t stat_mask;
};

// ------------------------------------------------------------------------------- K8, sparse over the Gaussians
// K7 reaches few Gaussians: behind the first opaque layers nothing receives a gradient (C3: 4-5 % of the Gaussians
// per view, 16 % in the union of four views; 2 M Gaussians: 8 %). A (Gaussian, view) pair whose ten K7 sums are all
// zero contributes exactly zero to every output of K8 -- every term of the chain rule is a product with one of them --
// so the ~1 200 instructions per pair, and the 236 B parameter row, are only worth touching for the Gaussians some
// view reached. Those are scattered (nearly every wave holds one), so the REACHED form of the kernel below compacts
// them inside the workgroup, which owns kK8Block = 1 024 consecutive Gaussians:
//   A. every thread classifies four Gaussians (radii + K7's marks, GsrGrads.reach, of every view; without marks: the K7
//      sums themselves) -> "reached by some view?". The workgroup clears the gradient rows (and the per-view rows) of its
//      1 024 Gaussians with coalesced stores (unless accumulating); a Gaussian nothing reached gets its visibility
//      statistics here and is done;
//   B. the reached ones are listed in LDS (ballot / popcount prefix, ascending) and the four waves walk the list in rounds
//      of 256 (wave slots rotated by the block index so that partial rounds do not pile up on one SIMD), running the dense
//      chain rule on them -- same arithmetic, same summation order over the views, bit-identical rows -- and writing each
//      row over the cleared one. (A row some view saw and no view reached is +0 here; the dense form's sigma_backward on an
//      all-zero dSigma can leave -0 in it: equal values, tests/test_k8_blocks.py.)
// Where a workgroup spends its time (tools/k8_stamps.py: realtime stamps inside the kernel; C3, 4 views, 489 workgroups of
// 1 024 Gaussians, 161 of them reached on average, all resident at once; us since the workgroup's entry, mean):
//   classified 14.5 | parameters + SH row in 27.6 | rows cleared 47.9 | views done 54.0 58.4 62.5 66.6 | rows stored 69.2
// and the launch takes 93 (the workgroups with two rounds). What the numbers say:
//  * the chain rule is ~1 400 instructions per view and lane and runs at ~7 cycles per instruction -- one wave per SIMD,
//    every instruction dependent on the last: 4.3 us per view whatever the occupancy of the lanes;
//  * every memory round trip on the critical path costs 3-10 us while all workgroups are in the same phase, so requests
//    are issued in batches (all slices and views of the classification at once; parameters, SH row and the first view's
//    sums at once; the next view's sums before the current view's arithmetic) and the per-view constants come through
//    scalar loads (load_view_const): on gfx9 a vector load issued behind a vector store waits for the store's
//    acknowledgement, which is how the per-view stores used to serialise the views;
//  * the 142 MB of zeros are 20 us of HBM writes during which nothing else progresses (all workgroups clear at the same
//    time). Next lead: clear from the idle wave(s) only, skipping the reached rows, so that it overlaps the chain rule;
//  * 230 -> 260 registers (the prefetch) halved the occupancy and cost 88 -> 121 us: amdgpu_waves_per_eu(2) pins it.
// Round 2 gave a workgroup 256 Gaussians and ONE wave of it the ~40 reached ones (three shifts of workgroups, 101 us);
// C3 in the opacity-0.1 initial state (67 % reached: three or four rounds per workgroup) is slower in this form than
// with the old dense fallback (151 vs 124 us per launch) -- 3 % of that step.
// Forms that were measured and dropped: (i) chunks of (Gaussian, view) pairs dealt to the waves with the results
// summed by ds_add_f32 into a 256-row LDS tile (0.5 ns per pair: slower than dense once 5 % are active); (ii) a separate
// classify launch appending to global lists kept in spare words of the K7 sums, then the dense kernel over the lists
// (one list: 31 000 same-address atomics at 2 M Gaussians; one list per 8 192 Gaussians: the live workgroups of the
// second launch all land on three of the eight XCDs); (iii) lane j of every wave holding the j-th reached Gaussian,
// wave w running view w, results added to an LDS tile view after view between barriers.
#ifndef GSR_K8_BLOCK
#define GSR_K8_BLOCK 1024
#endif
constexpr int kK8Block = GSR_K8_BLOCK;       // Gaussians per workgroup of the REACHED form (a multiple of 256)

// one lane's row of F floats -> global memory (dword-aligned 16-byte pieces)
template <int F>
__device__ __forceinline__ void store_row(float* __restrict__ dst, const float* src, bool accumulate) {
#pragma unroll
  for (int q = 0; q + 3 < F; q += 4) {
    gsr_f4u t;
    t.x = src[q]; t.y = src[q + 1]; t.z = src[q + 2]; t.w = src[q + 3];
    if (accumulate) {
      const gsr_f4u o = *reinterpret_cast<const gsr_f4u*>(dst + q);
      t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
    }
    *reinterpret_cast<gsr_f4u*>(dst + q) = t;
  }
#pragma unroll
  for (int q = F & ~3; q < F; ++q) dst[q] = accumulate ? dst[q] + src[q] : src[q];
}

// zeros over the rows of F floats [0, n) at dst (n <= 64) whose bit in `skip` is clear, one wave; rows stay whole: a
// 16-byte store never straddles into a skipped row (F % 4 == 0 and dst 16-byte aligned, or 4-byte stores)
template <int F>
__device__ __forceinline__ void wave_zero_rows(float* __restrict__ dst, int n, unsigned long long skip, int lane) {
  if ((~skip & (n >= 64 ? ~0ull : ((1ull << n) - 1ull))) == 0ull) return;       // (uniform: nothing to clear in this chunk)
  if constexpr (F % 4 == 0) {
    constexpr int Q = F / 4;
    float4* d = reinterpret_cast<float4*>(dst);
    for (int q = lane; q < n * Q; q += 64)
      if (!((skip >> (q / Q)) & 1ull)) d[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    for (int f = lane; f < n * F; f += 64)
      if (!((skip >> (f / F)) & 1ull)) dst[f] = 0.f;
  }
}

template <int KT, bool PVS, bool REACHED = false, int KPER = 4>   // PVS: per-view scales; REACHED: the sparse form described above;
// KPER: 256-Gaussian slices per workgroup of the REACHED form (4: 1 024 Gaussians, for grids that fill the chip once; 1: small P)
// (two waves per SIMD = two workgroups per CU: one resident wave of workgroups at 500 k Gaussians. Without the attribute the
//  allocator took 260 registers, one workgroup per CU, and the kernel ran its workgroups in two shifts: 88 -> 121 us)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
k_preprocess_bwd_views(const GsrView v, const GsrGaussians g, const K8Views vb, const GsrGrads out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int kPer = REACHED ? KPER : 1;                  // Gaussians classified per thread
  __shared__ uint32_t wcnt[REACHED ? 4 * kPer : 1];
  __shared__ uint16_t reached_list[REACHED ? 256 * KPER : 1];
  __shared__ unsigned long long lmask[REACHED ? 4 * kPer : 1];   // reached Gaussians of the 64-row chunk (slice, wave)
  __shared__ unsigned long long vmask[REACHED ? GSR_MAX_BATCH_VIEWS : 1][REACHED ? 4 * kPer : 1];   // ... per view (K7's marks)
  __shared__ uint32_t zero_next;                                  // next chunk nobody has cleared yet
  // GsrGrads.zero_outside: rows of chunk c that MAY be non-zero on entry (the previous writer's reached_mask; all ones: unknown)
  __shared__ unsigned long long omask[REACHED ? 4 * kPer : 1];
  constexpr int F = 3 * KT;
  const int W = v.image_width, H = v.image_height;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t P = v.P;
  // REACHED: the workgroup's 4 kPer chunks of 64 consecutive Gaussians lie gridDim.x * 64 apart -- how many Gaussians the
  // views reached varies along the index (C3: 161 of 1 024 on average, 566 in the densest contiguous block, 455 with four
  // slices of 256, and the kernel ends with the workgroup that has the most rounds); chunks from sixteen places average it.
  // Chunk c = 4 t + wave belongs to the lanes of `wave` in slice t of phase A. (tests/k8_layout.py restates this layout.)
  const auto chunk_base = [&](int c) { return ((int64_t)c * gridDim.x + blockIdx.x) * 64; };
  const int64_t first = REACHED ? chunk_base(0) : (int64_t)blockIdx.x * 256;
  int64_t i = first + tid;
  bool ok = i < P;
  constexpr bool sparse = REACHED;
  int cnt = 0;           // REACHED: entries of reached_list
#ifdef GSR_K8_STAMPS
  unsigned long long ts[12];
  int nts = 0;
#define GSR_K8_STAMP() do { if (nts < 12) ts[nts++] = wall_clock64(); } while (0)
#else
#define GSR_K8_STAMP() do { } while (0)
#endif
  GSR_K8_STAMP();   // 0: entry
  // phase A's verdicts (slice t of a thread = Gaussian chunk_base(4 t + wave) + lane)
  bool reached[kPer];
  unsigned long long rmask[kPer];
  if constexpr (REACHED) {
    // ---- A: which of the workgroup's Gaussians did some view reach?
    // The loads of all slices of a view are issued together (every one of them is a memory latency if it is consumed
    // where it is issued: 2 x 4 x 4 dependent round trips were 17 of this kernel's 95 us).
#pragma unroll
    for (int t = 0; t < kPer; ++t) { reached[t] = false; rmask[t] = 0ull; }
    if (vb.reach[0]) {
      // K7 marked the Gaussians it committed sums for (GsrGrads.reach: one bit per Gaussian and view): one 8-byte word per
      // (view, chunk) -- thread 4 kPer vv + c fetches it -- instead of the 40-byte sums of every visible Gaussian
      static_assert(GSR_MAX_BATCH_VIEWS * 4 * kPer <= 256, "one thread per (view, chunk) word");
      if (tid < vb.nv * 4 * kPer) {
        const int vv = tid / (4 * kPer), c = tid % (4 * kPer);
        const int64_t r0 = chunk_base(c);
        vmask[vv][c] = r0 < P ? vb.reach[vv][r0 >> 6] : 0ull;
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < kPer; ++t) {
        for (int vv = 0; vv < vb.nv; ++vv) rmask[t] |= vmask[vv][4 * t + wave];
        reached[t] = (rmask[t] >> lane) & 1ull;
      }
    } else {
      // without marks: the sums themselves (the loads of all slices of four views are issued together)
      for (int v0 = 0; v0 < vb.nv; v0 += 4) {
        int32_t r[4][kPer];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int t = 0; t < kPer; ++t) {
            const int64_t it = chunk_base(4 * t + wave) + lane;
            r[u][t] = ((v0 + u < vb.nv) && (it < P)) ? vb.radii[v0 + u][it] : 0;
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int t = 0; t < kPer; ++t) {
            if (r[u][t] > 0) {
              float4 pa, pb, pc;
              partial_rows(partial_load(vb.partials[v0 + u], chunk_base(4 * t + wave) + lane), pa, pb, pc);
              reached[t] = reached[t] || (pa.x != 0.f) || (pa.y != 0.f) || (pa.z != 0.f) || (pa.w != 0.f) || (pb.x != 0.f) ||
                           (pb.y != 0.f) || (pb.z != 0.f) || (pb.w != 0.f) || (pc.x != 0.f) || (pc.y != 0.f) ||
                           (pc.z != 0.f) || (pc.w != 0.f);
            }
          }
        }
      }
#pragma unroll
      for (int t = 0; t < kPer; ++t) rmask[t] = __ballot(reached[t]);
    }
#pragma unroll
    for (int t = 0; t < kPer; ++t)
      if (lane == 0) { wcnt[t * 4 + wave] = (uint32_t)__popcll(rmask[t]); lmask[t * 4 + wave] = rmask[t]; }
    if (tid < 4 * kPer) {
      // (the old word of chunk c is read here, by the workgroup that owns the chunk, before wave_exit stores the new one)
      const int64_t r0 = chunk_base(tid);
      omask[tid] = (out.zero_outside && !out.accumulate && out.reached_mask && r0 < P)
                       ? reinterpret_cast<const unsigned long long*>(out.reached_mask)[r0 >> 6] : ~0ull;
    }
    if (tid == 0) zero_next = 0u;
    GSR_K8_STAMP();   // 1: classified
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
      uint32_t off = 0;
      for (int q = 0; q < t * 4 + wave; ++q) off += wcnt[q];
      if (reached[t]) reached_list[off + (uint32_t)__popcll(rmask[t] & ((1ull << lane) - 1ull))] = (uint16_t)(t * 256 + tid);
    }
    for (int q = 0; q < 4 * kPer; ++q) cnt += (int)wcnt[q];
    __syncthreads();
    // (everything this phase STORES comes after the first loads of phase B, in the epilogue of round 0: vector-memory
    //  operations return in order on gfx9, so a load issued behind a store waits for the store's write acknowledgement)
  }
  const float mod = v.scale_modifier;
  constexpr int stride = F | 1;
  float* lw = lds + wave * (64 * stride);
  float* sh = lw + lane * stride;
  // ---- B (REACHED): rounds of 256 list entries, wave slot rotated by the block index; otherwise one pass, thread = Gaussian
  for (int round = 0;; round += 256) {
  bool active = true;    // REACHED: this wave has entries in this round (uniform over the wave)
  int entry = 0;         // REACHED: the lane's list entry
  if constexpr (REACHED) {
    const int chunk = round + ((wave + 4 - (int)(blockIdx.x & 3u)) & 3) * 64;
    active = chunk < cnt;
    ok = active && (chunk + lane < cnt);
    entry = ok ? (int)reached_list[chunk + lane] : 0;
    i = chunk_base(entry >> 6) + (entry & 63);      // (entry = 256 t + tid = 64 (4 t + wave) + lane)
  }
  const int64_t wave_first = (int64_t)blockIdx.x * 256 + wave * 64;      // (the dense form's coalesced write-back)
  const int n_valid = (int)min((int64_t)64, max((int64_t)0, P - wave_first));

  bool any = ok;         // REACHED: a listed Gaussian is visible in the view that reached it
  if constexpr (!REACHED) {
    any = false;
    for (int vv = 0; vv < vb.nv; ++vv) any = any || (ok && vb.radii[vv][i] > 0);
  }
  const unsigned long long amask = __ballot(any);

  // one view ahead: radius, K7's mark and (REACHED: unconditionally -- an unmarked row is zero or ignored) the K7 sums of
  // the next view are requested before the current view's arithmetic and before its stores
  int32_t r_nx = 0;
  uint32_t mk_nx = 1u;
  PartialRaw p_nx = partial_none();   // (raw words: the f64 -> f32 conversions wait for the loads, so they happen where the row is consumed)
  const auto prefetch_view = [&](int vv) {
    r_nx = ok ? vb.radii[vv][i] : 0;
    if (!vb.reach[0]) mk_nx = 1u;
    else if constexpr (REACHED) mk_nx = (uint32_t)((vmask[vv][entry >> 6] >> (entry & 63)) & 1ull);
    else mk_nx = ok ? (uint32_t)((vb.reach[vv][i >> 6] >> (i & 63)) & 1ull) : 0u;
    if constexpr (REACHED) {
      // (only the views that MARKED the Gaussian: a listed Gaussian is reached by 1.3 of the 4 views of a step on average, and
      //  a row is 96 bytes since the sums are doubles -- round 3 loaded the 48-byte rows of all views unconditionally. The mark
      //  comes from the LDS copy of K7's bit words: no memory round trip in front of the load)
      if (ok && mk_nx) p_nx = partial_load(vb.partials[vv], i);
      else p_nx = partial_none();
    }
  };
  // every request of the round goes out before anything is consumed: one memory latency, not four
  float px = 0, py = 0, pz = 0;
  float R[9], c6[6], s3[3] = {0.f, 0.f, 0.f};
  float4 q = make_float4(1, 0, 0, 0);
  if (any) {
    px = g.means3D[3 * i]; py = g.means3D[3 * i + 1]; pz = g.means3D[3 * i + 2];
    q = *reinterpret_cast<const float4*>(g.rotations + 4 * i);
    if constexpr (!PVS) { s3[0] = g.scales[3 * i]; s3[1] = g.scales[3 * i + 1]; s3[2] = g.scales[3 * i + 2]; }
  }
  prefetch_view(0);
  if (any) {
    load_row<F>(g.shs + (size_t)i * F, sh);      // the lane's own SH row, kept (read only) in its LDS row
    quat_to_R(q, R);
    if constexpr (!PVS) {
      s3[0] = mod * s3[0]; s3[1] = mod * s3[1]; s3[2] = mod * s3[2];
      cov3d_from(s3[0], s3[1], s3[2], R, c6);
    }
  }
  GSR_K8_STAMP();   // 2: parameters + SH row in, view 0 requested
  // ---- what a wave does when it has no (more) list entries: the words of the exchange mask and the visibility statistics
  // of its lanes' Gaussians, then zeros over the rows nothing reached -- 64-row chunks claimed from a counter, so the
  // waves that are idle from the start clear while the others run the chain rule, and nothing the chain rule loads
  // queues behind those stores (the reached rows are written by the chain rule alone: the two never touch the same row)
  const auto wave_exit = [&]() {
    if (vb.restore && vb.reach[0] && tid < vb.nv * 4 * kPer) {      // GsrGrads.scratch_clean: K7's marks back to zero
      const int64_t r0 = chunk_base(tid % (4 * kPer));
      if (r0 < P) vb.reach[tid / (4 * kPer)][r0 >> 6] = 0ull;
    }
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
      const int64_t base = chunk_base(4 * t + wave), it = base + lane;
      const unsigned long long rm = lmask[t * 4 + wave];      // (from LDS: nothing of phase A stays in registers)
      if (lane == 0 && out.reached_mask && base < P) {
        // the rows a gradient exchange has to move (GsrGrads.reached_mask): one word per wave and slice, owned by this wave
        unsigned long long* w = reinterpret_cast<unsigned long long*>(out.reached_mask) + (base >> 6);
        if (out.accumulate) *w |= rm; else *w = rm;
      }
      if (!((rm >> lane) & 1ull) && it < P && out.stat_denom) {   // visibility statistics (the reached ones: in the chain rule)
        float n = 0.f, rmax = 0.f;
        for (int vv = 0; vv < vb.nv; ++vv)
          if ((vb.stat_mask >> vv) & 1u) {
            const int32_t r = vb.radii[vv][it];
            if (r > 0) { n += 1.0f; rmax = fmaxf(rmax, (float)r); }
          }
        if (n > 0.f) {
          out.stat_denom[it] += n;
          out.stat_max_radii2D[it] = fmaxf(out.stat_max_radii2D[it], rmax);
        }
      }
    }
    for (;;) {
      uint32_t c = 0;
      if (lane == 0) c = atomicAdd(&zero_next, 1u);
      c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
      if (c >= (uint32_t)(4 * kPer)) break;
      const int64_t r0 = chunk_base((int)c);
      const int n = (int)max((int64_t)0, min((int64_t)64, P - r0));
      if (n == 0) continue;
      // rows to clear: the ones nothing reached now -- of those, with GsrGrads.zero_outside, only the ones the previous writer
      // of these buffers reached (everything else is zero already)
      const unsigned long long known0 = out.accumulate ? 0ull : ~omask[c];
      const unsigned long long skip = lmask[c] | ((out.zero_outside & 1) ? known0 : 0ull);
      const unsigned long long skip_pv = lmask[c] | ((out.zero_outside & 2) ? known0 : 0ull);
      if (!out.accumulate) {
        wave_zero_rows<F>(out.dL_dshs + r0 * F, n, skip, lane);
        wave_zero_rows<3>(out.dL_dmeans3D + r0 * 3, n, skip, lane);
        wave_zero_rows<1>(out.dL_dopacities + r0, n, skip, lane);
        if constexpr (!PVS) wave_zero_rows<3>(out.dL_dscales + r0 * 3, n, skip, lane);
        wave_zero_rows<4>(out.dL_drotations + r0 * 4, n, skip, lane);
      }
      for (int vv = 0; vv < vb.nv; ++vv) {      // the per-view rows: what the chain rule would produce from zeros
#ifdef GSR_K8_STAMPS
        if (c == 0 && vv == 0) continue;        // (the stamps are left there)
#endif
        wave_zero_rows<3>(vb.dL_dmeans2D[vv] + r0 * 3, n, skip_pv, lane);
        if constexpr (PVS) wave_zero_rows<3>(vb.dL_dscales[vv] + r0 * 3, n, skip_pv, lane);
      }
    }
  };
  GSR_K8_STAMP();   // 3
  if constexpr (REACHED) {
    if (!active) { wave_exit(); break; }
  }
  float drot[4] = {0.f, 0.f, 0.f, 0.f};

  float dsh[F];
#pragma unroll
  for (int k = 0; k < F; ++k) dsh[k] = 0.f;
  float dp[3] = {0.f, 0.f, 0.f}, dS[9], gop = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) dS[k] = 0.f;

  for (int vv = 0; vv < vb.nv; ++vv) {
    const int32_t rad_v = r_nx;
    const bool take = mk_nx != 0u;                      // (an unmarked Gaussian's sums are zero: not used)
    const PartialRaw p_cur = p_nx;
    float4 pa, pb, pc;
    if (vv + 1 < vb.nv) prefetch_view(vv + 1);
    if constexpr (!REACHED) {     // (the wave owns the mark word of its 64 Gaussians; the REACHED form: wave_exit)
      if (vb.restore && vb.reach[0] && ok && (i & 63) == 0) vb.reach[vv][i >> 6] = 0ull;
    }
    const bool vis = ok && (rad_v > 0);
    // A view that SAW the Gaussian but composited nothing of it (no mark: its ten K7 sums are zero) contributes exact zeros
    // to every output: its chain rule -- ~1 400 dependent instructions -- is skipped (round 4; a listed Gaussian is marked by
    // 1.3 of the 4 views of a step on average at C3, and the kernel is bound by that dependent chain). What does not depend
    // on the sums still happens below: the visibility statistics, the zero rows of dL/dmeans2D and of per-view scales.
    const bool work = vis && take;
    float gndx = 0.f, gndy = 0.f;
    if (work) {
      ViewConst vc;
      load_view_const(vb.viewmatrix[vv], vb.projmatrix[vv], vb.campos[vv], vc);
      const ViewDyn vd = view_dyn(vb.dyn[vv], vb.tanfovx[vv], vb.tanfovy[vv], vb.sh_degree[vv]);
      const float tfx = vd.tanfovx, tfy = vd.tanfovy;
      const int D = vd.sh_degree;
      const float fx = (float)W / (2.0f * tfx), fy = (float)H / (2.0f * tfy);
      const float limx = 1.3f * tfx, limy = 1.3f * tfy;
      if constexpr (!REACHED) {
        partial_rows(partial_load(vb.partials[vv], i), pa, pb, pc);
      } else {
        partial_rows(p_cur, pa, pb, pc);
      }
      pc.x += pc.z; pc.y += pc.w;      // (K7 commits the last two sums from the two halves of a wave: render_bwd.hip, reduce10)
      if (vb.restore) partial_zero(vb.partials[vv], i);     // GsrGrads.scratch_clean: leave the scratch as it was found
      gop += pb.y;
      const float grgb[3] = {pb.z, pb.w, pc.x};
      // (1) colour -> SH coefficients, view direction
      {
        const ViewDir d = view_dir(vc, px, py, pz);
        const float x = d.x, y = d.y, z = d.z, len = d.len;
        float b[16];
        sh_basis(D, x, y, z, b);
        float acc[3];
        sh_colour_n<KT>(D, sh, b, acc);
        float gch[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) gch[c] = (acc[c] + 0.5f < 0.0f) ? 0.0f : grgb[c];   // K1's clamp decision
        float s[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) s[k] = 0.f;
#define GSR_SH_ACC_BAND(K0, K1)                                                                      \
  _Pragma("unroll") for (int k = K0; k <= K1; ++k) {                                                 \
    s[k] = (sh[3 * k] * gch[0] + sh[3 * k + 1] * gch[1]) + sh[3 * k + 2] * gch[2];                   \
    dsh[3 * k] += b[k] * gch[0]; dsh[3 * k + 1] += b[k] * gch[1]; dsh[3 * k + 2] += b[k] * gch[2];   \
  }
        GSR_SH_ACC_BAND(0, 0)
        if constexpr (KT >= 4) {
          if (D > 0) {
            GSR_SH_ACC_BAND(1, 3)
            if constexpr (KT >= 9) {
              if (D > 1) {
                GSR_SH_ACC_BAND(4, 8)
                if constexpr (KT >= 16) {
                  if (D > 2) { GSR_SH_ACC_BAND(9, 15) }
                }
              }
            }
          }
        }
#undef GSR_SH_ACC_BAND
        float ddx, ddy, ddz;
        sh_ddir(D, x, y, z, s, ddx, ddy, ddz);
        const float dot = (x * ddx + y * ddy) + z * ddz;
        dp[0] += (ddx - x * dot) / len; dp[1] += (ddy - y * dot) / len; dp[2] += (ddz - z * dot) / len;
      }
      // (2)-(5) geometry of this view
      if constexpr (PVS) {
        const float* sc = vb.scales[vv];
        s3[0] = mod * sc[3 * i]; s3[1] = mod * sc[3 * i + 1]; s3[2] = mod * sc[3 * i + 2];
        cov3d_from(s3[0], s3[1], s3[2], R, c6);
      }
      Ewa e;
      ewa_forward(vc, px, py, pz, c6, fx, fy, limx, limy, e);
      float dSv[9], dview[12], dproj[12];
      geom_backward(vc, e, fx, fy, W, H, px, py, pz, pa.x, pa.y, pa.z, pa.w, pb.x, pc.y, false, gndx, gndy, dSv, dp, dview,
                    dproj);
      if constexpr (PVS) {      // this view's own scales: its own scale gradient; the quaternion's is summed
        float ds_v[3], dr_v[4];
        sigma_backward(dSv, R, s3, mod, q, ds_v, dr_v);
        float* o = vb.dL_dscales[vv];
        o[3 * i] = ds_v[0]; o[3 * i + 1] = ds_v[1]; o[3 * i + 2] = ds_v[2];
#pragma unroll
        for (int k = 0; k < 4; ++k) drot[k] += dr_v[k];
      } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) dS[k] += dSv[k];
      }
    }
    if (vis && out.stat_denom && ((vb.stat_mask >> vv) & 1u)) {
      out.stat_xyz_gradient_accum[i] += sqrtf(gndx * gndx + gndy * gndy);
      out.stat_denom[i] += 1.0f;
      out.stat_max_radii2D[i] = fmaxf(out.stat_max_radii2D[i], (float)rad_v);
    }
    if (ok) {
      float* m2 = vb.dL_dmeans2D[vv];
      m2[3 * i] = gndx; m2[3 * i + 1] = gndy; m2[3 * i + 2] = 0.f;
      if (PVS && !work) {
        float* o = vb.dL_dscales[vv];
        o[3 * i] = 0.f; o[3 * i + 1] = 0.f; o[3 * i + 2] = 0.f;
      }
    }
    GSR_K8_STAMP();   // 4..: a view done
  }

  float dscale[3] = {0.f, 0.f, 0.f};
  if (any && !PVS) sigma_backward(dS, R, s3, mod, q, dscale, drot);

  if (sparse) {   // the lane's own row over the cleared one
    if (ok && out.dL_dshs && !(out.accumulate && !any)) store_row<F>(out.dL_dshs + (size_t)i * F, dsh, out.accumulate != 0);
  } else {
    // gradient rows -> LDS (zeros for Gaussians no view saw) -> coalesced write-back
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (lane < n_valid) {
#pragma unroll
      for (int k = 0; k < F; ++k) sh[k] = dsh[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (out.dL_dshs && !(out.accumulate && amask == 0ull))
      stage_sh_out<KT>(out.dL_dshs, wave_first, n_valid, KT, lw, out.accumulate != 0);
  }

  if (ok && !(out.accumulate && !any)) {
    if (out.accumulate) {
      dp[0] += out.dL_dmeans3D[3 * i]; dp[1] += out.dL_dmeans3D[3 * i + 1]; dp[2] += out.dL_dmeans3D[3 * i + 2];
      gop += out.dL_dopacities[i];
      if constexpr (!PVS) {
        dscale[0] += out.dL_dscales[3 * i]; dscale[1] += out.dL_dscales[3 * i + 1]; dscale[2] += out.dL_dscales[3 * i + 2];
      }
      const float4 o = *reinterpret_cast<const float4*>(out.dL_drotations + 4 * i);
      drot[0] += o.x; drot[1] += o.y; drot[2] += o.z; drot[3] += o.w;
    }
    out.dL_dmeans3D[3 * i] = dp[0]; out.dL_dmeans3D[3 * i + 1] = dp[1]; out.dL_dmeans3D[3 * i + 2] = dp[2];
    out.dL_dopacities[i] = gop;
    if constexpr (!PVS) {
      out.dL_dscales[3 * i] = dscale[0]; out.dL_dscales[3 * i + 1] = dscale[1]; out.dL_dscales[3 * i + 2] = dscale[2];
    }
    *reinterpret_cast<float4*>(out.dL_drotations + 4 * i) = make_float4(drot[0], drot[1], drot[2], drot[3]);
  }
#ifdef GSR_K8_STAMPS
  GSR_K8_STAMP();     // rows stored (issued)
  if constexpr (REACHED) {
    // timing experiment only (results are destroyed): wave slot 0 of every workgroup leaves its stamps, as 10 ns ticks since
    // entry, in the first floats of view 0's dL_dmeans2D rows of this workgroup
    if (round == 0 && lane == 0 && ((wave + 4 - (int)(blockIdx.x & 3u)) & 3) == 0) {
      __builtin_amdgcn_s_waitcnt(0);
      const unsigned long long tend = wall_clock64();
      float* o = vb.dL_dmeans2D[0] + first * 3;
      for (int k = 0; k < nts; ++k) o[k] = (float)(ts[k] - ts[0]);
      o[nts] = (float)(tend - ts[0]);
      o[14] = (float)cnt; o[15] = (float)nts;
    }
  }
#endif
  if constexpr (!REACHED) break;
  else if (round + 256 + ((wave + 4 - (int)(blockIdx.x & 3u)) & 3) * 64 >= cnt) { wave_exit(); break; }
  }   // rounds
}

// K8 over several views of a SCENE: the raw rows are read once, every view has its own (possibly noisy) scales, the
// gradients of the raw leaves are summed over the views in registers and written once per model tensor.
template <int KT, bool GEN = false>
__global__ void __launch_bounds__(256)
k_preprocess_bwd_views_scene(const GsrView v, const SceneTab sc, const SceneGradTab sg, const K8Views vb,
                             const GsrGrads out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int F = 3 * KT;
  const int W = v.image_width, H = v.image_height;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const Rows rw = resolve_rows<true>(sc, v.P);
  const int64_t i = rw.i, row = rw.row, wave_first = rw.wave_row;
  const int m = rw.m, n_valid = rw.n_valid;
  const bool ok = rw.ok;
  const float mod = v.scale_modifier;
  constexpr int stride = F | 1;
  float* lw = lds + wave * (64 * stride);
  float* sh = lw + lane * stride;

  bool any = false, has_gs = false;
  for (int vv = 0; vv < vb.nv; ++vv) {
    any = any || (ok && vb.radii[vv][i] > 0);
    has_gs = has_gs || (vb.dL_dscales_out[vv] != nullptr);
  }
  const unsigned long long amask = __ballot(any);

  float px = 0, py = 0, pz = 0, R[9], aact[3] = {0.f, 0.f, 0.f}, qnorm = 1.0f;
  float4 q = make_float4(1, 0, 0, 0);
  if (ok && (any || has_gs)) {
#pragma unroll
    for (int k = 0; k < 3; ++k) aact[k] = expf(sc.scaling[m][3 * row + k]);
  }
  if (any) {
    const float* xyz = sc.xyz[m];
    px = xyz[3 * row]; py = xyz[3 * row + 1]; pz = xyz[3 * row + 2];
    q = *reinterpret_cast<const float4*>(sc.rotation[m] + 4 * row);
    qnorm = act_quat_norm(q);
    q = make_float4(q.x / qnorm, q.y / qnorm, q.z / qnorm, q.w / qnorm);
    quat_to_R(q, R);
    load_row<3>(sc.dc[m] + row * 3, sh);                     // raw SH row, kept (read only) in the lane's LDS row
    if constexpr (KT > 1) load_row<F - 3>(sc.rest[m] + row * (F - 3), sh + 3);
  }

  float dsh[F];
#pragma unroll
  for (int k = 0; k < F; ++k) dsh[k] = 0.f;
  float dp[3] = {0.f, 0.f, 0.f}, gop = 0.f, drot[4] = {0.f, 0.f, 0.f, 0.f}, dsraw[3] = {0.f, 0.f, 0.f};

  for (int vv = 0; vv < vb.nv; ++vv) {
    const bool vis = ok && (vb.radii[vv][i] > 0);
    float gndx = 0.f, gndy = 0.f;
    // this view's scales and their derivative w.r.t. the raw (log) scaling
    float sa[3] = {0.f, 0.f, 0.f}, dsc[3] = {0.f, 0.f, 0.f};
    // (the instantiations without the generator read the views' tensors as they always did: same registers as before)
    [[maybe_unused]] NoiseSrc nsrc;
    [[maybe_unused]] uint32_t nstream = 0u;
    if constexpr (GEN) {
      nsrc = vb.noise.view(vv);
      nstream = noise_stream<GEN>(nsrc);
    }
    if (ok && (vis || vb.dL_dscales_out[vv])) {
      [[maybe_unused]] const float* snt = vb.noise.scale[vv];
      [[maybe_unused]] float nsc[3] = {0.f, 0.f, 0.f};
      bool sn = snt != nullptr;
      if constexpr (GEN) {
        sn = noise_has_scale<GEN>(nsrc);
        noise_scale3<GEN>(nsrc, nstream, i, nsc);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float n;
        if constexpr (GEN) n = nsc[k];
        else n = snt ? snt[3 * i + k] : 0.f;
        const float pre = sn ? aact[k] + n * ((kSqrtPoint2 * aact[k]) / 4.0f) : aact[k];
        sa[k] = sn ? fmaxf(pre, 0.0f) : aact[k];
        dsc[k] = sn ? (pre >= 0.0f ? aact[k] * (1.0f + n * (kSqrtPoint2 / 4.0f)) : 0.0f) : aact[k];
      }
      if (vb.dL_dscales_out[vv]) {   // loss on the returned scales: reaches every Gaussian
        const float* gs = vb.dL_dscales_out[vv];
#pragma unroll
        for (int k = 0; k < 3; ++k) dsraw[k] += gs[3 * i + k] * dsc[k];
      }
    }
    if (vis) {
      ViewConst vc;
      load_view_const(vb.viewmatrix[vv], vb.projmatrix[vv], vb.campos[vv], vc);
      const ViewDyn vd = view_dyn(vb.dyn[vv], vb.tanfovx[vv], vb.tanfovy[vv], vb.sh_degree[vv]);
      const float tfx = vd.tanfovx, tfy = vd.tanfovy;
      const int D = vd.sh_degree;
      const float fx = (float)W / (2.0f * tfx), fy = (float)H / (2.0f * tfy);
      float4 pa, pb, pc;
      partial_rows(partial_load(vb.partials[vv], i), pa, pb, pc);
      pc.x += pc.z; pc.y += pc.w;      // (see k_preprocess_bwd)
      gop += pb.y;
      const float grgb[3] = {pb.z, pb.w, pc.x};
      // (1) colour -> SH coefficients (through this view's noise), view direction
      {
        const ViewDir d = view_dir(vc, px, py, pz);
        const float x = d.x, y = d.y, z = d.z, len = d.len;
        float b[16];
        sh_basis(D, x, y, z, b);
        // (every normal is needed twice, on both sides of the clamp decision of the whole colour: GEN keeps them in registers)
        [[maybe_unused]] const float* nzt = (!GEN && vb.noise.sh[vv]) ? vb.noise.sh[vv] + (size_t)i * F : nullptr;
        bool nz = nzt != nullptr;
        if constexpr (GEN) nz = noise_has_sh<GEN>(nsrc);
        [[maybe_unused]] float nzr[GEN ? F : 1];
        float shv[F];
        if constexpr (GEN) {
          if (nz) {
#pragma unroll
            for (int j = 0; j < (F + 3) / 4; ++j) {
              float n4[4];
              noise_sh4<GEN>(nsrc, nstream, i, j, F, n4);
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (4 * j + e < F) nzr[4 * j + e] = n4[e];
            }
          } else {
#pragma unroll
            for (int k = 0; k < F; ++k) nzr[k] = 0.f;
          }
#pragma unroll
          for (int k = 0; k < F; ++k) shv[k] = nz ? sh[k] + nzr[k] * (kSqrtPoint2 * sh[k]) : sh[k];
        } else {
#pragma unroll
          for (int k = 0; k < F; ++k) shv[k] = nzt ? sh[k] + nzt[k] * (kSqrtPoint2 * sh[k]) : sh[k];
        }
        float acc[3];
        sh_colour_n<KT>(D, shv, b, acc);
        float gch[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) gch[c] = (acc[c] + 0.5f < 0.0f) ? 0.0f : grgb[c];
        float s[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) s[k] = 0.f;
        const int nb = (D + 1) * (D + 1);
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          if (k < nb) {
            s[k] = (shv[3 * k] * gch[0] + shv[3 * k + 1] * gch[1]) + shv[3 * k + 2] * gch[2];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const float gk = b[k] * gch[c];
              if constexpr (GEN) dsh[3 * k + c] += nz ? gk * (1.0f + kSqrtPoint2 * nzr[3 * k + c]) : gk;
              else dsh[3 * k + c] += nzt ? gk * (1.0f + kSqrtPoint2 * nzt[3 * k + c]) : gk;
            }
          }
        }
        float ddx, ddy, ddz;
        sh_ddir(D, x, y, z, s, ddx, ddy, ddz);
        const float dot = (x * ddx + y * ddy) + z * ddz;
        dp[0] += (ddx - x * dot) / len; dp[1] += (ddy - y * dot) / len; dp[2] += (ddz - z * dot) / len;
      }
      // (2)-(6) geometry of this view with this view's scales
      const float s3[3] = {mod * sa[0], mod * sa[1], mod * sa[2]};
      float c6[6];
      cov3d_from(s3[0], s3[1], s3[2], R, c6);
      Ewa e;
      ewa_forward(vc, px, py, pz, c6, fx, fy, 1.3f * tfx, 1.3f * tfy, e);
      float dSv[9], dview[12], dproj[12];
      geom_backward(vc, e, fx, fy, W, H, px, py, pz, pa.x, pa.y, pa.z, pa.w, pb.x, pc.y, false, gndx, gndy, dSv, dp, dview,
                    dproj);
      float ds_v[3], dr_v[4];
      sigma_backward(dSv, R, s3, mod, q, ds_v, dr_v);
#pragma unroll
      for (int k = 0; k < 3; ++k) dsraw[k] += ds_v[k] * dsc[k];
#pragma unroll
      for (int k = 0; k < 4; ++k) drot[k] += dr_v[k];
      if (out.stat_denom && ((vb.stat_mask >> vv) & 1u)) {
        out.stat_xyz_gradient_accum[i] += sqrtf(gndx * gndx + gndy * gndy);
        out.stat_denom[i] += 1.0f;
        out.stat_max_radii2D[i] = fmaxf(out.stat_max_radii2D[i], (float)vb.radii[vv][i]);
      }
    }
    if (ok) {
      float* m2 = vb.dL_dmeans2D[vv];
      m2[3 * i] = gndx; m2[3 * i + 1] = gndy; m2[3 * i + 2] = 0.f;
    }
  }

  // gradient rows -> LDS (zeros for Gaussians no view saw) -> coalesced write-back into features_dc / features_rest
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  if (lane < n_valid) {
#pragma unroll
    for (int k = 0; k < F; ++k) sh[k] = dsh[k];
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const bool acc = out.accumulate != 0;
  if (!(acc && amask == 0ull)) {
    if (sg.dc[m]) stage_rows_out<3>(sg.dc[m] + wave_first * 3, 3, 0, stride, n_valid, lw, acc, amask);
    if constexpr (KT > 1) {
      if (sg.rest[m]) stage_rows_out<F - 3>(sg.rest[m] + wave_first * (F - 3), F - 3, 3, stride, n_valid, lw, acc, amask);
    }
  }

  if (ok) {
    if (acc && !any) {
      float* o = sg.scaling[m];
      if (has_gs && o) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[3 * row + k] += dsraw[k];
      }
    } else {
      // through q = raw / |raw| and sigmoid
      const float qd = ((q.x * drot[0] + q.y * drot[1]) + q.z * drot[2]) + q.w * drot[3];
      const float dr[4] = {(drot[0] - q.x * qd) / qnorm, (drot[1] - q.y * qd) / qnorm, (drot[2] - q.z * qd) / qnorm,
                           (drot[3] - q.w * qd) / qnorm};
      float gop_raw = 0.f;
      if (any) {
        const float sgm = act_sigmoid(sc.opacity[m][row]);
        gop_raw = gop * (sgm * (1.0f - sgm));
      }
      float* o;
      if ((o = sg.xyz[m])) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[3 * row + k] = acc ? o[3 * row + k] + dp[k] : dp[k];
      }
      if ((o = sg.scaling[m])) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[3 * row + k] = acc ? o[3 * row + k] + dsraw[k] : dsraw[k];
      }
      if ((o = sg.rotation[m])) {
        float4 t = make_float4(dr[0], dr[1], dr[2], dr[3]);
        if (acc) {
          const float4 old = *reinterpret_cast<const float4*>(o + 4 * row);
          t.x += old.x; t.y += old.y; t.z += old.z; t.w += old.w;
        }
        *reinterpret_cast<float4*>(o + 4 * row) = t;
      }
      if ((o = sg.opacity[m])) o[row] = acc ? o[row] + gop_raw : gop_raw;
    }
  }
}

}  // namespace

// GSR_K8_SPARSE=0 keeps the dense kernels (one chain rule per visible Gaussian and view) for comparison runs.
static bool gsr_k8_sparse() {
  static const bool on = [] {
    const char* e = getenv("GSR_K8_SPARSE");
    return !(e && e[0] == '0');
  }();
  return on;
}

namespace {
__global__ void __launch_bounds__(256) k_mask_all(unsigned long long* __restrict__ m, int64_t P) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nw = (P + 63) >> 6;
  if (w >= nw) return;
  const int64_t rest = P - (w << 6);
  m[w] = rest >= 64 ? ~0ull : ((1ull << rest) - 1ull);
}
}  // namespace
// a form of K8 that does not classify the reached Gaussians: every row may be non-zero
static void reached_mask_all(const GsrGrads& out, int32_t P, hipStream_t stream) {
  if (!out.reached_mask || P <= 0) return;
  const int64_t nw = ((int64_t)P + 63) >> 6;
  hipLaunchKernelGGL(k_mask_all, dim3((uint32_t)((nw + 255) / 256)), dim3(256), 0, stream,
                     reinterpret_cast<unsigned long long*>(out.reached_mask), (int64_t)P);
}

// K8 for n_views views of the same Gaussians in one pass. Supported: shs with K in {1, 4, 9, 16}, (scales, rotations),
// no camera gradients, no scene table (the caller falls back to one single-view K8 per view otherwise).
bool gsr_preprocess_bwd_views_supported(const GsrView& v, const GsrGaussians& g, const GsrGrads& out) {
  const int K = v.sh_stride;
  if (g.scene)
    return out.scene && (K == 1 || K == 4 || K == 9 || K == 16) && !out.dL_dview && !out.dL_dproj && !out.dL_dcampos;
  return g.shs && !g.scene && g.scales && g.rotations && !g.cov3D_precomp && !g.colors_precomp &&
         (K == 1 || K == 4 || K == 9 || K == 16) && !out.dL_dview && !out.dL_dproj && !out.dL_dcampos &&
         out.dL_dshs && out.dL_dscales && out.dL_drotations && out.dL_dmeans3D && out.dL_dopacities;
}

// ---- K8's form, chosen here and nowhere else: the launcher below follows it, and gsr_backward* clear the scratch by it.
//   one view (gsr_backward; gsr_backward_views view by view):
//     kSparseViews  no scene, K >= 9 and what the views kernel supports (gsr_preprocess_bwd_views_supported: SH rows,
//                   scales + rotations, no camera gradients, colours or precomputed covariances) -- the trainers' case
//     kSingleScene  otherwise, with a scene table: k_preprocess_bwd<KT, true, SceneTab, SceneGradTab>
//     kSingle       anything else: k_preprocess_bwd<KT>
//   n_views > 1 (gsr_backward_views, once gsr_preprocess_bwd_views_supported holds):
//     kSceneViews   a scene table: k_preprocess_bwd_views_scene<KT>
//     kSparseViews  K >= 9: k_preprocess_bwd_views<KT, PVS, true, KPER>
//     kDenseViews   K <= 4: k_preprocess_bwd_views<KT, PVS> (rows of 12 floats or fewer: skipping them saves less than
//                   the classification costs -- the 2 M indoor scene at K = 4 measured 36 us per view sparse, 33 dense)
//   GSR_K8_SPARSE=0: no kSparseViews -- one view takes kSingle, n_views > 1 kDenseViews.
// What follows from the form:
//   restores_scratch  the two non-scene views forms honour GsrGrads.scratch_clean (they zero the sums and marks they
//                     consume); after every other form gsr_backward* clears the scratch
//   marks_every_row   only kSparseViews classifies the reached Gaussians into GsrGrads.reached_mask; before every other
//                     form reached_mask_all sets every bit
//   big               kSparseViews: 1 024 Gaussians per workgroup when that gives every CU a workgroup, 256 otherwise
//                     (the form holds two workgroups per CU: 512 slots. 100 k Gaussians: 98 workgroups of 1 024 took
//                     51 us against 26 for 391 of 256 in one shift; from ~260 k on the small workgroups need two shifts
//                     and the large ones win)
enum class K8Form { kSingle, kSingleScene, kSparseViews, kDenseViews, kSceneViews };
struct K8Plan {
  K8Form form;
  bool restores_scratch, marks_every_row, big;
};

// (tests/k8_layout.py restates `big` and the launch grid that follows from it: change them together)
static K8Plan k8_plan(int n_views, const GsrView& v, const GsrGaussians& g, const GsrGrads& out) {
  const bool sparse = gsr_k8_sparse() && v.sh_stride >= 9;
  K8Form f;
  if (n_views == 1)
    f = !g.scene && sparse && !out.dL_dcolors && !out.dL_dcov3D && gsr_preprocess_bwd_views_supported(v, g, out)
            ? K8Form::kSparseViews
            : g.scene ? K8Form::kSingleScene : K8Form::kSingle;
  else
    f = g.scene ? K8Form::kSceneViews : sparse ? K8Form::kSparseViews : K8Form::kDenseViews;
  const bool views = f == K8Form::kSparseViews || f == K8Form::kDenseViews;
  return K8Plan{f, views && out.reach && out.scratch_clean, f != K8Form::kSparseViews,
                (int64_t)v.P >= (int64_t)256 * kK8Block};
}

// K8 of n_views views (1: one view) in the form k8_plan picks. *restored: the scratch (GsrGrads.partials + .reach) of
// every view is left zero under scratch_clean -- when false the caller clears it.
int gsr_launch_preprocess_bwd(int n_views, const GsrView* views, const GsrGaussians* gs, const GsrGeom* geoms,
                              const GsrGrads* outs, hipStream_t stream, bool* restored) {
  const GsrView& v = views[0];
  const GsrGaussians& g = gs[0];
  const K8Plan plan = k8_plan(n_views, v, g, outs[0]);
  *restored = plan.restores_scratch;
  if (plan.form == K8Form::kSingle || plan.form == K8Form::kSingleScene) {
    const GsrGeom& geom = geoms[0];
    const GsrGrads& out = outs[0];
    if (plan.marks_every_row) reached_mask_all(out, v.P, stream);
    if (plan.form == K8Form::kSingleScene) {
      SceneTab t; SceneGradTab gt;
      const uint32_t nbs = scene_tables(*g.scene, out.scene, t, gt);
      const size_t lds = gsr_preprocess_lds_bytes(v.sh_stride);
      return launch_sh<16, 9, 4, 1, 0>(fixed_sh(v.sh_stride), [&](auto kt) {
        with_flag(scene_noise_generated(1, &g), [&](auto gen) {
          hipLaunchKernelGGL((k_preprocess_bwd<kt, true, SceneTab, SceneGradTab, gen>), dim3(nbs), dim3(256), lds, stream, v,
                             g, t, gt, geom.radii, out.partials, out);
        });
      });
    }
    const uint32_t nb = gsr_num_blocks(v.P);
    const size_t lds = g.shs ? gsr_preprocess_lds_bytes(v.sh_stride) : 0;
    return launch_sh<16, 9, 4, 1, 0>(fixed_sh(g.shs ? v.sh_stride : 0), [&](auto kt) {
      hipLaunchKernelGGL(k_preprocess_bwd<kt>, dim3(nb), dim3(256), lds, stream, v, g, NoScene{}, NoScene{}, geom.radii,
                         out.partials, out);
    });
  }
  K8Views vb = K8Views{};
  vb.nv = n_views;
  fill_view_fields(vb, n_views, views, gs);
  for (int k = 0; k < n_views; ++k) {
    if (g.scene) vb.dL_dscales_out[k] = outs[k].scene ? outs[k].scene->dL_dscales_out : nullptr;
    vb.dL_dscales[k] = outs[k].dL_dscales;
    vb.radii[k] = geoms[k].radii; vb.partials[k] = outs[k].partials; vb.dL_dmeans2D[k] = outs[k].dL_dmeans2D;
    vb.reach[k] = g.scene ? nullptr : reinterpret_cast<unsigned long long*>(outs[k].reach);
    if ((outs[k].reach != nullptr) != (outs[0].reach != nullptr)) return GSR_EINVAL;
  }
  vb.restore = plan.restores_scratch ? 1 : 0;
  // densification statistics: the views whose GsrGrads entry names the statistics tensors (all the same ones)
  GsrGrads out0 = outs[0];
  out0.stat_max_radii2D = nullptr; out0.stat_xyz_gradient_accum = nullptr; out0.stat_denom = nullptr;
  for (int k = 0; k < n_views; ++k) {
    if (!outs[k].stat_denom) continue;
    if (out0.stat_denom && (outs[k].stat_denom != out0.stat_denom || outs[k].stat_max_radii2D != out0.stat_max_radii2D ||
                            outs[k].stat_xyz_gradient_accum != out0.stat_xyz_gradient_accum))
      return GSR_EINVAL;
    out0.stat_max_radii2D = outs[k].stat_max_radii2D; out0.stat_xyz_gradient_accum = outs[k].stat_xyz_gradient_accum;
    out0.stat_denom = outs[k].stat_denom;
    vb.stat_mask |= 1u << k;
  }
  const size_t lds = gsr_preprocess_lds_bytes(v.sh_stride);
  if (plan.marks_every_row) reached_mask_all(out0, v.P, stream);
  if (plan.form == K8Form::kSceneViews) {
    SceneTab t; SceneGradTab gt;
    const uint32_t nbs = scene_tables(*g.scene, outs[0].scene, t, gt);
    return launch_sh<16, 9, 4, 1>(v.sh_stride, [&](auto kt) {
      with_flag(scene_noise_generated(n_views, gs), [&](auto gen) {
        hipLaunchKernelGGL((k_preprocess_bwd_views_scene<kt, gen>), dim3(nbs), dim3(256), lds, stream, v, t, gt, vb, out0);
      });
    });
  }
  if (plan.form == K8Form::kSparseViews) {
    const int64_t per_wg = plan.big ? kK8Block : 256;
    const uint32_t nbr = (uint32_t)(((int64_t)v.P + per_wg - 1) / per_wg);
    return launch_sh<16, 9>(v.sh_stride, [&](auto kt) {
      with_flag(vb.per_view_scales, [&](auto pvs) {
        with_flag(plan.big, [&](auto big) {
          hipLaunchKernelGGL((k_preprocess_bwd_views<kt, pvs, true, big ? kK8Block / 256 : 1>), dim3(nbr), dim3(256), lds,
                             stream, v, g, vb, out0);
        });
      });
    });
  }
  const uint32_t nb = gsr_num_blocks(v.P);
  return launch_sh<16, 9, 4, 1>(v.sh_stride, [&](auto kt) {
    with_flag(vb.per_view_scales, [&](auto pvs) {
      hipLaunchKernelGGL((k_preprocess_bwd_views<kt, pvs>), dim3(nb), dim3(256), lds, stream, v, g, vb, out0);
    });
  });
}

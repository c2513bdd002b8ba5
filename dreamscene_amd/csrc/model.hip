// model.hip -- the three pieces of GaussianModel's lifecycle that are neither a render nor a densification, gfx950
// (include/gsrast.h, "model lifecycle"; dreamscene_amd/model.py; SEMANTICS.md section 15):
//   K_init   create_from_pcd (gs_renderer.py:582-608): the six leaves of a new model from points, colours and the kNN's mean
//            squared distances, in ONE launch. Lanes [0, P) take a row each (reads 28 bytes, writes 56); the lanes after them
//            clear f_rest, 16 bytes each where the tensor is 16-byte aligned (dword stores otherwise and in the tail).
//   K_reset  reset_opacity (:746-749 with :52-53): logit(min(sigmoid(x), cap)) into a tensor of its own and zeros over the two
//            Adam moments, one element per lane.
//   K_stats  add_densification_stats(_div) (:1061-1080): accum[i] += |grad[start + i].xy|, denom[i] += 1 where filter[i], one
//            row per lane; the expression is K8's (preprocess_bwd.hip, "densification statistics of this view").
// All three are streaming and element-wise: 256-thread blocks, a bounds check on the tail, no LDS, no atomics, nothing allocated,
// no memset (the launches stay capturable). One rounding per operator (this file is built with -ffp-contract=off); expf, logf,
// sqrtf and `/` are the full-precision forms, never the fast intrinsics.
#include "gsr_common.h"

namespace {

constexpr int kT = 256;                          // threads per block (4 waves)
constexpr float kC0 = 0.28209479177387814f;      // the fp32 rounding of utils/sh_utils.py's C0

__global__ void __launch_bounds__(kT) k_model_init(const float* __restrict__ points, const float* __restrict__ colors,
                                                   const float* __restrict__ dist2, const uint32_t P, const uint64_t rest_floats,
                                                   const int rest_vec, const float opacity_logit, float* __restrict__ xyz,
                                                   float* __restrict__ f_dc, float* __restrict__ f_rest,
                                                   float* __restrict__ scaling, float* __restrict__ rotation,
                                                   float* __restrict__ opacity) {
  const uint64_t e = (uint64_t)blockIdx.x * kT + threadIdx.x;
  if (e < P) {
    const size_t i = (size_t)e;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      xyz[3 * i + c] = points[3 * i + c];
      f_dc[3 * i + c] = (colors[3 * i + c] - 0.5f) / kC0;
    }
    const float s = logf(sqrtf(fmaxf(dist2[i], 1e-7f)));
    scaling[3 * i] = s; scaling[3 * i + 1] = s; scaling[3 * i + 2] = s;
    if ((reinterpret_cast<uintptr_t>(rotation) & 15u) == 0) {
      *reinterpret_cast<float4*>(rotation + 4 * i) = make_float4(1.f, 0.f, 0.f, 0.f);
    } else {
      rotation[4 * i] = 1.f; rotation[4 * i + 1] = 0.f; rotation[4 * i + 2] = 0.f; rotation[4 * i + 3] = 0.f;
    }
    opacity[i] = opacity_logit;
    return;
  }
  const uint64_t f0 = (e - P) * 4u;              // the first of this lane's 4 floats of f_rest
  if (f0 >= rest_floats) return;
  if (rest_vec && f0 + 4u <= rest_floats) {
    *reinterpret_cast<float4*>(f_rest + f0) = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    for (uint64_t k = f0; k < rest_floats && k < f0 + 4u; ++k) f_rest[k] = 0.f;
  }
}

__global__ void __launch_bounds__(kT) k_opacity_reset(const float* __restrict__ opacity, const uint32_t P, const float cap,
                                                      float* __restrict__ out, float* __restrict__ exp_avg,
                                                      float* __restrict__ exp_avg_sq) {
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i >= P) return;
  const float s = 1.f / (1.f + expf(-opacity[i]));
  const float m = (s != s) ? s : fminf(s, cap);                     // torch.min: a NaN propagates (fminf would drop it)
  out[i] = logf(m / (1.f - m));
  if (exp_avg) exp_avg[i] = 0.f;
  if (exp_avg_sq) exp_avg_sq[i] = 0.f;
}

__global__ void __launch_bounds__(kT) k_densify_stats(const float* __restrict__ grad, const uint8_t* __restrict__ filter,
                                                      const uint32_t start, const uint32_t n, float* __restrict__ accum,
                                                      float* __restrict__ denom) {
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i >= n || !filter[i]) return;
  const size_t r = 3 * ((size_t)start + i);
  const float gx = grad[r], gy = grad[r + 1];
  accum[i] += sqrtf(gx * gx + gy * gy);
  denom[i] += 1.0f;
}

bool misaligned4(const void* p) { return ((uintptr_t)p & 3u) != 0; }

// [a, a + na) and [b, b + nb) bytes share an address
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

}  // namespace

extern "C" int gsr_model_init(const float* points, const float* colors, const float* dist2, int32_t P, int32_t K,
                              float opacity_logit, float* xyz, float* f_dc, float* f_rest, float* scaling, float* rotation,
                              float* opacity, void* stream_) {
  if (P < 0 || !(K == 1 || K == 4 || K == 9 || K == 16)) return GSR_EINVAL;
  if (P == 0) return GSR_OK;
  if (!points || !colors || !dist2 || !xyz || !f_dc || !scaling || !rotation || !opacity || (K > 1 && !f_rest)) return GSR_EINVAL;
  if (misaligned4(points) || misaligned4(colors) || misaligned4(dist2) || misaligned4(xyz) || misaligned4(f_dc) ||
      misaligned4(scaling) || misaligned4(rotation) || misaligned4(opacity) || (K > 1 && misaligned4(f_rest)))
    return GSR_EINVAL;
  const uint64_t rest_floats = (uint64_t)P * 3u * (uint64_t)(K - 1);
  const int rest_vec = (K > 1 && ((uintptr_t)f_rest & 15u) == 0) ? 1 : 0;
  const uint64_t lanes = (uint64_t)P + (rest_floats + 3u) / 4u;
  const uint64_t blocks = (lanes + kT - 1) / kT;
  if (blocks > (uint64_t)INT32_MAX) return GSR_ECAPACITY;
  GsrDeviceGuard dev(xyz);
  hipLaunchKernelGGL(k_model_init, dim3((uint32_t)blocks), dim3(kT), 0, (hipStream_t)stream_, points, colors, dist2, (uint32_t)P,
                     rest_floats, rest_vec, opacity_logit, xyz, f_dc, K > 1 ? f_rest : (float*)nullptr, scaling, rotation, opacity);
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

extern "C" int gsr_opacity_reset(const float* opacity, int32_t P, float cap, float* opacity_out, float* exp_avg,
                                 float* exp_avg_sq, void* stream_) {
  if (P < 0) return GSR_EINVAL;
  if (P == 0) return GSR_OK;
  if (!opacity || !opacity_out || misaligned4(opacity) || misaligned4(opacity_out) || misaligned4(exp_avg) ||
      misaligned4(exp_avg_sq))
    return GSR_EINVAL;
  const size_t nb = (size_t)P * sizeof(float);
  if (overlap(opacity, nb, opacity_out, nb)) return GSR_EINVAL;     // the new logits go to a tensor of their own
  for (const float* m : {(const float*)exp_avg, (const float*)exp_avg_sq})
    if (m && (overlap(m, nb, opacity, nb) || overlap(m, nb, opacity_out, nb))) return GSR_EINVAL;
  if (exp_avg && exp_avg_sq && overlap(exp_avg, nb, exp_avg_sq, nb)) return GSR_EINVAL;
  GsrDeviceGuard dev(opacity_out);
  hipLaunchKernelGGL(k_opacity_reset, dim3(((uint32_t)P + kT - 1u) / kT), dim3(kT), 0, (hipStream_t)stream_, opacity, (uint32_t)P,
                     cap, opacity_out, exp_avg, exp_avg_sq);
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

extern "C" int gsr_densify_stats(const float* grad, int32_t P_total, const uint8_t* filter, int32_t start, int32_t n,
                                 float* accum, float* denom, void* stream_) {
  if (P_total < 0 || start < 0 || n < 0 || (int64_t)start + n > (int64_t)P_total) return GSR_EINVAL;
  if (n == 0) return GSR_OK;
  if (!grad || !filter || !accum || !denom || misaligned4(grad) || misaligned4(accum) || misaligned4(denom)) return GSR_EINVAL;
  const size_t nb = (size_t)n * sizeof(float);
  if (overlap(accum, nb, denom, nb)) return GSR_EINVAL;
  GsrDeviceGuard dev(accum);
  hipLaunchKernelGGL(k_densify_stats, dim3(((uint32_t)n + kT - 1u) / kT), dim3(kT), 0, (hipStream_t)stream_, grad, filter,
                     (uint32_t)start, (uint32_t)n, accum, denom);
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

// glue.hip -- the per-pixel glue between the rasterizer and the loss, gfx950: the disp post-processing of depth_alpha and
// the TV loss, forward and backward (include/gsrast.h, "per-pixel glue"; SEMANTICS.md "disp post-processing and tv_loss").
//
// disp (scene_gaussian.py:651-658, :874-881, :1023-1032):
//   disp = focal / (depth + alpha * 10 + 1e-5);  m = min(disp[alpha <= 0.1]) (or min(disp) when no pixel qualifies)
//   disp = clamp((disp - m) / (max(disp) - m), 0, 1)
// The per-pixel value is formed in torch's order of operations, one rounding per operator (this file is built with
// -ffp-contract=off): t = alpha * 10, u = (depth + t) + 1e-5, d = (1 / u) * focal (Python's `focal / tensor` is
// `tensor.reciprocal() * focal`). The masked minimum is chosen on the device: no boolean-mask gather, no host read.
//   forward   K_a: per view and block the partial (masked min, min, max, any masked); K_b: every block reduces its view's
//             partials (a few KB from L2), block 0 keeps (m, M, flag, M - m) for the backward, then disp and alpha are
//             written as [V,1,H,W]. Reads 2 x 8 bytes and writes 8 bytes per pixel.
//   backward  K_c: per view and block sum(h (d - m)), sum(h) in double and the tie counts, with h = g [0 <= q <= 1];
//             K_d: the fixed-order sum of those partials, then dL/d depth_alpha per pixel (d recomputed, not stored).
//             Reads 12 bytes, then 12 (16 with dL/dalpha), and writes 8 bytes per pixel.
// tv_loss (utils/system_utils.py:39-47): 2 (h_tv / count_h + w_tv / count_w) / B; differences and squares in fp32 as torch
// forms them, the sums in double through a fixed two-level reduction (the same bits on every run); the backward is one
// stencil pass that reads the upstream scalar from device memory.
// No float atomics anywhere: every sum has a fixed order.
#include "gsr_common.h"

namespace {

constexpr int kT = 256;                 // threads per block (4 waves)
constexpr int kDispMaxBlocks = 256;     // per view
constexpr int kTvMaxBlocks = 2048;      // Guideline 11: cap the grid, grid-stride the rest

struct DispPart {                       // one block of K_c
  double a, b;                          // sum h (d - m), sum h
  uint32_t n_m, n_M;                    // pixels of the selection set equal to m, pixels equal to M
  uint32_t pad_[2];
};
static_assert(sizeof(DispPart) == 32, "DispPart");

__device__ __forceinline__ float nan_min(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }

// torch's op chain for one pixel (see the file comment)
__device__ __forceinline__ float disp_u(float depth, float alpha) {
  const float t = alpha * 10.f;
  return (depth + t) + 1e-5f;
}
__device__ __forceinline__ float disp_d(float u, float focal) { return (1.f / u) * focal; }

// all 256 threads receive the result; the order of the combination is fixed (the same bits on every run)
template <class T, class Op>
__device__ __forceinline__ T block_reduce(T v, Op op, T* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  const T r = op(op(lds[0], lds[1]), op(lds[2], lds[3]));
  __syncthreads();
  return r;
}

struct FMin { __device__ float operator()(float a, float b) const { return nan_min(a, b); } };
struct FMax { __device__ float operator()(float a, float b) const { return nan_max(a, b); } };
struct UOr { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a | b; } };
struct UAdd { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };
struct DAdd { __device__ double operator()(double a, double b) const { return a + b; } };

// ---------------------------------------------------------------------------------------------------- disp forward
__global__ void __launch_bounds__(kT) k_disp_reduce(const GsrDispViews t, const uint32_t hw, float4* __restrict__ part) {
  __shared__ float lf[4];
  __shared__ uint32_t lu[4];
  const int v = blockIdx.y;
  const float* __restrict__ D = t.depth_alpha[v];
  const float* __restrict__ A = D + hw;
  const float focal = t.focal[v];
  float mmin = INFINITY, gmin = INFINITY, gmax = -INFINITY;
  uint32_t any = 0;
  for (uint32_t p = blockIdx.x * kT + threadIdx.x; p < hw; p += gridDim.x * kT) {
    const float a = A[p];
    const float d = disp_d(disp_u(D[p], a), focal);
    if (a <= 0.1f) {                  // torch compares in fp32: float32(0.1) itself is inside the mask
      mmin = nan_min(mmin, d);
      any = 1u;
    }
    gmin = nan_min(gmin, d);
    gmax = nan_max(gmax, d);
  }
  mmin = block_reduce(mmin, FMin(), lf);
  gmin = block_reduce(gmin, FMin(), lf);
  gmax = block_reduce(gmax, FMax(), lf);
  any = block_reduce(any, UOr(), lu);
  if (threadIdx.x == 0) part[(size_t)v * gridDim.x + blockIdx.x] = make_float4(mmin, gmin, gmax, __uint_as_float(any));
}

__global__ void __launch_bounds__(kT) k_disp_apply(const GsrDispViews t, const uint32_t hw, const float4* __restrict__ part,
                                                   const int nb, float* __restrict__ disp, float* __restrict__ alpha_out,
                                                   float4* __restrict__ stats) {
  __shared__ float lf[4];
  __shared__ uint32_t lu[4];
  const int v = blockIdx.y;
  float mmin = INFINITY, gmin = INFINITY, gmax = -INFINITY;
  uint32_t any = 0;
  for (int k = threadIdx.x; k < nb; k += kT) {
    const float4 q = part[(size_t)v * nb + k];
    mmin = nan_min(mmin, q.x);
    gmin = nan_min(gmin, q.y);
    gmax = nan_max(gmax, q.z);
    any |= __float_as_uint(q.w);
  }
  mmin = block_reduce(mmin, FMin(), lf);
  gmin = block_reduce(gmin, FMin(), lf);
  gmax = block_reduce(gmax, FMax(), lf);
  any = block_reduce(any, UOr(), lu);
  const float m = any ? mmin : gmin;   // the reference's try / except: the global minimum when the mask is empty
  const float M = gmax;
  const float r = M - m;
  if (blockIdx.x == 0 && threadIdx.x == 0) stats[v] = make_float4(m, M, any ? 1.f : 0.f, r);
  const float* __restrict__ D = t.depth_alpha[v];
  const float* __restrict__ A = D + hw;
  const float focal = t.focal[v];
  float* __restrict__ O = disp + (size_t)v * hw;
  float* __restrict__ OA = alpha_out + (size_t)v * hw;
  for (uint32_t p = blockIdx.x * kT + threadIdx.x; p < hw; p += gridDim.x * kT) {
    const float a = A[p];
    const float d = disp_d(disp_u(D[p], a), focal);
    const float q = (d - m) / r;                                   // a flat view: 0 / 0 = NaN, kept by the clamp
    O[p] = (q != q) ? q : fminf(fmaxf(q, 0.f), 1.f);
    OA[p] = a;
  }
}

// --------------------------------------------------------------------------------------------------- disp backward
__global__ void __launch_bounds__(kT) k_disp_bsum(const GsrDispViews t, const uint32_t hw, const float4* __restrict__ stats,
                                                  const float* __restrict__ g_disp, DispPart* __restrict__ part) {
  __shared__ double ld[4];
  __shared__ uint32_t lu[4];
  const int v = blockIdx.y;
  const float4 s = stats[v];
  const float m = s.x, M = s.y, r = s.w;
  const bool sel_all = s.z == 0.f;
  const double m64 = (double)m;
  const float* __restrict__ D = t.depth_alpha[v];
  const float* __restrict__ A = D + hw;
  const float* __restrict__ G = g_disp + (size_t)v * hw;
  const float focal = t.focal[v];
  double sa = 0.0, sb = 0.0;
  uint32_t nm = 0, nM = 0;
  for (uint32_t p = blockIdx.x * kT + threadIdx.x; p < hw; p += gridDim.x * kT) {
    const float a = A[p];
    const float d = disp_d(disp_u(D[p], a), focal);
    const float q = (d - m) / r;
    const double h = (q >= 0.f && q <= 1.f) ? (double)G[p] : 0.0;   // torch's clamp mask: inclusive, NaN -> 0
    sa += h * ((double)d - m64);
    sb += h;
    nm += ((sel_all || a <= 0.1f) && d == m) ? 1u : 0u;
    nM += (d == M) ? 1u : 0u;
  }
  sa = block_reduce(sa, DAdd(), ld);
  sb = block_reduce(sb, DAdd(), ld);
  nm = block_reduce(nm, UAdd(), lu);
  nM = block_reduce(nM, UAdd(), lu);
  if (threadIdx.x == 0) {
    DispPart o;
    o.a = sa; o.b = sb; o.n_m = nm; o.n_M = nM; o.pad_[0] = o.pad_[1] = 0u;
    part[(size_t)v * gridDim.x + blockIdx.x] = o;
  }
}

__global__ void __launch_bounds__(kT) k_disp_bapply(const GsrDispViews t, const uint32_t hw, const float4* __restrict__ stats,
                                                    const float* __restrict__ g_disp, const float* __restrict__ g_alpha,
                                                    const DispPart* __restrict__ part, const int nb) {
  __shared__ double ld[4];
  __shared__ uint32_t lu[4];
  const int v = blockIdx.y;
  double sa = 0.0, sb = 0.0;
  uint32_t nm = 0, nM = 0;
  for (int k = threadIdx.x; k < nb; k += kT) {        // fixed order: the same sums in every block and on every run
    const DispPart q = part[(size_t)v * nb + k];
    sa += q.a; sb += q.b; nm += q.n_m; nM += q.n_M;
  }
  sa = block_reduce(sa, DAdd(), ld);
  sb = block_reduce(sb, DAdd(), ld);
  nm = block_reduce(nm, UAdd(), lu);
  nM = block_reduce(nM, UAdd(), lu);
  const float4 s = stats[v];
  const float m = s.x, M = s.y, r = s.w;
  const bool sel_all = s.z == 0.f;
  const double r64 = (double)M - (double)m;
  const double dm = -sb / r64 + sa / (r64 * r64);       // dL/dm
  const double dM = -sa / (r64 * r64);                  // dL/dM
  const double share_m = dm / (double)nm, share_M = dM / (double)nM;   // torch's min() / max(): evenly among the ties
  const float* __restrict__ D = t.depth_alpha[v];
  const float* __restrict__ A = D + hw;
  const float* __restrict__ G = g_disp + (size_t)v * hw;
  const float* __restrict__ GA = g_alpha ? g_alpha + (size_t)v * hw : nullptr;
  float* __restrict__ OD = t.dL_ddepth_alpha[v];
  float* __restrict__ OA = OD + hw;
  const float focal = t.focal[v];
  const double focal64 = (double)focal;
  for (uint32_t p = blockIdx.x * kT + threadIdx.x; p < hw; p += gridDim.x * kT) {
    const float a = A[p];
    const float u = disp_u(D[p], a);
    const float d = disp_d(u, focal);
    const float q = (d - m) / r;
    const double h = (q >= 0.f && q <= 1.f) ? (double)G[p] : 0.0;
    double dd = h / r64;
    if ((sel_all || a <= 0.1f) && d == m) dd += share_m;
    if (d == M) dd += share_M;
    const double u64 = (double)u;
    const double du = -(dd * focal64) / (u64 * u64);    // d = focal / u
    OD[p] = (float)du;
    OA[p] = (float)(10.0 * du + (GA ? (double)GA[p] : 0.0));
  }
}

// --------------------------------------------------------------------------------------------------------------- TV
// Work unit: 4 consecutive pixels of one row of one [H,W] plane. vec: W % 4 == 0 and x 16-byte aligned (dwordx4 loads).
__device__ __forceinline__ void load4(const float* __restrict__ row, int j0, int W, bool vec, float v[4]) {
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(row + j0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (j0 + k < W) ? row[j0 + k] : 0.f;
  }
}

__global__ void __launch_bounds__(kT) k_tv_partial(const float* __restrict__ x, const int H, const int W, const uint32_t Q,
                                                   const uint32_t units, const int vec, double2* __restrict__ part) {
  __shared__ double ld[4];
  double sh = 0.0, sw = 0.0;
  for (uint32_t e = blockIdx.x * kT + threadIdx.x; e < units; e += gridDim.x * kT) {
    const uint32_t row = e / Q;
    const int j0 = (int)(e - row * Q) * 4;
    const int i = (int)(row % (uint32_t)H);
    const float* __restrict__ R = x + (size_t)row * W;
    float c[4], n[4];
    load4(R, j0, W, vec, c);
    if (i < H - 1) {
      load4(R + W, j0, W, vec, n);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j0 + k < W) {
          const float dh = n[k] - c[k];
          sh += (double)(dh * dh);
        }
    }
    const float right = (j0 + 4 < W) ? R[j0 + 4] : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (j0 + k < W - 1) {
        const float dw = (k < 3 ? c[k + 1] : right) - c[k];
        sw += (double)(dw * dw);
      }
  }
  sh = block_reduce(sh, DAdd(), ld);
  sw = block_reduce(sw, DAdd(), ld);
  if (threadIdx.x == 0) part[blockIdx.x] = make_double2(sh, sw);
}

__global__ void __launch_bounds__(kT) k_tv_final(const double2* __restrict__ part, const int nb, const double count_h,
                                                 const double count_w, const double batch, float* __restrict__ out) {
  __shared__ double ld[4];
  double sh = 0.0, sw = 0.0;
  for (int k = threadIdx.x; k < nb; k += kT) {
    const double2 q = part[k];
    sh += q.x;
    sw += q.y;
  }
  sh = block_reduce(sh, DAdd(), ld);
  sw = block_reduce(sw, DAdd(), ld);
  if (threadIdx.x == 0) out[0] = (float)(2.0 * (sh / count_h + sw / count_w) / batch);
}

__global__ void __launch_bounds__(kT) k_tv_bwd(const float* __restrict__ x, const int H, const int W, const uint32_t Q,
                                               const uint32_t units, const int vec, const float* __restrict__ g,
                                               const double ch, const double cw, float* __restrict__ gx) {
  const double gg = (double)g[0];
  for (uint32_t e = blockIdx.x * kT + threadIdx.x; e < units; e += gridDim.x * kT) {
    const uint32_t row = e / Q;
    const int j0 = (int)(e - row * Q) * 4;
    const int i = (int)(row % (uint32_t)H);
    const float* __restrict__ R = x + (size_t)row * W;
    float c[4], up[4] = {0.f, 0.f, 0.f, 0.f}, dn[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    load4(R, j0, W, vec, c);
    if (i > 0) load4(R - W, j0, W, vec, up);
    if (i < H - 1) load4(R + W, j0, W, vec, dn);
    const float left = j0 > 0 ? R[j0 - 1] : 0.f;
    const float right = (j0 + 4 < W) ? R[j0 + 4] : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = j0 + k;
      double acc = 0.0;
      if (i > 0) acc += ch * (double)(c[k] - up[k]);
      if (i < H - 1) acc -= ch * (double)(dn[k] - c[k]);
      const float lf = k > 0 ? c[k - 1] : left;
      const float rt = k < 3 ? c[k + 1] : right;
      if (j > 0) acc += cw * (double)(c[k] - lf);
      if (j < W - 1) acc -= cw * (double)(rt - c[k]);
      o[k] = (float)(gg * acc);
    }
    float* __restrict__ O = gx + (size_t)row * W;
    if (vec) {
      *reinterpret_cast<float4*>(O + j0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j0 + k < W) O[j0 + k] = o[k];
    }
  }
}

// ------------------------------------------------------------------------------------------------------ host helpers
int disp_blocks(uint32_t hw) { return (int)((hw + 1023u) / 1024u < (uint32_t)kDispMaxBlocks ? (hw + 1023u) / 1024u : kDispMaxBlocks); }

bool disp_shape_ok(int32_t n_views, int32_t h, int32_t w) {
  return n_views >= 1 && n_views <= GSR_MAX_DISP_VIEWS && h >= 1 && w >= 1 && (int64_t)h * w <= (int64_t)INT32_MAX;
}

int disp_validate(const GsrDispViews* t, bool backward) {
  if (!t || !disp_shape_ok(t->n_views, t->height, t->width)) return GSR_EINVAL;
  for (int k = 0; k < t->n_views; ++k) {
    if (!t->depth_alpha[k]) return GSR_EINVAL;
    if (backward && !t->dL_ddepth_alpha[k]) return GSR_EINVAL;
  }
  return GSR_OK;
}

struct TvShape {
  uint32_t Q = 0, units = 0, grid = 0;
};

bool tv_shape(int32_t B, int32_t C, int32_t H, int32_t W, TvShape* s) {
  if (B < 1 || C < 1 || H < 2 || W < 2) return false;
  const int64_t Q = ((int64_t)W + 3) / 4;
  const int64_t units = (int64_t)B * C * H * Q;
  if (units > (int64_t)INT32_MAX) return false;
  s->Q = (uint32_t)Q;
  s->units = (uint32_t)units;
  const int64_t g = (units + kT - 1) / kT;
  s->grid = (uint32_t)(g < kTvMaxBlocks ? g : kTvMaxBlocks);
  return true;
}

size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" size_t gsr_disp_scratch_bytes(int32_t n_views, int32_t height, int32_t width) {
  if (!disp_shape_ok(n_views, height, width)) return 0;
  const int nb = disp_blocks((uint32_t)((int64_t)height * width));
  return round256((size_t)n_views * nb * sizeof(DispPart));   // the backward's partials; the forward's (16 B) fit too
}

extern "C" int gsr_disp_forward(const GsrDispViews* views, float* disp, float* alpha, float* stats, void* scratch,
                                size_t scratch_bytes, void* stream_) {
  const int rc = disp_validate(views, false);
  if (rc) return rc;
  if (!disp || !alpha || !stats || !scratch || ((uintptr_t)scratch & 15u) || ((uintptr_t)stats & 15u)) return GSR_EINVAL;
  if (scratch_bytes < gsr_disp_scratch_bytes(views->n_views, views->height, views->width)) return GSR_ESCRATCH;
  const uint32_t hw = (uint32_t)((int64_t)views->height * views->width);
  const int nb = disp_blocks(hw);
  const dim3 grid((uint32_t)nb, (uint32_t)views->n_views);
  hipStream_t stream = (hipStream_t)stream_;
  GsrDeviceGuard dev(views->depth_alpha[0]);
  float4* part = reinterpret_cast<float4*>(scratch);
  hipLaunchKernelGGL(k_disp_reduce, grid, dim3(kT), 0, stream, *views, hw, part);
  GSR_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_disp_apply, grid, dim3(kT), 0, stream, *views, hw, (const float4*)part, nb, disp, alpha,
                     reinterpret_cast<float4*>(stats));
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

extern "C" int gsr_disp_backward(const GsrDispViews* views, const float* stats, const float* dL_ddisp, const float* dL_dalpha,
                                 void* scratch, size_t scratch_bytes, void* stream_) {
  const int rc = disp_validate(views, true);
  if (rc) return rc;
  if (!stats || !dL_ddisp || !scratch || ((uintptr_t)scratch & 15u) || ((uintptr_t)stats & 15u)) return GSR_EINVAL;
  if (scratch_bytes < gsr_disp_scratch_bytes(views->n_views, views->height, views->width)) return GSR_ESCRATCH;
  const uint32_t hw = (uint32_t)((int64_t)views->height * views->width);
  const int nb = disp_blocks(hw);
  const dim3 grid((uint32_t)nb, (uint32_t)views->n_views);
  hipStream_t stream = (hipStream_t)stream_;
  GsrDeviceGuard dev(views->depth_alpha[0]);
  DispPart* part = reinterpret_cast<DispPart*>(scratch);
  const float4* st = reinterpret_cast<const float4*>(stats);
  hipLaunchKernelGGL(k_disp_bsum, grid, dim3(kT), 0, stream, *views, hw, st, dL_ddisp, part);
  GSR_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_disp_bapply, grid, dim3(kT), 0, stream, *views, hw, st, dL_ddisp, dL_dalpha, (const DispPart*)part, nb);
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

extern "C" size_t gsr_tv_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
  TvShape s;
  if (!tv_shape(B, C, H, W, &s)) return 0;
  return round256((size_t)s.grid * sizeof(double2));
}

extern "C" int gsr_tv_forward(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, float* out, void* scratch,
                              size_t scratch_bytes, void* stream_) {
  TvShape s;
  if (!x || !out || !scratch || ((uintptr_t)scratch & 15u) || !tv_shape(B, C, H, W, &s)) return GSR_EINVAL;
  if (scratch_bytes < gsr_tv_scratch_bytes(B, C, H, W)) return GSR_ESCRATCH;
  const int vec = (W % 4 == 0 && ((uintptr_t)x & 15u) == 0) ? 1 : 0;
  hipStream_t stream = (hipStream_t)stream_;
  GsrDeviceGuard dev(x);
  double2* part = reinterpret_cast<double2*>(scratch);
  hipLaunchKernelGGL(k_tv_partial, dim3(s.grid), dim3(kT), 0, stream, x, (int)H, (int)W, s.Q, s.units, vec, part);
  GSR_HIP(hipGetLastError());
  const double count_h = (double)C * (H - 1) * W, count_w = (double)C * H * (W - 1);
  hipLaunchKernelGGL(k_tv_final, dim3(1), dim3(kT), 0, stream, (const double2*)part, (int)s.grid, count_h, count_w, (double)B,
                     out);
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

extern "C" int gsr_tv_backward(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, const float* dL_dout, float* dL_dx,
                               void* stream_) {
  TvShape s;
  if (!x || !dL_dout || !dL_dx || !tv_shape(B, C, H, W, &s)) return GSR_EINVAL;
  const int vec = (W % 4 == 0 && (((uintptr_t)x | (uintptr_t)dL_dx) & 15u) == 0) ? 1 : 0;
  const double count_h = (double)C * (H - 1) * W, count_w = (double)C * H * (W - 1);
  // d/dx of 2 (sum dh^2 / count_h + sum dw^2 / count_w) / B: 4 dh / (B count_h) per difference, 4 dw / (B count_w)
  const double ch = 4.0 / ((double)B * count_h), cw = 4.0 / ((double)B * count_w);
  hipStream_t stream = (hipStream_t)stream_;
  GsrDeviceGuard dev(x);
  hipLaunchKernelGGL(k_tv_bwd, dim3(s.grid), dim3(kT), 0, stream, x, (int)H, (int)W, s.Q, s.units, vec, dL_dout, ch, cw, dL_dx);
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

// photometric.hip -- the photometric loss between a rendered image and its target, gfx950 (include/gsrast.h, "photometric
// loss"; SEMANTICS.md section 14): per view  w_l2 mean((x-y)^2) + w_l1 mean|x-y| + w_dssim (1 - mean(ssim_map(x, y))),
// forward and backward (utils/system_utils.py:59-126: l1_loss, l2_loss, ssim).
//
// ssim_map: the 11x11 Gaussian window (sigma 1.5, zero padding 5, per channel) applied SEPARABLY, a horizontal pass of 11
// taps and a vertical pass of 11 taps, to the five moments x, y, x^2, y^2, xy; then per pixel
//   m = ((2 mu_x mu_y + C1)(2 s_xy + C2)) / ((mu_x^2 + mu_y^2 + C1)(s_x + s_y + C2)),  s = E[ab] - mu_a mu_b.
//   SSIM form   k_photo_ssim_fwd: one block per (32x32 tile, channel, view). The 42x42 halo of x and y goes to LDS (zeros
//               outside the image), 4 outputs per lane and row in the horizontal pass (16-byte LDS reads and writes), a
//               column of 4 outputs per lane in the vertical pass (consecutive lanes on consecutive banks). The L1 / L2
//               terms are folded in at the centre pixels. Per block one (sum m, sum |d|, sum d^2) in double; with a
//               `saved` buffer also the planes dm/dmu_x, dm/ds_x, dm/ds_xy which the backward needs.
//               k_photo_ssim_bwd: the same two passes over the three saved planes (the window is symmetric, so the
//               adjoint of the zero-padded convolution is the same convolution), dL/dx = -w_dssim (A + 2x B + y C) + the
//               L1 / L2 terms, times dL/dloss[v] / (C H W) read from device memory.
//   point-wise  k_photo_pw_fwd / k_photo_pw_bwd when w_dssim == 0: no halo, no LDS tile, no saved planes.
//   k_photo_final  per view the fixed-order sum of the partials, loss[v] and the three unweighted terms.
// All per-pixel arithmetic is fp32 (this file is built with -ffp-contract=off; the window sums name their fmaf), every
// sum over pixels is in double in a fixed order: no atomics, the same bits on every run. No host read, no allocation, no
// memset node: forward and backward are capturable.
#include <hip/hip_fp16.h>
#include <math.h>

#include "gsr_common.h"

namespace {

constexpr int kT = 256;                    // threads per block (4 waves)
constexpr int kTS = 32;                    // tile side (output pixels)
constexpr int kR = GSR_PHOTO_WINDOW / 2;   // 5
constexpr int kIN = kTS + 2 * kR;          // 42 halo rows / columns
constexpr int kP = 44;                     // LDS pitch of a halo row in floats: 8 units x 4 columns + 12, 16-byte rows
constexpr int kHP = kTS + 4;               // LDS pitch of a row of horizontal sums: 36 floats
constexpr int kUnits = kIN * (kTS / 4);    // 336 horizontal work units: 4 consecutive outputs of one halo row
// Unit e works on halo row e % 42, columns 4 (e / 42) ...: consecutive lanes take consecutive rows. The 16 lanes that one
// ds_read_b128 cycle serves then sit in 16 rows that differ mod 16, 44 floats = 11 four-bank slots apart, and 11 r mod 16 takes
// 16 different values: no conflict (except where a wave wraps from row 41 to row 0). The 8 lanes of a ds_write_b128 cycle sit
// in 8 consecutive rows, 36 floats = 9 slots apart: 8 different slots of the 8.
constexpr int kPwMaxBlocks = 256;          // point-wise form, per view
constexpr float kC1 = (float)(0.01 * 0.01);   // the reference's Python doubles, rounded where torch rounds them
constexpr float kC2 = (float)(0.03 * 0.03);

struct Win { float w[GSR_PHOTO_WINDOW]; };
struct Part { double m, l1, l2, pad_; };   // one block's sums
static_assert(sizeof(Part) == 32, "Part");

template <bool kHalfT>
__device__ __forceinline__ float load_target(const void* __restrict__ p, size_t i) {
  if constexpr (kHalfT) return __half2float(reinterpret_cast<const __half*>(p)[i]);   // exact widening
  else return reinterpret_cast<const float*>(p)[i];
}
// half_images: x rounded to fp16 (nearest even) and widened again, torch's .to(float16)
__device__ __forceinline__ float round_image(float x, bool to_half) { return to_half ? __half2float(__float2half_rn(x)) : x; }

// all 256 threads receive the sum; the order of the combination is fixed
__device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = (lds[0] + lds[1]) + (lds[2] + lds[3]);
  __syncthreads();
  return r;
}

// d|d|/dd as torch's abs gives it: 0 at 0
__device__ __forceinline__ double sign0(float d) { return d > 0.f ? 1.0 : (d < 0.f ? -1.0 : 0.0); }

// The horizontal pass of one unit: 4 consecutive outputs from 14 consecutive inputs (16 are read: four 16-byte reads).
__device__ __forceinline__ void load16(const float* __restrict__ row, float v[16]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 a = *reinterpret_cast<const float4*>(row + 4 * q);
    v[4 * q] = a.x; v[4 * q + 1] = a.y; v[4 * q + 2] = a.z; v[4 * q + 3] = a.w;
  }
}

// m and its three derivatives at one pixel. With mu_y, E[y^2] fixed, m is a function of (mu_x, E[x^2], E[xy]):
//   pb = dm/dE[x^2] = dm/ds_x = -m / B2,   pc = dm/dE[xy] = dm/ds_xy = 2 A1 / (B1 B2),
//   pa = dm/dmu_x (total: through A1, B1 and through s_x, s_xy) = 2 (mu_y (A2 - A1) + mu_x m (B1 - B2)) / (B1 B2).
// Written so that identical images give m = 1, pa = 0 and pc = -2 pb exactly (then dL/dx is exactly 0).
__device__ __forceinline__ void ssim_point(float mu1, float mu2, float e11, float e22, float e12, float& m, float& pa, float& pb,
                                           float& pc) {
  const float mu1s = mu1 * mu1, mu2s = mu2 * mu2, mu12 = mu1 * mu2;
  const float s1 = e11 - mu1s, s2 = e22 - mu2s, s12 = e12 - mu12;
  const float A1 = 2.f * mu12 + kC1, A2 = 2.f * s12 + kC2;
  const float B1 = (mu1s + mu2s) + kC1, B2 = (s1 + s2) + kC2;
  const float D = B1 * B2;
  m = (A1 * A2) / D;
  pb = -(m / B2);
  pc = (2.f * (A1 / B1)) / B2;
  const float t = mu2 * (A2 - A1) + (mu1 * m) * (B1 - B2);
  pa = (2.f * t) / D;
}

// ------------------------------------------------------------------------------------------------------ SSIM form, forward
template <bool kHalfT>
__global__ void __launch_bounds__(kT) k_photo_ssim_fwd(const GsrPhotoViews t, const Win win, const int tiles_x,
                                                       float* __restrict__ saved, const size_t plane,
                                                       Part* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float sx[kIN * kP];
  __shared__ __attribute__((aligned(16))) float sy[kIN * kP];
  __shared__ __attribute__((aligned(16))) float hm[5][kIN * kHP];
  __shared__ double ld[4];
  const int tid = threadIdx.x;
  const int v = blockIdx.z, c = blockIdx.y;
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int H = t.height, W = t.width;
  const int x0 = tx * kTS, y0 = ty * kTS;
  const size_t coff = (size_t)c * H * W;
  const float* __restrict__ X = t.image[v];
  const void* __restrict__ Y = t.target[v];
  const bool to_half = t.round_image_to_half != 0;

  for (int i = tid; i < kIN * kP; i += kT) {
    const int r = i / kP, cc = i - r * kP;
    const int gy = y0 - kR + r, gx = x0 - kR + cc;
    float xv = 0.f, yv = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const size_t o = coff + (size_t)gy * W + gx;
      xv = round_image(X[o], to_half);
      yv = load_target<kHalfT>(Y, o);
    }
    sx[i] = xv;
    sy[i] = yv;
  }
  __syncthreads();

  for (int e = tid; e < kUnits; e += kT) {
    const int u = e / kIN, r = e - u * kIN;
    float vx[16], vy[16];
    load16(sx + r * kP + 4 * u, vx);
    load16(sy + r * kP + 4 * u, vy);
    float acc[5][4];
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[q][j] = 0.f;
#pragma unroll
    for (int k = 0; k < GSR_PHOTO_WINDOW; ++k) {
      const float w = win.w[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float a = vx[j + k], b = vy[j + k];
        acc[0][j] = fmaf(w, a, acc[0][j]);
        acc[1][j] = fmaf(w, b, acc[1][j]);
        acc[2][j] = fmaf(w, a * a, acc[2][j]);
        acc[3][j] = fmaf(w, b * b, acc[3][j]);
        acc[4][j] = fmaf(w, a * b, acc[4][j]);
      }
    }
#pragma unroll
    for (int q = 0; q < 5; ++q)
      *reinterpret_cast<float4*>(&hm[q][r * kHP + 4 * u]) = make_float4(acc[q][0], acc[q][1], acc[q][2], acc[q][3]);
  }
  __syncthreads();

  const int col = tid & 31, rg = tid >> 5;
  float o[5][4];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    float hv[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) hv[k] = hm[q][(rg * 4 + k) * kHP + col];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < GSR_PHOTO_WINDOW; ++k) a = fmaf(win.w[k], hv[j + k], a);
      o[q][j] = a;
    }
  }
  double sm = 0.0, s1 = 0.0, s2 = 0.0;
  const int gx = x0 + col;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ly = rg * 4 + j, gy = y0 + ly;
    if (gy < H && gx < W) {
      float m, pa, pb, pc;
      ssim_point(o[0][j], o[1][j], o[2][j], o[3][j], o[4][j], m, pa, pb, pc);
      const float d = sx[(ly + kR) * kP + col + kR] - sy[(ly + kR) * kP + col + kR];
      sm += (double)m;
      s1 += (double)fabsf(d);
      s2 += (double)(d * d);
      if (saved) {
        const size_t p = ((size_t)v * t.channels + c) * ((size_t)H * W) + (size_t)gy * W + gx;
        saved[p] = pa;
        saved[plane + p] = pb;
        saved[2 * plane + p] = pc;
      }
    }
  }
  sm = block_sum(sm, ld);
  s1 = block_sum(s1, ld);
  s2 = block_sum(s2, ld);
  if (tid == 0) {
    Part q;
    q.m = sm; q.l1 = s1; q.l2 = s2; q.pad_ = 0.0;
    part[((size_t)v * t.channels + c) * gridDim.x + blockIdx.x] = q;
  }
}

// ----------------------------------------------------------------------------------------------------- SSIM form, backward
template <bool kHalfT>
__global__ void __launch_bounds__(kT) k_photo_ssim_bwd(const GsrPhotoViews t, const GsrPhotoWeights wt, const Win win,
                                                       const int tiles_x, const float* __restrict__ saved, const size_t plane,
                                                       const float* __restrict__ g, const double inv_n) {
  __shared__ __attribute__((aligned(16))) float sp[3][kIN * kP];
  __shared__ __attribute__((aligned(16))) float hm[3][kIN * kHP];
  const int tid = threadIdx.x;
  const int v = blockIdx.z, c = blockIdx.y;
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int H = t.height, W = t.width;
  const int x0 = tx * kTS, y0 = ty * kTS;
  const size_t coff = (size_t)c * H * W;
  const float* __restrict__ S = saved + ((size_t)v * t.channels + c) * ((size_t)H * W);

  for (int i = tid; i < kIN * kP; i += kT) {
    const int r = i / kP, cc = i - r * kP;
    const int gy = y0 - kR + r, gx = x0 - kR + cc;
    float a = 0.f, b = 0.f, cq = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const size_t p = (size_t)gy * W + gx;
      a = S[p];
      b = S[plane + p];
      cq = S[2 * plane + p];
    }
    sp[0][i] = a;
    sp[1][i] = b;
    sp[2][i] = cq;
  }
  __syncthreads();

  for (int e = tid; e < kUnits; e += kT) {
    const int u = e / kIN, r = e - u * kIN;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      float vv[16], acc[4] = {0.f, 0.f, 0.f, 0.f};
      load16(sp[q] + r * kP + 4 * u, vv);
#pragma unroll
      for (int k = 0; k < GSR_PHOTO_WINDOW; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fmaf(win.w[k], vv[j + k], acc[j]);
      *reinterpret_cast<float4*>(&hm[q][r * kHP + 4 * u]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
  }
  __syncthreads();

  const int col = tid & 31, rg = tid >> 5;
  float o[3][4];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    float hv[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) hv[k] = hm[q][(rg * 4 + k) * kHP + col];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < GSR_PHOTO_WINDOW; ++k) a = fmaf(win.w[k], hv[j + k], a);
      o[q][j] = a;
    }
  }
  const double scale = (double)g[v] * inv_n;
  const double w2 = 2.0 * (double)wt.l2, w1 = (double)wt.l1, wd = (double)wt.dssim;
  const bool to_half = t.round_image_to_half != 0;
  const int gx = x0 + col;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int gy = y0 + rg * 4 + j;
    if (gy < H && gx < W) {
      const size_t p = coff + (size_t)gy * W + gx;
      const float xv = round_image(t.image[v][p], to_half);
      const float yv = load_target<kHalfT>(t.target[v], p);
      const float d = xv - yv;
      // one rounding per operator: for identical images (2x) B and y C cancel exactly
      const float s = (o[0][j] + (2.f * xv) * o[1][j]) + yv * o[2][j];
      t.dL_dimage[v][p] = (float)((w2 * (double)d + w1 * sign0(d) - wd * (double)s) * scale);
    }
  }
}

// --------------------------------------------------------------------------------------------------------- point-wise form
// Work unit: 4 consecutive entries of one view's C H W. vec: every plane 16-byte aligned (fp16 targets: 8) and C H W % 4 == 0.
template <bool kHalfT>
__device__ __forceinline__ void pw_load(const GsrPhotoViews& t, int v, uint32_t i0, uint32_t n, bool vec, bool to_half,
                                        float x[4], float y[4]) {
  if (vec) {
    const float4 a = *reinterpret_cast<const float4*>(t.image[v] + i0);
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
    if constexpr (kHalfT) {
      const uint2 raw = *reinterpret_cast<const uint2*>(reinterpret_cast<const __half*>(t.target[v]) + i0);
      const __half2 h0 = *reinterpret_cast<const __half2*>(&raw.x), h1 = *reinterpret_cast<const __half2*>(&raw.y);
      y[0] = __low2float(h0); y[1] = __high2float(h0); y[2] = __low2float(h1); y[3] = __high2float(h1);
    } else {
      const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(t.target[v]) + i0);
      y[0] = b.x; y[1] = b.y; y[2] = b.z; y[3] = b.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool in = i0 + k < n;
      x[k] = in ? t.image[v][i0 + k] : 0.f;
      y[k] = in ? load_target<kHalfT>(t.target[v], i0 + k) : 0.f;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = round_image(x[k], to_half);
}

template <bool kHalfT>
__global__ void __launch_bounds__(kT) k_photo_pw_fwd(const GsrPhotoViews t, const uint32_t n, const uint32_t units, const int vec,
                                                     Part* __restrict__ part) {
  __shared__ double ld[4];
  const int v = blockIdx.y;
  const bool to_half = t.round_image_to_half != 0;
  double s1 = 0.0, s2 = 0.0;
  for (uint32_t e = blockIdx.x * kT + threadIdx.x; e < units; e += gridDim.x * kT) {
    float x[4], y[4];
    pw_load<kHalfT>(t, v, e * 4u, n, vec != 0, to_half, x, y);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = x[k] - y[k];       // past the end both are 0
      s1 += (double)fabsf(d);
      s2 += (double)(d * d);
    }
  }
  s1 = block_sum(s1, ld);
  s2 = block_sum(s2, ld);
  if (threadIdx.x == 0) {
    Part q;
    q.m = 0.0; q.l1 = s1; q.l2 = s2; q.pad_ = 0.0;
    part[(size_t)v * gridDim.x + blockIdx.x] = q;
  }
}

template <bool kHalfT>
__global__ void __launch_bounds__(kT) k_photo_pw_bwd(const GsrPhotoViews t, const GsrPhotoWeights wt, const uint32_t n,
                                                     const uint32_t units, const int vec, const float* __restrict__ g,
                                                     const double inv_n) {
  const int v = blockIdx.y;
  const bool to_half = t.round_image_to_half != 0;
  const double scale = (double)g[v] * inv_n;
  const double w2 = 2.0 * (double)wt.l2, w1 = (double)wt.l1;
  float* __restrict__ O = t.dL_dimage[v];
  for (uint32_t e = blockIdx.x * kT + threadIdx.x; e < units; e += gridDim.x * kT) {
    float x[4], y[4], o[4];
    const uint32_t i0 = e * 4u;
    pw_load<kHalfT>(t, v, i0, n, vec != 0, to_half, x, y);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = x[k] - y[k];
      o[k] = (float)((w2 * (double)d + w1 * sign0(d)) * scale);
    }
    if (vec) {
      *reinterpret_cast<float4*>(O + i0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (i0 + k < n) O[i0 + k] = o[k];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ final
__global__ void __launch_bounds__(kT) k_photo_final(const Part* __restrict__ part, const int npart, const double n,
                                                    const GsrPhotoWeights wt, const int has_ssim, float* __restrict__ loss,
                                                    float* __restrict__ terms) {
  __shared__ double ld[4];
  const int v = blockIdx.x;
  double sm = 0.0, s1 = 0.0, s2 = 0.0;
  for (int k = threadIdx.x; k < npart; k += kT) {        // fixed order: the same sums on every run
    const Part q = part[(size_t)v * npart + k];
    sm += q.m; s1 += q.l1; s2 += q.l2;
  }
  sm = block_sum(sm, ld);
  s1 = block_sum(s1, ld);
  s2 = block_sum(s2, ld);
  if (threadIdx.x == 0) {
    const double l2 = s2 / n, l1 = s1 / n, ds = 1.0 - sm / n;
    double total = (double)wt.l2 * l2 + (double)wt.l1 * l1;
    if (has_ssim) total += (double)wt.dssim * ds;
    loss[v] = (float)total;
    if (terms) {
      terms[3 * v] = (float)l2;
      terms[3 * v + 1] = (float)l1;
      terms[3 * v + 2] = has_ssim ? (float)ds : __int_as_float(0x7fc00000);   // not evaluated in the point-wise form
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ host helpers
bool photo_shape_ok(int32_t V, int32_t C, int32_t H, int32_t W) {
  return V >= 1 && V <= GSR_MAX_PHOTO_VIEWS && C >= 1 && C <= GSR_MAX_PHOTO_CHANNELS && H >= 1 && W >= 1 &&
         (int64_t)C * H * W <= (int64_t)INT32_MAX;
}

struct PhotoShape {
  uint32_t n = 0, units = 0, pw_blocks = 0;   // entries per view, point-wise units and blocks per view
  int tiles_x = 0, tiles = 0;                 // SSIM form: tiles per channel plane
};

PhotoShape photo_shape(int32_t C, int32_t H, int32_t W) {
  PhotoShape s;
  s.n = (uint32_t)((int64_t)C * H * W);
  s.units = (s.n + 3u) / 4u;
  const uint32_t b = (s.units + kT - 1) / kT;
  s.pw_blocks = b < (uint32_t)kPwMaxBlocks ? b : (uint32_t)kPwMaxBlocks;
  s.tiles_x = (W + kTS - 1) / kTS;
  s.tiles = s.tiles_x * ((H + kTS - 1) / kTS);
  return s;
}

size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

Win photo_window() {
  Win w;
  double sum = 0.0;
  for (int i = 0; i < GSR_PHOTO_WINDOW; ++i) {
    w.w[i] = (float)exp(-(double)((i - kR) * (i - kR)) / 4.5);
    sum += (double)w.w[i];
  }
  const float s = (float)sum;          // the correctly rounded fp32 sum of the fp32 taps
  for (int i = 0; i < GSR_PHOTO_WINDOW; ++i) w.w[i] = w.w[i] / s;
  return w;
}

int photo_validate(const GsrPhotoViews* t, const GsrPhotoWeights* w, bool backward) {
  if (!t || !w || !photo_shape_ok(t->n_views, t->channels, t->height, t->width)) return GSR_EINVAL;
  if (!(w->l2 == w->l2) || !(w->l1 == w->l1) || !(w->dssim == w->dssim)) return GSR_EINVAL;
  if (w->l2 == 0.f && w->l1 == 0.f && w->dssim == 0.f) return GSR_EINVAL;
  const uintptr_t tmask = t->target_is_half ? 1u : 3u;
  for (int k = 0; k < t->n_views; ++k) {
    if (!t->image[k] || !t->target[k] || ((uintptr_t)t->image[k] & 3u) || ((uintptr_t)t->target[k] & tmask)) return GSR_EINVAL;
    if (backward && (!t->dL_dimage[k] || ((uintptr_t)t->dL_dimage[k] & 3u))) return GSR_EINVAL;
  }
  return GSR_OK;
}

int photo_vec(const GsrPhotoViews* t, uint32_t n, bool backward) {
  if (n % 4u) return 0;
  const uintptr_t tmask = t->target_is_half ? 7u : 15u;
  for (int k = 0; k < t->n_views; ++k) {
    if (((uintptr_t)t->image[k] & 15u) || ((uintptr_t)t->target[k] & tmask)) return 0;
    if (backward && ((uintptr_t)t->dL_dimage[k] & 15u)) return 0;
  }
  return 1;
}

}  // namespace

extern "C" void gsr_photo_window(float* taps) {
  if (!taps) return;
  const Win w = photo_window();
  for (int i = 0; i < GSR_PHOTO_WINDOW; ++i) taps[i] = w.w[i];
}

extern "C" size_t gsr_photo_scratch_bytes(int32_t n_views, int32_t channels, int32_t height, int32_t width) {
  if (!photo_shape_ok(n_views, channels, height, width)) return 0;
  const PhotoShape s = photo_shape(channels, height, width);
  const size_t ssim = (size_t)channels * s.tiles, per_view = ssim > s.pw_blocks ? ssim : s.pw_blocks;
  return round256((size_t)n_views * per_view * sizeof(Part));
}

extern "C" int gsr_photo_forward(const GsrPhotoViews* views, const GsrPhotoWeights* weights, float* loss, float* terms,
                                 float* saved, void* scratch, size_t scratch_bytes, void* stream_) {
  const int rc = photo_validate(views, weights, false);
  if (rc) return rc;
  if (!loss || !scratch || ((uintptr_t)scratch & 15u)) return GSR_EINVAL;
  const int32_t V = views->n_views, C = views->channels, H = views->height, W = views->width;
  if (scratch_bytes < gsr_photo_scratch_bytes(V, C, H, W)) return GSR_ESCRATCH;
  const PhotoShape s = photo_shape(C, H, W);
  hipStream_t stream = (hipStream_t)stream_;
  GsrDeviceGuard dev(views->image[0]);
  Part* part = reinterpret_cast<Part*>(scratch);
  const bool ssim = weights->dssim != 0.f;
  int npart;
  if (ssim) {
    const Win win = photo_window();
    const size_t plane = (size_t)V * s.n;
    const dim3 grid((uint32_t)s.tiles, (uint32_t)C, (uint32_t)V);
    if (views->target_is_half)
      hipLaunchKernelGGL(k_photo_ssim_fwd<true>, grid, dim3(kT), 0, stream, *views, win, s.tiles_x, saved, plane, part);
    else
      hipLaunchKernelGGL(k_photo_ssim_fwd<false>, grid, dim3(kT), 0, stream, *views, win, s.tiles_x, saved, plane, part);
    npart = C * s.tiles;
  } else {
    const int vec = photo_vec(views, s.n, false);
    const dim3 grid(s.pw_blocks, (uint32_t)V);
    if (views->target_is_half)
      hipLaunchKernelGGL(k_photo_pw_fwd<true>, grid, dim3(kT), 0, stream, *views, s.n, s.units, vec, part);
    else
      hipLaunchKernelGGL(k_photo_pw_fwd<false>, grid, dim3(kT), 0, stream, *views, s.n, s.units, vec, part);
    npart = (int)s.pw_blocks;
  }
  GSR_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_photo_final, dim3((uint32_t)V), dim3(kT), 0, stream, (const Part*)part, npart, (double)s.n, *weights,
                     ssim ? 1 : 0, loss, terms);
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

extern "C" int gsr_photo_backward(const GsrPhotoViews* views, const GsrPhotoWeights* weights, const float* saved,
                                  const float* dL_dloss, void* stream_) {
  const int rc = photo_validate(views, weights, true);
  if (rc) return rc;
  const bool ssim = weights->dssim != 0.f;
  if (!dL_dloss || (ssim && !saved)) return GSR_EINVAL;
  const int32_t V = views->n_views, C = views->channels, H = views->height, W = views->width;
  const PhotoShape s = photo_shape(C, H, W);
  const double inv_n = 1.0 / (double)s.n;
  hipStream_t stream = (hipStream_t)stream_;
  GsrDeviceGuard dev(views->image[0]);
  if (ssim) {
    const Win win = photo_window();
    const size_t plane = (size_t)V * s.n;
    const dim3 grid((uint32_t)s.tiles, (uint32_t)C, (uint32_t)V);
    if (views->target_is_half)
      hipLaunchKernelGGL(k_photo_ssim_bwd<true>, grid, dim3(kT), 0, stream, *views, *weights, win, s.tiles_x, saved, plane,
                         dL_dloss, inv_n);
    else
      hipLaunchKernelGGL(k_photo_ssim_bwd<false>, grid, dim3(kT), 0, stream, *views, *weights, win, s.tiles_x, saved, plane,
                         dL_dloss, inv_n);
  } else {
    const int vec = photo_vec(views, s.n, true);
    const dim3 grid(s.pw_blocks, (uint32_t)V);
    if (views->target_is_half)
      hipLaunchKernelGGL(k_photo_pw_bwd<true>, grid, dim3(kT), 0, stream, *views, *weights, s.n, s.units, vec, dL_dloss, inv_n);
    else
      hipLaunchKernelGGL(k_photo_pw_bwd<false>, grid, dim3(kT), 0, stream, *views, *weights, s.n, s.units, vec, dL_dloss, inv_n);
  }
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

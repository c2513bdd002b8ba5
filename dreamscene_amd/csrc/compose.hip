// compose.hip -- object placement (SceneGaussian.add_objects_to_scene, scene_gaussian.py:318-427) as two launches, gfx950.
//
// One placement moves a trained object into the scene frame: xyz' = R S x + T, scaling' = scaling + log(scale),
// rotation' = q_R (x) rotation, and the SH bands 1..3 of f_rest rotated on their COEFFICIENT axis (SEMANTICS.md "Object
// placement"). With `ground` the object is set down on z = center.z: T.z = center.z - min_z(R S x), which is why the pass
// over xyz comes first.
//   k_place_bounds      grid-stride over the rows: min / max of fl32(R S x) per block -> partial[block][6] (plain stores);
//   k_place_apply<K>    one block per 256 rows. Every block reduces the z-minimum of the partials (<= 1024 floats, L2) itself,
//                       block 0 reduces all six and stores the box of the final xyz' and T. The rows of xyz, scaling and f_rest
//                       travel global -> LDS -> global in 16-byte units (a row of 3, 9, 24 or 45 floats is not a multiple of
//                       16 bytes, 256 rows of them are); each lane works on its own row in LDS, at an odd word stride (24 is
//                       padded to 25): conflict-free. rotation rows are 16 bytes: straight float4.
// R S, T, log(scale), q_R and the 83 band-matrix entries are kernel arguments: scalar loads, no table in memory.
// Plain vector stores only; no atomics: two runs give the same bits. Built with -ffp-contract=off: one rounding per operator.
#include <math.h>

#include "gsr_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / GSR_WAVE;
constexpr int kBoundsMaxBlocks = 1024;

struct PlaceConst {                 // by value in the kernel arguments
  float rs[9], t[3], log_scale[3], q[4], m1[9], m2[25], m3[49];
};

// row r of fl32(R S x): the SAME expression in both kernels, so the minimum of launch 1 is the minimum of launch 2's rows
__device__ __forceinline__ float rs_row(const float* __restrict__ m, const int r, const float x0, const float x1, const float x2) {
  return (m[3 * r] * x0 + m[3 * r + 1] * x1) + m[3 * r + 2] * x2;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

struct Rs9 { float m[9]; };

__global__ void __launch_bounds__(kBlock)
k_place_bounds(const float* __restrict__ xyz, const int32_t P, const Rs9 rs, float* __restrict__ partial) {
  __shared__ float w[6][kWaves];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < P; i += (int64_t)gridDim.x * kBlock) {
    const float x0 = xyz[3 * i], x1 = xyz[3 * i + 1], x2 = xyz[3 * i + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float y = rs_row(rs.m, r, x0, x1, x2);
      lo[r] = fminf(lo[r], y);
      hi[r] = fmaxf(hi[r], y);
    }
  }
  const int wave = threadIdx.x / GSR_WAVE;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float a = wave_min(lo[r]), b = wave_max(hi[r]);
    if (gsr_lane() == 0) { w[r][wave] = a; w[3 + r][wave] = b; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = w[threadIdx.x][0];
    for (int k = 1; k < kWaves; ++k) v = threadIdx.x < 3 ? fminf(v, w[threadIdx.x][k]) : fmaxf(v, w[threadIdx.x][k]);
    partial[(size_t)blockIdx.x * 6 + threadIdx.x] = v;
  }
}

// component c (0..2 minima, 3..5 maxima) over the nb partials, the same value in every thread of the block
__device__ __forceinline__ float block_bound(const float* __restrict__ partial, const int nb, const int c, float* __restrict__ red) {
  const bool is_min = c < 3;
  float v = is_min ? INFINITY : -INFINITY;
  for (int b = threadIdx.x; b < nb; b += kBlock) {
    const float p = partial[(size_t)b * 6 + c];
    v = is_min ? fminf(v, p) : fmaxf(v, p);
  }
  v = is_min ? wave_min(v) : wave_max(v);
  __syncthreads();                                   // red may still be read from the previous call
  if (gsr_lane() == 0) red[threadIdx.x / GSR_WAVE] = v;
  __syncthreads();
  v = red[0];
  for (int k = 1; k < kWaves; ++k) v = is_min ? fminf(v, red[k]) : fmaxf(v, red[k]);
  return v;
}

// rows of W floats, `nfloats` of them valid from g (16-byte aligned) <-> LDS rows of WP words
template <int W, int WP>
__device__ __forceinline__ void stage_in(const float* __restrict__ g, float* __restrict__ lds, const int nfloats) {
  const int units = nfloats >> 2;
  for (int u = threadIdx.x; u < units; u += kBlock) {
    const float4 v = reinterpret_cast<const float4*>(g)[u];
    if constexpr (W == WP) {
      reinterpret_cast<float4*>(lds)[u] = v;
    } else {
      const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int idx = 4 * u + k;
        lds[(idx / W) * WP + idx % W] = e[k];
      }
    }
  }
  for (int idx = (units << 2) + threadIdx.x; idx < nfloats; idx += kBlock) lds[(idx / W) * WP + idx % W] = g[idx];
}
template <int W, int WP>
__device__ __forceinline__ void stage_out(float* __restrict__ g, const float* __restrict__ lds, const int nfloats) {
  const int units = nfloats >> 2;
  for (int u = threadIdx.x; u < units; u += kBlock) {
    float4 v;
    if constexpr (W == WP) {
      v = reinterpret_cast<const float4*>(lds)[u];
    } else {
      float e[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int idx = 4 * u + k;
        e[k] = lds[(idx / W) * WP + idx % W];
      }
      v = make_float4(e[0], e[1], e[2], e[3]);
    }
    reinterpret_cast<float4*>(g)[u] = v;
  }
  for (int idx = (units << 2) + threadIdx.x; idx < nfloats; idx += kBlock) g[idx] = lds[(idx / W) * WP + idx % W];
}

// band of N coefficients starting at coefficient `first` of one row (stride 3: the colour channels are interleaved),
// k'[j] = sum_i k[i] M[i][j], summed in index order
template <int N>
__device__ __forceinline__ void rotate_band(float* __restrict__ row, const int first, const float* __restrict__ M) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float in[N], out[N];
#pragma unroll
    for (int i = 0; i < N; ++i) in[i] = row[3 * (first + i) + c];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      float s = in[0] * M[j];
#pragma unroll
      for (int i = 1; i < N; ++i) s = s + in[i] * M[i * N + j];
      out[j] = s;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) row[3 * (first + j) + c] = out[j];
  }
}

struct PlaceIO {
  const float* xyz;
  const float* scaling;
  const float* rotation;
  const float* f_rest;
  float* xyz_out;
  float* scaling_out;
  float* rotation_out;
  float* f_rest_out;
  const float* partial;      // [nb][6] of k_place_bounds
  float* bounds;             // [6]
  float* t_effective;        // [3] or NULL
  int32_t P, nb, ground;
};

template <int K>
__global__ void __launch_bounds__(kBlock)
k_place_apply(const PlaceIO io, const PlaceConst a) {
  constexpr int W = 3 * (K - 1);
  constexpr int WP = (W > 0 && W % 2 == 0) ? W + 1 : W;
  __shared__ __attribute__((aligned(16))) float s_x[kBlock * 3];
  __shared__ __attribute__((aligned(16))) float s_s[kBlock * 3];
  __shared__ __attribute__((aligned(16))) float s_f[W > 0 ? kBlock * WP : 4];
  __shared__ float s_red[kWaves];

  const int row0 = blockIdx.x * kBlock;
  const int nrows = min(kBlock, io.P - row0);
  const int row = row0 + threadIdx.x;
  const bool valid = threadIdx.x < nrows;

  // every global load of the block is issued before the first wait
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (valid) q = reinterpret_cast<const float4*>(io.rotation)[row];
  stage_in<3, 3>(io.xyz + (size_t)row0 * 3, s_x, nrows * 3);
  stage_in<3, 3>(io.scaling + (size_t)row0 * 3, s_s, nrows * 3);
  if constexpr (W > 0) stage_in<W, WP>(io.f_rest + (size_t)row0 * W, s_f, nrows * W);

  float tz = a.t[2];
  if (io.ground) tz = a.t[2] - block_bound(io.partial, io.nb, 2, s_red);      // one fp32 subtraction, the same in every block
  if (blockIdx.x == 0) {
    const float t[3] = {a.t[0], a.t[1], tz};
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const float b = block_bound(io.partial, io.nb, c, s_red);
      // x -> fl32(x + t) is monotone: the box of the sums is the sum of the box
      if (threadIdx.x == 0) io.bounds[c] = b + t[c % 3];
    }
    if (io.t_effective && threadIdx.x < 3) io.t_effective[threadIdx.x] = t[threadIdx.x];
  }
  __syncthreads();

  if (valid) {
    float* x = s_x + 3 * threadIdx.x;
    const float x0 = x[0], x1 = x[1], x2 = x[2];
    x[0] = rs_row(a.rs, 0, x0, x1, x2) + a.t[0];
    x[1] = rs_row(a.rs, 1, x0, x1, x2) + a.t[1];
    x[2] = rs_row(a.rs, 2, x0, x1, x2) + tz;
    float* s = s_s + 3 * threadIdx.x;
    s[0] = s[0] + a.log_scale[0];
    s[1] = s[1] + a.log_scale[1];
    s[2] = s[2] + a.log_scale[2];
    // q_R (x) q, real part first (quaternion_raw_multiply): no normalisation
    const float aw = a.q[0], ax = a.q[1], ay = a.q[2], az = a.q[3];
    float4 o;
    o.x = ((aw * q.x - ax * q.y) - ay * q.z) - az * q.w;
    o.y = ((aw * q.y + ax * q.x) + ay * q.w) - az * q.z;
    o.z = ((aw * q.z - ax * q.w) + ay * q.x) + az * q.y;
    o.w = ((aw * q.w + ax * q.z) - ay * q.y) + az * q.x;
    reinterpret_cast<float4*>(io.rotation_out)[row] = o;
    if constexpr (W > 0) {
      float* f = s_f + WP * threadIdx.x;
      rotate_band<3>(f, 0, a.m1);
      if constexpr (K >= 9) rotate_band<5>(f, 3, a.m2);
      if constexpr (K >= 16) rotate_band<7>(f, 8, a.m3);
    }
  }
  __syncthreads();
  stage_out<3, 3>(io.xyz_out + (size_t)row0 * 3, s_x, nrows * 3);
  stage_out<3, 3>(io.scaling_out + (size_t)row0 * 3, s_s, nrows * 3);
  if constexpr (W > 0) stage_out<W, WP>(io.f_rest_out + (size_t)row0 * W, s_f, nrows * W);
}

inline int32_t bounds_blocks(int32_t P) {
  const int64_t nb = ((int64_t)P + kBlock - 1) / kBlock;
  return (int32_t)(nb < 1 ? 1 : nb > kBoundsMaxBlocks ? kBoundsMaxBlocks : nb);
}
inline bool rows_fit(int32_t P) { return (int64_t)P * 45 < 2147483648LL; }      // int offsets inside a block's row range

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || na == 0 || nb == 0) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

}  // namespace

extern "C" size_t gsr_place_scratch_bytes(int32_t P) {
  if (P < 0 || !rows_fit(P)) return 0;
  return (((size_t)bounds_blocks(P) * 6 * sizeof(float)) + 255) & ~(size_t)255;
}

extern "C" int gsr_place(const GsrPlacement* p, void* scratch, size_t scratch_bytes, void* stream_) {
  if (!p || !scratch) return GSR_EINVAL;
  const int32_t P = p->P, K = p->K;
  if (P < 0 || !rows_fit(P) || !(K == 1 || K == 4 || K == 9 || K == 16)) return GSR_EINVAL;
  if (((uintptr_t)scratch & 15u) || scratch_bytes < gsr_place_scratch_bytes(P)) return GSR_EINVAL;
  if (!p->bounds) return GSR_EINVAL;
  const size_t W = 3 * (size_t)(K - 1);
  // (input, output, floats per row, read by the kernels)
  const struct { const float* in; float* out; size_t w; bool used; } leaf[6] = {
      {p->xyz, p->xyz_out, 3, true},          {p->scaling, p->scaling_out, 3, true}, {p->rotation, p->rotation_out, 4, true},
      {p->opacity, nullptr, 1, false},        {p->features_dc, nullptr, 3, false},   {p->features_rest, p->features_rest_out, W, W > 0}};
  if (P > 0) {
    for (int i = 0; i < 6; ++i) {
      if (!leaf[i].used) continue;
      if (!leaf[i].in || !leaf[i].out) return GSR_EINVAL;
      if (((uintptr_t)leaf[i].in & 15u) || ((uintptr_t)leaf[i].out & 15u)) return GSR_EINVAL;
    }
    // an output may be its own input (in place); it may not touch any other leaf, output, the box or the scratch
    for (int o = 0; o < 6; ++o) {
      if (!leaf[o].used) continue;
      const size_t no = (size_t)P * leaf[o].w * sizeof(float);
      for (int i = 0; i < 6; ++i) {
        const size_t ni = (size_t)P * leaf[i].w * sizeof(float);
        if (overlap(leaf[o].out, no, leaf[i].in, ni) && !(i == o && leaf[o].out == leaf[i].in)) return GSR_EINVAL;
        if (i != o && leaf[i].used && overlap(leaf[o].out, no, leaf[i].out, ni)) return GSR_EINVAL;
      }
      if (overlap(leaf[o].out, no, p->bounds, 6 * sizeof(float)) || overlap(leaf[o].out, no, p->t_effective, 3 * sizeof(float)) ||
          overlap(leaf[o].out, no, scratch, scratch_bytes))
        return GSR_EINVAL;
    }
  }
  if (overlap(p->bounds, 6 * sizeof(float), p->t_effective, 3 * sizeof(float))) return GSR_EINVAL;
  if (P == 0) return GSR_OK;                         // nothing to place: the box of no points is left as it is

  hipStream_t stream = (hipStream_t)stream_;
  GsrDeviceGuard dev(scratch);
  const int32_t nb = bounds_blocks(P);
  Rs9 rs;
  PlaceConst a;
  for (int i = 0; i < 9; ++i) { rs.m[i] = p->rs[i]; a.rs[i] = p->rs[i]; a.m1[i] = p->m1[i]; }
  for (int i = 0; i < 3; ++i) { a.t[i] = p->t[i]; a.log_scale[i] = p->log_scale[i]; }
  for (int i = 0; i < 4; ++i) a.q[i] = p->q[i];
  for (int i = 0; i < 25; ++i) a.m2[i] = p->m2[i];
  for (int i = 0; i < 49; ++i) a.m3[i] = p->m3[i];
  float* partial = reinterpret_cast<float*>(scratch);
  hipLaunchKernelGGL(k_place_bounds, dim3((uint32_t)nb), dim3(kBlock), 0, stream, p->xyz, P, rs, partial);
  GSR_HIP(hipGetLastError());

  PlaceIO io;
  io.xyz = p->xyz; io.scaling = p->scaling; io.rotation = p->rotation; io.f_rest = p->features_rest;
  io.xyz_out = p->xyz_out; io.scaling_out = p->scaling_out; io.rotation_out = p->rotation_out; io.f_rest_out = p->features_rest_out;
  io.partial = partial; io.bounds = p->bounds; io.t_effective = p->t_effective;
  io.P = P; io.nb = nb; io.ground = p->ground ? 1 : 0;
  const dim3 grid((uint32_t)(((int64_t)P + kBlock - 1) / kBlock));
  switch (K) {
    case 1: hipLaunchKernelGGL(k_place_apply<1>, grid, dim3(kBlock), 0, stream, io, a); break;
    case 4: hipLaunchKernelGGL(k_place_apply<4>, grid, dim3(kBlock), 0, stream, io, a); break;
    case 9: hipLaunchKernelGGL(k_place_apply<9>, grid, dim3(kBlock), 0, stream, io, a); break;
    default: hipLaunchKernelGGL(k_place_apply<16>, grid, dim3(kBlock), 0, stream, io, a); break;
  }
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

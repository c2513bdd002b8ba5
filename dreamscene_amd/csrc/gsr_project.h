// gsr_project.h -- what K1 (preprocess.hip) and K8 (preprocess_bwd.hip) share: view constants, scene tables, activations,
// cov3D, the EWA chain, the SH basis, the input staging and the host helpers of both launchers.
#pragma once
#include "gsr_common.h"
#include "gsr_rng.h"
#include <type_traits>

namespace {

struct ViewConst {
  float V[16];
  float PV[16];
  float cam[3];
};

__device__ __forceinline__ void load_view(const GsrView& v, ViewConst& c) {
#pragma unroll
  for (int i = 0; i < 16; ++i) { c.V[i] = v.viewmatrix[i]; c.PV[i] = v.projmatrix[i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) c.cam[i] = v.campos[i];
}

// The constants of view vv inside a loop over the views of a batched launch: read through the CONSTANT address space, i.e.
// with scalar loads (s_load, counted by lgkmcnt). As ordinary global loads (the address is uniform but the compiler cannot
// prove that the kernel's own stores leave it alone) they are vector-memory operations, and on gfx9 those return IN ORDER
// with the vector-memory stores: the first load of view vv + 1 waited for the write acknowledgement of everything view vv
// had just stored -- one HBM write latency per view and wave in K1 and K8.
typedef const __attribute__((address_space(4))) float gsr_cfloat;
__device__ __forceinline__ gsr_cfloat* gsr_const(const float* p) { return (gsr_cfloat*)(uintptr_t)p; }
__device__ __forceinline__ void load_view_const(const float* viewmatrix, const float* projmatrix, const float* campos, ViewConst& c) {
  gsr_cfloat* V = gsr_const(viewmatrix);
  gsr_cfloat* PV = gsr_const(projmatrix);
  gsr_cfloat* cam = gsr_const(campos);
#pragma unroll
  for (int i = 0; i < 16; ++i) { c.V[i] = V[i]; c.PV[i] = PV[i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) c.cam[i] = cam[i];
}

constexpr float kSqrtPoint2 = 0.44721359549995793f;   // 0.2 ** 0.5 (scene_render's augmentations, below)

// ---- Where the N(0,1) samples of the scene path's augmentations come from (GsrScene): a tensor, the generator (gsr_rng.h), or
// nowhere. Passed by value in the kernel arguments; K8 gets what K1 got, so it regenerates exactly what K1 saw.
struct NoiseSrc {
  const float* scale;           // [P,3] samples or NULL
  const float* sh;              // [P,K,3] samples or NULL
  const uint32_t* stream_dev;   // NULL, or device u32[1]: the stream id, read when the kernel runs
  uint32_t seed_lo, seed_hi, stream, flags;   // flags: GSR_NOISE_* -- that noise comes from the generator
};
// GEN: the kernel is instantiated for the generator. The instantiations without it hold none of its code (K1 is
// register-sensitive: DESIGN.md), and flags are only honoured with it: the launchers pick GEN whenever a flag is set.
template <bool GEN>
__device__ __forceinline__ bool noise_has_scale(const NoiseSrc& z) {
  return z.scale != nullptr || (GEN && (z.flags & GSR_NOISE_SCALES));
}
template <bool GEN>
__device__ __forceinline__ bool noise_has_sh(const NoiseSrc& z) {
  return z.sh != nullptr || (GEN && (z.flags & GSR_NOISE_SHS));
}
template <bool GEN>
__device__ __forceinline__ uint32_t noise_stream(const NoiseSrc& z) {
  if constexpr (GEN) {
    if (z.stream_dev) return *(const __attribute__((address_space(4))) uint32_t*)(uintptr_t)z.stream_dev;   // (scalar load)
    return z.stream;
  }
  return 0u;
}
// the three scale normals of Gaussian i (zeros without scale noise)
template <bool GEN>
__device__ __forceinline__ void noise_scale3(const NoiseSrc& z, uint32_t stream, int64_t i, float n[3]) {
  if (GEN && (z.flags & GSR_NOISE_SCALES)) {
    float b[4];
    noise_block(z.seed_lo, z.seed_hi, stream, kNoiseTagScale, (uint32_t)i, 0u, b);
    n[0] = b[0]; n[1] = b[1]; n[2] = b[2];
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = z.scale ? z.scale[3 * i + k] : 0.f;
  }
}
// the SH normals 4j .. 4j+3 of Gaussian i's flattened [K,3] row of F floats (past the row: zeros); needs noise_has_sh
template <bool GEN>
__device__ __forceinline__ void noise_sh4(const NoiseSrc& z, uint32_t stream, int64_t i, int j, int F, float n[4]) {
  if (GEN && (z.flags & GSR_NOISE_SHS)) {
    noise_block(z.seed_lo, z.seed_hi, stream, kNoiseTagSh, (uint32_t)i, (uint32_t)j, n);
  } else {
    const float* row = z.sh + (size_t)i * F + 4 * j;
#pragma unroll
    for (int e = 0; e < 4; ++e) n[e] = (4 * j + e < F) ? row[e] : 0.f;
  }
}
// sh_e <- sh_e + n_e * (sqrt(0.2) * sh_e) over a row of F coefficients, the normals taken a block of four at a time: a register
// row (compile-time F, constant indices) ...
template <bool GEN, int F>
__device__ __forceinline__ void sh_noise_apply(const NoiseSrc& z, uint32_t stream, int64_t i, float* sh) {
#pragma unroll
  for (int j = 0; j < (F + 3) / 4; ++j) {
    float n[4];
    noise_sh4<GEN>(z, stream, i, j, F, n);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * j + e < F) sh[4 * j + e] = sh[4 * j + e] + n[e] * (kSqrtPoint2 * sh[4 * j + e]);
  }
}
// ... or the lane's LDS row (runtime F)
template <bool GEN>
__device__ __forceinline__ void sh_noise_apply_n(const NoiseSrc& z, uint32_t stream, int64_t i, int F, float* sh) {
#pragma unroll 1
  for (int j = 0; 4 * j < F; ++j) {
    float n[4];
    noise_sh4<GEN>(z, stream, i, j, F, n);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * j + e < F) sh[4 * j + e] = sh[4 * j + e] + n[e] * (kSqrtPoint2 * sh[4 * j + e]);
  }
}
// K8: dL/dsh_e <- dL/dsh_e * (1 + sqrt(0.2) n_e) over the first F_active entries of the lane's LDS row of F
template <bool GEN>
__device__ __forceinline__ void sh_noise_chain_n(const NoiseSrc& z, uint32_t stream, int64_t i, int F, int F_active, float* dsh) {
#pragma unroll 1
  for (int j = 0; 4 * j < F_active; ++j) {
    float n[4];
    noise_sh4<GEN>(z, stream, i, j, F, n);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * j + e < F_active) dsh[4 * j + e] = dsh[4 * j + e] * (1.0f + kSqrtPoint2 * n[e]);
  }
}
// The noise sources of the views of a batched launch, compact: K8's scene kernel takes SceneTab, SceneGradTab, K8Views and
// GsrGrads by value, and a NoiseSrc per view would carry its kernel arguments past 4 KB. The views of a batch therefore share the
// seed, and their device stream words, when given, are consecutive (view k reads stream_dev[k]); a batch that does not fit runs
// view by view (gsr_batch_noise_fits).
struct NoiseViews {
  const float* scale[GSR_MAX_BATCH_VIEWS];
  const float* sh[GSR_MAX_BATCH_VIEWS];
  const uint32_t* stream_dev;
  uint32_t seed_lo, seed_hi;
  uint32_t stream[GSR_MAX_BATCH_VIEWS];
  uint8_t flags[GSR_MAX_BATCH_VIEWS];
  __device__ __forceinline__ NoiseSrc view(int k) const {
    NoiseSrc z;
    z.scale = scale[k]; z.sh = sh[k]; z.stream_dev = (stream_dev && flags[k]) ? stream_dev + k : nullptr;
    z.seed_lo = seed_lo; z.seed_hi = seed_hi; z.stream = stream[k]; z.flags = flags[k];
    return z;
  }
};
static NoiseSrc noise_src(const GsrScene& sc) {
  NoiseSrc z;
  z.scale = sc.scale_noise; z.sh = sc.sh_noise; z.stream_dev = sc.noise_stream_dev;
  z.seed_lo = (uint32_t)sc.noise_seed; z.seed_hi = (uint32_t)(sc.noise_seed >> 32);
  z.stream = sc.noise_stream; z.flags = sc.noise_flags;
  return z;
}

// ---- multi-model ("scene") input: GsrScene flattened for the kernels (passed by value in the kernel arguments).
// A workgroup never straddles two models: model m owns the workgroups [fblk[m], fblk[m+1]) and its Gaussians keep
// their place first[m] + row in the concatenated index space every other kernel works in.
struct SceneTab {
  int32_t n;
  int32_t first[GSR_MAX_MODELS + 1];
  int32_t fblk[GSR_MAX_MODELS + 1];
  const float* xyz[GSR_MAX_MODELS];
  const float* scaling[GSR_MAX_MODELS];
  const float* rotation[GSR_MAX_MODELS];
  const float* opacity[GSR_MAX_MODELS];
  const float* dc[GSR_MAX_MODELS];
  const float* rest[GSR_MAX_MODELS];
  NoiseSrc noise;
  float* scales_out;
  float* rotations_out;
  float* opacities_out;
};
struct SceneGradTab {
  const float* dL_dscales_out;
  float* xyz[GSR_MAX_MODELS];
  float* scaling[GSR_MAX_MODELS];
  float* rotation[GSR_MAX_MODELS];
  float* opacity[GSR_MAX_MODELS];
  float* dc[GSR_MAX_MODELS];
  float* rest[GSR_MAX_MODELS];
};
struct NoScene {};

// Which rows this thread / wave works on. Without a scene: row == concatenated index.
struct Rows {
  int m;               // model (0 without a scene)
  int64_t i;           // concatenated Gaussian index
  int64_t row;         // row inside the model's tensors
  int64_t wave_row;    // row of the wave's first lane
  int64_t wave_i;      // concatenated index of the wave's first lane
  int n_valid;         // rows of this wave that exist
  bool ok;             // this lane's row exists
};
template <bool SCENE, typename TAB>
__device__ __forceinline__ Rows resolve_rows(const TAB& sc, int P) {
  const int tid = threadIdx.x, wave = tid >> 6;
  Rows r;
  if constexpr (SCENE) {
    int m = 0;
    for (int k = 1; k < sc.n; ++k) m += ((int)blockIdx.x >= sc.fblk[k]) ? 1 : 0;
    const int64_t cnt = (int64_t)sc.first[m + 1] - sc.first[m];
    const int64_t b0 = ((int64_t)blockIdx.x - sc.fblk[m]) * 256;
    r.m = m;
    r.row = b0 + tid;
    r.wave_row = b0 + wave * 64;
    r.i = sc.first[m] + r.row;
    r.wave_i = sc.first[m] + r.wave_row;
    r.n_valid = (int)min((int64_t)64, max((int64_t)0, cnt - r.wave_row));
    r.ok = r.row < cnt;
  } else {
    r.m = 0;
    r.i = r.row = (int64_t)blockIdx.x * 256 + tid;
    r.wave_i = r.wave_row = (int64_t)blockIdx.x * 256 + wave * 64;
    r.n_valid = (int)min((int64_t)64, max((int64_t)0, (int64_t)P - r.wave_row));
    r.ok = r.i < P;
  }
  return r;
}

// The activations of GaussianModel (gs_renderer.py:464-488) and scene_render's augmentations (scene_gaussian.py:844-852)
struct ActScale { float act, pre, out; };              // exp(raw); after the noise; after the clamp
__device__ __forceinline__ ActScale act_scale(float raw, bool noisy, float n) {
  ActScale a;
  a.act = expf(raw);
  a.pre = noisy ? a.act + n * ((kSqrtPoint2 * a.act) / 4.0f) : a.act;
  a.out = noisy ? fmaxf(a.pre, 0.0f) : a.act;
  return a;
}
__device__ __forceinline__ float act_quat_norm(const float4 q) {
  return fmaxf(sqrtf(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w), 1e-12f);
}
__device__ __forceinline__ float act_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ void quat_to_R(const float4 q, float R[9]) {
  const float r = q.x, x = q.y, y = q.z, z = q.w;
  R[0] = 1.0f - 2.0f * (y * y + z * z);
  R[1] = 2.0f * (x * y - r * z);
  R[2] = 2.0f * (x * z + r * y);
  R[3] = 2.0f * (x * y + r * z);
  R[4] = 1.0f - 2.0f * (x * x + z * z);
  R[5] = 2.0f * (y * z - r * x);
  R[6] = 2.0f * (x * z - r * y);
  R[7] = 2.0f * (y * z + r * x);
  R[8] = 1.0f - 2.0f * (x * x + y * y);
}

__device__ __forceinline__ void cov3d_from(const float s0, const float s1, const float s2, const float R[9],
                                           float c6[6]) {
  float L[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    L[3 * i + 0] = R[3 * i + 0] * s0;
    L[3 * i + 1] = R[3 * i + 1] * s1;
    L[3 * i + 2] = R[3 * i + 2] * s2;
  }
#define GSR_SIG(i, j) ((L[3 * i] * L[3 * j] + L[3 * i + 1] * L[3 * j + 1]) + L[3 * i + 2] * L[3 * j + 2])
  c6[0] = GSR_SIG(0, 0); c6[1] = GSR_SIG(0, 1); c6[2] = GSR_SIG(0, 2);
  c6[3] = GSR_SIG(1, 1); c6[4] = GSR_SIG(1, 2); c6[5] = GSR_SIG(2, 2);
#undef GSR_SIG
}

// The EWA chain shared by K1 and K8 (identical operator order => identical values in both).
struct Ewa {
  float tx, ty, tz, txc, tyc, J00, J02, J11, J12;
  float M0[3], M1[3], U0[3], U1[3];
  float ca, cb, cc, det;
  bool clx, cly;
};

__device__ __forceinline__ void ewa_forward(const ViewConst& vc, float px, float py, float pz, const float c6[6],
                                            float fx, float fy, float limx, float limy, Ewa& e) {
  const float* V = vc.V;
  e.tx = ((V[0] * px + V[4] * py) + V[8] * pz) + V[12];
  e.ty = ((V[1] * px + V[5] * py) + V[9] * pz) + V[13];
  e.tz = ((V[2] * px + V[6] * py) + V[10] * pz) + V[14];
  const float S[9] = {c6[0], c6[1], c6[2], c6[1], c6[3], c6[4], c6[2], c6[4], c6[5]};
  const float txz = e.tx / e.tz, tyz = e.ty / e.tz;
  e.clx = (txz < -limx) || (txz > limx);
  e.cly = (tyz < -limy) || (tyz > limy);
  e.txc = fminf(limx, fmaxf(-limx, txz)) * e.tz;
  e.tyc = fminf(limy, fmaxf(-limy, tyz)) * e.tz;
  e.J00 = fx / e.tz;
  e.J02 = -(fx * e.txc) / (e.tz * e.tz);
  e.J11 = fy / e.tz;
  e.J12 = -(fy * e.tyc) / (e.tz * e.tz);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    e.M0[r] = e.J00 * V[4 * r + 0] + e.J02 * V[4 * r + 2];
    e.M1[r] = e.J11 * V[4 * r + 1] + e.J12 * V[4 * r + 2];
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    e.U0[j] = (e.M0[0] * S[j] + e.M0[1] * S[3 + j]) + e.M0[2] * S[6 + j];
    e.U1[j] = (e.M1[0] * S[j] + e.M1[1] * S[3 + j]) + e.M1[2] * S[6 + j];
  }
  e.ca = ((e.U0[0] * e.M0[0] + e.U0[1] * e.M0[1]) + e.U0[2] * e.M0[2]) + GSR_LOWPASS;
  e.cb = (e.U0[0] * e.M1[0] + e.U0[1] * e.M1[1]) + e.U0[2] * e.M1[2];
  e.cc = ((e.U1[0] * e.M1[0] + e.U1[1] * e.M1[1]) + e.U1[2] * e.M1[2]) + GSR_LOWPASS;
  e.det = e.ca * e.cc - e.cb * e.cb;
}

__device__ __forceinline__ void sh_basis(int D, float x, float y, float z, float b[16]) {
  b[0] = GSR_SH_C0;
  if (D > 0) {
    b[1] = -GSR_SH_C1 * y; b[2] = GSR_SH_C1 * z; b[3] = -GSR_SH_C1 * x;
    if (D > 1) {
      const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
      b[4] = GSR_SH_C2_0 * xy; b[5] = GSR_SH_C2_1 * yz; b[6] = GSR_SH_C2_2 * (2.0f * zz - xx - yy);
      b[7] = GSR_SH_C2_3 * xz; b[8] = GSR_SH_C2_4 * (xx - yy);
      if (D > 2) {
        b[9] = GSR_SH_C3_0 * y * (3.0f * xx - yy);
        b[10] = GSR_SH_C3_1 * xy * z;
        b[11] = GSR_SH_C3_2 * y * (4.0f * zz - xx - yy);
        b[12] = GSR_SH_C3_3 * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
        b[13] = GSR_SH_C3_4 * x * (4.0f * zz - xx - yy);
        b[14] = GSR_SH_C3_5 * z * (xx - yy);
        b[15] = GSR_SH_C3_6 * x * (xx - 3.0f * yy);
      }
    }
  }
}

// colour_c = sum_k b_k sh[k][c] accumulated in ascending k (the oracle's order), written so that every index into the
// register array b[] is a compile-time constant (a runtime-indexed register array costs s_set_gpr_idx round trips).
#define GSR_SH_BAND(K0, K1)                                   \
  _Pragma("unroll") for (int k = K0; k <= K1; ++k) {          \
    acc[0] = acc[0] + b[k] * sh[3 * k];                       \
    acc[1] = acc[1] + b[k] * sh[3 * k + 1];                   \
    acc[2] = acc[2] + b[k] * sh[3 * k + 2];                   \
  }
__device__ __forceinline__ void sh_colour(int D, const float* sh, const float b[16], float acc[3]) {
  acc[0] = b[0] * sh[0]; acc[1] = b[0] * sh[1]; acc[2] = b[0] * sh[2];
  if (D > 0) {
    GSR_SH_BAND(1, 3)
    if (D > 1) {
      GSR_SH_BAND(4, 8)
      if (D > 2) { GSR_SH_BAND(9, 15) }
    }
  }
}
// same, for a register row of exactly KN coefficients (bands beyond KN cannot be active: D is validated against K)
template <int KN>
__device__ __forceinline__ void sh_colour_n(int D, const float* sh, const float b[16], float acc[3]) {
  acc[0] = b[0] * sh[0]; acc[1] = b[0] * sh[1]; acc[2] = b[0] * sh[2];
  if constexpr (KN >= 4) {
    if (D > 0) {
      GSR_SH_BAND(1, 3)
      if constexpr (KN >= 9) {
        if (D > 1) {
          GSR_SH_BAND(4, 8)
          if constexpr (KN >= 16) {
            if (D > 2) { GSR_SH_BAND(9, 15) }
          }
        }
      }
    }
  }
}
#undef GSR_SH_BAND

// Unit view direction camera -> p (the argument of the SH basis) and the length it was divided by.
struct ViewDir { float x, y, z, len; };
__device__ __forceinline__ ViewDir view_dir(const ViewConst& vc, float px, float py, float pz) {
  const float dx = px - vc.cam[0], dy = py - vc.cam[1], dz = pz - vc.cam[2];
  ViewDir d;
  d.len = sqrtf((dx * dx + dy * dy) + dz * dz);
  d.x = dx / d.len; d.y = dy / d.len; d.z = dz / d.len;
  return d;
}

// Row stride (in floats) of one Gaussian's SH block inside the LDS transpose buffer: odd => the 64 lanes of a
// wave reading "their" row element k hit 64 different banks pairs (ds_read_b32, 32-lane groups).
__host__ __device__ __forceinline__ int sh_lds_stride(int K) { return (3 * K) | 1; }

// Coalesced global -> LDS load of the wave's SH block. `vis` = ballot of lanes whose Gaussian needs its row.
template <int KT>
__device__ __forceinline__ void stage_sh_in(const float* __restrict__ shs, int64_t wave_first, int n_valid, int K,
                                            unsigned long long vis, float* lds_wave) {
  const int F = KT > 0 ? 3 * KT : 3 * K;          // compile-time for the common strides: / and % become mul-shift
  const int stride = F | 1;
  const int total = n_valid * F;                                   // floats in the wave's block
  const float* src = shs + wave_first * (int64_t)F;
  const int lane = gsr_lane();
  for (int q = lane * 4; q < total; q += 64 * 4) {
    const int g0 = q / F, g1 = (q + 3) / F;
    const bool need = ((vis >> g0) & 1ull) || ((g1 < 64) && ((vis >> g1) & 1ull));
    if (!need) continue;
    float4 v;
    if (q + 3 < total) {
      v = *reinterpret_cast<const float4*>(src + q);
    } else {
      v.x = src[q];
      v.y = (q + 1 < total) ? src[q + 1] : 0.f;
      v.z = (q + 2 < total) ? src[q + 2] : 0.f;
      v.w = 0.f;
    }
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int f = q + k;
      if (f < total) {
        const int g = f / F, o = f - g * F;
        lds_wave[g * stride + o] = e[k];
      }
    }
  }
}

// Scene input: rows of F floats (features_dc: 3, features_rest: 3K-3) land at float offset o0 of the lanes' LDS rows.
__device__ __forceinline__ void stage_rows_in(const float* __restrict__ src, int F, int o0, int lds_stride, int n_valid,
                                              unsigned long long vis, float* lds_wave) {
  const int total = n_valid * F;
  const int lane = gsr_lane();
  for (int f = lane; f < total; f += 64) {
    const int g = f / F, o = f - g * F;
    if ((vis >> g) & 1ull) lds_wave[g * lds_stride + o0 + o] = src[f];
  }
}
// 16-byte vector with dword alignment: rows of 3K-3 floats start on 4-byte boundaries; gfx950 global loads / stores of
// dwordx4 only need dword alignment
typedef float gsr_f4u __attribute__((ext_vector_type(4), aligned(4)));

// One lane's row of F floats straight from global memory (dst may be registers or the lane's LDS row).
template <int F>
__device__ __forceinline__ void load_row(const float* __restrict__ src, float* dst) {
#pragma unroll
  for (int q = 0; q + 3 < F; q += 4) {
    const gsr_f4u t = *reinterpret_cast<const gsr_f4u*>(src + q);
    dst[q] = t.x; dst[q + 1] = t.y; dst[q + 2] = t.z; dst[q + 3] = t.w;
  }
#pragma unroll
  for (int q = F & ~3; q < F; ++q) dst[q] = src[q];
}

// tanfov and the active SH degree travel by value in GsrView -- unless GsrView.dynamic names a device f32[4]
// (tanfovx, tanfovy, sh_degree, reserved): then the kernels take them from there WHEN THEY RUN, which is what lets a
// captured graph (hipGraph) of a step be replayed with the next step's cameras (dreamscene_amd/graph.py).
struct ViewDyn {
  float tanfovx, tanfovy;
  int sh_degree;
};
__device__ __forceinline__ ViewDyn view_dyn(const float* __restrict__ dyn, float tfx, float tfy, int D) {
  ViewDyn d;
  d.tanfovx = tfx; d.tanfovy = tfy; d.sh_degree = D;
  if (dyn) {
    gsr_cfloat* c = gsr_const(dyn);     // (scalar loads: see load_view_const)
    d.tanfovx = c[0]; d.tanfovy = c[1]; d.sh_degree = (int)c[2];
  }
  return d;
}

}  // namespace

static inline size_t gsr_preprocess_lds_bytes(int K) { return (size_t)4 * 64 * sh_lds_stride(K) * sizeof(float); }

// GsrScene (host) -> the by-value kernel tables
static uint32_t scene_tables(const GsrScene& sc, const GsrSceneGrads* sgr, SceneTab& t, SceneGradTab& gt) {
  t = SceneTab{};
  gt = SceneGradTab{};
  t.n = sc.n_models;
  gt.dL_dscales_out = sgr ? sgr->dL_dscales_out : nullptr;
  int32_t first = 0, blk = 0;
  for (int m = 0; m < sc.n_models; ++m) {
    const GsrModel& md = sc.models[m];
    t.first[m] = first; t.fblk[m] = blk;
    first += md.count; blk += (md.count + 255) / 256;
    t.xyz[m] = md.xyz; t.scaling[m] = md.scaling; t.rotation[m] = md.rotation; t.opacity[m] = md.opacity;
    t.dc[m] = md.features_dc; t.rest[m] = md.features_rest;
    if (sgr) {
      const GsrModelGrads& mg = sgr->models[m];
      gt.xyz[m] = mg.xyz; gt.scaling[m] = mg.scaling; gt.rotation[m] = mg.rotation; gt.opacity[m] = mg.opacity;
      gt.dc[m] = mg.features_dc; gt.rest[m] = mg.features_rest;
    }
  }
  for (int m = sc.n_models; m <= GSR_MAX_MODELS; ++m) { t.first[m] = first; t.fblk[m] = blk; }
  t.noise = noise_src(sc);
  t.scales_out = sc.scales_out; t.rotations_out = sc.rotations_out; t.opacities_out = sc.opacities_out;
  return (uint32_t)blk;
}

// The per-view fields K1Views and K8Views share (same names, own layouts: both are kernel arguments) of a batched launch.
template <class VB>
static void fill_view_fields(VB& vb, int n_views, const GsrView* views, const GsrGaussians* gs) {
  for (int k = 0; k < n_views; ++k) {
    if (gs[0].scene) {
      const GsrScene& sc = *gs[k].scene;
      vb.noise.scale[k] = sc.scale_noise; vb.noise.sh[k] = sc.sh_noise;
      vb.noise.stream[k] = sc.noise_stream; vb.noise.flags[k] = (uint8_t)sc.noise_flags;
      if (sc.noise_flags) {     // (the same for every view that has flags: gsr_batch_noise_fits)
        vb.noise.seed_lo = (uint32_t)sc.noise_seed; vb.noise.seed_hi = (uint32_t)(sc.noise_seed >> 32);
        vb.noise.stream_dev = sc.noise_stream_dev ? sc.noise_stream_dev - k : nullptr;
      }
    }
    vb.scales[k] = gs[k].scales;
    if (gs[k].scales != gs[0].scales) vb.per_view_scales = 1;
    vb.viewmatrix[k] = views[k].viewmatrix; vb.projmatrix[k] = views[k].projmatrix; vb.campos[k] = views[k].campos;
    vb.tanfovx[k] = views[k].tanfovx; vb.tanfovy[k] = views[k].tanfovy; vb.sh_degree[k] = views[k].sh_degree;
    vb.dyn[k] = views[k].dynamic;
  }
}

// One launch for the runtime SH stride K: f(std::integral_constant<int, KT>) for the KT of KTs that equals K, then the
// launch check. Only the listed KTs are instantiated; any other K is GSR_EINVAL.
template <int... KTs, class F>
static int launch_sh(int K, F&& f) {
  if (!((K == KTs && (f(std::integral_constant<int, KTs>{}), true)) || ...)) return GSR_EINVAL;
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}
// the single-view kernels: compile-time strides read their rows directly (no LDS); every other stride runs the generic
// KT = 0 kernel, which stages the rows through LDS
static int fixed_sh(int K) { return K == 16 || K == 9 || K == 4 || K == 1 ? K : 0; }
// does any of the views' scenes draw noise from the generator? (then the launchers take the GEN instantiations)
static bool scene_noise_generated(int n_views, const GsrGaussians* gs) {
  bool gen = false;
  for (int k = 0; k < n_views; ++k) gen = gen || (gs[k].scene && gs[k].scene->noise_flags != 0u);
  return gen;
}
// a runtime flag -> std::true_type / std::false_type
template <class F>
static void with_flag(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

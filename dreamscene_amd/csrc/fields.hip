// fields.hip -- GaussianModel.extract_fields of the reference (gs_renderer.py:490-573 with gaussian_3d_coeff, :95-121): the
// opacity-weighted density of a model on a resolution^3 grid (include/gsrast.h, "occupancy field"; dreamscene_amd/fields.py;
// SEMANTICS.md section 18).
//   gsr_fields_bounds   clear, k_field_bounds, finish: the per-axis min and max of the rows whose opacity passes 0.005 and their
//                       count, into the head of the scratch. Integer atomics on the order-preserving key of the float (gsr_common.h;
//                       select.hip shares it), so the result is exact and has the same bits on every run.
//   gsr_extract_fields  k_field_prepare, k_field_eval. Prepare writes one 12-float record a row (normalised centre, the six
//                       inverse-covariance coefficients, opacity) and one membership word (the inclusive chunk range of the row
//                       on each axis, 8 bits a bound). Eval gives every chunk triple its own workgroups; each walks ALL rows'
//                       membership words in tiles of 256, compacts the members' records into an LDS ring in index order (ballot
//                       and prefix within the wave, the waves in order) and, whenever 256 of them wait, adds their partial sum to
//                       each of its voxels. No pair list, no capacity, no atomics: every voxel is written once, by one thread,
//                       in an order that depends on nothing but the inputs.
// One rounding per operator (built with -ffp-contract=off); expf, sqrtf and `/` are the full-precision forms.
#include "gsr_common.h"

namespace {

constexpr int kT = 256;                          // threads per block (4 waves)
constexpr int kWaves = kT / GSR_WAVE;
constexpr int kMaxBlocks = 1024;                 // k_field_bounds' grid cap; a block strides over the rows past it
constexpr int kHeadWords = 8;                    // scratch head: mn[3], mx[3] (keys, then fp32), count, one spare word
constexpr int kRecVec = 3;                       // a record: three float4 (10 floats used)
constexpr int kBatch = 256;                      // members a partial sum covers
constexpr int kRing = 2 * kBatch;                // LDS ring, in records: fewer than kBatch wait when a tile adds up to kT
constexpr int kMaxChunks = 255;                  // a chunk index is 8 bits of the membership word
constexpr int kMaxResolution = 1024;             // resolution^3 voxels stay below 2^31
constexpr uint32_t kNoChunks = 0x00010001u;      // (first 1, last 0) twice: an empty range on two axes
constexpr float kMinOpacity = 0.005f;
static_assert(kT <= kBatch && (kRing & (kRing - 1)) == 0, "the ring holds a waiting remainder and one tile");

__device__ __forceinline__ float opacity_of(float raw) { return 1.0f / (1.0f + expf(-raw)); }

__global__ void __launch_bounds__(64) k_field_clear(uint32_t* __restrict__ head) {
  if (threadIdx.x < kHeadWords) head[threadIdx.x] = threadIdx.x < 3 ? 0xFFFFFFFFu : 0u;
}

__global__ void __launch_bounds__(kT) k_field_bounds(const float* __restrict__ xyz, const float* __restrict__ opacity_raw,
                                                     const uint32_t P, uint32_t* __restrict__ head) {
  __shared__ uint32_t s_part[kWaves][kHeadWords];
  const int tid = threadIdx.x, lane = tid & (GSR_WAVE - 1), w = tid / GSR_WAVE;
  uint32_t v[7] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u, 0u};
  for (uint32_t i = blockIdx.x * kT + tid; i < P; i += gridDim.x * kT) {
    if (!(opacity_of(opacity_raw[i]) > kMinOpacity)) continue;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const uint32_t k = gsr_float_key(xyz[3 * (size_t)i + a]);
      v[a] = k < v[a] ? k : v[a];
      v[3 + a] = k > v[3 + a] ? k : v[3 + a];
    }
    v[6] += 1u;
  }
#pragma unroll
  for (int o = GSR_WAVE / 2; o > 0; o >>= 1) {
#pragma unroll
    for (int a = 0; a < 7; ++a) {
      const uint32_t t = (uint32_t)__shfl_xor((int)v[a], o, GSR_WAVE);
      v[a] = a < 3 ? (t < v[a] ? t : v[a]) : a < 6 ? (t > v[a] ? t : v[a]) : v[a] + t;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 7; ++a) s_part[w][a] = v[a];
  }
  __syncthreads();
  if (tid < 7) {
    uint32_t r = s_part[0][tid];
    for (int j = 1; j < kWaves; ++j) {
      const uint32_t t = s_part[j][tid];
      r = tid < 3 ? (t < r ? t : r) : tid < 6 ? (t > r ? t : r) : r + t;
    }
    if (tid < 3) atomicMin(&head[tid], r);
    else if (tid < 6) atomicMax(&head[tid], r);
    else if (r) atomicAdd(&head[6], r);
  }
}

__global__ void __launch_bounds__(64) k_field_bounds_finish(uint32_t* __restrict__ head) {
  if (threadIdx.x < 6) head[threadIdx.x] = __float_as_uint(gsr_key_float(head[threadIdx.x]));
}

struct PrepareArgs {
  const float* xyz;
  const float* opacity_raw;
  const float* scaling_raw;
  const float* rotation_raw;
  const float* gate_lo;      // [n_chunks]
  const float* gate_hi;      // [n_chunks]
  float4* rec;               // [P][kRecVec]
  uint2* memb;               // [P]
  uint32_t P;
  int n_chunks;
  float cx, cy, cz, scale;
};

// the inclusive range of chunks c with lo[c] < x < hi[c] as first | last << 8; both tables ascend, so the chunks are contiguous
__device__ __forceinline__ uint32_t chunk_range(const float x, const float* __restrict__ lo, const float* __restrict__ hi,
                                                const int n_chunks, bool& any) {
  uint32_t first = 1u, last = 0u;
  bool found = false;
  for (int c = 0; c < n_chunks; ++c) {
    if (lo[c] < x && x < hi[c]) {
      if (!found) first = (uint32_t)c;
      last = (uint32_t)c;
      found = true;
    }
  }
  any = any && found;
  return first | (last << 8);
}

__global__ void __launch_bounds__(kT) k_field_prepare(const PrepareArgs a) {
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i >= a.P) return;
  const size_t i3 = 3 * (size_t)i, i4 = 4 * (size_t)i;
  const float opacity = opacity_of(a.opacity_raw[i]);
  const float x = (a.xyz[i3] - a.cx) * a.scale, y = (a.xyz[i3 + 1] - a.cy) * a.scale, z = (a.xyz[i3 + 2] - a.cz) * a.scale;
  const float s0 = expf(a.scaling_raw[i3]) * a.scale, s1 = expf(a.scaling_raw[i3 + 1]) * a.scale,
              s2 = expf(a.scaling_raw[i3 + 2]) * a.scale;
  // build_rotation (gs_renderer.py:124-145)
  const float r0 = a.rotation_raw[i4], r1 = a.rotation_raw[i4 + 1], r2 = a.rotation_raw[i4 + 2], r3 = a.rotation_raw[i4 + 3];
  const float norm = sqrtf(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
  const float qr = r0 / norm, qx = r1 / norm, qy = r2 / norm, qz = r3 / norm;
  // L = R diag(s)
  const float l00 = (1.f - 2.f * (qy * qy + qz * qz)) * s0, l01 = (2.f * (qx * qy - qr * qz)) * s1,
              l02 = (2.f * (qx * qz + qr * qy)) * s2;
  const float l10 = (2.f * (qx * qy + qr * qz)) * s0, l11 = (1.f - 2.f * (qx * qx + qz * qz)) * s1,
              l12 = (2.f * (qy * qz - qr * qx)) * s2;
  const float l20 = (2.f * (qx * qz - qr * qy)) * s0, l21 = (2.f * (qy * qz + qr * qx)) * s1,
              l22 = (1.f - 2.f * (qx * qx + qy * qy)) * s2;
  // the upper triangle of L L^T
  const float ca = l00 * l00 + l01 * l01 + l02 * l02, cb = l00 * l10 + l01 * l11 + l02 * l12,
              cc = l00 * l20 + l01 * l21 + l02 * l22, cd = l10 * l10 + l11 * l11 + l12 * l12,
              ce = l10 * l20 + l11 * l21 + l12 * l22, cf = l20 * l20 + l21 * l21 + l22 * l22;
  // gaussian_3d_coeff (gs_renderer.py:109-115), operator by operator
  const float inv_det = 1.f / (ca * cd * cf + 2.f * ce * cc * cb - ce * ce * ca - cc * cc * cd - cb * cb * cf + 1e-24f);
  const float inv_a = (cd * cf - ce * ce) * inv_det, inv_b = (ce * cc - cb * cf) * inv_det, inv_c = (ce * cb - cc * cd) * inv_det,
              inv_d = (ca * cf - cc * cc) * inv_det, inv_e = (cb * cc - ce * ca) * inv_det, inv_f = (ca * cd - cb * cb) * inv_det;
  float4* rec = a.rec + (size_t)kRecVec * i;
  rec[0] = make_float4(x, y, z, inv_a);
  rec[1] = make_float4(inv_b, inv_c, inv_d, inv_e);
  rec[2] = make_float4(inv_f, opacity, 0.f, 0.f);
  bool member = opacity > kMinOpacity;
  const uint32_t mx = chunk_range(x, a.gate_lo, a.gate_hi, a.n_chunks, member);
  const uint32_t my = chunk_range(y, a.gate_lo, a.gate_hi, a.n_chunks, member);
  const uint32_t mz = chunk_range(z, a.gate_lo, a.gate_hi, a.n_chunks, member);
  // a filtered row and a row outside every chunk on some axis stay in place with an empty range: index order is kept
  a.memb[i] = member ? make_uint2(mx | (my << 16), mz) : make_uint2(kNoChunks, kNoChunks & 0xFFFFu);
}

struct EvalArgs {
  const float4* rec;
  const uint2* memb;
  const float* coords;       // [resolution]
  float* occ;                // [resolution]^3
  uint32_t P;
  int resolution, split_size, n_chunks, parts;
};

// The partial sum of ring entries [start, start + n) at the thread's VPT voxels. The entry is the same for every lane: the three
// 16-byte LDS reads are broadcasts.
template <int VPT>
__device__ __forceinline__ void eval_batch(const float4* __restrict__ s_rec, const uint32_t start, const uint32_t n,
                                           const float (&px)[VPT], const float (&py)[VPT], const float (&pz)[VPT],
                                           float (&total)[VPT]) {
  float part[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) part[j] = 0.f;
  for (uint32_t m = 0; m < n; ++m) {
    const float4* r = s_rec + kRecVec * ((start + m) & (uint32_t)(kRing - 1));
    const float4 A = r[0], B = r[1], C = r[2];
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const float x = px[j] - A.x, y = py[j] - A.y, z = pz[j] - A.z;
      // gs_renderer.py:117
      const float power = -0.5f * (x * x * A.w + y * y * B.z + z * z * C.x) - x * y * B.x - x * z * B.y - y * z * B.w;
      const float wgt = power > 0.f ? 0.f : expf(power);
      part[j] += C.y * wgt;
    }
  }
#pragma unroll
  for (int j = 0; j < VPT; ++j) total[j] += part[j];
}

template <int VPT>
__global__ void __launch_bounds__(kT) k_field_eval(const EvalArgs a) {
  __shared__ float4 s_rec[kRing * kRecVec];
  __shared__ uint32_t s_cnt[2][kWaves];
  const int tid = threadIdx.x, lane = tid & (GSR_WAVE - 1), w = tid / GSR_WAVE;
  const int n = a.n_chunks, R = a.resolution, split = a.split_size;
  const int triple = (int)(blockIdx.x / (uint32_t)a.parts), part = (int)(blockIdx.x % (uint32_t)a.parts);
  const int cz = triple % n, cy = (triple / n) % n, cx = triple / (n * n);
  if (cx >= n) return;                           // the whole block: the grid is n^3 * parts
  const int x0 = cx * split, y0 = cy * split, z0 = cz * split;
  const int nx = min(split, R - x0), ny = min(split, R - y0), nz = min(split, R - z0);
  const int nvox = nx * ny * nz;                 // > 0: n = ceil(R / split)
  float px[VPT], py[VPT], pz[VPT], total[VPT];
  int at[VPT];                                   // the voxel's index in occ, -1: none
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int v = (part * VPT + j) * kT + tid;
    const int ix = v / (ny * nz), rem = v - ix * (ny * nz), iy = rem / nz, iz = rem - iy * nz;
    const int gx = x0 + ix, gy = y0 + iy, gz = z0 + iz;
    const bool ok = v < nvox && gx < R && gy < R && gz < R;
    at[j] = ok ? (gx * R + gy) * R + gz : -1;
    px[j] = ok ? a.coords[gx] : 0.f;
    py[j] = ok ? a.coords[gy] : 0.f;
    pz[j] = ok ? a.coords[gz] : 0.f;
    total[j] = 0.f;
  }
  uint32_t wr = 0u, rd = 0u;                     // ring entries written and consumed so far: the same in every thread
  int parity = 0;
  for (uint32_t base = 0u; base < a.P; base += kT, parity ^= 1) {
    const uint32_t row = base + tid;
    bool member = false;
    if (row < a.P) {
      const uint2 m = a.memb[row];
      member = (uint32_t)cx >= (m.x & 255u) && (uint32_t)cx <= ((m.x >> 8) & 255u) && (uint32_t)cy >= ((m.x >> 16) & 255u) &&
               (uint32_t)cy <= (m.x >> 24) && (uint32_t)cz >= (m.y & 255u) && (uint32_t)cz <= ((m.y >> 8) & 255u);
    }
    const uint64_t ballot = __ballot(member);
    if (lane == 0) s_cnt[parity][w] = (uint32_t)__popcll(ballot);
    __syncthreads();                             // the only barrier of a tile that ends no batch (s_cnt alternates)
    uint32_t before = 0u, all = 0u;
#pragma unroll
    for (int j = 0; j < kWaves; ++j) {
      const uint32_t c = s_cnt[parity][j];
      before += j < w ? c : 0u;
      all += c;
    }
    before = (uint32_t)__builtin_amdgcn_readfirstlane((int)before);      // wave-uniform: the ring positions stay scalar
    all = (uint32_t)__builtin_amdgcn_readfirstlane((int)all);
    if (member) {
      const uint32_t pos = (wr + before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull))) & (uint32_t)(kRing - 1);
      const float4* src = a.rec + (size_t)kRecVec * row;
      s_rec[kRecVec * pos] = src[0];
      s_rec[kRecVec * pos + 1] = src[1];
      s_rec[kRecVec * pos + 2] = src[2];
    }
    wr += all;
    if (wr - rd >= (uint32_t)kBatch) {           // at most kBatch - 1 waited and at most kT came: one batch, never two
      __syncthreads();
      eval_batch<VPT>(s_rec, rd, (uint32_t)kBatch, px, py, pz, total);
      rd += (uint32_t)kBatch;                    // its slots are written again only behind the next tile's barrier
    }
  }
  __syncthreads();
  if (wr != rd) eval_batch<VPT>(s_rec, rd, wr - rd, px, py, pz, total);
#pragma unroll
  for (int j = 0; j < VPT; ++j)
    if (at[j] >= 0) a.occ[at[j]] = total[j];
}

bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// [a, a + na) and [b, b + nb) bytes share an address
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && x < y + nb && y < x + na;
}

bool finite(float f) { return f - f == 0.f; }

size_t memb_at() { return (size_t)kHeadWords * 4u; }
size_t rec_at(int32_t P) { return memb_at() + ((size_t)P * 8u + 15u) / 16u * 16u; }

template <int VPT>
hipError_t launch_eval(const EvalArgs& a, uint32_t grid, hipStream_t stream) {
  hipLaunchKernelGGL(k_field_eval<VPT>, dim3(grid), dim3(kT), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

extern "C" size_t gsr_fields_scratch_bytes(int32_t P) {
  if (P <= 0) return 0;
  return rec_at(P) + (size_t)P * kRecVec * 16u;
}

extern "C" int gsr_fields_bounds(const float* xyz, const float* opacity_raw, int32_t P, void* scratch, size_t scratch_bytes,
                                 void* stream_) {
  if (P <= 0) return GSR_EINVAL;
  if (!xyz || !opacity_raw || !scratch || misaligned(xyz, 4) || misaligned(opacity_raw, 4) || misaligned(scratch, 16))
    return GSR_EINVAL;
  const size_t need = gsr_fields_scratch_bytes(P);
  if (scratch_bytes < need) return GSR_ESCRATCH;
  if (overlap(scratch, need, xyz, (size_t)P * 12u) || overlap(scratch, need, opacity_raw, (size_t)P * 4u)) return GSR_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  uint32_t* head = reinterpret_cast<uint32_t*>(scratch);
  GsrDeviceGuard dev(scratch);
  hipLaunchKernelGGL(k_field_clear, dim3(1), dim3(64), 0, stream, head);
  GSR_HIP(hipGetLastError());
  const uint32_t tiles = ((uint32_t)P + kT - 1u) / kT;
  hipLaunchKernelGGL(k_field_bounds, dim3(tiles < (uint32_t)kMaxBlocks ? tiles : (uint32_t)kMaxBlocks), dim3(kT), 0, stream, xyz,
                     opacity_raw, (uint32_t)P, head);
  GSR_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_field_bounds_finish, dim3(1), dim3(64), 0, stream, head);
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

extern "C" int gsr_extract_fields(const float* xyz, const float* opacity_raw, const float* scaling_raw, const float* rotation_raw,
                                  int32_t P, const float* center, float scale, const float* coords, const float* gate_lo,
                                  const float* gate_hi, int32_t resolution, int32_t split_size, int32_t n_chunks, float* occ,
                                  void* scratch, size_t scratch_bytes, void* stream_) {
  if (P <= 0 || resolution < 1 || resolution > kMaxResolution || split_size < 1 || split_size > resolution) return GSR_EINVAL;
  if (n_chunks != (resolution + split_size - 1) / split_size || n_chunks > kMaxChunks) return GSR_EINVAL;
  if (!center || !finite(center[0]) || !finite(center[1]) || !finite(center[2]) || !finite(scale)) return GSR_EINVAL;
  const void* in[] = {xyz, opacity_raw, scaling_raw, rotation_raw, coords, gate_lo, gate_hi};
  const size_t P_ = (size_t)P, R_ = (size_t)resolution;
  const size_t in_bytes[] = {P_ * 12u, P_ * 4u, P_ * 12u, P_ * 16u, R_ * 4u, (size_t)n_chunks * 4u, (size_t)n_chunks * 4u};
  if (!occ || !scratch || misaligned(occ, 4) || misaligned(scratch, 16)) return GSR_EINVAL;
  for (const void* p : in)
    if (!p || misaligned(p, 4)) return GSR_EINVAL;
  const size_t need = gsr_fields_scratch_bytes(P), occ_bytes = R_ * R_ * R_ * 4u;
  if (scratch_bytes < need) return GSR_ESCRATCH;
  if (overlap(scratch, need, occ, occ_bytes)) return GSR_EINVAL;
  for (int j = 0; j < 7; ++j)
    if (overlap(scratch, need, in[j], in_bytes[j]) || overlap(occ, occ_bytes, in[j], in_bytes[j])) return GSR_EINVAL;
  // the largest triple has split_size^3 voxels; 256 * VPT of them a workgroup
  const uint64_t vox = (uint64_t)split_size * split_size * split_size;
  const int vpt = vox <= (uint64_t)kT ? 1 : vox <= 2u * kT ? 2 : 4;
  const uint64_t parts = (vox + (uint64_t)(kT * vpt) - 1u) / (uint64_t)(kT * vpt);
  const uint64_t grid = (uint64_t)n_chunks * n_chunks * n_chunks * parts;
  if (grid > 0x7FFFFFFFull) return GSR_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  char* base = reinterpret_cast<char*>(scratch);
  GsrDeviceGuard dev(scratch);
  PrepareArgs p = {};
  p.xyz = xyz;
  p.opacity_raw = opacity_raw;
  p.scaling_raw = scaling_raw;
  p.rotation_raw = rotation_raw;
  p.gate_lo = gate_lo;
  p.gate_hi = gate_hi;
  p.memb = reinterpret_cast<uint2*>(base + memb_at());
  p.rec = reinterpret_cast<float4*>(base + rec_at(P));
  p.P = (uint32_t)P;
  p.n_chunks = n_chunks;
  p.cx = center[0];
  p.cy = center[1];
  p.cz = center[2];
  p.scale = scale;
  hipLaunchKernelGGL(k_field_prepare, dim3(((uint32_t)P + kT - 1u) / kT), dim3(kT), 0, stream, p);
  GSR_HIP(hipGetLastError());
  EvalArgs e = {};
  e.rec = p.rec;
  e.memb = p.memb;
  e.coords = coords;
  e.occ = occ;
  e.P = (uint32_t)P;
  e.resolution = resolution;
  e.split_size = split_size;
  e.n_chunks = n_chunks;
  e.parts = (int)parts;
  if (vpt == 1) GSR_HIP(launch_eval<1>(e, (uint32_t)grid, stream));
  else if (vpt == 2) GSR_HIP(launch_eval<2>(e, (uint32_t)grid, stream));
  else GSR_HIP(launch_eval<4>(e, (uint32_t)grid, stream));
  return GSR_OK;
}

// densify.hip -- the densification itself (GaussianModel.densify_and_prune / prune / prune_points, gs_renderer.py:889-1059)
// as one planning pass, one host read of the new sizes and one gather pass over memory, gfx950.
//
// The reference clones, splits and prunes through boolean-mask gathers and torch.cat on every parameter and both of its Adam
// moments: every row is read and re-written about four times through well over a hundred launches. Here (SEMANTICS.md
// "densify_and_prune"):
//   k_densify_plan / k_densify_plan_mask   one thread per ORIGINAL row: classify it (keep / clone / split), evaluate the final
//                       prune test for the row, its clone and its children (all children of a row share one verdict: they share
//                       opacity and scaling), store three bits per row and three counts per 256-row block;
//   k_densify_scan      one block: exclusive scan of the block counts, the 2 + N segment sizes and P_out to device memory and
//                       to a page-locked host word;
//   (the host reads the sizes and allocates)
//   k_densify_index     src[j] = the original row of output row j. The KIND of row j follows from j and the segment sizes:
//                       [0,S) survivors | [S,S+C) clones | then N runs of Kc children, copy 0 first;
//   k_densify_gather    flat over the float4s of every output tensor: parameter, both moments and the statistics of all six
//                       groups in ONE launch. Children's xyz / scaling are computed here, moments of new rows are zeros.
// Plain vector stores only; no atomics. Built with -ffp-contract=off: one rounding per operator, as torch's op chain.
#include <math.h>

#include "gsr_common.h"
#include "gsr_rng.h"

namespace {

constexpr int kPlanBlock = 256;
constexpr int kScanBlock = 1024;
constexpr int kMaxJobs = 3 * GSR_DENSIFY_TENSORS + 3;

enum : int32_t { kCopy = 0, kCopyZeroNew = 1, kZero = 2, kXyz = 3, kScaling = 4 };

__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || a > b) ? a : b; }   // torch.max: NaN wins
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

struct PlanArgs {
  const float* scaling;      // [P,3] log
  const float* opacity;      // [P] logit
  const float* accum;        // [P]
  const float* denom;        // [P]
  const float* radii;        // [P] or NULL (treated as 0: densify_and_prune tests AFTER the statistics were reset)
  int32_t P;
  int32_t densify;           // 0: prune only (nothing is cloned or split)
  int32_t use_screen;
  float max_grad, dense, min_opacity, big_ws, max_screen, child_div;
};

// three counts of a 256-thread block -> counts[block][3]
__device__ __forceinline__ void block_counts(const bool s, const bool c, const bool k, uint32_t* __restrict__ counts) {
  __shared__ uint32_t w[3][kPlanBlock / GSR_WAVE];
  const uint64_t bs = __ballot(s), bc = __ballot(c), bk = __ballot(k);
  const int wave = threadIdx.x / GSR_WAVE;
  if (gsr_lane() == 0) {
    w[0][wave] = (uint32_t)__popcll(bs);
    w[1][wave] = (uint32_t)__popcll(bc);
    w[2][wave] = (uint32_t)__popcll(bk);
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    uint32_t t = 0;
    for (int i = 0; i < kPlanBlock / GSR_WAVE; ++i) t += w[threadIdx.x][i];
    counts[(size_t)blockIdx.x * 3 + threadIdx.x] = t;
  }
}

__global__ void __launch_bounds__(kPlanBlock)
k_densify_plan(const PlanArgs a, uint8_t* __restrict__ flags, uint32_t* __restrict__ counts) {
  const int i = blockIdx.x * kPlanBlock + threadIdx.x;
  bool keep = false, clone = false, kids = false;
  if (i < a.P) {
    const float s0 = expf(a.scaling[3 * (size_t)i]), s1 = expf(a.scaling[3 * (size_t)i + 1]), s2 = expf(a.scaling[3 * (size_t)i + 2]);
    const float smax = nan_max(nan_max(s0, s1), s2);
    const float op = sigmoidf_(a.opacity[i]);
    bool is_clone = false, is_split = false;
    if (a.densify) {
      float g = a.accum[i] / a.denom[i];
      if (g != g) g = 0.0f;                      // only NaN: x / 0 = inf stays inf and is selected
      const bool sel = g >= a.max_grad;
      is_clone = sel && smax <= a.dense;
      is_split = sel && smax > a.dense;
    }
    const float radius = a.radii ? a.radii[i] : 0.0f;
    const bool pruned = op < a.min_opacity || (a.use_screen && (radius > a.max_screen || smax > a.big_ws));
    keep = !is_split && !pruned;
    clone = is_clone && !pruned;                 // a clone has its source's values, hence its source's verdict
    if (is_split) {
      const float c0 = expf(logf(s0 / a.child_div)), c1 = expf(logf(s1 / a.child_div)), c2 = expf(logf(s2 / a.child_div));
      const float cmax = nan_max(nan_max(c0, c1), c2);
      kids = !(op < a.min_opacity || (a.use_screen && (0.0f > a.max_screen || cmax > a.big_ws)));
    }
    flags[i] = (uint8_t)((keep ? 1 : 0) | (clone ? 2 : 0) | (kids ? 4 : 0));
  }
  block_counts(keep, clone, kids, counts);
}

__global__ void __launch_bounds__(kPlanBlock)
k_densify_plan_mask(const uint8_t* __restrict__ mask, const int32_t P, uint8_t* __restrict__ flags, uint32_t* __restrict__ counts) {
  const int i = blockIdx.x * kPlanBlock + threadIdx.x;
  bool keep = false;
  if (i < P) {
    keep = mask[i] == 0;
    flags[i] = keep ? 1 : 0;
  }
  block_counts(keep, false, false, counts);
}

// counts[nb][3] -> exclusive prefixes in place; sizes[0] = S, [1] = C, [2 .. 2+N) = Kc, [GSR_DENSIFY_SIZE_WORDS-1] = P_out
__global__ void __launch_bounds__(kScanBlock)
k_densify_scan(uint32_t* __restrict__ counts, const int32_t nb, const int32_t N, int32_t* __restrict__ sizes_dev,
               int32_t* __restrict__ sizes_host) {
  __shared__ uint32_t sh[3][kScanBlock];
  const int t = threadIdx.x;
  const int chunk = (nb + kScanBlock - 1) / kScanBlock;
  const int b0 = t * chunk, b1 = min(nb, b0 + chunk);
  uint32_t sum[3] = {0u, 0u, 0u};
  for (int b = b0; b < b1; ++b)
    for (int k = 0; k < 3; ++k) sum[k] += counts[(size_t)b * 3 + k];
  for (int k = 0; k < 3; ++k) sh[k][t] = sum[k];
  __syncthreads();
  for (int o = 1; o < kScanBlock; o <<= 1) {
    uint32_t v[3];
    for (int k = 0; k < 3; ++k) v[k] = t >= o ? sh[k][t - o] : 0u;
    __syncthreads();
    for (int k = 0; k < 3; ++k) sh[k][t] += v[k];
    __syncthreads();
  }
  uint32_t run[3];
  for (int k = 0; k < 3; ++k) run[k] = sh[k][t] - sum[k];
  for (int b = b0; b < b1; ++b)
    for (int k = 0; k < 3; ++k) {
      const uint32_t c = counts[(size_t)b * 3 + k];
      counts[(size_t)b * 3 + k] = run[k];
      run[k] += c;
    }
  if (t < GSR_DENSIFY_SIZE_WORDS) {
    const uint32_t S = sh[0][kScanBlock - 1], C = sh[1][kScanBlock - 1], K = sh[2][kScanBlock - 1];
    int32_t v = 0;
    if (t == 0) v = (int32_t)S;
    else if (t == 1) v = (int32_t)C;
    else if (t < 2 + N) v = (int32_t)K;
    else if (t == GSR_DENSIFY_SIZE_WORDS - 1) v = (int32_t)(S + C + (uint32_t)N * K);
    sizes_dev[t] = v;
    if (sizes_host) sizes_host[t] = v;           // page-locked host words, written straight from the kernel
  }
}

__global__ void __launch_bounds__(kPlanBlock)
k_densify_index(const uint8_t* __restrict__ flags, const uint32_t* __restrict__ offs, const int32_t P, const int32_t N,
                const int32_t S, const int32_t C, const int32_t Kc, const int32_t P_out, int32_t* __restrict__ src) {
  __shared__ uint32_t w[3][kPlanBlock / GSR_WAVE];
  const int i = blockIdx.x * kPlanBlock + threadIdx.x;
  const uint32_t f = i < P ? flags[i] : 0u;
  const uint64_t lt = (1ull << gsr_lane()) - 1ull;
  const int wave = threadIdx.x / GSR_WAVE;
  uint32_t pre[3];
  for (int k = 0; k < 3; ++k) {
    const uint64_t b = __ballot((f >> k) & 1u);
    pre[k] = (uint32_t)__popcll(b & lt);
    if (gsr_lane() == 0) w[k][wave] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  for (int k = 0; k < 3; ++k) {
    for (int j = 0; j < wave; ++j) pre[k] += w[k][j];
    pre[k] += offs[(size_t)blockIdx.x * 3 + k];
  }
  // the positions come from device data and the extents from the caller: a row that does not fit is not written
  if ((f & 1u) && pre[0] < (uint32_t)S) src[pre[0]] = i;
  if ((f & 2u) && pre[1] < (uint32_t)C) src[(size_t)S + pre[1]] = i;
  if ((f & 4u) && pre[2] < (uint32_t)Kc)
    for (int c = 0; c < N; ++c) {
      const size_t j = (size_t)S + C + (size_t)c * Kc + pre[2];
      if (j < (size_t)P_out) src[j] = i;
    }
}

// ---- three standard normals as a pure function of (seed, row, copy): Philox-4x32-10 + Box-Muller (gsr_rng.h)
__device__ __forceinline__ void normals3(uint64_t seed, uint32_t row, uint32_t copy, float n[3]) {
  uint32_t r[4];
  philox4x32_10(row, copy, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
  const float ra = sqrtf(-2.0f * logf(u01(r[0]))), ta = 6.283185307179586f * u01(r[1]);
  const float rb = sqrtf(-2.0f * logf(u01(r[2]))), tb = 6.283185307179586f * u01(r[3]);
  n[0] = ra * cosf(ta);
  n[1] = ra * sinf(ta);
  n[2] = rb * cosf(tb);
}

struct Job {
  const float* src;
  float* dst;
  int32_t width;     // floats per row
  int32_t mode;
  uint32_t units;    // float4 units of dst (the last one may be partial)
  uint32_t vec4;     // width == 4 and src 16-byte aligned: one 16-byte load per row
};
struct GatherTab {
  int32_t n;
  uint32_t fblk[kMaxJobs + 1];
  Job job[kMaxJobs];
  const int32_t* rows;       // src[P_out]
  const float* xyz;          // the originals the children are computed from
  const float* scaling;
  const float* rotation;
  const float* noise;        // [N,P,3] or NULL
  uint64_t seed;
  int32_t P, P_out, S, C, Kc;
  float child_div;
};

// element `col` of the xyz of child `copy` of original row i (gs_renderer.py:982-986 with build_rotation, :124-145)
__device__ __forceinline__ float child_xyz(const GatherTab& t, const int32_t i, const int32_t copy, const int32_t col) {
  const float* q = t.rotation + 4 * (size_t)i;
  const float qr = q[0], qx = q[1], qy = q[2], qz = q[3];
  const float norm = sqrtf(qr * qr + qx * qx + qy * qy + qz * qz);
  const float r = qr / norm, x = qx / norm, y = qy / norm, z = qz / norm;
  float n[3];
  if (t.noise) {
    const float* p = t.noise + ((size_t)copy * t.P + i) * 3;
    n[0] = p[0]; n[1] = p[1]; n[2] = p[2];
  } else {
    normals3(t.seed, (uint32_t)i, (uint32_t)copy, n);
  }
  const float* s = t.scaling + 3 * (size_t)i;
  const float v0 = n[0] * expf(s[0]), v1 = n[1] * expf(s[1]), v2 = n[2] * expf(s[2]);
  float a, b, c;
  if (col == 0)      { a = 1.0f - 2.0f * (y * y + z * z); b = 2.0f * (x * y - r * z);        c = 2.0f * (x * z + r * y); }
  else if (col == 1) { a = 2.0f * (x * y + r * z);        b = 1.0f - 2.0f * (x * x + z * z); c = 2.0f * (y * z - r * x); }
  else               { a = 2.0f * (x * z - r * y);        b = 2.0f * (y * z + r * x);        c = 1.0f - 2.0f * (x * x + y * y); }
  return ((a * v0 + b * v1) + c * v2) + t.xyz[3 * (size_t)i + col];
}

__device__ __forceinline__ float gather_one(const GatherTab& t, const Job& jb, const uint32_t row, const uint32_t col) {
  if (jb.mode == kCopyZeroNew && row >= (uint32_t)t.S) return 0.0f;
  const int32_t i = t.rows[row];
  if ((uint32_t)i >= (uint32_t)t.P) return 0.0f;                 // cannot happen with a plan of this P; never read outside
  const uint32_t first_child = (uint32_t)(t.S + t.C);
  if (row >= first_child && jb.mode >= kXyz) {
    if (jb.mode == kScaling) return logf(expf(jb.src[(size_t)i * 3 + col]) / t.child_div);
    return child_xyz(t, i, (int32_t)((row - first_child) / (uint32_t)t.Kc), (int32_t)col);
  }
  return jb.src[(size_t)i * jb.width + col];
}

__global__ void __launch_bounds__(256)
k_densify_gather(const GatherTab t) {
  int ji = 0;
  for (int k = 1; k < t.n; ++k) ji += (blockIdx.x >= t.fblk[k]) ? 1 : 0;
  const Job& jb = t.job[ji];
  const uint32_t u = (blockIdx.x - t.fblk[ji]) * 256u + threadIdx.x;
  if (u >= jb.units) return;
  const uint32_t total = (uint32_t)t.P_out * (uint32_t)jb.width;
  const uint32_t e0 = u * 4u;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (jb.mode != kZero) {
    if (jb.vec4 && !(jb.mode == kCopyZeroNew && u >= (uint32_t)t.S)) {
      const int32_t i = t.rows[u];
      if ((uint32_t)i < (uint32_t)t.P) v = *reinterpret_cast<const float4*>(jb.src + (size_t)i * 4);
    } else if (!jb.vec4) {
      uint32_t row = e0 / (uint32_t)jb.width, col = e0 - row * (uint32_t)jb.width;
      float e[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (e0 + k < total) e[k] = gather_one(t, jb, row, col);
        if (++col == (uint32_t)jb.width) { col = 0; ++row; }
      }
      v = make_float4(e[0], e[1], e[2], e[3]);
    }
  }
  if (e0 + 3 < total) {
    *reinterpret_cast<float4*>(jb.dst + e0) = v;
  } else {
    const float e[4] = {v.x, v.y, v.z, v.w};
    for (uint32_t k = 0; e0 + k < total; ++k) jb.dst[e0 + k] = e[k];
  }
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int32_t plan_blocks(int32_t P) { return (int32_t)(((int64_t)P + kPlanBlock - 1) / kPlanBlock); }
inline bool rows_fit(int32_t P, int32_t N) {
  // output offsets are int32 and the gather's flat element index is uint32: at most max(2, N) P rows of <= 45 floats
  const int64_t rows = (int64_t)P * (N > 2 ? N : 2);
  return rows * 45 < 2147483648LL;
}
struct Scratch {
  uint8_t* flags;
  uint32_t* counts;
};
inline Scratch carve(void* scratch, int32_t P) {
  Scratch s;
  s.flags = reinterpret_cast<uint8_t*>(scratch);
  s.counts = reinterpret_cast<uint32_t*>(s.flags + align256((size_t)P));
  return s;
}

int plan_tail(const Scratch& s, int32_t P, int32_t N, int32_t* sizes_dev, int32_t* sizes_host, hipStream_t stream) {
  hipLaunchKernelGGL(k_densify_scan, dim3(1), dim3(kScanBlock), 0, stream, s.counts, plan_blocks(P), N, sizes_dev, sizes_host);
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

}  // namespace

extern "C" size_t gsr_densify_scratch_bytes(int32_t P, int32_t N) {
  if (P < 0 || N < 1 || N > GSR_DENSIFY_MAX_SPLIT || !rows_fit(P, N)) return 0;
  return align256((size_t)P) + align256((size_t)plan_blocks(P) * 3 * sizeof(uint32_t)) + 256;
}

extern "C" int gsr_densify_plan(const GsrDensifyPlan* plan, void* scratch, size_t scratch_bytes, int32_t* sizes_dev,
                                int32_t* sizes_host, void* stream_) {
  if (!plan || !scratch || !sizes_dev) return GSR_EINVAL;
  const int32_t P = plan->P, N = plan->N;
  if (P < 0 || N < 1 || N > GSR_DENSIFY_MAX_SPLIT) return GSR_EINVAL;
  if (!rows_fit(P, N)) return GSR_ECAPACITY;
  if (P > 0 && (!plan->scaling || !plan->opacity)) return GSR_EINVAL;
  if (P > 0 && plan->densify && (!plan->xyz_gradient_accum || !plan->denom)) return GSR_EINVAL;
  if (plan->densify && !(plan->max_grad > 0.0f)) return GSR_EINVAL;   // clones are never split only because 0 < max_grad
  if ((uintptr_t)scratch & 255u) return GSR_EINVAL;
  if (scratch_bytes < gsr_densify_scratch_bytes(P, N)) return GSR_ESCRATCH;
  hipStream_t stream = (hipStream_t)stream_;
  GsrDeviceGuard dev(scratch);
  const Scratch s = carve(scratch, P);
  if (P > 0) {
    PlanArgs a;
    a.scaling = plan->scaling; a.opacity = plan->opacity; a.accum = plan->xyz_gradient_accum; a.denom = plan->denom;
    a.radii = plan->max_radii2D; a.P = P; a.densify = plan->densify ? 1 : 0; a.use_screen = plan->use_screen_size ? 1 : 0;
    a.max_grad = plan->max_grad; a.dense = plan->dense_threshold; a.min_opacity = plan->min_opacity;
    a.big_ws = plan->world_size_threshold; a.max_screen = plan->max_screen_size; a.child_div = plan->child_divisor;
    hipLaunchKernelGGL(k_densify_plan, dim3((uint32_t)plan_blocks(P)), dim3(kPlanBlock), 0, stream, a, s.flags, s.counts);
    GSR_HIP(hipGetLastError());
  }
  return plan_tail(s, P, N, sizes_dev, sizes_host, stream);
}

extern "C" int gsr_densify_plan_mask(const uint8_t* mask, int32_t P, void* scratch, size_t scratch_bytes, int32_t* sizes_dev,
                                     int32_t* sizes_host, void* stream_) {
  if (!scratch || !sizes_dev || P < 0 || (P > 0 && !mask)) return GSR_EINVAL;
  if (!rows_fit(P, 1)) return GSR_ECAPACITY;
  if ((uintptr_t)scratch & 255u) return GSR_EINVAL;
  if (scratch_bytes < gsr_densify_scratch_bytes(P, 1)) return GSR_ESCRATCH;
  hipStream_t stream = (hipStream_t)stream_;
  GsrDeviceGuard dev(scratch);
  const Scratch s = carve(scratch, P);
  if (P > 0) {
    hipLaunchKernelGGL(k_densify_plan_mask, dim3((uint32_t)plan_blocks(P)), dim3(kPlanBlock), 0, stream, mask, P, s.flags, s.counts);
    GSR_HIP(hipGetLastError());
  }
  return plan_tail(s, P, 1, sizes_dev, sizes_host, stream);
}

extern "C" int gsr_densify_apply(const GsrDensifyTable* tab, const void* scratch, size_t scratch_bytes, int32_t* src,
                                 void* stream_) {
  if (!tab || !scratch) return GSR_EINVAL;
  const int32_t P = tab->P, N = tab->N, S = tab->n_survivors, C = tab->n_clones, Kc = tab->n_children, P_out = tab->P_out;
  if (P < 0 || N < 1 || N > GSR_DENSIFY_MAX_SPLIT || S < 0 || C < 0 || Kc < 0) return GSR_EINVAL;
  if (!rows_fit(P, N)) return GSR_ECAPACITY;
  if (S > P || C > P || Kc > P || (int64_t)S + C + (int64_t)N * Kc != (int64_t)P_out) return GSR_EINVAL;
  if ((uintptr_t)scratch & 255u) return GSR_EINVAL;
  if (scratch_bytes < gsr_densify_scratch_bytes(P, N)) return GSR_ESCRATCH;
  if (P_out == 0) return GSR_OK;
  if (!src) return GSR_EINVAL;
  if (Kc > 0 && (!tab->t[GSR_DENSIFY_XYZ].src || !tab->t[GSR_DENSIFY_SCALING].src || !tab->t[GSR_DENSIFY_ROTATION].src))
    return GSR_EINVAL;
  if (Kc > 0 && !(tab->child_divisor > 0.0f)) return GSR_EINVAL;

  GatherTab g = GatherTab{};
  g.rows = src; g.noise = tab->noise; g.seed = tab->seed; g.P = P; g.P_out = P_out; g.S = S; g.C = C; g.Kc = Kc > 0 ? Kc : 1;
  g.child_div = tab->child_divisor;
  g.xyz = tab->t[GSR_DENSIFY_XYZ].src; g.scaling = tab->t[GSR_DENSIFY_SCALING].src; g.rotation = tab->t[GSR_DENSIFY_ROTATION].src;
  uint32_t blk = 0;
  int n = 0;
  auto add = [&](const float* s, float* d, int32_t width, int32_t mode, bool required) -> int {
    if (!d) return required ? GSR_EINVAL : GSR_OK;      // a parameter is required; moments and statistics are optional
    if (mode != kZero && !s) return GSR_EINVAL;
    if ((uintptr_t)d & 15u) return GSR_EINVAL;
    Job& jb = g.job[n];
    jb.src = s; jb.dst = d; jb.width = width; jb.mode = mode;
    jb.units = (uint32_t)(((int64_t)P_out * width + 3) / 4);
    jb.vec4 = (width == 4 && mode != kZero && ((uintptr_t)s & 15u) == 0) ? 1u : 0u;
    g.fblk[n] = blk;
    blk += (jb.units + 255u) / 256u;
    ++n;
    return GSR_OK;
  };
  for (int k = 0; k < GSR_DENSIFY_TENSORS; ++k) {
    const GsrDensifyTensor& t = tab->t[k];
    if (t.width < 0 || t.width > 45) return GSR_EINVAL;
    if (t.width == 0) continue;                  // f_rest at K = 1
    if ((k == GSR_DENSIFY_XYZ || k == GSR_DENSIFY_SCALING) && t.width != 3) return GSR_EINVAL;
    if (k == GSR_DENSIFY_ROTATION && t.width != 4) return GSR_EINVAL;
    const int32_t mode = k == GSR_DENSIFY_XYZ ? kXyz : k == GSR_DENSIFY_SCALING ? kScaling : kCopy;
    int rc = add(t.src, t.dst, t.width, mode, true);
    if (rc == GSR_OK) rc = add(t.m1_src, t.m1_dst, t.width, kCopyZeroNew, false);
    if (rc == GSR_OK) rc = add(t.m2_src, t.m2_dst, t.width, kCopyZeroNew, false);
    if (rc != GSR_OK) return rc;
  }
  for (int k = 0; k < 3; ++k) {
    const int rc = add(tab->stat_src[k], tab->stat_dst[k], 1, tab->zero_stats ? kZero : kCopy, false);
    if (rc != GSR_OK) return rc;
  }
  g.n = n;
  for (int i = n; i <= kMaxJobs; ++i) g.fblk[i] = blk;

  hipStream_t stream = (hipStream_t)stream_;
  GsrDeviceGuard dev(scratch);
  const Scratch s = carve(const_cast<void*>(scratch), P);
  hipLaunchKernelGGL(k_densify_index, dim3((uint32_t)plan_blocks(P)), dim3(kPlanBlock), 0, stream, s.flags, s.counts, P, N, S, C, Kc,
                     P_out, src);
  GSR_HIP(hipGetLastError());
  if (blk > 0) {
    hipLaunchKernelGGL(k_densify_gather, dim3(blk), dim3(256), 0, stream, g);
    GSR_HIP(hipGetLastError());
  }
  return GSR_OK;
}

// select.hip -- an exact k-th order statistic of an fp32 array that stays in device memory, and on it the middle of the
// reference's 3D Gaussian filtering (include/gsrast.h, "k-th value select"; dreamscene_amd/filtering.py; SEMANTICS.md section 16):
//   gsr_kth_value          the value torch.sort(x)[0][k] has, written to device memory: clear, four histogram passes, one finish
//   gsr_importance_filter  calculate_v_imp_score + the mask of prune_gaussians (scene_gaussian.py:1046-1061, gs_renderer.py:
//                          1082-1087): clear, volume + pass 0, three passes, v + pass 0, three passes, mask -- ten launches
// The select is an MSD radix select on the order-preserving 32-bit key of the float (sign bit of non-negatives flipped, all bits
// of negatives flipped, every NaN the largest key), 8 bits a pass. A pass is ONE launch: every block first derives the prefix and
// the residual rank chosen so far from the earlier passes' 256-bin histograms (redundantly: it is a 256-entry scan per pass),
// histograms the elements that match the prefix in LDS (a histogram per wave), and adds its non-empty bins to the pass's global
// histogram with integer atomics. The launch boundary is the only hand-off between workgroups: no last-block-done counter, no
// flag, no fence inside a launch. Counts are integers, so the result has the same bits on every run. The grid is capped at
// kMaxBlocks; a block strides over the tiles past it. Nothing is allocated and nothing is read by the host (capturable); the
// scratch is cleared by a kernel, never by a memset node (gsr_common.h). One rounding per operator (built with
// -ffp-contract=off); expf, powf and `/` are the full-precision forms.
#include "gsr_common.h"

namespace {

constexpr int kT = 256;                          // threads per block (4 waves)
constexpr int kItems = 8;                        // elements per thread and tile
constexpr int kBlockItems = kT * kItems;         // elements per tile: 2048
constexpr int kMaxBlocks = 1024;                 // grid cap: 4 blocks on each of 256 CUs
constexpr int kWaves = kT / GSR_WAVE;
constexpr int kBins = 256;
constexpr int kPasses = 4;
constexpr int kHistWords = kPasses * kBins;      // one select's histograms
// scratch, in 32-bit words: the histograms of select A (the volume's, or gsr_kth_value's), those of select B (v's), the state
// block (float kth, float thr, two spare words), then n floats (the volumes, overwritten in place by v when v_list is NULL)
constexpr int kStateAt = 2 * kHistWords;
constexpr int kValuesAt = kStateAt + 4;
static_assert(kT == kBins, "one thread per bin in the scans and the flush");
static_assert((kValuesAt * 4) % 16 == 0, "the values start on a 16-byte boundary");

enum { kPlain = 0, kVolume = 1, kScore = 2 };    // what a pass's element is

struct Chosen {
  uint32_t prefix;                               // the key's leading 8 * npass bits, in place
  uint32_t k;                                    // the rank among the elements that share them
};

// The state after `npass` passes, from their histograms. Every thread of the block calls it and gets the same answer.
// s_wave [kWaves], s_sel [2]: LDS. The bins of pass q count the elements that match the prefix of the passes before it, so
// exactly one bin holds the residual rank.
__device__ Chosen derive(const uint32_t* __restrict__ hist, const int npass, const uint32_t k, uint32_t* s_wave, uint32_t* s_sel) {
  const int tid = threadIdx.x, lane = tid & (GSR_WAVE - 1), w = tid / GSR_WAVE;
  if (tid == 0) {
    s_sel[0] = 0u;
    s_sel[1] = k;
  }
  __syncthreads();
  for (int q = 0; q < npass; ++q) {
    const uint32_t c = hist[q * kBins + tid];
    uint32_t incl = c;
#pragma unroll
    for (int o = 1; o < GSR_WAVE; o <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)incl, o, GSR_WAVE);
      if (lane >= o) incl += t;
    }
    if (lane == GSR_WAVE - 1) s_wave[w] = incl;
    __syncthreads();
    for (int j = 0; j < w; ++j) incl += s_wave[j];
    const uint32_t excl = incl - c;
    const uint32_t kk = s_sel[1];
    __syncthreads();                             // every thread has read s_wave and s_sel[1] of this pass
    if (excl <= kk && kk < incl) {
      s_sel[0] |= (uint32_t)tid << (24 - 8 * q);
      s_sel[1] = kk - excl;
    }
    __syncthreads();
  }
  Chosen r;
  r.prefix = s_sel[0];
  r.k = s_sel[1];
  return r;
}

struct PassArgs {
  const float* x;            // kPlain: the values; kScore: the volumes
  float* store;              // kVolume: the volumes; kScore: v (may be x: element i is read and written by one thread)
  const float* scaling;      // kVolume: [n,3]
  const float* imp;          // kScore: [n]
  uint32_t* hist;            // this select's histograms, kPasses x kBins
  const uint32_t* hist_prev; // kScore: the volume select's histograms, complete
  float* state;              // kScore: state[0] = kth, for whoever wants to look at it
  uint32_t n, k, k_prev;
  int pass;                  // 0..3 (kVolume and kScore: 0)
  int activated;             // kVolume: scaling is already exp'ed
  float v_pow;
};

template <int MODE>
__global__ void __launch_bounds__(kT) k_select_pass(const PassArgs a) {
  __shared__ uint32_t s_hist[kWaves][kBins];
  __shared__ uint32_t s_wave[kWaves];
  __shared__ uint32_t s_sel[2];
  const int tid = threadIdx.x, w = tid / GSR_WAVE;
#pragma unroll
  for (int j = 0; j < kWaves; ++j) s_hist[j][tid] = 0u;
  float kth = 0.f;
  if (MODE == kScore) {
    kth = gsr_key_float(derive(a.hist_prev, kPasses, a.k_prev, s_wave, s_sel).prefix);
    if (blockIdx.x == 0 && tid == 0) a.state[0] = kth;
  }
  uint32_t prefix = 0u, care = 0u;
  if (a.pass > 0) {
    prefix = derive(a.hist, a.pass, a.k, s_wave, s_sel).prefix;
    care = 0xFFFFFFFFu << (32 - 8 * a.pass);
  }
  const int shift = 24 - 8 * a.pass;
  __syncthreads();
  for (uint64_t base = (uint64_t)blockIdx.x * kBlockItems; base < a.n; base += (uint64_t)gridDim.x * kBlockItems) {
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
      const uint64_t i = base + (uint64_t)j * kT + tid;
      if (i >= a.n) break;
      float f;
      if (MODE == kVolume) {
        float s0 = a.scaling[3 * i], s1 = a.scaling[3 * i + 1], s2 = a.scaling[3 * i + 2];
        if (!a.activated) {
          s0 = expf(s0);
          s1 = expf(s1);
          s2 = expf(s2);
        }
        f = (s0 * s1) * s2;                      // torch.prod's order over the row
        a.store[i] = f;
      } else if (MODE == kScore) {
        f = powf(a.x[i] / kth, a.v_pow) * a.imp[i];
        a.store[i] = f;
      } else {
        f = a.x[i];
      }
      const uint32_t key = gsr_float_key(f);
      if (((key ^ prefix) & care) == 0u) atomicAdd(&s_hist[w][(key >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  uint32_t c = 0u;
#pragma unroll
  for (int j = 0; j < kWaves; ++j) c += s_hist[j][tid];
  if (c) atomicAdd(&a.hist[a.pass * kBins + tid], c);
}

__global__ void __launch_bounds__(kT) k_select_clear(uint32_t* __restrict__ words, const uint32_t n_words, int32_t* __restrict__ count) {
  for (uint32_t i = blockIdx.x * kT + threadIdx.x; i < n_words; i += gridDim.x * kT) words[i] = 0u;
  if (count && blockIdx.x == 0 && threadIdx.x == 0) *count = 0;
}

__global__ void __launch_bounds__(kT) k_select_finish(const uint32_t* __restrict__ hist, const uint32_t k, float* __restrict__ out) {
  __shared__ uint32_t s_wave[kWaves];
  __shared__ uint32_t s_sel[2];
  const float v = gsr_key_float(derive(hist, kPasses, k, s_wave, s_sel).prefix);
  if (threadIdx.x == 0) *out = v;
}

__global__ void __launch_bounds__(kT) k_filter_mask(const float* __restrict__ v, const uint32_t n, const uint32_t* __restrict__ hist,
                                                    const uint32_t k, uint8_t* __restrict__ mask, int32_t* __restrict__ count,
                                                    float* __restrict__ state) {
  __shared__ uint32_t s_wave[kWaves];
  __shared__ uint32_t s_sel[2];
  const int tid = threadIdx.x, lane = tid & (GSR_WAVE - 1), w = tid / GSR_WAVE;
  const float thr = gsr_key_float(derive(hist, kPasses, k, s_wave, s_sel).prefix);
  if (blockIdx.x == 0 && tid == 0) state[1] = thr;
  uint32_t mine = 0u;
  for (uint64_t base = (uint64_t)blockIdx.x * kBlockItems; base < n; base += (uint64_t)gridDim.x * kBlockItems) {
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
      const uint64_t i = base + (uint64_t)j * kT + tid;
      if (i >= n) break;
      const bool pruned = v[i] <= thr;           // false for a NaN on either side
      mask[i] = pruned ? 1 : 0;
      mine += pruned ? 1u : 0u;
    }
  }
  if (!count) return;
#pragma unroll
  for (int o = GSR_WAVE / 2; o > 0; o >>= 1) mine += (uint32_t)__shfl_xor((int)mine, o, GSR_WAVE);
  if (lane == 0) s_wave[w] = mine;               // derive's last barrier is behind every read of s_wave
  __syncthreads();
  if (tid == 0) {
    uint32_t total = 0u;
    for (int j = 0; j < kWaves; ++j) total += s_wave[j];
    if (total) atomicAdd(count, (int32_t)total);
  }
}

bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// [a, a + na) and [b, b + nb) bytes share an address
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && x < y + nb && y < x + na;
}

uint32_t grid_for(uint32_t n) {
  const uint32_t tiles = (n + kBlockItems - 1u) / kBlockItems;
  return tiles < (uint32_t)kMaxBlocks ? tiles : (uint32_t)kMaxBlocks;
}

template <int MODE>
hipError_t launch_pass(const PassArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_select_pass<MODE>, dim3(grid_for(a.n)), dim3(kT), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

extern "C" size_t gsr_select_scratch_bytes(int32_t n) {
  if (n <= 0) return 0;
  return (((size_t)kValuesAt + (size_t)n) * 4u + 15u) / 16u * 16u;
}

extern "C" int gsr_kth_value(const float* x, int32_t n, int32_t k, float* out, void* scratch, size_t scratch_bytes, void* stream_) {
  if (n <= 0 || k < 0 || k >= n) return GSR_EINVAL;
  if (!x || !out || !scratch || misaligned(x, 4) || misaligned(out, 4) || misaligned(scratch, 16)) return GSR_EINVAL;
  if (scratch_bytes < gsr_select_scratch_bytes(n)) return GSR_ESCRATCH;
  if (overlap(scratch, (size_t)kValuesAt * 4u, x, (size_t)n * 4u) || overlap(scratch, (size_t)kValuesAt * 4u, out, 4u))
    return GSR_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  uint32_t* hist = reinterpret_cast<uint32_t*>(scratch);
  GsrDeviceGuard dev(x);
  hipLaunchKernelGGL(k_select_clear, dim3((kHistWords + kT - 1) / kT), dim3(kT), 0, stream, hist, (uint32_t)kHistWords,
                     (int32_t*)nullptr);
  GSR_HIP(hipGetLastError());
  PassArgs a = {};
  a.x = x;
  a.hist = hist;
  a.n = (uint32_t)n;
  a.k = (uint32_t)k;
  for (a.pass = 0; a.pass < kPasses; ++a.pass) GSR_HIP(launch_pass<kPlain>(a, stream));
  hipLaunchKernelGGL(k_select_finish, dim3(1), dim3(kT), 0, stream, hist, (uint32_t)k, out);
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

extern "C" int gsr_importance_filter(const float* scaling, int32_t activated, const float* imp, int32_t n, float v_pow,
                                     int32_t k_volume, int32_t k_threshold, uint8_t* mask, float* v_list, int32_t* n_pruned,
                                     void* scratch, size_t scratch_bytes, void* stream_) {
  if (n <= 0) return GSR_EINVAL;
  const bool score = scaling != nullptr, cut = mask != nullptr;
  if (!score && !cut) return GSR_EINVAL;
  if (score && (k_volume < 0 || k_volume >= n || !imp)) return GSR_EINVAL;
  if (cut && (k_threshold < 0 || k_threshold >= n)) return GSR_EINVAL;
  if ((!score || !cut) && !v_list) return GSR_EINVAL;              // v is the one form's output and the other's input
  if (n_pruned && !cut) return GSR_EINVAL;
  if (!scratch || misaligned(scratch, 16) || misaligned(scaling, 4) || misaligned(imp, 4) || misaligned(v_list, 4) ||
      misaligned(n_pruned, 4))
    return GSR_EINVAL;
  const size_t need = gsr_select_scratch_bytes(n);
  if (scratch_bytes < need) return GSR_ESCRATCH;
  const size_t nb = (size_t)n * 4u;
  if (overlap(scratch, need, scaling, 3u * nb) || overlap(scratch, need, imp, nb) || overlap(scratch, need, v_list, nb) ||
      overlap(scratch, need, mask, (size_t)n) || overlap(scratch, need, n_pruned, 4u))
    return GSR_EINVAL;
  if (overlap(v_list, nb, mask, (size_t)n) || overlap(v_list, nb, n_pruned, 4u) || overlap(mask, (size_t)n, n_pruned, 4u) ||
      (score && (overlap(v_list, nb, scaling, 3u * nb) || overlap(v_list, nb, imp, nb))))
    return GSR_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  uint32_t* words = reinterpret_cast<uint32_t*>(scratch);
  uint32_t* hist_a = words;
  uint32_t* hist_b = words + kHistWords;
  float* state = reinterpret_cast<float*>(words + kStateAt);
  float* values = reinterpret_cast<float*>(words + kValuesAt);
  float* v = v_list ? v_list : values;
  GsrDeviceGuard dev(scratch);
  hipLaunchKernelGGL(k_select_clear, dim3((kValuesAt + kT - 1) / kT), dim3(kT), 0, stream, words, (uint32_t)kValuesAt, n_pruned);
  GSR_HIP(hipGetLastError());
  PassArgs a = {};
  a.n = (uint32_t)n;
  a.state = state;
  if (score) {
    a.scaling = scaling;
    a.activated = activated;
    a.store = values;
    a.hist = hist_a;
    a.k = (uint32_t)k_volume;
    a.pass = 0;
    GSR_HIP(launch_pass<kVolume>(a, stream));
    a.x = values;
    for (a.pass = 1; a.pass < kPasses; ++a.pass) GSR_HIP(launch_pass<kPlain>(a, stream));
    a.store = v;
    a.imp = imp;
    a.v_pow = v_pow;
    a.hist_prev = hist_a;
    a.k_prev = (uint32_t)k_volume;
    a.hist = hist_b;
    a.k = (uint32_t)(cut ? k_threshold : 0);
    a.pass = 0;
    GSR_HIP(launch_pass<kScore>(a, stream));
    if (!cut) return GSR_OK;
  } else {
    a.x = v;
    a.hist = hist_b;
    a.k = (uint32_t)k_threshold;
    a.pass = 0;
    GSR_HIP(launch_pass<kPlain>(a, stream));
  }
  a.x = v;
  for (a.pass = 1; a.pass < kPasses; ++a.pass) GSR_HIP(launch_pass<kPlain>(a, stream));
  hipLaunchKernelGGL(k_filter_mask, dim3(grid_for((uint32_t)n)), dim3(kT), 0, stream, (const float*)v, (uint32_t)n,
                     (const uint32_t*)hist_b, (uint32_t)k_threshold, mask, n_pruned, state);
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

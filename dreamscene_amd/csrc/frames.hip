// frames.hip -- frame export, gfx950: the uint8 tail of the reference's inference paths (include/gsrast.h, "frame export";
// SEMANTICS.md "Frame export"). video_inference (training/object_trainer.py:81-118), scene_video_inference and scene_cams_record
// (training/scene_trainer.py:261-340) end every frame with
//   image  = clamp(rgb, 0, 1) .cpu().permute(1, 2, 0).numpy();               (image  * 255).round().astype(np.uint8)
//   depths = clamp(depth / depth.max(), 0, 1) .cpu().permute(1, 2, 0).numpy(); (depths * 255).round().astype(np.uint8)
// Here the chain runs per pixel on the device, one rounding per operator (this file is built with -ffp-contract=off):
//   byte = rint(fl32(clamp(x, 0, 1) * 255))      rint = round half to even (numpy's round), never floor(x + 0.5)
// with x the colour, or fl32(depth / M): a correctly rounded fp32 DIVISION by the frame's own maximum M of the depth plane, not
// a multiplication by 1 / M. A NaN (only 0 / 0 of an all-zero depth frame, where numpy's cast is undefined) gives byte 0.
// Inputs are finite: that is the precondition.
//   K_max    per frame and block the maximum of the depth plane -> scratch (the two-level partials of glue.hip: a maximum does
//            not depend on the order, and there is no atomic anywhere)
//   K_quant  every block reduces its frame's partials (at most 1 KB from L2), then writes the bytes: rgb [F,H,W,3] interleaved
//            and depth [F,H,W,1]. Without depth K_max is not launched.
// Work unit: 4 consecutive pixels of one frame per lane. The planes are read with one 16-byte load each where every plane base
// is 16-byte aligned and H*W is a multiple of 4 (dword loads otherwise), the 12 interleaved colour bytes leave as three dwords
// and the 4 depth bytes as one. A frame whose first output byte is not 4-byte aligned (H*W*3 not a multiple of 4 puts the
// frames k >= 1 there) and the last, partial unit of a frame take byte stores.
// Per pixel: reads 12 bytes (16 with depth, the depth plane twice: 20) and writes 3 (4).
#include "gsr_common.h"

namespace {

constexpr int kT = 256;                 // threads per block (4 waves)
constexpr int kMaxBlocks = 256;         // K_max, per frame: its partials are reduced by ONE pass of a 256-thread block
constexpr int kQuantBlocks = 2048;      // K_quant, per frame: cap the grid, grid-stride the rest

struct alignas(4) Bytes12 { uint32_t a, b, c; };

__device__ __forceinline__ float block_max(float v, float* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3]));
}

// n valid pixels from p0 on; vec: the plane is 16-byte aligned and p0 + 4 <= hw
__device__ __forceinline__ void load4(const float* __restrict__ plane, uint32_t p0, uint32_t n, bool vec, float fill, float v[4]) {
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(plane + p0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) v[k] = (k < n) ? plane[p0 + k] : fill;
  }
}

// clamp to [0, 1] (NaN -> 0), one fp32 multiplication, round half to even
__device__ __forceinline__ uint32_t byte_of(float x) {
  float c = (x > 0.f) ? x : 0.f;
  c = (c < 1.f) ? c : 1.f;
  return (uint32_t)rintf(c * 255.f);
}

__global__ void __launch_bounds__(kT) k_frames_max(const GsrFrameViews t, const uint32_t hw, const int vec, float* __restrict__ part) {
  __shared__ float lds[4];
  const float* __restrict__ D = t.depth_alpha[blockIdx.y];
  const uint32_t units = (hw + 3u) / 4u;
  float m = -INFINITY;
  for (uint32_t e = blockIdx.x * kT + threadIdx.x; e < units; e += gridDim.x * kT) {
    const uint32_t p0 = e * 4u, n = hw - p0 < 4u ? hw - p0 : 4u;
    float d[4];
    load4(D, p0, n, vec != 0, -INFINITY, d);
    m = fmaxf(fmaxf(m, fmaxf(d[0], d[1])), fmaxf(d[2], d[3]));
  }
  m = block_max(m, lds);
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = m;
}

template <bool DEPTH>
__global__ void __launch_bounds__(kT) k_frames_quant(const GsrFrameViews t, const uint32_t hw, const int vec,
                                                     const float* __restrict__ part, const int nb, uint8_t* __restrict__ rgb,
                                                     uint8_t* __restrict__ depth) {
  __shared__ float lds[4];
  const int f = blockIdx.y;
  float M = 0.f;
  if (DEPTH) {
    M = -INFINITY;
    for (int k = threadIdx.x; k < nb; k += kT) M = fmaxf(M, part[(size_t)f * nb + k]);
    M = block_max(M, lds);
  }
  const float* __restrict__ R = t.image[f];
  const float* __restrict__ G = R + hw;
  const float* __restrict__ B = G + hw;
  const float* __restrict__ D = DEPTH ? t.depth_alpha[f] : nullptr;
  uint8_t* __restrict__ O = rgb + (size_t)f * hw * 3u;
  uint8_t* __restrict__ OD = DEPTH ? depth + (size_t)f * hw : nullptr;
  const bool o4 = (reinterpret_cast<uintptr_t>(O) & 3u) == 0;       // this frame's bytes start on a dword
  const bool d4 = (reinterpret_cast<uintptr_t>(OD) & 3u) == 0;
  const uint32_t units = (hw + 3u) / 4u;
  for (uint32_t e = blockIdx.x * kT + threadIdx.x; e < units; e += gridDim.x * kT) {
    const uint32_t p0 = e * 4u, n = hw - p0 < 4u ? hw - p0 : 4u;
    float r[4], g[4], b[4];
    load4(R, p0, n, vec != 0, 0.f, r);
    load4(G, p0, n, vec != 0, 0.f, g);
    load4(B, p0, n, vec != 0, 0.f, b);
    uint32_t q[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      q[3 * k] = byte_of(r[k]);
      q[3 * k + 1] = byte_of(g[k]);
      q[3 * k + 2] = byte_of(b[k]);
    }
    uint8_t* __restrict__ o = O + (size_t)p0 * 3u;
    if (n == 4u && o4) {
      Bytes12 w;
      w.a = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
      w.b = q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24);
      w.c = q[8] | (q[9] << 8) | (q[10] << 16) | (q[11] << 24);
      *reinterpret_cast<Bytes12*>(o) = w;
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 12; ++k)
        if (k < 3u * n) o[k] = (uint8_t)q[k];
    }
    if (DEPTH) {
      float d[4];
      load4(D, p0, n, vec != 0, 0.f, d);
      uint32_t z[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) z[k] = byte_of(d[k] / M);          // 0 / 0 (an all-zero frame): NaN -> byte 0
      if (n == 4u && d4) {
        *reinterpret_cast<uint32_t*>(OD + p0) = z[0] | (z[1] << 8) | (z[2] << 16) | (z[3] << 24);
      } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
          if (k < n) OD[p0 + k] = (uint8_t)z[k];
      }
    }
  }
}

bool frames_shape_ok(int32_t n_views, int32_t h, int32_t w) {
  return n_views >= 1 && n_views <= GSR_MAX_FRAME_VIEWS && h >= 1 && w >= 1 && (int64_t)h * w <= (int64_t)INT32_MAX;
}

int max_blocks(uint32_t hw) {
  const uint32_t b = (hw + 4u * kT - 1u) / (4u * kT);
  return (int)(b < (uint32_t)kMaxBlocks ? b : (uint32_t)kMaxBlocks);
}

}  // namespace

extern "C" size_t gsr_frames_scratch_bytes(int32_t n_views, int32_t height, int32_t width) {
  if (!frames_shape_ok(n_views, height, width)) return 0;
  const size_t b = (size_t)n_views * max_blocks((uint32_t)((int64_t)height * width)) * sizeof(float);
  return (b + 255) & ~(size_t)255;
}

extern "C" int gsr_frames_quantize(const GsrFrameViews* views, uint8_t* rgb, uint8_t* depth, void* scratch, size_t scratch_bytes,
                                   void* stream_) {
  if (!views || !frames_shape_ok(views->n_views, views->height, views->width) || !rgb) return GSR_EINVAL;
  const uint32_t hw = (uint32_t)((int64_t)views->height * views->width);
  uintptr_t low = 0;                                   // the low address bits of every plane base
  for (int k = 0; k < views->n_views; ++k) {
    if (!views->image[k] || (depth && !views->depth_alpha[k])) return GSR_EINVAL;
    if (((uintptr_t)views->image[k] & 3u) || (depth && ((uintptr_t)views->depth_alpha[k] & 3u))) return GSR_EINVAL;
    low |= (uintptr_t)views->image[k] | (depth ? (uintptr_t)views->depth_alpha[k] : 0);
  }
  if (depth) {
    if (!scratch || ((uintptr_t)scratch & 15u)) return GSR_EINVAL;
    if (scratch_bytes < gsr_frames_scratch_bytes(views->n_views, views->height, views->width)) return GSR_ESCRATCH;
  }
  const int vec = ((low & 15u) == 0 && hw % 4u == 0) ? 1 : 0;
  const uint32_t units = (hw + 3u) / 4u;
  const uint32_t gq = (units + kT - 1u) / kT < (uint32_t)kQuantBlocks ? (units + kT - 1u) / kT : (uint32_t)kQuantBlocks;
  const dim3 grid(gq, (uint32_t)views->n_views);
  hipStream_t stream = (hipStream_t)stream_;
  GsrDeviceGuard dev(rgb);
  if (!depth) {
    hipLaunchKernelGGL(k_frames_quant<false>, grid, dim3(kT), 0, stream, *views, hw, vec, (const float*)nullptr, 0, rgb, depth);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
  }
  const int nb = max_blocks(hw);
  float* part = reinterpret_cast<float*>(scratch);
  hipLaunchKernelGGL(k_frames_max, dim3((uint32_t)nb, (uint32_t)views->n_views), dim3(kT), 0, stream, *views, hw, vec, part);
  GSR_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_frames_quant<true>, grid, dim3(kT), 0, stream, *views, hw, vec, (const float*)part, nb, rgb, depth);
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

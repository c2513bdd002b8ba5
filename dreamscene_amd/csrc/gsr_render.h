// gsr_render.h -- what K6 (render_fwd.hip) and K7 (render_bwd.hip) share: the compositing arithmetic defined operation by
// operation, the pixel <-> lane map of a tile, the exact block culling, and the layouts the two kernels agree on (staged
// splat record, checkpoint rows, (item, view) grid).
//  * Splat records (3 x float4, written by K1) are gathered by list index 256 at a time into an LDS stage.
//  * At staging time every thread tests "its" splat EXACTLY against the four pixel blocks of the workgroup (minimum of
//    the conic form over the block rectangle vs the splat's tau: block_reach). Splats that cannot touch a wave's
//    pixels cost it no vector instructions; the per-pixel gates (power > 0, alpha < 1/255, T < 1e-4) are evaluated
//    unchanged on the survivors, as 64-bit lane masks on the scalar unit.
//  * Both kernels are bound by VALU issue (SQ counters: > 80 % of the issue slots): their code is shaped by
//    instruction count (scalar lane masks, v_med3, v_rcp, integer min on float bits, no packed fp32 -- both files are
//    built with -fno-slp-vectorize, see build.py and DESIGN.md).
// Semantics: SURVEY.md Appendix A.2 / A.3, SEMANTICS.md; outputs as consumed at scene_gaussian.py:1012-1032.
#pragma once
#include <type_traits>

#include "gsr_common.h"
#include "gsr_launch.h"

// exp() and the quadratic form of the compositing loops are DEFINED operation by operation (SEMANTICS.md section 4) and
// evaluated identically here and in oracle/gsr_oracle.c (orc_exp, orc_power): the hard gates (power > 0,
// alpha < 1/255, T < 1e-4) are discontinuities, and any rounding difference in front of them puts about one
// (pixel, splat) pair per 10^6 pixels on the other side. With IEEE operations only (no v_exp_f32, whose bits are the
// hardware's) both sides produce the same bits, so n_contrib and final_T are bit-exact against the oracle.
//   exp:   t = x * float(log2 e); n = rint(t); f = t - n; p = Horner degree 5 in f (fma); result = ldexp(p, int(n))
//          (10 full-rate VALU operations; the former compensated v_exp_f32 version took 6 incl. one transcendental)
//   power: dx * (hA dx + nB dy) + (hC dy) dy with hA = -A/2, nB = -B, hC = -C/2 formed (exactly) when a splat is
//          staged: 3 multiplies + 2 fma per evaluation instead of 5 + 2.
namespace {

constexpr int kBatch = 256;

// One IEEE rounding per operation, never contracted into an FMA (HIP's __fmul_rn / __fsub_rn are plain operators and
// WOULD be contracted under the default -ffp-contract=fast; the pragma removes the `contract` flag from the
// instructions generated inside these functions, and inlining keeps instruction flags).
__device__ __forceinline__ float gsr_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float gsr_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
__device__ __forceinline__ float gsr_exp(float x) {
  const float t = gsr_mul(x, 1.44269502162933349609375f);
  const float n = __builtin_rintf(t);
  const float f = gsr_sub(t, n);
  float p = 0.001326472731307149f;
  p = __fmaf_rn(p, f, 0.009671512991189957f);
  p = __fmaf_rn(p, f, 0.05550733581185341f);
  p = __fmaf_rn(p, f, 0.24022242426872253f);
  p = __fmaf_rn(p, f, 0.6931470036506653f);
  p = __fmaf_rn(p, f, 1.0f);
  return __builtin_amdgcn_ldexpf(p, gsr_f2i_sat_fast(n));
}
// power from the staged (hA, nB, hC) = (-A/2, -B, -C/2)
__device__ __forceinline__ float gsr_power(float hA, float nB, float hC, float dx, float dy) {
  return __fmaf_rn(dx, __fmaf_rn(hA, dx, gsr_mul(nB, dy)), gsr_mul(gsr_mul(hC, dy), dy));
}

// The first two rows of a splat record (three rows of the K1 output) as they are staged: the conic as (hA, nB, hC) =
// (-A/2, -B, -C/2), what gsr_power takes (exact scalings); K7 stages the depth relative to zref.
__device__ __forceinline__ float4 stage_row0(const float4 n0) { return make_float4(n0.x, n0.y, -0.5f * n0.z, -n0.w); }
__device__ __forceinline__ float4 stage_row1(const float4 n1, const float zref = 0.f) {
  return make_float4(-0.5f * n1.x, n1.y, n1.z - zref, n1.w);     // (x - 0.f is x, bit for bit)
}
__device__ __forceinline__ uint32_t stage_mask(const float4& s2row) { return __float_as_uint(s2row.w); }

struct TilePix {
  int px, py, bx, by;   // pixel, and origin of the wave's 8x8 block
  bool inside;
};

__device__ __forceinline__ TilePix tile_pixel(int tile, int gx, int W, int H) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int ty = tile / gx, tx = tile - ty * gx;
  TilePix p;
  p.bx = tx * GSR_TILE + (wave & 1) * 8;
  p.by = ty * GSR_TILE + (wave >> 1) * 8;
  p.px = p.bx + (lane & 7);
  p.py = p.by + (lane >> 3);
  p.inside = (p.px < W) && (p.py < H);
  return p;
}

// The contract between K6 and K7: the checkpoint of the per-pixel prefix state at list position pos (a multiple of KB,
// counted from the start of the whole point list) is six planes of 256 floats -- T, C0, C1, C2, depth, alpha at offsets
// 0, 256, ... 1280 -- in slot pos / KB, at pixel (px, py) of the 16x16 tile with origin (x0, y0). Boundaries of one list
// are KB apart and the first boundary of a tile lies >= KB entries after the end of the previous tile's list, so slots
// never collide.
template <int KB, class F>
__device__ __forceinline__ F* ckpt_row(F* ckpt, uint32_t pos, int py, int y0, int px, int x0) {
  return ckpt + (size_t)(pos / KB) * (6 * 256) + ((py - y0) * GSR_TILE + (px - x0));
}

// Load balance: tiles differ in cost by orders of magnitude (empty / silhouette / deep). The work lists are ordered
// heaviest-first on the device (k_work_order_fwd / _bwd) and workgroup b simply takes item b: the hardware dispatcher
// hands workgroups out in index order as slots free up, i.e. longest-processing-time-first scheduling. Several views share
// a launch through a 1-D grid over (work item, view). per_view = 0: the VIEW runs fastest -- workgroup b takes item
// b / n_views of view b % n_views, so the dispatcher (index order) hands out the heaviest items of all views first and the
// empty tail of every view's list last (skewed lists, C3: K7 64 -> 58 us per view). per_view = items per view: the views
// run one after the other -- when thousands of tiles weigh about the same (camera inside a room) the order does not matter
// for balance and keeping one view's splat records in the L2s at a time does (indoor: 8 % faster this way).
struct ItemView { uint32_t item; int view; };
__device__ __forceinline__ ItemView item_view(const uint32_t n_views, const uint32_t per_view) {
  const uint32_t item = per_view ? blockIdx.x % per_view : blockIdx.x / n_views;
  return {item, (int)(per_view ? blockIdx.x / per_view : blockIdx.x - item * n_views)};
}

// Can the splat pass the alpha gate anywhere on the W1 x W1 pixel block with origin (bx, by)?  Exact up to the
// inflation of tau: minimum of the convex form q(d) = A dx^2 + 2 B dx dy + C dy^2 over the block's rectangle (in
// d = centre - pixel coordinates) compared with tau. A convex function whose free minimum (d = 0) lies outside the
// rectangle takes its minimum on a face the centre sees from outside -- at most one vertical and one horizontal
// face. ex / ey = the coordinate of the rectangle nearest to 0 on each axis (the facing face, or 0 when the centre
// is inside that axis range, which only adds interior points); on each of the two lines q is a parabola with a
// clamped vertex. Centre inside the rectangle: ex = ey = 0 and both candidates are 0.
template <int W1>
__device__ __forceinline__ bool block_reach(float A, float C, float B2, float nBiA, float nBiC, float tau, float cx,
                                            float cy, float bx, float by) {
  const float dx1 = cx - bx, dx0 = dx1 - (float)(W1 - 1), dy1 = cy - by, dy0 = dy1 - (float)(W1 - 1);
  const float ex = __builtin_amdgcn_fmed3f(dx0, 0.f, dx1), ey = __builtin_amdgcn_fmed3f(dy0, 0.f, dy1);
  const float y = __builtin_amdgcn_fmed3f(dy0, nBiC * ex, dy1);
  const float q1 = A * ex * ex + (B2 * ex + C * y) * y;
  const float x = __builtin_amdgcn_fmed3f(dx0, nBiA * ey, dx1);
  const float q2 = C * ey * ey + (B2 * ey + A * x) * x;
  return fminf(q1, q2) <= tau;
}

// 4-bit mask over the 2x2 grid of W1 x W1 blocks with origin (x0, y0): bit (wave index) set = the splat can reach it.
// W1 = 8: the four 8x8 blocks of a 16x16 tile (K7); W1 = 4: the four 4x4 blocks of an 8x8 quarter (K6).
template <int W1>
__device__ __forceinline__ uint32_t block_mask_t(const float4 q0, const float4 q1, const float4 q2, int x0i, int y0i) {
  const float tau = q2.z;
  if (!(tau >= 0.f)) return 0u;
  const float A = q0.z, B = q0.w, C = q1.x;
  // vertex of q along a vertical line dx = e: dy = -B e / C; along a horizontal line dy = e: dx = -B e / A
  const float nBiA = -B * __builtin_amdgcn_rcpf(A), nBiC = -B * __builtin_amdgcn_rcpf(C), B2 = 2.f * B;
  const float x0 = (float)x0i, y0 = (float)y0i;
  uint32_t m = 0;
  m |= (uint32_t)block_reach<W1>(A, C, B2, nBiA, nBiC, tau, q0.x, q0.y, x0, y0);
  m |= (uint32_t)block_reach<W1>(A, C, B2, nBiA, nBiC, tau, q0.x, q0.y, x0 + (float)W1, y0) << 1;
  m |= (uint32_t)block_reach<W1>(A, C, B2, nBiA, nBiC, tau, q0.x, q0.y, x0, y0 + (float)W1) << 2;
  m |= (uint32_t)block_reach<W1>(A, C, B2, nBiA, nBiC, tau, q0.x, q0.y, x0 + (float)W1, y0 + (float)W1) << 3;
  return m;
}

// One launch for the runtime checkpoint distance kb (gsr_seg_len): f(std::integral_constant<int, KB>) for the KB of KBs
// that equals kb, then the launch check. Only the listed KBs are instantiated; any other kb is GSR_EINVAL.
template <int... KBs, class F>
int launch_kb(uint32_t kb, F&& f) {
  if (!((kb == (uint32_t)KBs && (f(std::integral_constant<int, KBs>{}), true)) || ...)) return GSR_EINVAL;
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

}  // namespace

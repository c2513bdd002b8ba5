// render_bwd.hip -- K7, the reverse-order backward of the compositing K6 (render_fwd.hip), gfx950; shared: gsr_render.h.
// Work items, not tiles: K7 takes one (tile, seg_len-entry segment) per 256-thread workgroup with one 8x8 block per wave,
// restarted from the per-pixel checkpoints K6 leaves at every segment boundary.
//  * K7's waves walk a 64-bit ballot of the staged entries' block test with scalar code.
//  * K7 reduces the 10 per-splat gradient sums over the wave's 64 pixels with a transposed butterfly (reduce10) that
//    leaves them in 12 different lanes: ONE global_atomic_add_f64 instruction commits a splat's row.
//  * Load balance: the work list is ordered heaviest-first on the device (k_work_order_bwd), see gsr_render.h.
#include "gsr_render.h"

namespace {

// Several views at once: workgroup blockIdx.x builds the list of view blockIdx.x (pointer tables in the kernel arguments).
struct WorkBwdViews {
  const uint32_t* tile_depth[GSR_MAX_BATCH_VIEWS];
  uint32_t* items[GSR_MAX_BATCH_VIEWS];
  uint32_t items_cap[GSR_MAX_BATCH_VIEWS];
  uint32_t seg_len[GSR_MAX_BATCH_VIEWS];
};

// Backward work list: one item (tile, segment) per started kb-entry segment of [0, tile_depth[tile]) -- kb = GsrBinning.seg_len,
// the distance of the forward's checkpoints. Order = longest processing time first for the in-order hardware dispatch: full
// segments by what is left of the tile's depth behind their start (r = d - kb s: the more is left, the more pixels are still
// alive; segment 0 of a deep tile is the heaviest item there is, the last full segment of any tile the lightest), 16
// buckets of 256 entries; then the partial tails, longest first, 16 buckets. (Round 4, one call: against "all full segments in
// tile order, then the tails" K7 -1 % ... -2 % in every configuration and this kernel 8.8 -> 6.7 us.)
// items[0] = number of items, items[2 + 2 i] = tile, items[3 + 2 i] = segment. Single workgroup per view.
__global__ void __launch_bounds__(1024)
k_work_order_bwd(const uint32_t n_tiles, const WorkBwdViews wv) {
  const uint32_t* __restrict__ tile_depth = wv.tile_depth[blockIdx.x];
  uint32_t* __restrict__ items = wv.items[blockIdx.x];
  const uint32_t items_cap = wv.items_cap[blockIdx.x];
  const uint32_t kb = wv.seg_len[blockIdx.x];
  __shared__ uint32_t cnt[32], cur[32];
  const int tid = threadIdx.x;
  if (tid < 32) cnt[tid] = 0;
  __syncthreads();
  for (uint32_t t = tid; t < n_tiles; t += 1024) {
    const uint32_t d = tile_depth[t];
    if (d == 0) continue;
    const uint32_t full = d / kb, tail = d % kb;
    for (uint32_t sgi = 0; sgi < full; ++sgi) atomicAdd(&cnt[15u - min(15u, (d - kb * sgi - 1u) >> 8)], 1u);
    if (tail) atomicAdd(&cnt[16u + 15u - ((tail - 1u) * 16u) / kb], 1u);
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t run = 0;
    for (int b = 0; b < 32; ++b) { cur[b] = run; run += cnt[b]; }
    items[0] = min(run, items_cap);
  }
  __syncthreads();
  for (uint32_t t = tid; t < n_tiles; t += 1024) {
    const uint32_t d = tile_depth[t];
    if (d == 0) continue;
    const uint32_t full = d / kb, tail = d % kb;
    for (uint32_t sgi = 0; sgi < full; ++sgi) {
      const uint32_t i = atomicAdd(&cur[15u - min(15u, (d - kb * sgi - 1u) >> 8)], 1u);
      if (i < items_cap) { items[2 + 2 * i] = t; items[3 + 2 * i] = sgi; }
    }
    if (tail) {
      const uint32_t i = atomicAdd(&cur[16u + 15u - ((tail - 1u) * 16u) / kb], 1u);
      if (i < items_cap) { items[2 + 2 * i] = t; items[3 + 2 * i] = full; }
    }
  }
}

// --------------------------------------------------------------------------------------------------------- K7
// Transposed butterfly over the 64 lanes for 10 values (see file header): at every step a lane keeps one register of a
// pair and hands the other one to its partner, so the number of live registers halves while the sums grow:
//   10 -> 5 over lane bit 3 (row_ror:8 = lane ^ 8), -> 3 over bit 2 (row_half_mirror = lane ^ 7), -> 2 over bit 5
//   (permlane32 swap), -> 1 over bit 4 (permlane16 swap), then quad_perm xor 2 and xor 1 complete the sums.
// The steps with the most pairs use the cheapest primitive (issue costs): bits 3 and 2 are also BANKS of a
// DPP row (lanes 4i..4i+3), so "select, then add the partner's other register" is two DPP adds with complementary bank
// masks (a bank-masked DPP write leaves the other lanes' destination alone: 2 x 1.85 ns per pair); a permlane swap +
// add is 4.7 ns per pair and is left for the two steps with 2 and 1 pairs. Round 3 had the order bit 5, 4, 3, 2
// (5 + 3 swaps): 50.5 ns of issue per splat, this order 47.4.
// On return lane L (b_k = bit k of L) holds, in rows 0 and 2 (b4 = 0), the wave total of component b3 + 2 b2 + 4 b5; in row 1
// the total over lanes 0-31 of component 8 + b3 and in row 3 the total over lanes 32-63 of the same (word 10 + b3).
__device__ __forceinline__ float add_swap32(float a, float b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float add_swap16(float a, float b) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float reduce10(const float v[10]) {
  // (s_nop: the inputs come straight from VALU instructions and a DPP operand needs two wait states after its producer;
  //  the hazard recognizer does not look inside an asm block)
  float p0, p1, p2, p3, p4, q0, q1, q2;
  asm("s_nop 1\n\t"
      "v_add_f32_dpp %0, %8, %8 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
      "v_add_f32_dpp %0, %9, %9 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
      "v_add_f32_dpp %1, %10, %10 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
      "v_add_f32_dpp %1, %11, %11 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
      "v_add_f32_dpp %2, %12, %12 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
      "v_add_f32_dpp %2, %13, %13 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
      "v_add_f32_dpp %3, %14, %14 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
      "v_add_f32_dpp %3, %15, %15 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
      "v_add_f32_dpp %4, %16, %16 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
      "v_add_f32_dpp %4, %17, %17 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
      "s_nop 1\n\t"
      "v_add_f32_dpp %5, %0, %0 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"
      "v_add_f32_dpp %5, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
      "v_add_f32_dpp %6, %2, %2 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"
      "v_add_f32_dpp %6, %3, %3 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
      "v_add_f32_dpp %7, %4, %4 row_half_mirror row_mask:0xf bank_mask:0xf"
      : "=&v"(p0), "=&v"(p1), "=&v"(p2), "=&v"(p3), "=&v"(p4), "=&v"(q0), "=&v"(q1), "=&v"(q2)
      : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]), "v"(v[8]), "v"(v[9]));
  // q0: components b3 + 2 b2, q1: 4 + b3 + 2 b2, q2: 8 + b3 (in all lanes: its pair partner is the pad)
  const float r0 = add_swap32(q0, q1);      // lanes 0-31: q0 (components b3 + 2 b2), lanes 32-63: q1 (4 + ...)
  // q2 has no partner register: it skips the bit-5 step (a swap with a zero register, an add) and is committed from BOTH
  // halves of the wave into DIFFERENT words of the 12-float row -- row 1 adds its half's sums of components 8, 9 to words
  // 8, 9, row 3 to words 10, 11, K8 adds the two. (Into the same words it would be two lanes of one atomic instruction on
  // one address, and those serialise: 55 -> 102 us per view.)
  float R = add_swap16(r0, q2);             // rows 0, 2: r0 (complete), rows 1, 3: q2 summed over rows {0,1} / {2,3}
  asm("s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
      : "+v"(R));
  return R;
}

// Accumulates into partials [P,16 doubles], with q = dL/dG * G per (pixel, splat), d = centre - pixel and (u, v) = -Sigma^-1 d =
// (-(A dx + B dy), -(C dy + B dx)) (Sigma^-1 = the conic):
//   (sum q u, sum q v, sum q u^2, sum q u v, sum q v^2, dL/dopacity, dL/dr, dL/dg, dL/db, dL/ddepth, dL/db', dL/ddepth', -, -, -, -)
// (the last two pairs: the sums over the lower / upper half of a wave, added by K8 -- see reduce10)
// Inside a wave the sums are reduced in fp32 in a FIXED order (reduce10); ACROSS waves they are added by atomics in whatever
// order the workgroups arrive. In fp32 that order showed: the covariance chain amplifies sum q u^2 / q u v / q v^2 by
// cond(Sigma)^2 on needle-shaped splats and dL/dopacity collects the 7e4-weighted extremal pixels of the reference's disp
// normalisation (scene_gaussian.py:1025-1032) -- the worst dL/drotations entry of the needle case moved between 2.7e-6 and
// 1.5e-5 from run to run, dL/dopacity of the boundary records between 1e-5 and 1e-4 (round 3). Now every wave result is
// added in DOUBLE (global_atomic_add_f64: 29 spare mantissa bits over the fp32 addends -- the sum of a splat's wave results is
// exact, hence the same in every order, as long as the addends' exponents span less than 2^29; beyond that span -- the 7e4-
// weighted extremal pixels of the disp normalisation next to a near-zero contribution -- an addend can move the double by
// 2^-53 of the sum, visible in fp32 only on a rounding tie) and K8 rounds the total to fp32 once: the backward is
// order-independent within that span (tests: same bits over eight runs, <= 4 one-ulp ties per tensor allowed).
// One atomic instruction per (splat, block) as before -- 12 lanes, one 128-byte row. (Measured first: doubles for the four
// sensitive sums only, in a second atomic instruction next to the f32 one: K7 217 -> 238 us -- two atomic instructions per
// iteration run into the atomic issue limit of ~80 ns per instruction and SIMD, DESIGN.md "Issue costs".)
// dG/dd = G (u, v), so the first two sums are dL/d(pixel centre), and dL/dSigma = 1/2 sum q (Sigma^-1 d)(Sigma^-1 d)^T, so
// the other three are the gradient of the 2-D covariance itself (K8 only scales them) -- both formed PER PIXEL, as the
// scalar oracle does (gsr_oracle.c, orc_pixel_bwd; SEMANTICS.md section 5). Rounds 1-2 summed the raw moments of d
// (sum q dx, ..., sum q dy^2) and contracted them with the conic afterwards: exact in exact arithmetic, but the
// contraction cancels digits on needle-shaped splats -- A dx and B dy are of opposite sign and equal size along the
// needle -- and the lineage's conic -> covariance step amplifies the rounding of the sums by cond(Sigma)^2 (measured
// against float64 autograd: 1e-1 on dL/dscales of 1000 : 1 splats, which the reference's scale noise + clamp(.., 0)
// produces, scene_gaussian.py:1005-1008).
//
// Work item = (tile, segment): the <= 256 list entries [256 s, min(256 (s+1), tile_depth)) of one tile, for all of
// its 256 pixels, traversed back to front. The reverse traversal of a pixel is a serial recurrence over its whole
// depth (up to thousands of splats), and the deepest tiles used to set the kernel time; segments make the items
// uniform and independent. A pixel whose last contributor lies beyond the segment starts from the forward's
// checkpoint at the segment end (prefix transmittance T_c and prefix sums C_c, D_c, W_c): the colour / depth /
// alpha composited BEHIND that point, normalised to start there, is (X_final - X_c) / T_c, which is exactly the
// `rec` state the sequential traversal would carry at that position. Other pixels start from their final state.
// Round 3, measured and not kept (both bit-identical in their results; A/B in one gpurun call, C3, 4-view launch):
//  * two pixels per lane (a wave owns a 16x8 half tile, 2 waves per item, the reduction and the atomic shared by the two
//    8x8 blocks; NOT v_pk_* arithmetic: v_pk_fma_f32 issues at half the rate of v_fma_f32 on gfx950, tools/probe): 279 us
//    against 238 -- what the shared reduction saves (37 of ~95 instructions per block) the three-way control flow and
//    its register copies give back, and half as many waves hide less latency;
//  * the four waves of a workgroup adding their sums of a splat into an LDS row (ds_add_f32, ten lanes) and the workgroup
//    committing every staged entry once at the end (2.5x fewer global lane-atomics, 16x fewer atomic instructions):
//    444 us against 238 -- float atomics on LDS are an order of magnitude slower than the global ones they replace;
//  * (and the control: the same kernel with the global atomic compiled out runs 236 us against 238 -- the atomics are
//    free, the loop is bound by instruction issue);
//  * the launch zero-filling the 142 MB of gradient buffers K8's sparse form otherwise clears itself ("K7 is VALU-bound,
//    the stores are free"): K8 100 -> 86 us, K7 236 -> 274 us. The stores are not free: K7's atomics share the path.
template <int KB>
__device__ __forceinline__ void
render_bwd_body(const uint32_t item, const int W, const int H, const uint32_t* __restrict__ items, const uint32_t* __restrict__ tile_depth,
             const float* __restrict__ ckpt,
             const uint32_t* __restrict__ ranges, const uint32_t* __restrict__ point_list,
             const float4* __restrict__ splat, const float* __restrict__ bg, const float* __restrict__ color,
             const float* __restrict__ depth_alpha, const float* __restrict__ final_T,
             const uint32_t* __restrict__ n_contrib, const float* __restrict__ dL_dcolor,
             const float* __restrict__ dL_dda, float* __restrict__ partials, unsigned long long* __restrict__ reach) {
  __shared__ float4 s0[KB], s1[KB], s2[KB];
  __shared__ uint32_t sid[KB], smask[KB];
  __shared__ unsigned long long hitw[KB / 64];    // staged entries some wave committed sums for (-> GsrGrads.reach)
  const int gx = (W + GSR_TILE - 1) / GSR_TILE;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (item >= items[0]) return;
 {
  const int tile = (int)items[2 + 2 * item];
  const uint32_t seg = items[3 + 2 * item];
  const uint32_t depth = tile_depth[tile];
  const uint32_t lo = seg * KB, hi = min(lo + (uint32_t)KB, depth);
  const int n = (int)(hi - lo);

  const TilePix p = tile_pixel(tile, gx, W, H);
  const int tile_x0 = p.bx - (wave & 1) * 8, tile_y0 = p.by - (wave >> 1) * 8;
  const float pxf = (float)p.px, pyf = (float)p.py;
  const uint32_t r0 = ranges[2 * tile];
  const size_t pix = (size_t)p.py * W + p.px, HW = (size_t)H * W;

  // Depths are staged RELATIVE to the depth of the segment's last entry (uniform: two scalar loads). The loop carries
  // R' = sum_k w_k (s_k - c) over the splats k composited behind, with s = <(colour, depth, 1), upstream gradient> and the
  // per-pixel constant c = zref g_depth + g_alpha, next to A = sum_k w_k (the alpha composited behind): s - R = (s' - R') +
  // c (1 - A). With the reference's disp normalisation |g_depth|, |g_alpha| reach 7e4 on the extremal pixels
  // (scene_gaussian.py:1025-1032): s and R are then ~4e5 each and, in front of an opaque object (A -> 1), cancel to
  // g_depth (z - z_behind) ~ 1e3 -- in the plain form that difference carried eps x 4e5 of rounding (dL/dopacity of the
  // boundary records: 2e-5 .. 9e-5 of max|ref|, deterministic since the sums are added in double); in this form the large
  // part c (1 - A) vanishes exactly where the cancellation happens and s' - R' is a difference of terms ~ g_depth x 0.1.
  const float zref = reinterpret_cast<const float*>(splat + 3 * (size_t)point_list[r0 + (hi - 1u)] + 1)[2];
  // stage the segment, last entry first (one gather per thread)
  {
    float4 n0 = make_float4(0, 0, 0, 0), n1 = n0, n2 = make_float4(0, 0, -1.f, -1.f);
    uint32_t nid = 0;
    if (tid < n) {      // (K6's gather_splat, spelled out: the helper changes this kernel's register allocation)
      nid = point_list[r0 + (hi - 1u - (uint32_t)tid)];
      const float4* r = splat + 3 * (size_t)nid;
      n0 = r[0]; n1 = r[1]; n2 = r[2];
    }
    if (tid < KB) {                                                        // (256 threads, KB <= 256 staged rows)
      s0[tid] = stage_row0(n0);
      s1[tid] = stage_row1(n1, zref);
      s2[tid] = n2;
      sid[tid] = nid;
      smask[tid] = (tid < n) ? block_mask_t<8>(n0, n1, n2, tile_x0, tile_y0) : 0u;
    }
    if (tid < KB / 64) hitw[tid] = 0ull;
  }

  const float Tf = p.inside ? final_T[pix] : 0.f;
  const uint32_t last = p.inside ? n_contrib[pix] : 0u;
  float gC0 = 0.f, gC1 = 0.f, gC2 = 0.f, gD = 0.f, gA = 0.f;
  if (p.inside) {
    gC0 = dL_dcolor[pix]; gC1 = dL_dcolor[HW + pix]; gC2 = dL_dcolor[2 * HW + pix];
    gD = dL_dda[pix]; gA = dL_dda[HW + pix];
  }
  const float bg0 = bg[0], bg1 = bg[1], bg2 = bg[2];
  const float bg_dot = (bg0 * gC0 + bg1 * gC1) + bg2 * gC2;

  float T = Tf;
  float R = 0.f, A = 0.f;
  if (last > hi) {
    // this pixel keeps compositing beyond the segment: start from the forward's checkpoint at position hi
    const float* ck = ckpt_row<KB>(ckpt, r0 + hi, p.py, tile_y0, p.px, tile_x0);
    const float Tc = ck[0];
    const float inv = 1.0f / Tc;
    T = Tc;
    const float rc0 = ((color[pix] - Tf * bg0) - ck[256]) * inv;
    const float rc1 = ((color[HW + pix] - Tf * bg1) - ck[512]) * inv;
    const float rc2 = ((color[2 * HW + pix] - Tf * bg2) - ck[768]) * inv;
    const float rec_z = (depth_alpha[pix] - ck[1024]) * inv;
    const float rec_a = (depth_alpha[HW + pix] - ck[1280]) * inv;
    R = rc0 * gC0 + rc1 * gC1 + rc2 * gC2 + (rec_z - zref * rec_a) * gD;     // = R - c A  (the g_alpha terms cancel exactly)
    A = rec_a;
  }
  const float cshift = zref * gD + gA;

  // one lane per quad commits with the single atomic of a splat's 10 sums; its component: bit 3 -> 1, bit 2 -> 2, bit 5 -> 4, bit 4 -> 8 (see reduce10)
  const int b2 = (lane >> 2) & 1, b3 = (lane >> 3) & 1, b4 = (lane >> 4) & 1, b5 = (lane >> 5) & 1;
  const int comp = b4 ? 8 + 2 * b5 + b3 : (b3 | (b2 << 1) | (b5 << 2));      // double of the 16-double row (see reduce10)
  const bool commit = ((lane & 3) == 0) && !(b4 && b2);                      // 8 + 4 lanes, twelve different doubles
  __syncthreads();

  for (int k = 0; k < KB / 64; ++k) {
    if (k * 64 >= n) break;
    unsigned long long bits = __ballot((smask[k * 64 + lane] >> wave) & 1u);
    unsigned long long hitk = 0ull;       // (scalar unit: free next to the vector instructions of the other waves)
    while (bits) {
      const int jb = __builtin_ctzll(bits);
      const int j = k * 64 + jb;
      bits &= bits - 1ull;
      const uint32_t pos = hi - 1u - (uint32_t)j;      // 0-based list position
      const unsigned long long livem = __builtin_amdgcn_ballot_w64(pos < last);
      if (livem == 0ull) continue;
      const float4 a = s0[j];
      const float4 b = s1[j];
      const float dx = a.x - pxf, dy = a.y - pyf;
      const float power = gsr_power(a.z, a.w, b.x, dx, dy);
      const float G = gsr_exp(power);
      const float alpha = fminf(GSR_ALPHA_MAX, gsr_mul(b.y, G));
      // the gates as 64-bit lane masks on the scalar unit
      const unsigned long long hitm = livem & __builtin_amdgcn_ballot_w64(power <= 0.0f) &
                                      __builtin_amdgcn_ballot_w64(alpha >= GSR_ALPHA_MIN);
      if (hitm == 0ull) continue;
      hitk |= 1ull << jb;
      const bool hit = __builtin_amdgcn_inverse_ballot_w64(hitm);
      // per-lane factors of the 10 sums; lanes without a hit contribute zeros (only these three are cleared)
      float qv = 0.f, wv = 0.f, gdl = 0.f;
      if (hit) {
        const float4 c = s2[j];
        // v_rcp_f32 (1 ulp): T is only reconstructed for the gradient weights here, no gate depends on it. (A Newton step
        // on the reciprocal was tried against the reference-derived boundary records, where dL/dopacity sits at 2e-5 ..
        // 9e-5: no change -- that error is the fp32 noise of the 7e4 upstream spike, tests/test_boundary_fixture.py.)
        const float inv = __builtin_amdgcn_rcpf(1.0f - alpha);
        T = T * inv;
        const float w = alpha * T;
        // R = <(colour, depth, alpha) composited behind this splat, normalised to start here; upstream gradient>: the
        // recurrence of the behind-state is linear, so its dot product with the pixel's upstream gradient can be
        // carried instead of its five components (dL/dalpha only ever needs that dot product)
        const float sdot = b.w * gC0 + c.x * gC1 + c.y * gC2 + b.z * gD;       // s - c  (b.z is staged relative to zref)
        const float t1 = 1.0f - A;
        float dL_dalpha = ((sdot - R) + cshift * t1) * T;
        dL_dalpha -= (Tf * inv) * bg_dot;
        R = alpha * sdot + (1.0f - alpha) * R;
        A = __fmaf_rn(alpha, t1, A);
        // raw moments of q = dL/dG * G over the pixels; K8 turns them into dL/dmean2D and dL/dconic
        qv = (b.y * dL_dalpha) * G;
        gdl = G * dL_dalpha;
        wv = w;
      }
      float v[10];
      {
        // (u, v) = -Sigma^-1 d:  u = -(A dx + B dy) = fma(2 hA, dx, nB dy),  v = -(C dy + B dx) = fma(2 hC, dy, nB dx)
        // (hA = -A/2, nB = -B, hC = -C/2: the doublings are exact; the same expression tree as orc_pixel_bwd)
        const float u = __fmaf_rn(a.z + a.z, dx, gsr_mul(a.w, dy)), w2 = __fmaf_rn(b.x + b.x, dy, gsr_mul(a.w, dx));
        const float m1 = qv * u, m2 = qv * w2;
        v[0] = m1; v[1] = m2;
        v[2] = m1 * u; v[3] = m1 * w2; v[4] = m2 * w2;
        v[5] = gdl;
        v[6] = wv * gC0; v[7] = wv * gC1; v[8] = wv * gC2;
        v[9] = wv * gD;
      }
      const float sred = reduce10(v);
      if (commit) unsafeAtomicAdd(reinterpret_cast<double*>(partials) + (GSR_PARTIAL_WORDS / 2) * (size_t)sid[j] + comp, (double)sred);
    }
    if (reach && hitk && lane == 0) atomicOr(&hitw[k], hitk);
  }
  if (reach) {
    // the Gaussians this item committed sums for: one bit each, set by the thread that staged the entry (outside the loop:
    // a handful of 64-bit atomics per item)
    __syncthreads();
    if (tid < n && ((hitw[tid >> 6] >> (tid & 63)) & 1ull)) atomicOr(reach + (sid[tid] >> 6), 1ull << (sid[tid] & 63u));
  }
 }
}

}  // namespace

struct BwdViews {
  const uint32_t* items[GSR_MAX_BATCH_VIEWS];
  const uint32_t* tile_depth[GSR_MAX_BATCH_VIEWS];
  const float* ckpt[GSR_MAX_BATCH_VIEWS];
  const uint32_t* ranges[GSR_MAX_BATCH_VIEWS];
  const uint32_t* point_list[GSR_MAX_BATCH_VIEWS];
  const float4* splat[GSR_MAX_BATCH_VIEWS];
  const float* bg[GSR_MAX_BATCH_VIEWS];
  const float* color[GSR_MAX_BATCH_VIEWS];
  const float* depth_alpha[GSR_MAX_BATCH_VIEWS];
  const float* final_T[GSR_MAX_BATCH_VIEWS];
  const uint32_t* n_contrib[GSR_MAX_BATCH_VIEWS];
  const float* dL_dcolor[GSR_MAX_BATCH_VIEWS];
  const float* dL_dda[GSR_MAX_BATCH_VIEWS];
  float* partials[GSR_MAX_BATCH_VIEWS];
  unsigned long long* reach[GSR_MAX_BATCH_VIEWS];
};

template <int KB = kBatch>
__global__ void __launch_bounds__(256)
k_render_bwd(const int W, const int H, const BwdViews bv, const uint32_t n_views, const uint32_t per_view) {
  const auto [item, y] = item_view(n_views, per_view);
  render_bwd_body<KB>(item, W, H, bv.items[y], bv.tile_depth[y], bv.ckpt[y], bv.ranges[y], bv.point_list[y], bv.splat[y], bv.bg[y],
                  bv.color[y], bv.depth_alpha[y], bv.final_T[y], bv.n_contrib[y], bv.dL_dcolor[y], bv.dL_dda[y],
                  bv.partials[y], bv.reach[y]);
}

int gsr_launch_work_order_bwd(int n, const GsrView* views, const GsrBinning* bs, const GsrImages* imgs, hipStream_t stream) {
  const uint32_t tiles = gsr_num_tiles(views[0].image_height, views[0].image_width);
  WorkBwdViews wv = WorkBwdViews{};
  for (int k = 0; k < n; ++k) {
    wv.tile_depth[k] = imgs[k].tile_depth; wv.items[k] = bs[k].tile_work + tiles; wv.items_cap[k] = bs[k].bwd_items_cap;
    wv.seg_len[k] = gsr_seg_len(bs[k]);
  }
  hipLaunchKernelGGL(k_work_order_bwd, dim3((uint32_t)n), dim3(1024), 0, stream, tiles, wv);
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

// K7 of n views in one launch (work lists built; same image size and the same seg_len: the caller checks).
int gsr_launch_render_bwd_views(int n, const GsrView* views, const GsrGeom* geoms, const GsrBinning* bs,
                                const GsrImages* imgs, const GsrImageGrads* igs, GsrGrads* outs, hipStream_t stream,
                                GsrProfile* prof) {
  const GsrView& v = views[0];
  const uint32_t tiles = gsr_num_tiles(v.image_height, v.image_width);
  BwdViews bv = BwdViews{};
  uint32_t items_cap = 0;
  for (int k = 0; k < n; ++k) {
    bv.items[k] = bs[k].tile_work + tiles; bv.tile_depth[k] = imgs[k].tile_depth; bv.ckpt[k] = imgs[k].ckpt;
    bv.ranges[k] = bs[k].ranges; bv.point_list[k] = bs[k].point_list;
    bv.splat[k] = reinterpret_cast<const float4*>(geoms[k].splat); bv.bg[k] = views[k].bg; bv.color[k] = imgs[k].color;
    bv.depth_alpha[k] = imgs[k].depth_alpha; bv.final_T[k] = imgs[k].final_T; bv.n_contrib[k] = imgs[k].n_contrib;
    bv.dL_dcolor[k] = igs[k].dL_dcolor; bv.dL_dda[k] = igs[k].dL_ddepth_alpha; bv.partials[k] = outs[k].partials;
    bv.reach[k] = reinterpret_cast<unsigned long long*>(outs[k].reach);
    items_cap = bs[k].bwd_items_cap > items_cap ? bs[k].bwd_items_cap : items_cap;
  }
  // The stage timer brackets the compositing kernel alone (not the work-list kernel), as the forward's does.
  GsrStageTimer timer(prof, stream, GSR_STAGE_RENDER_BWD);
  return launch_kb<64, 128, 256>(gsr_seg_len(bs[0]), [&](auto kb) {
    // (per_view: the same regime switch as the forward variant)
    hipLaunchKernelGGL(k_render_bwd<kb>, dim3(items_cap * (uint32_t)n), dim3(256), 0, stream, v.image_width, v.image_height,
                       bv, (uint32_t)n, bs[0].fwd_mode == 1 ? items_cap : 0u);
  });
}

// render_fwd.hip -- K6, front-to-back alpha compositing, gfx950 (wave64). Backward: render_bwd.hip; shared: gsr_render.h.
// Work items, not tiles: K6 takes one 8x8 pixel quarter of a 16x16 tile per 256-thread workgroup (four lanes share a
// pixel and take four consecutive candidates of the list per step; a whole-tile variant with one pixel per lane serves
// scenes of thousands of shallow tiles) and leaves per-pixel checkpoints at every seg_len-entry boundary for K7.
//  * The LDS stage of the splat records is double-buffered: the gather of batch b+1 is issued before batch b is
//    consumed, ONE workgroup barrier per batch.
//  * K6's waves compact the survivors of the block test for their block into a byte list in LDS.
//  * Load balance: the work list is ordered heaviest-first on the device (k_work_order_fwd), see gsr_render.h.
#include "gsr_render.h"

namespace {

template <int CTRL>
__device__ __forceinline__ int gsr_dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
// sum over the four slots of a pixel (the banks of a DPP row: row_ror:4, :8); all lanes take part
__device__ __forceinline__ float fold_slots(float x) { x += gsr_dpp<0x124>(x); return x + gsr_dpp<0x128>(x); }

// The splat record (three rows of the K1 output) of list entry `pos`, and its Gaussian id. (The whole-tile variant and
// K7 spell this gather out: with the reference parameters their register allocation changes, profiles/HISTORY.md.)
__device__ __forceinline__ void gather_splat(const uint32_t* point_list, const float4* splat, uint32_t pos, uint32_t& nid,
                                             float4& n0, float4& n1, float4& n2) {
  nid = point_list[pos];
  const float4* r = splat + 3 * (size_t)nid;
  n0 = r[0]; n1 = r[1]; n2 = r[2];
}

// The outputs of pixel `pix` of an H x W image (HW = H * W); the colour sums get the background behind them. (The empty
// tiles' store stays spelled out: 0 + 1 * bg is not bg for the compiler.)
__device__ __forceinline__ void store_pixel(size_t pix, size_t HW, float T, uint32_t last, float c0, float c1, float c2,
                                            float depth, float alpha, const float* bg, float* out_color, float* out_da,
                                            float* final_T, uint32_t* n_contrib) {
  final_T[pix] = T;
  n_contrib[pix] = last;
  out_color[pix] = c0 + T * bg[0]; out_color[HW + pix] = c1 + T * bg[1]; out_color[2 * HW + pix] = c2 + T * bg[2];
  out_da[pix] = depth; out_da[HW + pix] = alpha;
}

// Forward work list: tile ids ordered heaviest-first (length classes of floor(log2(len)) with GSR_ORDER_FRAC_BITS more bits,
// descending; the order inside a class is arbitrary); zeroes tile_depth. Single workgroup.
// Several views at once: workgroup blockIdx.x builds the list of view blockIdx.x (pointer tables in the kernel arguments).
struct WorkFwdViews {
  const uint32_t* ranges[GSR_MAX_BATCH_VIEWS];
  uint32_t* tile_depth[GSR_MAX_BATCH_VIEWS];
  uint32_t* work[GSR_MAX_BATCH_VIEWS];
  uint32_t* stats_host[GSR_MAX_BATCH_VIEWS];
};

// Length classes per octave of the forward work list = 2^GSR_ORDER_FRAC_BITS. Round 6, one call, two interleaved runs each: 1 / 4 /
// 8 classes per octave: K6 44.6 / 44.3 / 44.2 us per view at C3 (value 5 059 / 5 088 / 4 994), 108.4 / 107.6 / 107.8 in the
// opacity-0.1 state -- the heaviest-first order inside an octave is worth half a percent, finer than 4 nothing (gpurun_out/r6f).
#ifndef GSR_ORDER_FRAC_BITS
#define GSR_ORDER_FRAC_BITS 2
#endif
constexpr int kOrderFrac = GSR_ORDER_FRAC_BITS;
constexpr int kOrderClasses = 2 + (32 << kOrderFrac);
__device__ __forceinline__ uint32_t order_class(uint32_t len) {
  if (len == 0u) return 0u;
  const int msb = 31 - __clz(len);
  if constexpr (kOrderFrac == 0) return (uint32_t)msb + 1u;
  const uint32_t frac = (msb >= kOrderFrac ? (len >> (msb - kOrderFrac)) : (len << (kOrderFrac - msb))) & ((1u << kOrderFrac) - 1u);
  return 1u + ((uint32_t)msb << kOrderFrac) + frac;
}
__global__ void __launch_bounds__(1024)
k_work_order_fwd(const uint32_t n_tiles, const WorkFwdViews wv) {
  const uint32_t* __restrict__ ranges = wv.ranges[blockIdx.x];
  uint32_t* __restrict__ tile_depth = wv.tile_depth[blockIdx.x];
  uint32_t* __restrict__ work = wv.work[blockIdx.x];
  uint32_t* __restrict__ stats_host = wv.stats_host[blockIdx.x];
  __shared__ uint32_t cnt[kOrderClasses], cur[kOrderClasses];
  const int tid = threadIdx.x;
  if (tid < kOrderClasses) cnt[tid] = 0;
  __syncthreads();
  for (uint32_t t = tid; t < n_tiles; t += 1024) {
    const uint32_t len = ranges[2 * t + 1] - ranges[2 * t];
    atomicAdd(&cnt[order_class(len)], 1u);
    tile_depth[t] = 0;
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t run = 0;
    for (int b = kOrderClasses - 1; b >= 0; --b) { cur[b] = run; run += cnt[b]; }
    work[n_tiles] = n_tiles - cnt[0];          // number of non-empty tiles (a statistic for the host's mode choice)
    if (stats_host) *stats_host = n_tiles - cnt[0];   // page-locked host word, written straight from the kernel
  }
  __syncthreads();
  for (uint32_t t = tid; t < n_tiles; t += 1024) {
    const uint32_t len = ranges[2 * t + 1] - ranges[2 * t];
    work[atomicAdd(&cur[order_class(len)], 1u)] = t;
  }
}

// Double-buffered staging of 256 list entries. The reach mask of an entry rides in the unused fourth component of its
// third splat row (s2[..].w): 24 KB instead of 29 KB per workgroup = one more workgroup per CU; the Gaussian ids are only
// staged by the score variant.
template <bool SCORE, int PAD = 0>
struct Stage {
  float4 s0[2][kBatch + PAD], s1[2][kBatch + PAD], s2[2][kBatch + PAD];
  uint32_t sid[SCORE ? 2 : 1][SCORE ? kBatch : 1];
  // score variant, pixel counts (score_mode 0 / 2): per staged entry, the pixels of the workgroup's 8x8 quarter that composited
  // it -- added with LDS integer atomics by the four waves while they walk the batch and flushed to the global counters ONCE per
  // batch by the thread that staged the entry (round 5: one global atomic per (wave, step, slot) made k_render_fwd<true> 2.4x
  // the plain kernel: 127 vs 53 us for one view of C3, profiles/r05_score_kernel_stats.txt)
  uint32_t cnt[SCORE ? 2 : 1][SCORE ? kBatch : 1];
};

// --------------------------------------------------------------------------------------------------------- K6
// Forward compositing, "list-parallel lanes": FOUR lanes share a pixel and take four consecutive candidates of
// the list per step:
//   * work item = one 8x8 pixel quarter of a 16x16 tile, handled by a 256-thread workgroup; wave = 4x4 pixels;
//     lane = 16 (pixel row) + 4 slot + pixel column;
//   * each lane evaluates alpha of "its" candidate; the transmittance in front of it is T * (exclusive product
//     of the earlier slots' (1-alpha)) -- three bank-masked DPP multiplies (row_shr:4), no LDS; the T < 1e-4 stop is one
//     comparison per lane; the new T is the minimum over the slots of the survivors' T(1-alpha) (row_ror:4, :8);
//   * colour / depth / alpha partial sums stay per lane and are folded over the slots once, at the end.
// 4x more (and 4x finer) work items, tighter 4x4 culling; same gates in the same list order on the same bits (the
// transmittance is multiplied up in list order inside the quad; only the colour / depth / alpha SUMS associate
// differently from a sequential loop, at the 1e-7 level).
// KB = distance of the checkpoints in list entries (GsrBinning.seg_len: 256, 128 or 64). The batches stay 256 entries long;
// for KB < 256 a wave's candidate list is padded to a multiple of four at every KB boundary inside the batch, so that a
// step never straddles one, and the state is written out when the loop reaches that point.
template <bool SCORE, int KB>
__device__ __forceinline__ void
render_fwd_body(const uint32_t item, const int W, const int H, const uint32_t* __restrict__ work, float* __restrict__ ckpt,
             const uint32_t* __restrict__ ranges,
             const uint32_t* __restrict__ point_list, const float4* __restrict__ splat, const float* __restrict__ bg,
             float* __restrict__ out_color, float* __restrict__ out_da, float* __restrict__ final_T,
             uint32_t* __restrict__ n_contrib, uint32_t* __restrict__ tile_depth, float* __restrict__ score,
             const int score_mode) {
  // Row kBatch of every staged array is a candidate no pixel takes (opacity 0 -> alpha 0 < 1/255): the per-wave candidate
  // lists are padded with it to a multiple of four, so the compositing loop has no partial step.
  __shared__ Stage<SCORE, 1> st;
  __shared__ uint16_t cand[4][kBatch + 16];  // per wave: the batch's candidates for its 4x4 block, in list order (+ padding)
  if (threadIdx.x < 2) {
    st.s0[threadIdx.x][kBatch] = make_float4(0.f, 0.f, 0.f, 0.f);
    st.s1[threadIdx.x][kBatch] = make_float4(0.f, 0.f, 0.f, 0.f);
    st.s2[threadIdx.x][kBatch] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if constexpr (SCORE) { st.cnt[0][threadIdx.x] = 0u; st.cnt[1][threadIdx.x] = 0u; }
  // pixel counts of the batch staged in buffer b -> the global counters (thread t flushes the entry it staged, then clears it)
  auto flush_counts = [&](const int b) {
    if constexpr (SCORE) {
      const uint32_t c = st.cnt[b][threadIdx.x];
      if (c) {
        atomicAdd(reinterpret_cast<uint32_t*>(score) + st.sid[b][threadIdx.x], c);
        st.cnt[b][threadIdx.x] = 0u;
      }
    }
  };
  const int gx = (W + GSR_TILE - 1) / GSR_TILE;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // lane = 16 (pixel row) + 4 slot + (pixel column): the slots of a pixel are the four BANKS of a DPP row, so a step of the
  // transmittance scan is one bank-masked v_mul_f32_dpp row_shr:4 (lanes of the other banks keep their value) instead of a
  // quad_perm multiply plus a select
  const int slot = (lane >> 2) & 3, pcol = lane & 3, prow = lane >> 4;
  const float bg0 = bg[0], bg1 = bg[1], bg2 = bg[2];
  {
    // Workgroup b takes item b of the heaviest-first work list: the hardware dispatcher hands workgroups out in
    // index order as CU slots free up, i.e. it performs longest-processing-time-first scheduling for us.
    const uint32_t tile = work[item >> 2];
    const int quarter = (int)(item & 3u);
    const int ty = (int)tile / gx, tx = (int)tile - ty * gx;
    const int q_x0 = tx * GSR_TILE + (quarter & 1) * 8, q_y0 = ty * GSR_TILE + (quarter >> 1) * 8;
    const int px = q_x0 + (wave & 1) * 4 + pcol, py = q_y0 + (wave >> 1) * 4 + prow;
    const bool inside = (px < W) && (py < H);
    const float pxf = (float)px, pyf = (float)py;
    const uint32_t r0 = ranges[2 * tile], r1 = ranges[2 * tile + 1];
    if (r0 == r1) {
      // empty tile (most of the image around an object): background only. The workgroup of quarter 0 writes the whole
      // 16x16 tile, one pixel per thread; the other three leave (a quarter's full prologue / fold / store path costs
      // ~100 instructions per wave, and four fifths of C3's workgroups are of this kind).
      if (quarter == 0) {
        const int ex = tx * GSR_TILE + (tid & 15), ey = ty * GSR_TILE + (tid >> 4);
        if (ex < W && ey < H) {
          const size_t pix = (size_t)ey * W + ex, HW = (size_t)H * W;
          final_T[pix] = 1.0f;
          n_contrib[pix] = 0u;
          out_color[pix] = bg0; out_color[HW + pix] = bg1; out_color[2 * HW + pix] = bg2;
          out_da[pix] = 0.f; out_da[HW + pix] = 0.f;
        }
      }
      return;
    }

    // pixels that are finished, as a 64-bit lane mask of the wave: all the gate logic below runs on the scalar unit
    unsigned long long donem = __builtin_amdgcn_ballot_w64(!inside);
    float T = 1.0f, C0 = 0.f, C1 = 0.f, C2 = 0.f, Dp = 0.f, Wt = 0.f;
    uint32_t last = 0;

    uint32_t nid = 0;
    float4 n0 = make_float4(0, 0, 0, 0), n1 = n0, n2 = n0;
    if (r0 + tid < r1) gather_splat(point_list, splat, r0 + tid, nid, n0, n1, n2);
    int buf = 0;
    for (uint32_t base = r0; base < r1; base += kBatch, buf ^= 1) {
      const int n = (int)min((uint32_t)kBatch, r1 - base);
      st.s0[buf][tid] = stage_row0(n0);
      st.s1[buf][tid] = stage_row1(n1);
      st.s2[buf][tid] = make_float4(n2.x, n2.y, n2.z,
                                    __uint_as_float((tid < n) ? block_mask_t<4>(n0, n1, n2, q_x0, q_y0) : 0u));
      if constexpr (SCORE) st.sid[buf][tid] = nid;      // (the previous batch's ids and counts live in buffer buf ^ 1)
      const int n_done = __syncthreads_count(__builtin_amdgcn_inverse_ballot_w64(donem));
      // every wave is past the compositing of the previous batch (buffer buf ^ 1): its counts are complete
      if (score_mode != 1 && base != r0) flush_counts(buf ^ 1);
      if (n_done == 256) break;
      // checkpoint of the per-pixel prefix state at list position pos (r0 + a multiple of KB): lets the backward start a
      // traversal there (k_render_bwd splits deep tiles into independent segments of KB entries)
      auto checkpoint = [&](const uint32_t pos) {
        if (ckpt == nullptr) return;     // forward only (GsrImages.ckpt NULL): nobody will start a backward traversal here
        const float f0 = fold_slots(C0), f1 = fold_slots(C1), f2 = fold_slots(C2), f3 = fold_slots(Dp), f4 = fold_slots(Wt);
        if (slot == 0 && inside) {
          float* ck = ckpt_row<KB>(ckpt, pos, py, ty * GSR_TILE, px, tx * GSR_TILE);
          ck[0] = T; ck[256] = f0; ck[512] = f1; ck[768] = f2; ck[1024] = f3; ck[1280] = f4;
        }
      };
      if (base != r0) checkpoint(base);
      if (base + kBatch + tid < r1) gather_splat(point_list, splat, base + kBatch + tid, nid, n0, n1, n2);
      // this wave's candidates of the batch (entries whose reach mask has the wave's 4x4 block), compacted in list
      // order into a byte list of its own: the compositing loop then reads "its" candidate with one LDS load instead
      // of peeling four bits off a 64-bit scalar mask per step, and only the last step of a batch can be partial
      int cnt = 0;
      int cut_at[3] = {-1, -1, -1};        // step index of the KB boundaries inside the batch (KB < 256)
#pragma unroll
      for (int k = 0; k < kBatch / 64; ++k) {
        if (k * 64 >= n) break;
        const bool m = (stage_mask(st.s2[buf][k * 64 + lane]) >> wave) & 1u;
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(m);
        if (m) cand[wave][cnt + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))] = (uint8_t)(k * 64 + lane);
        cnt += (int)__popcll(bal);
        if constexpr (KB < kBatch) {
          if (((k + 1) * 64) % KB == 0 && k + 1 < kBatch / 64 && (k + 1) * 64 < n) {
            const int pad = (-cnt) & 3;
            if (lane < pad) cand[wave][cnt + lane] = (uint16_t)kBatch;
            cnt += pad;
            cut_at[(k + 1) * 64 / KB - 1] = cnt;
          }
        }
      }
      if (lane < 3) cand[wave][cnt + lane] = (uint16_t)kBatch;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      {
        for (int i = 0;; i += 4) {
          if (donem == ~0ull) break;       // (no pixel of the wave composites any further: nobody reads its checkpoints)
          if constexpr (KB < kBatch) {
#pragma unroll
            for (int c = 0; c < kBatch / KB - 1; ++c)
              if (i == cut_at[c]) checkpoint(base + (uint32_t)((c + 1) * KB));
          }
          if (i >= cnt) break;
          const int j = (int)cand[wave][i + slot];
          const float4 a = st.s0[buf][j];
          const float4 b = st.s1[buf][j];
          const float2 c = *reinterpret_cast<const float2*>(&st.s2[buf][j]);
          const float dx = a.x - pxf, dy = a.y - pyf;
          const float power = gsr_power(a.z, a.w, b.x, dx, dy);
          const float alpha = fminf(GSR_ALPHA_MAX, gsr_mul(b.y, gsr_exp(power)));
          const unsigned long long gm = ~donem & __builtin_amdgcn_ballot_w64(power <= 0.0f) &
                                        __builtin_amdgcn_ballot_w64(alpha >= GSR_ALPHA_MIN);
          const bool g = __builtin_amdgcn_inverse_ballot_w64(gm);
          // transmittance after this slot, multiplied up in LIST ORDER -- ((T f0) f1) f2 ... with f = 1 - alpha of a
          // gated slot, 1 otherwise -- so that it carries the bits of the sequential recurrence T <- T (1 - alpha) (the
          // T < 1e-4 stop is a hard gate: SEMANTICS.md section 4). Three dependent quad steps: after step k slot k is final.
          const float fgate = g ? gsr_sub(1.0f, alpha) : 1.0f;
          float test_T = gsr_mul(T, fgate);
          // (each step: the lanes of slots >= k take test_T of slot - 1 times their own factor; s_nop: a DPP operand needs two
          //  wait states after its producer and the hazard recognizer does not look inside an asm block)
          asm("s_nop 1\n\t"
              "v_mul_f32_dpp %0, %0, %1 row_shr:4 row_mask:0xf bank_mask:0xe\n\t"
              "s_nop 1\n\t"
              "v_mul_f32_dpp %0, %0, %1 row_shr:4 row_mask:0xf bank_mask:0xc\n\t"
              "s_nop 1\n\t"
              "v_mul_f32_dpp %0, %0, %1 row_shr:4 row_mask:0xf bank_mask:0x8"
              : "+v"(test_T) : "v"(fgate));
          // alpha times the transmittance in FRONT of the slot: T for slot 0, test_T of slot - 1 for the others
          float w_all = alpha * T;
          asm("s_nop 1\n\t"
              "v_mul_f32_dpp %0, %1, %2 row_shr:4 row_mask:0xf bank_mask:0xe"
              : "+v"(w_all) : "v"(test_T), "v"(alpha));
          // The first slot (in list order) whose own contribution would drop T below the threshold stops the pixel, it
          // and everything behind it. A pixel still in play holds T >= 1e-4 and the slots' test_T only decrease along the
          // list (factors <= 1, one rounding each), so "a gated slot <= mine fell below the threshold" IS "my test_T is
          // below it": no scan over the quad, and the quad's stop flag is slot 3's comparison.
          const unsigned long long stopm = __builtin_amdgcn_ballot_w64(test_T < GSR_T_MIN);
          const bool hit = __builtin_amdgcn_inverse_ballot_w64(gm & ~stopm);
          const float w = hit ? w_all : 0.0f;
          C0 = fmaf(b.w, w, C0); C1 = fmaf(c.x, w, C1); C2 = fmaf(c.y, w, C2);
          Dp = fmaf(b.z, w, Dp);
          Wt += w;
          last = hit ? ((base - r0) + (uint32_t)j + 1u) : last;
          if constexpr (SCORE) {
            // the pixels of the wave that composite slot s's splat: the 16 lanes holding this slot
            const unsigned long long hm = __ballot(hit) & (0x000F000F000F000Full << (4 * slot));
            if (score_mode != 1) {
              // weight = opacity per contributing (pixel, splat): the kernel counts the pixels -- integer atomics, exact and
              // independent of the order -- and k_score_finalize multiplies by the opacity once (mode 0) or the caller does
              // (mode 2: raw counts, summed over many views first). A float sum of thousands of EQUAL increments rounds the
              // same way every time (measured 6e-5 relative on the sum over 48 views).
              // (LDS integer atomic: the four waves of the quarter meet in one counter per staged entry; the padding row
              //  kBatch never hits: alpha 0)
              if (hm != 0ull && lane == 4 * slot) atomicAdd(&st.cnt[buf][j & (kBatch - 1)], (uint32_t)__popcll(hm));
            } else {
              float ws = w;                               // sum over the lanes sharing the slot: xor 1, 2, 16, 32
              ws += gsr_dpp<0xB1>(ws);                    // quad_perm [1,0,3,2]
              ws += gsr_dpp<0x4E>(ws);                    // quad_perm [2,3,0,1]
              ws += __shfl_xor(ws, 16, 64);
              ws += __shfl_xor(ws, 32, 64);
              if (hm != 0ull && lane == 4 * slot) unsafeAtomicAdd(score + st.sid[buf][j & (kBatch - 1)], ws);
            }
          }
          // T after the quad: the survivors' T(1-alpha) only decrease along the list -> quad minimum (T >= 1e-4 > 0:
          // the order of positive floats is the order of their bit patterns, and v_min_u32 takes a DPP operand)
          uint32_t tn = __float_as_uint(hit ? test_T : T);
          tn = min(tn, (uint32_t)gsr_dpp_i<0x124>((int)tn));   // row_ror:4
          tn = min(tn, (uint32_t)gsr_dpp_i<0x128>((int)tn));   // row_ror:8
          T = __uint_as_float(tn);
          // slot 3's flag -> all four lanes of its quad. On the SCALAR unit: its instructions issue beside the vector
          // instructions of the other waves (removing 22 of them from this loop changed nothing: A/B in one gpurun call,
          // 44.0 vs 45.0 us per view -- the loop is bound by its ~50 vector instructions), so mask arithmetic belongs there
          unsigned long long quad_stop = (stopm >> 12) & 0x000F000F000F000Full;
          quad_stop |= quad_stop << 4;
          quad_stop |= quad_stop << 8;
          donem |= quad_stop;
        }
      }
    }
    if constexpr (SCORE) {
      // the counts of the last batch that was composited (buffer buf ^ 1 after the loop's own flip; all zero when the loop left
      // through the "everything finished" exit, whose flush ran already)
      __syncthreads();
      if (score_mode != 1) flush_counts(buf ^ 1);
    }
    // fold the four slots of each pixel
    C0 = fold_slots(C0); C1 = fold_slots(C1); C2 = fold_slots(C2); Dp = fold_slots(Dp); Wt = fold_slots(Wt);
    {
      int l = (int)last;
      l = max(l, gsr_dpp_i<0x124>(l));
      l = max(l, gsr_dpp_i<0x128>(l));
      last = (uint32_t)l;
    }
    if (inside && slot == 0) {
      const size_t pix = (size_t)py * W + px, HW = (size_t)H * W;
      store_pixel(pix, HW, T, last, C0, C1, C2, Dp, Wt, bg, out_color, out_da, final_T, n_contrib);
    }
    // deepest contributor of the tile: the backward's cost key and its starting depth
    const uint32_t wm = gsr_wave_max_u32(last);
    if (lane == 0 && wm) atomicMax(tile_depth + tile, wm);
  }
}

// K6, whole-tile variant: work item = one 16x16 tile, 4 waves = four 8x8 blocks, ONE pixel per lane. It spends the
// fewest instructions per (pixel, splat) evaluation (about half of the list-parallel kernel) and is the right
// choice when thousands of similar, shallow tiles saturate the machine (camera inside a room: every tile active,
// ~250 entries each); with few, deep tiles its long per-pixel chains make the tail (1 M Gaussians at 512^2:
// 377 us vs 124 us). The host picks the variant per call from the previous view's statistics
// (GsrBinning.fwd_mode); both produce the same images up to the association of the transmittance product.
template <bool SCORE>
__device__ __forceinline__ void
render_fwd_tile_body(const uint32_t item, const int W, const int H, const uint32_t* __restrict__ work, float* __restrict__ ckpt,
                  const uint32_t* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                  const float4* __restrict__ splat, const float* __restrict__ bg, float* __restrict__ out_color,
                  float* __restrict__ out_da, float* __restrict__ final_T, uint32_t* __restrict__ n_contrib,
                  uint32_t* __restrict__ tile_depth, float* __restrict__ score, const int score_mode) {
  __shared__ Stage<SCORE> st;
  const int gx = (W + GSR_TILE - 1) / GSR_TILE;
  const int tile = (int)work[item];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const TilePix p = tile_pixel(tile, gx, W, H);
  const int tile_x0 = p.bx - (wave & 1) * 8, tile_y0 = p.by - (wave >> 1) * 8;
  const float pxf = (float)p.px, pyf = (float)p.py;
  const uint32_t r0 = ranges[2 * tile], r1 = ranges[2 * tile + 1];
  unsigned long long donem = __builtin_amdgcn_ballot_w64(!p.inside);   // finished pixels, as a lane mask
  float T = 1.0f, C0 = 0.f, C1 = 0.f, C2 = 0.f, Dp = 0.f, Wt = 0.f;
  uint32_t last = 0;
  uint32_t nid = 0;
  float4 n0 = make_float4(0, 0, 0, 0), n1 = n0, n2 = n0;
  if (r0 + tid < r1) {      // (gather_splat, spelled out: see there)
    nid = point_list[r0 + tid];
    const float4* r = splat + 3 * (size_t)nid;
    n0 = r[0]; n1 = r[1]; n2 = r[2];
  }
  int buf = 0;
  for (uint32_t base = r0; base < r1; base += kBatch, buf ^= 1) {
    const int n = (int)min((uint32_t)kBatch, r1 - base);
    st.s0[buf][tid] = stage_row0(n0);
    st.s1[buf][tid] = stage_row1(n1);
    st.s2[buf][tid] = make_float4(n2.x, n2.y, n2.z,
                                  __uint_as_float((tid < n) ? block_mask_t<8>(n0, n1, n2, tile_x0, tile_y0) : 0u));
    if constexpr (SCORE) st.sid[buf][tid] = nid;
    if (__syncthreads_count(__builtin_amdgcn_inverse_ballot_w64(donem)) == 256) break;
    if (base != r0 && p.inside && ckpt != nullptr) {
      float* ck = ckpt_row<kBatch>(ckpt, base, p.py, tile_y0, p.px, tile_x0);
      ck[0] = T; ck[256] = C0; ck[512] = C1; ck[768] = C2; ck[1024] = Dp; ck[1280] = Wt;
    }
    {
      const uint32_t idx = base + kBatch + tid;
      if (idx < r1) {
        nid = point_list[idx];
        const float4* r = splat + 3 * (size_t)nid;
        n0 = r[0]; n1 = r[1]; n2 = r[2];
      }
    }
    for (int k = 0; k < kBatch / 64; ++k) {
      if (k * 64 >= n) break;
      unsigned long long bits = __ballot((stage_mask(st.s2[buf][k * 64 + lane]) >> wave) & 1u);
      while (bits) {
        if (donem == ~0ull) break;
        const int j = k * 64 + __builtin_ctzll(bits);
        bits &= bits - 1ull;
        const float4 a = st.s0[buf][j];
        const float4 b = st.s1[buf][j];
        const float4 c = st.s2[buf][j];
        const float dx = a.x - pxf, dy = a.y - pyf;
        const float power = gsr_power(a.z, a.w, b.x, dx, dy);
        const float alpha = fminf(GSR_ALPHA_MAX, gsr_mul(b.y, gsr_exp(power)));
        const float test_T = gsr_mul(T, gsr_sub(1.0f, alpha));
        const unsigned long long gm = ~donem & __builtin_amdgcn_ballot_w64(power <= 0.0f) &
                                      __builtin_amdgcn_ballot_w64(alpha >= GSR_ALPHA_MIN);
        const unsigned long long stopm = gm & __builtin_amdgcn_ballot_w64(test_T < GSR_T_MIN);
        donem |= stopm;
        const bool hit = __builtin_amdgcn_inverse_ballot_w64(gm & ~stopm);
        const float w = hit ? alpha * T : 0.0f;
        if constexpr (SCORE) {
          const unsigned long long hm = __ballot(hit);       // one atomic per (wave, splat), not per pixel
          if (hm) {
            if (score_mode != 1) {      // pixel counts, integer atomics (see render_fwd_body)
              if (lane == 0) atomicAdd(reinterpret_cast<uint32_t*>(score) + st.sid[buf][j], (uint32_t)__popcll(hm));
            } else {
              float sc = gsr_wave_sum_to_lane63(w);
              sc = __shfl(sc, 63, 64);
              if (lane == 0) unsafeAtomicAdd(score + st.sid[buf][j], sc);
            }
          }
        }
        C0 = fmaf(b.w, w, C0); C1 = fmaf(c.x, w, C1); C2 = fmaf(c.y, w, C2);
        Dp = fmaf(b.z, w, Dp);
        Wt += w;
        T = hit ? test_T : T;
        last = hit ? ((base - r0) + (uint32_t)j + 1u) : last;
      }
    }
  }
  if (p.inside) {
    const size_t pix = (size_t)p.py * W + p.px, HW = (size_t)H * W;
    store_pixel(pix, HW, T, last, C0, C1, C2, Dp, Wt, bg, out_color, out_da, final_T, n_contrib);
  }
  const uint32_t wm = gsr_wave_max_u32(last);
  if (lane == 0 && wm) atomicMax(tile_depth + tile, wm);
}

}  // namespace

// ---- kernels: 1-D grids over (work item, view), see item_view. Pointer tables in the kernel arguments; one view = tables of one
struct FwdViews {
  const uint32_t* work[GSR_MAX_BATCH_VIEWS];
  float* ckpt[GSR_MAX_BATCH_VIEWS];
  const uint32_t* ranges[GSR_MAX_BATCH_VIEWS];
  const uint32_t* point_list[GSR_MAX_BATCH_VIEWS];
  const float4* splat[GSR_MAX_BATCH_VIEWS];
  const float* bg[GSR_MAX_BATCH_VIEWS];
  float* out_color[GSR_MAX_BATCH_VIEWS];
  float* out_da[GSR_MAX_BATCH_VIEWS];
  float* final_T[GSR_MAX_BATCH_VIEWS];
  uint32_t* n_contrib[GSR_MAX_BATCH_VIEWS];
  uint32_t* tile_depth[GSR_MAX_BATCH_VIEWS];
  float* score[GSR_MAX_BATCH_VIEWS];
};

template <bool SCORE, int KB = kBatch>
__global__ void __launch_bounds__(256)
k_render_fwd(const int W, const int H, const FwdViews fv, const int score_mode, const uint32_t n_views,
             const uint32_t per_view) {
  const auto [item, y] = item_view(n_views, per_view);
  render_fwd_body<SCORE, KB>(item, W, H, fv.work[y], fv.ckpt[y], fv.ranges[y], fv.point_list[y], fv.splat[y], fv.bg[y],
                         fv.out_color[y], fv.out_da[y], fv.final_T[y], fv.n_contrib[y], fv.tile_depth[y], fv.score[y],
                         score_mode);
}
template <bool SCORE>
__global__ void __launch_bounds__(256)
k_render_fwd_tile(const int W, const int H, const FwdViews fv, const int score_mode, const uint32_t n_views,
                  const uint32_t per_view) {
  const auto [item, y] = item_view(n_views, per_view);
  render_fwd_tile_body<SCORE>(item, W, H, fv.work[y], fv.ckpt[y], fv.ranges[y], fv.point_list[y], fv.splat[y], fv.bg[y],
                              fv.out_color[y], fv.out_da[y], fv.final_T[y], fv.n_contrib[y], fv.tile_depth[y],
                              fv.score[y], score_mode);
}

// The stage timer (GSR_STAGE_RENDER_FWD) brackets the compositing kernel alone (not the work-list kernel), so that
// bench.py's roofline entry and the rocprofv3 average of that kernel measure the same thing.
// Work lists of n views (same image size) in one launch.
int gsr_launch_work_order_fwd(int n, const GsrView* views, const GsrBinning* bs, const GsrImages* imgs, hipStream_t stream) {
  const uint32_t tiles = gsr_num_tiles(views[0].image_height, views[0].image_width);
  WorkFwdViews wv = WorkFwdViews{};
  for (int k = 0; k < n; ++k) {
    wv.ranges[k] = bs[k].ranges; wv.tile_depth[k] = imgs[k].tile_depth; wv.work[k] = bs[k].tile_work;
    wv.stats_host[k] = bs[k].stats_host;
  }
  hipLaunchKernelGGL(k_work_order_fwd, dim3((uint32_t)n), dim3(1024), 0, stream, tiles, wv);
  GSR_HIP(hipGetLastError());
  return GSR_OK;
}

// score_mode 0: pixel counts (u32, left by K6 in the score buffer) -> opacity x count, in place
struct ScoreViews {
  float* score[GSR_MAX_BATCH_VIEWS];
  const float* splat[GSR_MAX_BATCH_VIEWS];
  const int32_t* radii[GSR_MAX_BATCH_VIEWS];
};
namespace {
__global__ void __launch_bounds__(256) k_score_finalize(const ScoreViews sv, const int32_t P) {
  const int32_t i = (int32_t)(blockIdx.x * 256u + threadIdx.x);
  if (i >= P) return;
  float* sc = sv.score[blockIdx.y];
  const uint32_t c = reinterpret_cast<const uint32_t*>(sc)[i];
  // (rows of culled Gaussians are never written: their count is 0 and their opacity is not read)
  sc[i] = (c && sv.radii[blockIdx.y][i] > 0) ? sv.splat[blockIdx.y][12 * (size_t)i + 5] * (float)c : 0.0f;
}
}  // namespace

// K6 of n views in one launch (their work lists must have been built; same image size, forward variant and score
// output for all of them -- the caller checks).
int gsr_launch_render_fwd_views(int n, const GsrView* views, const GsrGeom* geoms, const GsrBinning* bs, GsrImages* imgs,
                                hipStream_t stream, GsrProfile* prof) {
  const GsrView& v = views[0];
  const uint32_t tiles = gsr_num_tiles(v.image_height, v.image_width);
  FwdViews fv = FwdViews{};
  for (int k = 0; k < n; ++k) {
    fv.work[k] = bs[k].tile_work; fv.ckpt[k] = imgs[k].ckpt; fv.ranges[k] = bs[k].ranges;
    fv.point_list[k] = bs[k].point_list; fv.splat[k] = reinterpret_cast<const float4*>(geoms[k].splat);
    fv.bg[k] = views[k].bg; fv.out_color[k] = imgs[k].color; fv.out_da[k] = imgs[k].depth_alpha;
    fv.final_T[k] = imgs[k].final_T; fv.n_contrib[k] = imgs[k].n_contrib; fv.tile_depth[k] = imgs[k].tile_depth;
    fv.score[k] = imgs[k].important_score;
  }
  const bool score = imgs[0].important_score != nullptr;
  const uint32_t ny = (uint32_t)n;
  const bool whole_tile = bs[0].fwd_mode == 1;     // (checkpoints every kBatch entries only: one instantiation per SCORE)
  auto launch = [&](auto sc, auto kb) {
    const int score_mode = sc ? v.score_mode : 0;
    const int W = v.image_width, H = v.image_height;
    if (whole_tile) hipLaunchKernelGGL(k_render_fwd_tile<sc>, dim3(tiles * ny), dim3(256), 0, stream, W, H, fv, score_mode, ny, tiles);
    else hipLaunchKernelGGL((k_render_fwd<sc, kb>), dim3(tiles * 4 * ny), dim3(256), 0, stream, W, H, fv, score_mode, ny, 0u);
  };
  GsrStageTimer timer(prof, stream, GSR_STAGE_RENDER_FWD);
  const int rc = launch_kb<64, 128, 256>(gsr_seg_len(bs[0]), [&](auto kb) {
    if (score) launch(std::true_type{}, kb);
    else launch(std::false_type{}, kb);
  });
  if (rc) return rc;
  timer.stop();
  if (score && v.score_mode == 0 && v.P > 0) {
    ScoreViews sv = ScoreViews{};
    for (int k = 0; k < n; ++k) { sv.score[k] = imgs[k].important_score; sv.splat[k] = geoms[k].splat; sv.radii[k] = geoms[k].radii; }
    hipLaunchKernelGGL(k_score_finalize, dim3(((uint32_t)v.P + 255u) / 256u, ny), dim3(256), 0, stream, sv, v.P);
    GSR_HIP(hipGetLastError());
  }
  return GSR_OK;
}

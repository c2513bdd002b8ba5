// sample.hip -- the point clouds a new model starts from, drawn on the device from (seed, cloud, index), gfx950
// (include/gsrast.h, "seeded point clouds"; dreamscene_amd/pointcloud.py; SEMANTICS.md section 17). The reference draws them on the
// host with numpy's float64 stream (gs_renderer.py:218-408); here a row is a pure function of its counter, so every replica that
// holds the seed holds the same cloud and nothing crosses the bus.
//   k_env_indoor     five wall sheets of n rows each around a box read from DEVICE memory (:221-248)
//   k_floor_indoor   one sheet under the box (:282-296)
//   k_shell          env outdoor: the shell 0.95 <= mu <= 1.05 of a sphere, upper half with zero_ground (:250-275)
//   k_disc           floor outdoor: a disc of thickness 0.1 under box[2] (:298-319)
//   k_ball           the `default` object cloud: a uniform ball with SH-range colours (:353-376)
//   k_jitter         the `pointe` object cloud: `copies` shared offsets around every seed point (:380-408)
//   k_tri_area, k_mesh, k_center   the `shapes` object cloud: area-weighted points on a triangle mesh (:328-345)
// Randomness: philox4x32_10 and u01 of gsr_rng.h only; counter (i, block, cloud id, 3); uniform e of a row is slot e % 4 of block
// e / 4. One thread per index i, 256-thread blocks, a bounds check on the tail, no LDS, no atomics, nothing allocated. All
// arithmetic is fp32 in the written order (built with -ffp-contract=off); `/` is IEEE division; sqrtf, cbrtf, sinf and cosf are
// the full-precision forms. The work is a few MB of dword stores behind one launch: launch latency, not bandwidth, is what it
// costs, and the 12-byte rows are left as three dword stores (adjacent lanes fill every cache line between them).
#include "gsr_common.h"
#include "gsr_rng.h"

namespace {

constexpr int kT = 256;
constexpr uint32_t kTagSample = 3u;              // disjoint from densify (0), scale noise (1) and SH noise (2) under one seed
constexpr float kC0 = 0.28209479177387814f;      // gsr_model_init's
constexpr float kTwoPi = 6.283185307179586f;
constexpr float kPi = 3.141592653589793f;

// uniforms 4j .. 4j+3 of (seed, cloud, i)
__device__ __forceinline__ void uniforms4(uint32_t k0, uint32_t k1, uint32_t cloud, uint32_t i, uint32_t j, float u[4]) {
  uint32_t r[4];
  philox4x32_10(i, j, cloud, kTagSample, k0, k1, r);
#pragma unroll
  for (int s = 0; s < 4; ++s) u[s] = u01(r[s]);
}

__device__ __forceinline__ void store3(float* __restrict__ p, size_t row, float x, float y, float z) {
  p[3 * row] = x; p[3 * row + 1] = y; p[3 * row + 2] = z;
}

// a point of the sphere of radius r: direction (cos of the polar angle c, azimuth phi)
__device__ __forceinline__ void sphere_point(float r, float c, float phi, float out[3]) {
  const float s = sqrtf(fmaxf(0.f, 1.f - c * c));
  out[0] = r * s * cosf(phi);
  out[1] = r * s * sinf(phi);
  out[2] = r * c;
}

__global__ void __launch_bounds__(kT) k_env_indoor(const uint32_t k0, const uint32_t k1, const float* __restrict__ box,
                                                   const uint32_t n, float* __restrict__ points, float* __restrict__ colors) {
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  float a[4], b[4], c[4];
  uniforms4(k0, k1, GSR_CLOUD_ENV, i, 0, a);     // jl0 jl1 jl2 jh0
  uniforms4(k0, k1, GSR_CLOUD_ENV, i, 1, b);     // jh1 jh2 ux uy
  uniforms4(k0, k1, GSR_CLOUD_ENV, i, 2, c);     // uz
  float bx[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) bx[k] = box[k];
  const float lo_x = bx[0] - a[0] / 50.f, lo_y = bx[1] - a[1] / 50.f;
  const float hi_x = bx[3] + a[3] / 50.f, hi_y = bx[4] + b[0] / 50.f, hi_z = bx[5] + b[1] / 50.f;
  const float xs = b[2] * (bx[3] - bx[0]) + bx[0];
  const float ys = b[3] * (bx[4] - bx[1]) + bx[1];
  const float zs = c[0] * (bx[5] - bx[2]) + bx[2];
  const size_t N = n;
  store3(points, i, lo_x, ys, zs);
  store3(points, N + i, hi_x, ys, zs);
  store3(points, 2 * N + i, xs, lo_y, zs);
  store3(points, 3 * N + i, xs, hi_y, zs);
  store3(points, 4 * N + i, xs, ys, hi_z);
  store3(colors, i, 0.5f, 0.5f, 0.5f);
  store3(colors, N + i, 0.5f, 0.5f, 0.5f);
  store3(colors, 2 * N + i, 0.7f, 0.7f, 0.7f);
  store3(colors, 3 * N + i, 0.7f, 0.7f, 0.7f);
  store3(colors, 4 * N + i, 0.9f, 0.9f, 0.9f);
}

__global__ void __launch_bounds__(kT) k_floor_indoor(const uint32_t k0, const uint32_t k1, const float* __restrict__ box,
                                                     const float cr, const float cg, const float cb, const uint32_t n,
                                                     float* __restrict__ points, float* __restrict__ colors) {
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  float u[4];
  uniforms4(k0, k1, GSR_CLOUD_FLOOR, i, 0, u);   // jz ux uy
  const float x0 = box[0], y0 = box[1], z0 = box[2];
  const float xs = u[1] * (box[3] - x0) + x0;
  const float ys = u[2] * (box[4] - y0) + y0;
  store3(points, i, xs, ys, z0 + u[0] / 50.f - 0.01f);
  store3(colors, i, cr, cg, cb);
}

__global__ void __launch_bounds__(kT) k_shell(const uint32_t k0, const uint32_t k1, const float radius, const int zero_ground,
                                              const float cr, const float cg, const float cb, const uint32_t n,
                                              float* __restrict__ points, float* __restrict__ colors) {
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  float u[4], p[3];
  uniforms4(k0, k1, GSR_CLOUD_ENV, i, 0, u);     // phi, cos(theta), mu
  const float phi = kTwoPi * u[0];
  const float c = zero_ground ? u[1] : 2.f * u[1] - 1.f;
  const float mu = u[2] / 10.f + 0.95f;
  sphere_point(radius * cbrtf(mu), c, phi, p);
  store3(points, i, p[0], p[1], p[2]);
  store3(colors, i, cr, cg, cb);
}

__global__ void __launch_bounds__(kT) k_disc(const uint32_t k0, const uint32_t k1, const float radius, const float z0,
                                             const float cr, const float cg, const float cb, const uint32_t n,
                                             float* __restrict__ points, float* __restrict__ colors) {
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  float u[4];
  uniforms4(k0, k1, GSR_CLOUD_FLOOR, i, 0, u);   // mu, phi, z
  const float r = radius * sqrtf(u[0]), phi = kTwoPi * u[1];
  store3(points, i, r * cosf(phi), r * sinf(phi), u[2] / 10.f - 0.1f + z0);
  store3(colors, i, cr, cg, cb);
}

__device__ __forceinline__ float sh_colour(float u) { return u / 255.f * kC0 + 0.5f; }

__global__ void __launch_bounds__(kT) k_ball(const uint32_t k0, const uint32_t k1, const float radius, const uint32_t n,
                                             float* __restrict__ points, float* __restrict__ colors) {
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  float a[4], b[4], p[3];
  uniforms4(k0, k1, GSR_CLOUD_BALL, i, 0, a);    // phi, cos(theta), mu, sh0
  uniforms4(k0, k1, GSR_CLOUD_BALL, i, 1, b);    // sh1, sh2
  sphere_point(radius * cbrtf(a[2]), 2.f * a[1] - 1.f, kTwoPi * a[0], p);
  store3(points, i, p[0], p[1], p[2]);
  store3(colors, i, sh_colour(a[3]), sh_colour(b[0]), sh_colour(b[1]));
}

// row = seed point * copies + copy. The offset of a copy is the same for every seed point (cloud 3, index = copy); the three
// colour uniforms are the row's own (cloud 4, index = row).
__global__ void __launch_bounds__(kT) k_jitter(const uint32_t k0, const uint32_t k1, const float* __restrict__ seed_points,
                                               const float* __restrict__ seed_colors, const uint32_t rows, const uint32_t copies,
                                               const float radius, float* __restrict__ points, float* __restrict__ colors) {
  const uint32_t row = blockIdx.x * kT + threadIdx.x;
  if (row >= rows) return;
  const uint32_t i = row / copies, copy = row - i * copies;
  float o[4], u[4];
  uniforms4(k0, k1, GSR_CLOUD_JITTER_OFFSETS, copy, 0, o);     // theta, phi, rho
  uniforms4(k0, k1, GSR_CLOUD_JITTER_COLORS, row, 0, u);
  const float theta = kPi * o[0], phi = kTwoPi * o[1], rho = radius * o[2];
  const float st = sinf(theta);
  const float ox = rho * st * sinf(phi), oy = rho * st * cosf(phi), oz = rho * cosf(theta);
  const size_t s = 3 * (size_t)i;
  store3(points, row, seed_points[s] + ox, -seed_points[s + 1] + oy, seed_points[s + 2] + 0.15f + oz);
  if (seed_colors) {
    store3(colors, row, seed_colors[s] + 1e-4f * u[0], seed_colors[s + 1] + 1e-4f * u[1], seed_colors[s + 2] + 1e-4f * u[2]);
  } else {
    store3(colors, row, sh_colour(u[0]), sh_colour(u[1]), sh_colour(u[2]));
  }
}

__device__ __forceinline__ bool face_ok(const int32_t* __restrict__ f, int32_t n_vertices) {
  return (uint32_t)f[0] < (uint32_t)n_vertices && (uint32_t)f[1] < (uint32_t)n_vertices && (uint32_t)f[2] < (uint32_t)n_vertices;
}

// area[t] in double (what torch.cumsum then adds up); a face that names a vertex outside [0, n_vertices) has area 0 and is
// never chosen
__global__ void __launch_bounds__(kT) k_tri_area(const float* __restrict__ vertices, const int32_t n_vertices,
                                                 const int32_t* __restrict__ faces, const uint32_t n_faces,
                                                 double* __restrict__ area) {
  const uint32_t t = blockIdx.x * kT + threadIdx.x;
  if (t >= n_faces) return;
  const int32_t* f = faces + 3 * (size_t)t;
  if (!face_ok(f, n_vertices)) { area[t] = 0.0; return; }
  const float* a = vertices + 3 * (size_t)f[0];
  const float* b = vertices + 3 * (size_t)f[1];
  const float* c = vertices + 3 * (size_t)f[2];
  const float e0x = b[0] - a[0], e0y = b[1] - a[1], e0z = b[2] - a[2];
  const float e1x = c[0] - a[0], e1y = c[1] - a[1], e1z = c[2] - a[2];
  const float nx = e0y * e1z - e0z * e1y, ny = e0z * e1x - e0x * e1z, nz = e0x * e1y - e0y * e1x;
  area[t] = (double)(0.5f * sqrtf(nx * nx + ny * ny + nz * nz));
}

// cdf [n_faces]: non-decreasing, cdf[n_faces - 1] == 1. The triangle of u is the first t with u < cdf[t].
__global__ void __launch_bounds__(kT) k_mesh(const uint32_t k0, const uint32_t k1, const float* __restrict__ vertices,
                                             const int32_t n_vertices, const int32_t* __restrict__ faces, const uint32_t n_faces,
                                             const double* __restrict__ cdf, const uint32_t n, float* __restrict__ points,
                                             float* __restrict__ colors, int32_t* __restrict__ triangle) {
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  float a4[4], b4[4];
  uniforms4(k0, k1, GSR_CLOUD_MESH, i, 0, a4);   // triangle, u1, u2, sh0
  uniforms4(k0, k1, GSR_CLOUD_MESH, i, 1, b4);   // sh1, sh2
  const double u = (double)a4[0];
  uint32_t lo = 0, hi = n_faces - 1;             // the answer is in [lo, hi]
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (u < cdf[mid]) hi = mid; else lo = mid + 1;
  }
  const int32_t* f = faces + 3 * (size_t)lo;
  float x = 0.f, y = 0.f, z = 0.f;
  if (face_ok(f, n_vertices)) {
    const float q = sqrtf(a4[1]);
    const float wa = 1.f - q, wb = q * (1.f - a4[2]), wc = q * a4[2];
    const float* va = vertices + 3 * (size_t)f[0];
    const float* vb = vertices + 3 * (size_t)f[1];
    const float* vc = vertices + 3 * (size_t)f[2];
    x = wa * va[0] + wb * vb[0] + wc * vc[0];
    y = wa * va[1] + wb * vb[1] + wc * vc[1];
    z = wa * va[2] + wb * vb[2] + wc * vc[2];
  }
  store3(points, i, x, z, y);                    // the reference's axis swap
  store3(colors, i, sh_colour(a4[3]), sh_colour(b4[0]), sh_colour(b4[1]));
  if (triangle) triangle[i] = (int32_t)lo;
}

// points[i] = (points[i] - fl32(mean)) / 80
__global__ void __launch_bounds__(kT) k_center(const double* __restrict__ mean, const uint32_t n, float* __restrict__ points) {
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const float mx = (float)mean[0], my = (float)mean[1], mz = (float)mean[2];
  store3(points, i, (points[3 * (size_t)i] - mx) / 80.f, (points[3 * (size_t)i + 1] - my) / 80.f,
         (points[3 * (size_t)i + 2] - mz) / 80.f);
}

bool bad4(const void* p) { return !p || ((uintptr_t)p & 3u) != 0; }
bool bad8(const void* p) { return !p || ((uintptr_t)p & 7u) != 0; }
uint32_t blocks_for(uint32_t n) { return (n + kT - 1u) / kT; }
// rows of 3 floats up to the 32-bit row counter of the generator
bool bad_count(int64_t rows) { return rows <= 0 || rows > (int64_t)INT32_MAX; }

}  // namespace

#define GSR_SAMPLE_LAUNCH(kernel, n, ...)                                                                          \
  do {                                                                                                             \
    hipLaunchKernelGGL(kernel, dim3(blocks_for((uint32_t)(n))), dim3(kT), 0, (hipStream_t)stream_, __VA_ARGS__);   \
    GSR_HIP(hipGetLastError());                                                                                    \
  } while (0)

extern "C" int gsr_sample_env_indoor(uint64_t seed, const float* box, int32_t n, float* points, float* colors, void* stream_) {
  if (bad_count(5 * (int64_t)n) || bad4(box) || bad4(points) || bad4(colors)) return GSR_EINVAL;
  GsrDeviceGuard dev(points);
  GSR_SAMPLE_LAUNCH(k_env_indoor, n, (uint32_t)seed, (uint32_t)(seed >> 32), box, (uint32_t)n, points, colors);
  return GSR_OK;
}

extern "C" int gsr_sample_floor_indoor(uint64_t seed, const float* box, float r, float g, float b, int32_t n, float* points,
                                       float* colors, void* stream_) {
  if (bad_count(n) || bad4(box) || bad4(points) || bad4(colors)) return GSR_EINVAL;
  GsrDeviceGuard dev(points);
  GSR_SAMPLE_LAUNCH(k_floor_indoor, n, (uint32_t)seed, (uint32_t)(seed >> 32), box, r, g, b, (uint32_t)n, points, colors);
  return GSR_OK;
}

extern "C" int gsr_sample_shell(uint64_t seed, float radius, int32_t zero_ground, float r, float g, float b, int32_t n,
                                float* points, float* colors, void* stream_) {
  if (bad_count(n) || !isfinite(radius) || bad4(points) || bad4(colors)) return GSR_EINVAL;
  GsrDeviceGuard dev(points);
  GSR_SAMPLE_LAUNCH(k_shell, n, (uint32_t)seed, (uint32_t)(seed >> 32), radius, zero_ground ? 1 : 0, r, g, b, (uint32_t)n, points,
                    colors);
  return GSR_OK;
}

extern "C" int gsr_sample_disc(uint64_t seed, float radius, float z0, float r, float g, float b, int32_t n, float* points,
                               float* colors, void* stream_) {
  if (bad_count(n) || !isfinite(radius) || !isfinite(z0) || bad4(points) || bad4(colors)) return GSR_EINVAL;
  GsrDeviceGuard dev(points);
  GSR_SAMPLE_LAUNCH(k_disc, n, (uint32_t)seed, (uint32_t)(seed >> 32), radius, z0, r, g, b, (uint32_t)n, points, colors);
  return GSR_OK;
}

extern "C" int gsr_sample_ball(uint64_t seed, float radius, int32_t n, float* points, float* colors, void* stream_) {
  if (bad_count(n) || !isfinite(radius) || bad4(points) || bad4(colors)) return GSR_EINVAL;
  GsrDeviceGuard dev(points);
  GSR_SAMPLE_LAUNCH(k_ball, n, (uint32_t)seed, (uint32_t)(seed >> 32), radius, (uint32_t)n, points, colors);
  return GSR_OK;
}

extern "C" int gsr_sample_jitter(uint64_t seed, const float* seed_points, const float* seed_colors, int32_t n_seeds,
                                 int32_t copies, float radius, float* points, float* colors, void* stream_) {
  if (n_seeds <= 0 || copies <= 0 || bad_count((int64_t)n_seeds * copies) || !isfinite(radius)) return GSR_EINVAL;
  if (bad4(seed_points) || ((uintptr_t)seed_colors & 3u) != 0 || bad4(points) || bad4(colors)) return GSR_EINVAL;
  const uint32_t rows = (uint32_t)n_seeds * (uint32_t)copies;
  GsrDeviceGuard dev(points);
  GSR_SAMPLE_LAUNCH(k_jitter, rows, (uint32_t)seed, (uint32_t)(seed >> 32), seed_points, seed_colors, rows, (uint32_t)copies,
                    radius, points, colors);
  return GSR_OK;
}

extern "C" int gsr_mesh_areas(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces, double* area,
                              void* stream_) {
  if (n_vertices <= 0 || bad_count(n_faces) || bad4(vertices) || bad4(faces) || bad8(area)) return GSR_EINVAL;
  GsrDeviceGuard dev(area);
  GSR_SAMPLE_LAUNCH(k_tri_area, n_faces, vertices, n_vertices, faces, (uint32_t)n_faces, area);
  return GSR_OK;
}

extern "C" int gsr_sample_mesh(uint64_t seed, const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces,
                               const double* cdf, int32_t n, float* points, float* colors, int32_t* triangle, void* stream_) {
  if (n_vertices <= 0 || bad_count(n_faces) || bad_count(n) || bad4(vertices) || bad4(faces) || bad8(cdf)) return GSR_EINVAL;
  if (bad4(points) || bad4(colors) || ((uintptr_t)triangle & 3u) != 0) return GSR_EINVAL;
  GsrDeviceGuard dev(points);
  GSR_SAMPLE_LAUNCH(k_mesh, n, (uint32_t)seed, (uint32_t)(seed >> 32), vertices, n_vertices, faces, (uint32_t)n_faces, cdf,
                    (uint32_t)n, points, colors, triangle);
  return GSR_OK;
}

extern "C" int gsr_mesh_center(const double* mean, int32_t n, float* points, void* stream_) {
  if (bad_count(n) || bad8(mean) || bad4(points)) return GSR_EINVAL;
  GsrDeviceGuard dev(points);
  GSR_SAMPLE_LAUNCH(k_center, n, mean, (uint32_t)n, points);
  return GSR_OK;
}

// Fused Instant-NGP volume render for gfx950 (forward + backward w.r.t. field parameters).
//
// What it replaces: NeRFRenderer.run (external/nerf/renderer_df.py:310-468) driving
// NeRFNetwork.common_forward (external/nerf/network_grid.py:77-88) three times per render plus
// ~40 unfused torch elementwise/sort/gather/cumprod kernels.  MI355X-first restructuring:
//   * the field is evaluated ONCE per sample (128/ray instead of the reference's 256: its third
//     pass re-evaluates the same points; value-identical, and the gradient of one evaluation
//     with both upstream grads equals the sum of the reference's two paths);
//   * encode + MLP + activations are one kernel, MLP weights live in LDS and are read as
//     broadcasts; nothing but sigma/rgb per sample is written to HBM;
//   * sampling (inverse-CDF), merge-sort and alpha compositing are per-ray kernels whose
//     per-thread scratch columns live in LDS ([k][lane] layout: bank-conflict free);
//   * backward RECOMPUTES the field forward instead of saving activations (VALU is cheap, HBM is
//     not); MLP weight gradients are formed per 256-point tile as LDS-staged outer-product
//     sums, one atomic flush per workgroup; table gradients are scattered with device atomics (ngp_scatter.h) or binned and reduced
//     in LDS (ngp_scatter_bin.h).
// This file keeps the host code, k_ngp_field, k_ngp_sample_fine and k_fix_to_f32; every other kernel lives in a header written against
// sf_dev.h.  Per-thread math lives in ngp_device.h, the backward's host plan (chunks, launch geometry, level split, workspace sizes) in
// ngp_bwd_plan.h (all also compiled for the host by tests/hostemu).
//
// Layouts (row-major): z_c,sig_c [N,T]; rgb_c [N,T,3]; z_f,sig_f,rgb_f same; z_sorted,sigma_s
// [N,2T]; rgb_s [N,2T,3]; image [N,3]; depth, weights_sum, nears, fars [N].

#include "sf_common.h"
#include "ngp_device.h"
#include "ngp_bwd_plan.h"
#include "ngp_field_lds.h"
#include "ngp_bwd_mfma.h"
#include "ngp_bwd_pipe.h"
#include "ngp_field_mfma.h"
#include "ngp_composite_wave.h"
#include "ngp_scatter.h"
#include "ngp_scatter_bin.h"
#include "ngp_shade.h"
#include "ngp_shade_bwd.h"
#include <stdlib.h>
#include <atomic>
#include <mutex>

struct GridLevels;  // gridencoder.hip
int sf_fill_levels(GridLevels* lv, const int32_t* offsets_dev, const int32_t* h_offsets, uint32_t L, float S,
                   uint32_t H, hipStream_t st);

// mode 0: z from stratified coarse rule (writes z_out); mode 1: z read from z_in; mode 2: xyz given.
template <int MODE>
__global__ __launch_bounds__(256) void k_ngp_field(
    FieldPtrs f, NgpLevels lv, const float* __restrict__ rays_o, const float* __restrict__ rays_d,
    const float* __restrict__ aabb, const float* __restrict__ nears, const float* __restrict__ fars,
    const float* __restrict__ lin, const float* __restrict__ u, const float* __restrict__ z_in,
    const float* __restrict__ xyz_in, uint32_t P, uint32_t T, float* __restrict__ z_out,
    float* __restrict__ sigma, float* __restrict__ rgb, float* __restrict__ feat_out = nullptr) {
  __shared__ __attribute__((aligned(16))) float W[NGP_WTOTAL];
  load_weights_lds(W, f);
  __syncthreads();
  float box[6];
  if (MODE != 2) {
#pragma unroll
    for (int i = 0; i < 6; ++i) box[i] = aabb[i];
  }
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
    // Memory clobber: stops LLVM from hoisting the 6.5k loop-invariant LDS weight reads out of the
    // grid-stride loop (which would pin them in 512 registers and spill).
    asm volatile("" ::: "memory");
    float x[3];
    if (MODE == 2) {
      x[0] = xyz_in[p * 3 + 0]; x[1] = xyz_in[p * 3 + 1]; x[2] = xyz_in[p * 3 + 2];
    } else {
      const uint32_t n = p / T, k = p - n * T;
      float z;
      if (MODE == 0) {
        z = ngp_coarse_z(nears[n], fars[n], lin[k], u ? u[p] : -1.0f, T);
        z_out[p] = z;
      } else {
        z = z_in[p];
      }
      const float o[3] = {rays_o[n * 3], rays_o[n * 3 + 1], rays_o[n * 3 + 2]};
      const float d[3] = {rays_d[n * 3], rays_d[n * 3 + 1], rays_d[n * 3 + 2]};
      ngp_point(o, d, z, box, x);
    }
    float x01[3];
    const bool inside = ngp_unit(x, f.bound, x01);
    float feat[NGP_FEAT], h1[NGP_HID], h2[NGP_HID], out[NGP_OUT];
    ngp_encode(lv, f.table, x01, inside, feat);
    if (feat_out) {                                   // field cache for the backward (sf_ngp_render_forward): one 128-byte row per point
#pragma unroll
      for (int j = 0; j < NGP_FEAT / 4; ++j)
        *reinterpret_cast<float4*>(feat_out + (size_t)p * NGP_FEAT + 4 * j) = make_float4(feat[4 * j], feat[4 * j + 1], feat[4 * j + 2], feat[4 * j + 3]);
    }
    ngp_mlp_forward(W, feat, h1, h2, out);
    sigma[p] = expf(out[0] + ngp_blob(x));
    rgb[p * 3 + 0] = ngp_sigmoid(out[1]);
    rgb[p * 3 + 1] = ngp_sigmoid(out[2]);
    rgb[p * 3 + 2] = ngp_sigmoid(out[3]);
  }
}

// thread per ray; dynamic LDS = 2 * T * 64 floats (cdf, bins columns)
__global__ __launch_bounds__(64) void k_ngp_sample_fine(
    const float* __restrict__ z_c, const float* __restrict__ sig_c, const float* __restrict__ u,
    uint32_t u_row_stride, const float* __restrict__ nears, const float* __restrict__ fars, uint32_t N,
    uint32_t T, float* __restrict__ z_f) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const uint32_t n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  SfCol cdf{smem + threadIdx.x, 64};
  SfCol bins{smem + (size_t)T * 64 + threadIdx.x, 64};
  ngp_sample_fine(z_c + (size_t)n * T, sig_c + (size_t)n * T, u + (size_t)n * u_row_stride, nears[n], fars[n], T,
                  cdf, bins, z_f + (size_t)n * T);
}

// Fixed-point gradient sums (sf_dev.h) -> the caller's fp32 gradients: dst[i] += acc[i] * 2^-44.  Segments are consecutive in acc.
#define FIX_SEGS 7
struct FixSegs { float* dst[FIX_SEGS]; uint64_t end[FIX_SEGS]; };
__global__ __launch_bounds__(256) void k_fix_to_f32(const long long* __restrict__ acc, FixSegs sg) {
  const uint64_t total = sg.end[FIX_SEGS - 1];
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    int k = 0;
    while (i >= sg.end[k]) ++k;
    const long long v = acc[i];
    if (v != 0 && sg.dst[k]) {
      const uint64_t j = i - (k ? sg.end[k - 1] : 0);
      sg.dst[k][j] += (float)((double)v * SF_FIX_INV);
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int sf_ngp_make_levels(const sf_ngp_field* f, NgpLevels* out, hipStream_t st) {
  if (!f || !f->h_offsets) SF_FAIL(SF_ERR_INVALID, "ngp: field/h_offsets must be given");
  if (f->L > NGP_MAX_LEVELS) SF_FAIL(SF_ERR_INVALID, "ngp: at most %d levels", NGP_MAX_LEVELS);
  struct { float scale[32]; uint32_t resolution[32]; uint32_t offset[32]; uint32_t hsize[32]; } tmp;
  if (int rc = sf_fill_levels(reinterpret_cast<GridLevels*>(&tmp), nullptr, f->h_offsets, f->L, f->S, f->H, st)) return rc;
  for (uint32_t l = 0; l < NGP_MAX_LEVELS; ++l) {
    const bool on = l < f->L;
    out->scale[l] = on ? tmp.scale[l] : 0.f;
    out->resolution[l] = on ? tmp.resolution[l] : 1;
    out->offset[l] = on ? tmp.offset[l] : 0;
    out->hsize[l] = on ? tmp.hsize[l] : 1;
  }
  out->L = f->L;
  out->gridtype = f->gridtype;
  return SF_OK;
}

static FieldPtrs field_ptrs(const sf_ngp_field* f) { return sf_ngp_field_ptrs(f); }

extern "C" int sf_ngp_density(const sf_ngp_field* f, const float* xyz, uint32_t P, float* sigma, float* albedo,
                              void* stream) {
  hipStream_t st = (hipStream_t)stream;
  NgpLevels lv;
  if (int rc = sf_ngp_make_levels(f, &lv, st)) return rc;
  if (P == 0) return SF_OK;
  k_ngp_field<2><<<sf_grid_cap(sf_div_up(P, 256)), 256, 0, st>>>(field_ptrs(f), lv, nullptr, nullptr, nullptr, nullptr,
                                                                 nullptr, nullptr, nullptr, nullptr, xyz, P, 1, nullptr,
                                                                 sigma, albedo);
  SF_CHECK_LAUNCH("ngp_density");
  return SF_OK;
}

// workspace sizes: the formulas and the layouts behind them are in ngp_bwd_plan.h
extern "C" uint64_t sf_ngp_render_workspace_bytes(uint32_t N, uint32_t T) { return ngp_render_workspace_bytes(N, T); }

extern "C" uint64_t sf_ngp_render_forward_workspace_bytes(uint32_t N, uint32_t T) { return ngp_render_forward_workspace_bytes(N, T); }

// Grid of k_ngp_field_mfma: 256 CUs x the two 256-thread workgroups its registers leave room for, every workgroup resident from the
// start (a workgroup stages the weights once).  Render forward at 128 x 128 rays, 512 / 1024 / 2048 workgroups: 0.89 / 0.91 / 0.93 ms;
// 256: 1.19 ms (profiles/ngp_field_mfma_ab.log).
#ifndef FM_GRID_CAP
#define FM_GRID_CAP 512u
#endif
// Which kernel runs the two field passes of sf_ngp_render_forward (and of everything built on it): 1 = k_ngp_field_mfma (the
// default), 0 = k_ngp_field.  on < 0 only asks.  Returns the previous setting.  Process-wide.
static std::atomic<int> g_field_mfma{1};
extern "C" int sf_ngp_field_mfma(int on) {
  const int was = g_field_mfma.load(std::memory_order_relaxed);
  if (on >= 0) g_field_mfma.store(on ? 1 : 0, std::memory_order_relaxed);
  return was;
}

// Which kernel runs the field backward of sf_ngp_render_backward when the forward left a field cache: 1 = k_ngp_field_bwd_pipe
// (ngp_bwd_pipe.h: the same values, operands a trip ahead), 0 = k_ngp_field_bwd_mfma.  Without a cache (the re-gather path) it is
// always k_ngp_field_bwd_mfma.  on < 0 only asks.  Returns the previous setting.  Process-wide.
static std::atomic<int> g_field_bwd_pipe{SF_FIELD_BWD_PIPE_DEFAULT};
static std::atomic<uint64_t> g_field_bwd_launches[2];      // launches of [0] k_ngp_field_bwd_mfma, [1] k_ngp_field_bwd_pipe
extern "C" int sf_ngp_field_bwd_pipe(int on) {
  const int was = g_field_bwd_pipe.load(std::memory_order_relaxed);
  if (on >= 0) g_field_bwd_pipe.store(on ? 1 : 0, std::memory_order_relaxed);
  return was;
}
extern "C" void sf_ngp_field_bwd_launches(uint64_t* counts) {
  counts[0] = g_field_bwd_launches[0].load(std::memory_order_relaxed);
  counts[1] = g_field_bwd_launches[1].load(std::memory_order_relaxed);
}

extern "C" uint64_t sf_ngp_render_cache_bytes(uint32_t N, uint32_t T) {
  return ((uint64_t)2 * N * T * NGP_FEAT + (uint64_t)N * 2 * T) * sizeof(float);
}

extern "C" int sf_ngp_render_forward(const sf_ngp_field* f, const float* rays_o, const float* rays_d,
                                     const float* aabb, uint32_t N, uint32_t T, float min_near,
                                     const float* lin, const float* u_coarse, const float* u_fine,
                                     uint32_t u_fine_row_stride, float bg_color, float* nears, float* fars,
                                     float* z_sorted, float* sigma_s, float* rgb_s, float* image, float* depth,
                                     float* weights_sum, float* field_cache, float* workspace, uint64_t workspace_bytes,
                                     void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) return SF_OK;
  if (T < 4 || T > 64) SF_FAIL(SF_ERR_INVALID, "ngp_render: T must be in [4,64]");
  if (workspace_bytes < sf_ngp_render_forward_workspace_bytes(N, T)) SF_FAIL(SF_ERR_INVALID, "ngp_render: workspace too small");
  if (!lin || !u_fine) SF_FAIL(SF_ERR_INVALID, "ngp_render: lin and u_fine tables are required");
  NgpLevels lv;
  if (int rc = sf_ngp_make_levels(f, &lv, st)) return rc;
  if (int rc = sf_near_far_from_aabb(rays_o, rays_d, aabb, N, min_near, nears, fars, stream)) return rc;
  const uint64_t NT = (uint64_t)N * T;
  float* z_c = workspace;           float* sig_c = z_c + NT;     float* rgb_c = sig_c + NT;
  float* z_f = rgb_c + 3 * NT;      float* sig_f = z_f + NT;     float* rgb_f = sig_f + NT;
  const FieldPtrs fp = field_ptrs(f);
  const uint32_t P = (uint32_t)NT;
  const uint32_t gridp = sf_grid_cap(sf_div_up(P, 256));
  // field cache (or NULL): [N*T][32] coarse features | [N*T][32] fine features | [N][2T] u32 sort permutation
  float* feat_c = field_cache;
  float* feat_f = field_cache ? field_cache + NT * NGP_FEAT : nullptr;
  uint32_t* perm = field_cache ? reinterpret_cast<uint32_t*>(field_cache + 2 * NT * NGP_FEAT) : nullptr;
  // the two field passes: k_ngp_field_mfma (ngp_field_mfma.h; same bits, the hidden layers on the matrix cores), or the lane-per-point
  // k_ngp_field it is checked against (sf_ngp_field_mfma(0))
  const bool mfma = g_field_mfma.load(std::memory_order_relaxed) != 0;
  FMArgs fm{};
  fm.table = fp.table; fm.w0 = fp.w0; fm.b0 = fp.b0; fm.w1 = fp.w1; fm.b1 = fp.b1; fm.w2 = fp.w2; fm.b2 = fp.b2; fm.bound = fp.bound;
  fm.lv = lv; fm.rays_o = rays_o; fm.rays_d = rays_d; fm.aabb = aabb; fm.nears = nears; fm.fars = fars; fm.P = P; fm.T = T;
  const uint32_t gridm = sf_div_up(sf_div_up(P, FM_PTS), 4) < FM_GRID_CAP ? sf_div_up(sf_div_up(P, FM_PTS), 4) : FM_GRID_CAP;
  const size_t ldsm = FM_LDS_FLOATS * sizeof(float);
  if (mfma) {
    fm.lin = lin; fm.u = u_coarse; fm.z_out = z_c; fm.sigma = sig_c; fm.rgb = rgb_c; fm.feat_out = feat_c;
    k_ngp_field_mfma<0><<<gridm, 256, ldsm, st>>>(fm);
  } else {
    k_ngp_field<0><<<gridp, 256, 0, st>>>(fp, lv, rays_o, rays_d, aabb, nears, fars, lin, u_coarse, nullptr, nullptr, P, T,
                                          z_c, sig_c, rgb_c, feat_c);
  }
  SF_CHECK_LAUNCH("ngp_field_coarse");
  const uint32_t gridr = sf_div_up(N, 64);
  k_ngp_sample_fine<<<gridr, 64, 2 * T * 64 * sizeof(float), st>>>(z_c, sig_c, u_fine, u_fine_row_stride, nears, fars,
                                                                  N, T, z_f);
  SF_CHECK_LAUNCH("ngp_sample_fine");
  if (mfma) {
    fm.lin = nullptr; fm.u = nullptr; fm.z_in = z_f; fm.z_out = nullptr; fm.sigma = sig_f; fm.rgb = rgb_f; fm.feat_out = feat_f;
    k_ngp_field_mfma<1><<<gridm, 256, ldsm, st>>>(fm);
  } else {
    k_ngp_field<1><<<gridp, 256, 0, st>>>(fp, lv, rays_o, rays_d, aabb, nears, fars, nullptr, nullptr, z_f, nullptr, P, T,
                                          nullptr, sig_f, rgb_f, feat_f);
  }
  SF_CHECK_LAUNCH("ngp_field_fine");
  // one WAVE per ray: rank sort of cat([coarse, fine]) by readlane keys + scans (ngp_composite_wave.h)
  k_ngp_composite_wave<<<sf_div_up(N, 4), 256, 4 * 5 * 2 * T * sizeof(float), st>>>(
      CompositeArgs{z_c, sig_c, rgb_c, z_f, sig_f, rgb_f, nears, fars, N, T, bg_color, z_sorted, sigma_s, rgb_s, image, depth,
                    weights_sum, perm});
  SF_CHECK_LAUNCH("ngp_composite");
  return SF_OK;
}

extern "C" uint64_t sf_ngp_render_shaded_workspace_bytes(uint32_t N, uint32_t T) { return sf_ngp_render_forward_workspace_bytes(N, T); }

// Shaded render without gradient (ngp_shade.h).  The albedo forward runs first and unchanged: sample_pdf needs the coarse sigmas
// before any normal can be placed, and it leaves the sorted ray the two kernels below work on.  Every check comes before the
// first launch.  grad_s / w_s (both or none): what the backward needs per sorted sample next to the other outputs
// (sf_ngp_render_shaded_forward_train); every other output is the same bits with or without them.
static int ngp_render_shaded_forward_body(const sf_ngp_field* f, const float* rays_o, const float* rays_d, const float* aabb,
                                          uint32_t N, uint32_t T, float min_near, const float* lin, const float* u_coarse,
                                          const float* u_fine, uint32_t u_fine_row_stride, float bg_color, const float* light_d,
                                          float ambient_ratio, float epsilon, float* nears, float* fars, float* z_sorted,
                                          float* sigma_s, float* rgb_s, float* normal_s, float* rgb_shaded_s, float* xyz_s,
                                          float* grad_s, float* w_s, float* image, float* normal_image, float* orient, float* depth,
                                          float* weights_sum, float* workspace, uint64_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!light_d) SF_FAIL(SF_ERR_INVALID, "ngp_render_shaded: null light_d");
  if (!isfinite(epsilon) || !(epsilon > 0.0f)) SF_FAIL(SF_ERR_INVALID, "ngp_render_shaded: epsilon must be finite and > 0");
  if (!isfinite(ambient_ratio)) SF_FAIL(SF_ERR_INVALID, "ngp_render_shaded: ambient_ratio must be finite");
  if (N == 0) return SF_OK;
  if (T < 4 || T > 64) SF_FAIL(SF_ERR_INVALID, "ngp_render_shaded: T must be in [4,64]");
  if ((uint64_t)N * 2 * T >= (1ull << 32)) SF_FAIL(SF_ERR_INVALID, "ngp_render_shaded: N * 2T must be below 2^32");
  if (workspace_bytes < sf_ngp_render_shaded_workspace_bytes(N, T)) SF_FAIL(SF_ERR_INVALID, "ngp_render_shaded: workspace too small");
  if (!lin || !u_fine) SF_FAIL(SF_ERR_INVALID, "ngp_render_shaded: lin and u_fine tables are required");
  if (!f || !rays_o || !rays_d || !aabb || !nears || !fars || !z_sorted || !sigma_s || !rgb_s || !normal_s || !rgb_shaded_s || !image ||
      !depth || !weights_sum || !workspace)
    SF_FAIL(SF_ERR_INVALID, "ngp_render_shaded: null pointer");
  NgpLevels lv;
  if (int rc = sf_ngp_make_levels(f, &lv, st)) return rc;
  if (int rc = sf_ngp_render_forward(f, rays_o, rays_d, aabb, N, T, min_near, lin, u_coarse, u_fine, u_fine_row_stride, bg_color, nears,
                                     fars, z_sorted, sigma_s, rgb_s, image, depth, weights_sum, nullptr, workspace, workspace_bytes, stream))
    return rc;
  const uint32_t P = N * 2 * T;
  ShadeArgs s{};
  s.f = field_ptrs(f); s.lv = lv;
  s.rays_o = rays_o; s.rays_d = rays_d; s.aabb = aabb; s.z_s = z_sorted; s.rgb_s = rgb_s; s.light_d = light_d;
  s.P = P; s.T2 = 2 * T; s.ratio = ambient_ratio; s.eps = epsilon;
  s.normal_s = normal_s; s.rgb_shaded_s = rgb_shaded_s; s.xyz_s = xyz_s; s.grad_s = grad_s;
  k_ngp_shade<<<sf_grid_cap(sf_div_up(P, 256)), 256, 0, st>>>(s);
  SF_CHECK_LAUNCH("ngp_shade");
  // image, depth and weights_sum are written again: the same scan on the same sorted ray (depth and weights_sum come out bit for bit)
  k_ngp_composite_sorted_wave<<<sf_div_up(N, 4), 256, 0, st>>>(
      CompositeSortedArgs{z_sorted, sigma_s, rgb_shaded_s, normal_s, rays_d, nears, fars, N, T, bg_color, image, depth, weights_sum,
                          normal_image, orient, w_s});
  SF_CHECK_LAUNCH("ngp_composite_sorted");
  return SF_OK;
}

extern "C" int sf_ngp_render_shaded_forward(const sf_ngp_field* f, const float* rays_o, const float* rays_d, const float* aabb,
                                            uint32_t N, uint32_t T, float min_near, const float* lin, const float* u_coarse,
                                            const float* u_fine, uint32_t u_fine_row_stride, float bg_color, const float* light_d,
                                            float ambient_ratio, float epsilon, float* nears, float* fars, float* z_sorted,
                                            float* sigma_s, float* rgb_s, float* normal_s, float* rgb_shaded_s, float* xyz_s,
                                            float* image, float* normal_image, float* orient, float* depth, float* weights_sum,
                                            float* workspace, uint64_t workspace_bytes, void* stream) {
  return ngp_render_shaded_forward_body(f, rays_o, rays_d, aabb, N, T, min_near, lin, u_coarse, u_fine, u_fine_row_stride, bg_color, light_d,
                                        ambient_ratio, epsilon, nears, fars, z_sorted, sigma_s, rgb_s, normal_s, rgb_shaded_s, xyz_s, nullptr,
                                        nullptr, image, normal_image, orient, depth, weights_sum, workspace, workspace_bytes, stream);
}

// The shaded forward of a render that will be differentiated (sf_ngp_render_shaded_backward): the same launches, which also keep the
// un-normalised gradient grad_s [N,2T,3] and the weights w_s [N,2T] of every sorted sample.
extern "C" int sf_ngp_render_shaded_forward_train(const sf_ngp_field* f, const float* rays_o, const float* rays_d, const float* aabb,
                                                  uint32_t N, uint32_t T, float min_near, const float* lin, const float* u_coarse,
                                                  const float* u_fine, uint32_t u_fine_row_stride, float bg_color, const float* light_d,
                                                  float ambient_ratio, float epsilon, float* nears, float* fars, float* z_sorted,
                                                  float* sigma_s, float* rgb_s, float* normal_s, float* rgb_shaded_s, float* grad_s,
                                                  float* w_s, float* image, float* normal_image, float* orient, float* depth,
                                                  float* weights_sum, float* workspace, uint64_t workspace_bytes, void* stream) {
  if (!grad_s || !w_s) SF_FAIL(SF_ERR_INVALID, "ngp_render_shaded_forward_train: null grad_s / w_s");
  return ngp_render_shaded_forward_body(f, rays_o, rays_d, aabb, N, T, min_near, lin, u_coarse, u_fine, u_fine_row_stride, bg_color, light_d,
                                        ambient_ratio, epsilon, nears, fars, z_sorted, sigma_s, rgb_s, normal_s, rgb_shaded_s, nullptr, grad_s,
                                        w_s, image, normal_image, orient, depth, weights_sum, workspace, workspace_bytes, stream);
}


// ---------------------------------------------------------------------------
// backward: what the library keeps per device, and the two guards of a call
// ---------------------------------------------------------------------------
static constexpr size_t FB_LDS_BYTES = (size_t)FB_LDS_FLOATS * sizeof(float);

static int ngp_bwd_raise_lds_limits() {             // raised dynamic-LDS limits are per-device function attributes
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ngp_field_bwd_mfma_t<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FB_LDS_BYTES) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ngp_field_bwd_pipe), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FB_LDS_BYTES) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ngp_scatter<1024, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SC_LDS_BYTES) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ngp_field_bwd_mfma_t<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FB_LDS_BYTES) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ngp_scatter<1024, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SC_LDS_BYTES) != hipSuccess)
    SF_FAIL(SF_ERR_LAUNCH, "ngp_render_backward: cannot raise the dynamic LDS limits");
  return SF_OK;
}

// One per device (the first 32), filled on first use under g_bwd_dev_mu and kept for the life of the process.
struct NgpBwdDevice {
  // the gradient accumulators come from a memory pool this library owns (kept mapped between calls so a call does not re-map it); the
  // device's default pool and its settings are left alone
  hipMemPool_t pool;
  // The side stream and its fork / join events are ONE set per device: two host threads (or two caller streams) rendering on the
  // same device would re-record each other's events, so the whole fork .. join section of a call runs under g_bwd_side_mu (host-side
  // enqueue only: microseconds).
  hipStream_t side; hipEvent_t fork, join;
  bool lds_raised;
};
static std::mutex g_bwd_dev_mu, g_bwd_side_mu;
static NgpBwdDevice g_bwd_dev[32] = {};

// The state of device dev_id with the LDS limits raised, and with a side stream if the call wants one.  Devices beyond the 32nd keep no
// state (*out = nullptr: hipMallocAsync, no side stream) and have their limits raised by every call.
static int ngp_bwd_device(int dev_id, bool want_side, NgpBwdDevice** out) {
  *out = nullptr;
  if (dev_id >= 32) return ngp_bwd_raise_lds_limits();
  std::lock_guard<std::mutex> lk(g_bwd_dev_mu);
  NgpBwdDevice& d = g_bwd_dev[dev_id];
  if (!d.pool) {
    hipMemPoolProps props{};
    props.allocType = hipMemAllocationTypePinned;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = dev_id;
    hipMemPool_t np = nullptr;
    uint64_t keep = UINT64_MAX;
    if (hipMemPoolCreate(&np, &props) != hipSuccess) SF_FAIL(SF_ERR_LAUNCH, "ngp_render_backward: cannot create the scratch pool");
    if (hipMemPoolSetAttribute(np, hipMemPoolAttrReleaseThreshold, &keep) != hipSuccess) {
      (void)hipMemPoolDestroy(np);
      SF_FAIL(SF_ERR_LAUNCH, "ngp_render_backward: cannot configure the scratch pool");
    }
    d.pool = np;
  }
  if (!d.lds_raised) {
    if (int rc = ngp_bwd_raise_lds_limits()) return rc;
    d.lds_raised = true;
  }
  if (want_side && !d.side) {
    hipStream_t s = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&join, hipEventDisableTiming) != hipSuccess) {
      if (fork) (void)hipEventDestroy(fork);
      if (s) (void)hipStreamDestroy(s);
      SF_FAIL(SF_ERR_LAUNCH, "ngp_render_backward: cannot create the side stream");
    }
    d.fork = fork; d.join = join; d.side = s;
  }
  *out = &d;
  return SF_OK;
}

// the gradient accumulators of one call: freed on the stream, behind everything the call enqueued
struct FixBuf {
  long long* p = nullptr; hipStream_t st = nullptr;
  ~FixBuf() { if (p) (void)hipFreeAsync(p, st); }
};

// Joins the side stream into the caller's stream on EVERY exit path of a call that forked, error returns included.
struct SideJoin {
  NgpBwdDevice* dev = nullptr; hipStream_t st = nullptr; bool forked = false;
  int fork() {                                     // the side stream continues from here
    if (hipEventRecord(dev->fork, st) != hipSuccess || hipStreamWaitEvent(dev->side, dev->fork, 0) != hipSuccess) return 1;
    forked = true;
    return 0;
  }
  int join() { const bool f = forked; forked = false; return (!f || (hipEventRecord(dev->join, dev->side) == hipSuccess && hipStreamWaitEvent(st, dev->join, 0) == hipSuccess)) ? 0 : 1; }
  ~SideJoin() { (void)join(); }
};

static int ngp_bwd_field_scatter(const sf_ngp_field* f, const sf_ngp_field_grad* g, const NgpLevels& lv, const float* rays_o,
                                 const float* rays_d, const float* aabb, uint32_t N, uint32_t T, const float* z_sorted, uint32_t rays_per_row,
                                 const float* field_cache, float* workspace, const float* ds_off, uint32_t e_begin, uint32_t e_end, float eps,
                                 hipStream_t st);

extern "C" int sf_ngp_render_backward(const sf_ngp_field* f, const sf_ngp_field_grad* g, const float* rays_o,
                                      const float* rays_d, const float* aabb, uint32_t N, uint32_t T,
                                      const float* nears, const float* fars, const float* z_sorted,
                                      const float* sigma_s, const float* rgb_s, float bg_color,
                                      const float* grad_image, const float* grad_weights_sum, uint32_t rays_per_row,
                                      const float* field_cache, float* workspace, uint64_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) return SF_OK;
  if (T < 4 || T > 64) SF_FAIL(SF_ERR_INVALID, "ngp_render: T must be in [4,64]");
  if (workspace_bytes < sf_ngp_render_workspace_bytes(N, T)) SF_FAIL(SF_ERR_INVALID, "ngp_render: workspace too small");
  if (!grad_image) SF_FAIL(SF_ERR_INVALID, "ngp_render_backward: grad_image required");
  NgpLevels lv;
  if (int rc = sf_ngp_make_levels(f, &lv, st)) return rc;
  const uint64_t M = (uint64_t)N * 2 * T;
  float* dsig = workspace;
  float* drgb = dsig + M;

  // wave-per-ray backward: the forward's scans run in reverse (suffix sums in double)
  k_ngp_composite_bwd_wave<<<sf_div_up(N, 4), 256, 0, st>>>(
      CompositeBwdArgs{z_sorted, sigma_s, rgb_s, nears, fars, N, T, bg_color, grad_image, grad_weights_sum, dsig, drgb});
  SF_CHECK_LAUNCH("ngp_composite_bwd");
  return ngp_bwd_field_scatter(f, g, lv, rays_o, rays_d, aabb, N, T, z_sorted, rays_per_row, field_cache, workspace, nullptr, 0, 1, 0.0f, st);
}

// Everything of a render backward behind the composite backward: the field backward and the table-gradient scatter of the sorted samples,
// with d(sigma) [M] | d(albedo) [3M] at the head of `workspace` (the layout of ngp_bwd_plan.h), summed in fixed point and converted into
// g's buffers.  Passes e = e_begin .. e_end - 1: pass 0 is the samples themselves (the albedo backward, sf_ngp_render_backward, is [0, 1)),
// pass e = 1 .. 6 their offset points e of step `eps` with d(sigma) in plane e - max(e_begin, 1) of ds_off [.][M] (ngp_shade_bwd.h; the
// OFF = 1 instantiations: d(albedo) = 0).  All passes add into the SAME accumulators, converted once; d(feat) is one pass wide and reused.
static int ngp_bwd_field_scatter(const sf_ngp_field* f, const sf_ngp_field_grad* g, const NgpLevels& lv, const float* rays_o,
                                 const float* rays_d, const float* aabb, uint32_t N, uint32_t T, const float* z_sorted, uint32_t rays_per_row,
                                 const float* field_cache, float* workspace, const float* ds_off, uint32_t e_begin, uint32_t e_end, float eps,
                                 hipStream_t st) {
  const uint64_t M = (uint64_t)N * 2 * T;
  const uint32_t T2 = 2 * T;
  const uint32_t passes = e_end - e_begin, plane0 = e_begin ? e_begin : 1;
  float* dsig = workspace;
  float* drgb = dsig + M;
  float* dfeat = g->g_embeddings ? drgb + 3 * M : nullptr;        // NULL table gradient = table frozen
  uint32_t* bin_cursor = reinterpret_cast<uint32_t*>(workspace + ngp_bwd_grad_floats(N, T));
  f32x4* bin_ent = reinterpret_cast<f32x4*>(bin_cursor + SB_CURSOR_WORDS);      // (16-byte aligned: 72 N T floats + 2^13 words)
  // the plan (ngp_bwd_plan.h): which kernel scatters which level, and the ray chunks (the entries buffer is sized for this chunking)
  const NgpScatterPlan sp = ngp_scatter_plan(lv, dfeat != nullptr, N, T);
  const bool per_chunk = dfeat && sp.last < lv.L;                 // levels [last, L) are scattered chunk by chunk
  const NgpChunks plan = per_chunk ? ngp_bwd_plan(N) : ngp_bwd_one_chunk(N);
  const float thr_mlp = ngp_bwd_thr_mlp(plan.n * passes);       // (every pass adds its per-chunk addends to the same sums)
  // a fixed-point sum receives at most 8 addends per sample (the 8 corners of a cell, hash collisions included): thresholds per
  // sf_dev.h keep every table sum below 2^18; larger addends take the fp32 atomics (sf_grad_add)
  const float thr_tab = sf_fix_thr(8.0 * (double)passes * (double)M);

  int dev_id = 0;
  if (hipGetDevice(&dev_id) != hipSuccess) SF_FAIL(SF_ERR_LAUNCH, "hipGetDevice failed");
  NgpBwdDevice* dev = nullptr;
  if (int rc = ngp_bwd_device(dev_id, per_chunk, &dev)) return rc;

  // every gradient is first summed in 64-bit fixed point (sf_dev.h: order-independent, so the result is the same on every run) in a
  // stream-ordered scratch buffer: [table rows x 2 | w0 | b0 | w1 | b1 | w2 | b2], converted into the caller's buffers at the end
  const uint64_t tab_n = dfeat ? (uint64_t)f->h_offsets[f->L] * 2 : 0;
  FixSegs segs{};
  {
    float* dst[FIX_SEGS] = {g->g_embeddings, g->g_w0, g->g_b0, g->g_w1, g->g_b1, g->g_w2, g->g_b2};
    const uint64_t len[FIX_SEGS] = {tab_n, NGP_HID * NGP_FEAT, NGP_HID, NGP_HID * NGP_HID, NGP_HID, NGP_OUT * NGP_HID, NGP_OUT};
    uint64_t e = 0;
    for (int k = 0; k < FIX_SEGS; ++k) { segs.dst[k] = dst[k]; e += len[k]; segs.end[k] = e; }
  }
  FixBuf fix;
  fix.st = st;
  const uint64_t fix_bytes = segs.end[FIX_SEGS - 1] * sizeof(long long);
  const hipError_t alloc = dev ? hipMallocFromPoolAsync(reinterpret_cast<void**>(&fix.p), fix_bytes, dev->pool, st)
                               : hipMallocAsync(reinterpret_cast<void**>(&fix.p), fix_bytes, st);
  if (alloc != hipSuccess || !fix.p)
    SF_FAIL(SF_ERR_LAUNCH, "ngp_render_backward: cannot allocate the gradient accumulators");
  if (hipMemsetAsync(fix.p, 0, fix_bytes, st) != hipSuccess) SF_FAIL(SF_ERR_LAUNCH, "ngp_render_backward: memset failed");
  long long* acc_tab = fix.p;
  if (sp.binned && hipMemsetAsync(bin_cursor, 0, (size_t)sp.total_buckets * 4, st) != hipSuccess) SF_FAIL(SF_ERR_LAUNCH, "ngp_render_backward: memset failed");

  // what every chunk's launches share
  FBArgs a{};
  a.table = f->embeddings; a.w0 = f->w0; a.b0 = f->b0; a.w1 = f->w1; a.b1 = f->b1; a.w2 = f->w2; a.b2 = f->b2; a.bound = f->bound;
  a.g_w0 = fix.p + segs.end[0]; a.g_b0 = fix.p + segs.end[1]; a.g_w1 = fix.p + segs.end[2];
  a.g_b1 = fix.p + segs.end[3]; a.g_w2 = fix.p + segs.end[4]; a.g_b2 = fix.p + segs.end[5];
  a.f_w0 = g->g_w0; a.f_b0 = g->g_b0; a.f_w1 = g->g_w1; a.f_b1 = g->g_b1; a.f_w2 = g->g_w2; a.f_b2 = g->g_b2; a.thr = thr_mlp;
  a.lv = lv; a.aabb = aabb; a.dfeat_out = dfeat; a.T2 = T2; a.dfeat_P = (uint32_t)M;
  a.feat_c = field_cache;                           // (or all three null: the kernel re-gathers the features)
  a.feat_f = field_cache ? field_cache + (size_t)N * T * NGP_FEAT : nullptr;
  a.perm = field_cache ? reinterpret_cast<const uint32_t*>(field_cache + 2 * (size_t)N * T * NGP_FEAT) : nullptr;
  SBArgs b{};
  b.lv = lv; b.bound = f->bound; b.aabb = aabb; b.dfeat = dfeat;
  b.gtable = acc_tab; b.gtable_f = g->g_embeddings; b.thr = thr_tab; b.cursor = bin_cursor; b.ent = bin_ent;
  b.T2 = T2; b.first_level = sp.first_bin; b.P_stride = (uint32_t)M; b.cap = sp.bin_cap;
  SBRArgs r{};
  r.lv = lv; r.gtable = acc_tab; r.gtable_f = g->g_embeddings; r.thr = thr_tab; r.cursor = bin_cursor; r.ent = bin_ent; r.first_level = sp.first_bin; r.cap = sp.bin_cap;
  for (uint32_t l = 0; l <= NGP_MAX_LEVELS; ++l) { b.bucket0[l] = sp.bucket0[l]; r.bucket0[l] = sp.bucket0[l]; }
  SCArgs s{};                                       // k_ngp_scatter_fine (ngp_scatter.h): the rays of a launch are set at the launch
  s.lv = lv; s.bound = f->bound; s.aabb = aabb; s.dfeat = dfeat; s.gtable = acc_tab; s.gtable_f = g->g_embeddings; s.thr = thr_tab; s.T2 = T2;
  s.first_level = sp.last; s.P_stride = (uint32_t)M;

  // ---- the pipeline (r03).  Three kernels with three different bottlenecks: the field backward (fp32 MFMA + 113 KB of LDS,
  // one workgroup per CU), the fine-level scatter (memory-side atomic unit, no LDS, VALU idle) and the cached-level scatter
  // (LDS atomics, 96 KB).  The rays are cut into chunks; the fine-level scatter of chunk c runs on a side stream while the
  // field backward of chunk c + 1 occupies the CUs, and the last one runs beside the cached-level scatter (one launch over
  // all rays, its LDS cache wants every ray of an 8x8 patch).  dfeat keeps the level-major layout of the whole ray set.
  // (r03 A/B: 1 / 2 / 4 / 8 chunks 5.96 / 5.65 / 5.64 / 6.00 ms, no overlap 6.33 ms; the switches were retired in r04.)
  const bool fork = per_chunk && dev;
  std::unique_lock<std::mutex> side_lk(g_bwd_side_mu, std::defer_lock);
  SideJoin side_join;                               // (declared behind the lock: joins before the lock is released)
  if (fork) {
    side_lk.lock();
    side_join.dev = dev; side_join.st = st;
  }
  // pass 0: the samples themselves; passes e = 1 .. 6 (the shaded backward): their offset points e
  for (uint32_t e = e_begin; e < e_end; ++e) {
    a.off_e = e; a.off_eps = eps; b.off_e = e; b.off_eps = eps; s.off_e = e; s.off_eps = eps;
    for (uint32_t c = 0; c < plan.n; ++c) {
      const uint32_t n0 = plan.start[c], Nc = plan.start[c + 1] - n0;
      const uint32_t Pc = Nc * T2, P0 = n0 * T2;
      // matrix-core field backward of chunk c: one wave per 32 points and trip, six fp32 GEMMs on v_mfma_f32_16x16x4_f32 (ngp_bwd_mfma.h)
      a.rays_o = rays_o + (size_t)n0 * 3; a.rays_d = rays_d + (size_t)n0 * 3;
      a.z_s = z_sorted + (size_t)P0; a.dsig = (e ? ds_off + (size_t)(e - plane0) * M : dsig) + (size_t)P0; a.drgb = drgb + (size_t)P0 * 3;
      a.P = Pc; a.p_off = P0;
      const uint32_t grid = ngp_field_bwd_grid(Pc, FB_PTS);
      // with a field cache: k_ngp_field_bwd_pipe (ngp_bwd_pipe.h; same trips, same LDS image, same values) unless switched off
      const int pipe = field_cache && g_field_bwd_pipe.load(std::memory_order_relaxed) != 0 ? 1 : 0;
      (e ? &k_ngp_field_bwd_mfma_t<1> : pipe ? &k_ngp_field_bwd_pipe : &k_ngp_field_bwd_mfma_t<0>)<<<grid, 256, FB_LDS_BYTES, st>>>(a);
      SF_CHECK_LAUNCH(e ? "ngp_field_bwd_mfma_off" : pipe ? "ngp_field_bwd_pipe" : "ngp_field_bwd_mfma");
      if (!e) g_field_bwd_launches[pipe].fetch_add(1, std::memory_order_relaxed);
      if (!per_chunk) continue;
      if (fork && side_join.fork()) SF_FAIL(SF_ERR_LAUNCH, "ngp_render_backward: fork failed");
      hipStream_t sf = fork ? dev->side : st;
      if (sp.binned) {
        b.rays_o = a.rays_o; b.rays_d = a.rays_d; b.z_s = a.z_s; b.P = Pc; b.p_off = P0;
        const uint32_t tiles = sf_div_up(Pc, SB_THREADS);
        (e ? &k_ngp_bin_t<1> : &k_ngp_bin_t<0>)<<<tiles < 1024 ? tiles : 1024, SB_THREADS, 0, sf>>>(b);
        SF_CHECK_LAUNCH("ngp_bin");
        k_ngp_bin_reduce<<<sp.total_buckets, SBR_THREADS, 0, sf>>>(r);         // leaves the cursors at zero for the next chunk
        SF_CHECK_LAUNCH("ngp_bin_reduce");
      } else {
        const uint64_t items = (uint64_t)4 * Pc * (lv.L - sp.last);
        const uint32_t grid_f = (uint32_t)(items / 256 < 16384 ? (items + 255) / 256 : 16384);
        s.rays_o = a.rays_o; s.rays_d = a.rays_d; s.z_s = a.z_s; s.N = Nc; s.p_off = P0;
        (e ? &k_ngp_scatter_fine<1> : &k_ngp_scatter_fine<0>)<<<grid_f, 256, 0, sf>>>(s);
        SF_CHECK_LAUNCH("ngp_scatter_fine");
      }
    }
    if (dfeat && sp.last > 0) {
      const uint32_t grid_sc = sf_div_up(N, SC_RAYS);
      (e ? &k_ngp_scatter<1024, 1> : &k_ngp_scatter<1024, 0>)<<<grid_sc, 1024, SC_LDS_BYTES, st>>>(lv, f->bound, acc_tab, g->g_embeddings, thr_tab, rays_o, rays_d, aabb, z_sorted, dfeat, N, T2, rays_per_row, sp.cached, sp.last, SC_RUN, e, eps);
      SF_CHECK_LAUNCH("ngp_scatter");
    }
    // the next pass rewrites d(feat): the side stream's last bin / scatter of this pass must have read it
    if (e + 1 < e_end && side_join.join()) SF_FAIL(SF_ERR_LAUNCH, "ngp_render_backward: join failed");
  }
  if (side_join.join()) SF_FAIL(SF_ERR_LAUNCH, "ngp_render_backward: join failed");
  {
    const uint64_t total = segs.end[FIX_SEGS - 1];
    const uint32_t grid_x = (uint32_t)(total / 256 < 4096 ? (total + 255) / 256 : 4096);
    k_fix_to_f32<<<grid_x, 256, 0, st>>>(fix.p, segs);
    SF_CHECK_LAUNCH("fix_to_f32");
  }
  return SF_OK;                                    // (fix frees the accumulators on the stream, behind the conversion)
}

// ---------------------------------------------------------------------------
// backward of the shaded render (ngp_shade_bwd.h): albedo, and the density through the finite-difference normal
// ---------------------------------------------------------------------------
extern "C" uint64_t sf_ngp_render_shaded_backward_workspace_bytes(uint32_t N, uint32_t T) {
  return ngp_render_workspace_bytes(N, T) + (uint64_t)6 * N * 2 * T * sizeof(float);      // the albedo backward's, then ds_off [6][N * 2T]
}

// 1. k_ngp_composite_bwd_wave on the SHADED colour: d(sigma) of the centres (the weights inside the orientation term are detached, so
//    grad_orient adds nothing here) and d(col);  2. k_ngp_shade_bwd: d(albedo) over d(col), d(sigma) at the six offset points;
// 3. the field backward + scatter stage seven times into one set of accumulators (ngp_bwd_field_scatter).  With ambient_ratio == 1 and no
// grad_orient the upstream of the six offset passes is exactly zero and they are skipped -- stricter than running them in one case: a
// non-finite d(col) would make k_ngp_shade_bwd write NaN (0 * inf) into ds_off, which the skip does not carry into the offset passes
// (the centre pass still carries it: d(albedo) = d(col) lam).  Every check comes before the first launch.
extern "C" int sf_ngp_render_shaded_backward(const sf_ngp_field* f, const sf_ngp_field_grad* g, const float* rays_o, const float* rays_d,
                                             const float* aabb, uint32_t N, uint32_t T, const float* nears, const float* fars,
                                             const float* z_sorted, const float* sigma_s, const float* rgb_s, const float* normal_s,
                                             const float* rgb_shaded_s, const float* grad_s, const float* w_s, const float* light_d,
                                             float ambient_ratio, float epsilon, float bg_color, const float* grad_image,
                                             const float* grad_weights_sum, const float* grad_orient, uint32_t rays_per_row,
                                             float* workspace, uint64_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!f || !g || !rays_o || !rays_d || !aabb || !nears || !fars || !z_sorted || !sigma_s || !rgb_s || !normal_s || !rgb_shaded_s || !grad_s ||
      !w_s || !light_d || !grad_image)
    SF_FAIL(SF_ERR_INVALID, "ngp_render_shaded_backward: null pointer");
  if (!isfinite(epsilon) || !(epsilon > 0.0f)) SF_FAIL(SF_ERR_INVALID, "ngp_render_shaded_backward: epsilon must be finite and > 0");
  if (!isfinite(ambient_ratio)) SF_FAIL(SF_ERR_INVALID, "ngp_render_shaded_backward: ambient_ratio must be finite");
  if (N == 0) return SF_OK;
  if (T < 4 || T > 64) SF_FAIL(SF_ERR_INVALID, "ngp_render_shaded_backward: T must be in [4,64]");
  if ((uint64_t)N * 2 * T >= (1ull << 32)) SF_FAIL(SF_ERR_INVALID, "ngp_render_shaded_backward: N * 2T must be below 2^32");
  if (!workspace || workspace_bytes < sf_ngp_render_shaded_backward_workspace_bytes(N, T))
    SF_FAIL(SF_ERR_INVALID, "ngp_render_shaded_backward: workspace too small");
  NgpLevels lv;
  if (int rc = sf_ngp_make_levels(f, &lv, st)) return rc;
  const uint64_t M = (uint64_t)N * 2 * T;
  float* dsig = workspace;
  float* dcol = dsig + M;                                          // d(col), overwritten in place by d(albedo)
  float* ds_off = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + ngp_render_workspace_bytes(N, T));
  const bool offsets = ambient_ratio != 1.0f || grad_orient != nullptr;
  k_ngp_composite_bwd_wave<<<sf_div_up(N, 4), 256, 0, st>>>(
      CompositeBwdArgs{z_sorted, sigma_s, rgb_shaded_s, nears, fars, N, T, bg_color, grad_image, grad_weights_sum, dsig, dcol});
  SF_CHECK_LAUNCH("ngp_composite_bwd");
  ShadeBwdArgs sb{};
  sb.dcol = dcol; sb.rgb_s = rgb_s; sb.normal_s = normal_s; sb.grad_s = grad_s; sb.w_s = w_s; sb.rays_d = rays_d; sb.light_d = light_d;
  sb.g_orient = grad_orient; sb.P = (uint32_t)M; sb.T2 = 2 * T; sb.ratio = ambient_ratio; sb.eps = epsilon; sb.dalb = dcol; sb.ds_off = ds_off;
  k_ngp_shade_bwd<<<sf_grid_cap(sf_div_up((uint32_t)M, 256)), 256, 0, st>>>(sb);
  SF_CHECK_LAUNCH("ngp_shade_bwd");
  return ngp_bwd_field_scatter(f, g, lv, rays_o, rays_d, aabb, N, T, z_sorted, rays_per_row, nullptr, workspace, ds_off, 0, offsets ? 7 : 1, epsilon, st);
}

// ONE offset pass on its own: adds to g's buffers the gradient of sum_p ds_e[p] sigma(offset point e of sorted sample p), e = 1 .. 6 -- the
// stage sf_ngp_render_shaded_backward runs six times, for callers (and tests) that hold d(sigma) at one offset.  Workspace as
// sf_ngp_render_backward's; d(feat) of the pass is left at floats [4M, 36M) of it, level-major, M = N * 2T.
extern "C" int sf_ngp_render_offset_backward(const sf_ngp_field* f, const sf_ngp_field_grad* g, const float* rays_o, const float* rays_d,
                                             const float* aabb, uint32_t N, uint32_t T, const float* z_sorted, const float* ds_e, uint32_t e,
                                             float epsilon, uint32_t rays_per_row, float* workspace, uint64_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!f || !g || !rays_o || !rays_d || !aabb || !z_sorted || !ds_e) SF_FAIL(SF_ERR_INVALID, "ngp_render_offset_backward: null pointer");
  if (e < 1 || e > 6) SF_FAIL(SF_ERR_INVALID, "ngp_render_offset_backward: e must be in [1,6]");
  if (!isfinite(epsilon) || !(epsilon > 0.0f)) SF_FAIL(SF_ERR_INVALID, "ngp_render_offset_backward: epsilon must be finite and > 0");
  if (N == 0) return SF_OK;
  if (T < 4 || T > 64) SF_FAIL(SF_ERR_INVALID, "ngp_render_offset_backward: T must be in [4,64]");
  if ((uint64_t)N * 2 * T >= (1ull << 32)) SF_FAIL(SF_ERR_INVALID, "ngp_render_offset_backward: N * 2T must be below 2^32");
  if (!workspace || workspace_bytes < sf_ngp_render_workspace_bytes(N, T)) SF_FAIL(SF_ERR_INVALID, "ngp_render_offset_backward: workspace too small");
  NgpLevels lv;
  if (int rc = sf_ngp_make_levels(f, &lv, st)) return rc;
  return ngp_bwd_field_scatter(f, g, lv, rays_o, rays_d, aabb, N, T, z_sorted, rays_per_row, nullptr, workspace, ds_e, e, e + 1, epsilon, st);
}

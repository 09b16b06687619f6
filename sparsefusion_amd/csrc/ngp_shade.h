// Lambertian-shaded render of the fused coarse + fine sampler, no gradient (NeRFRenderer.run with shading='lambertian',
// external/nerf/renderer_df.py:404-456; NeRFNetwork.forward, external/nerf/network_grid.py:129-153).  Two kernels that run BEHIND
// the albedo forward of ngp_render.hip, on the sorted ray it leaves (z_sorted, sigma_s, albedo rgb_s):
//   k_ngp_shade                    thread per sorted sample: the sample's point, its finite-difference normal (the six offset
//                                  evaluations of ngp_point_attrs.h; the centre is NOT re-evaluated, sigma_s / rgb_s are that point's
//                                  values) and the shaded colour albedo * (ratio + (1 - ratio) * max(n . -l, 0));
//   k_ngp_composite_sorted_wave    wave per ray: the scan half of k_ngp_composite_wave (ngp_composite_wave.h:85-123) operation for
//                                  operation on the shaded colour, plus sum w n (normal image) and sum w max(n . d, 0)^2 (the
//                                  orientation term) -- a third copy of the scan next to the forward's and the backward's, so the
//                                  benchmark's hot kernel stays what it is.
// Written against sf_dev.h and ngp_device.h so that tests/hostemu runs the same source on CPU threads (tests/test_hostemu_shade.py).
// FieldPtrs / load_weights_lds come from ngp_field_lds.h, a HIP-only header: the host harness supplies its own before this file.
#pragma once
#include "sf_dev.h"
#include "ngp_device.h"
#include "ngp_point_attrs.h"
#ifndef SF_HOST_EMU
#include "ngp_field_lds.h"
#endif

struct ShadeArgs {
  FieldPtrs f; NgpLevels lv;
  const float* rays_o; const float* rays_d; const float* aabb;   // [N][3], [N][3], [6]
  const float* z_s; const float* rgb_s;                          // sorted ray [N][2T], albedo [N][2T][3]
  const float* light_d;                                          // [3] on the device (a randomly drawn light is never read by the host)
  uint32_t P, T2;                                                // N * 2T sorted samples, 2T
  float ratio, eps;
  float* normal_s; float* rgb_shaded_s; float* xyz_s;            // [N][2T][3] each; xyz_s or null
  float* grad_s;                                                 // [N][2T][3] or null: the un-normalised gradient (kept for the backward, ngp_shade_bwd.h)
};

// ngp_lambertian (ambient + diffuse factor of one sample) lives in ngp_point_attrs.h, next to the normal it shades
SF_KERNEL(256) void k_ngp_shade(ShadeArgs a) {
  SF_SHARED __attribute__((aligned(16))) float W[NGP_WTOTAL];
  load_weights_lds(W, a.f);
  sf_sync();
  float box[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) box[i] = a.aabb[i];
  const float l[3] = {a.light_d[0], a.light_d[1], a.light_d[2]};
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.P; p += (uint64_t)gridDim.x * blockDim.x) {
    // Memory clobber: stops LLVM from hoisting the loop-invariant LDS weight reads out of the grid-stride loop (k_ngp_field)
    asm volatile("" ::: "memory");
    const uint32_t n = (uint32_t)(p / a.T2);
    const float o[3] = {a.rays_o[n * 3], a.rays_o[n * 3 + 1], a.rays_o[n * 3 + 2]};
    const float d[3] = {a.rays_d[n * 3], a.rays_d[n * 3 + 1], a.rays_d[n * 3 + 2]};
    float x[3];
    ngp_point(o, d, a.z_s[p], box, x);                           // the fp32 point the field kernels evaluated for this sample
    NgpPointAttrs at;
    ngp_point_attrs(a.lv, a.f.table, W, a.f.bound, x, a.eps, 7, at, 1);
    const float lam = ngp_lambertian(at.normal, l, a.ratio);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      a.normal_s[p * 3 + c] = at.normal[c];
      a.rgb_shaded_s[p * 3 + c] = SF_MUL(a.rgb_s[p * 3 + c], lam);
      if (a.xyz_s) a.xyz_s[p * 3 + c] = x[c];
      if (a.grad_s) a.grad_s[p * 3 + c] = at.grad[c];
    }
  }
}

struct CompositeSortedArgs {
  const float* z_s; const float* sig_s; const float* col_s; const float* nrm_s;   // sorted ray [N][2T], [N][2T], [N][2T][3], [N][2T][3]
  const float* rays_d; const float* nears; const float* fars;                     // [N][3], [N], [N]
  uint32_t N, T;
  float bg;
  float* image; float* depth; float* weights_sum;                                 // [N][3], [N], [N]
  float* normal_image; float* orient;                                             // or null: [N][3] sum w n, [N] sum w max(n . d, 0)^2
  float* w_s;                                                                     // or null: [N][2T] the weights (kept for the backward)
};

SF_KERNEL(256) void k_ngp_composite_sorted_wave(CompositeSortedArgs a) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t n = blockIdx.x * 4 + wave;
  if (n >= a.N) return;                                        // whole waves leave together; no workgroup barrier below
  const uint32_t T = a.T, M = 2 * T;
  // ---- sorted positions 2 lane, 2 lane + 1
  const uint32_t m0 = 2 * lane;
  const bool live = m0 < M;                                    // M is even: both positions or none
  const size_t q = (size_t)n * M + (live ? m0 : 0);
  const float z0 = a.z_s[q], z1 = a.z_s[q + 1], s0 = a.sig_s[q], s1 = a.sig_s[q + 1];
  float c0[3], c1[3], n0[3], n1[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    c0[c] = a.col_s[q * 3 + c]; c1[c] = a.col_s[q * 3 + 3 + c];
    n0[c] = a.nrm_s[q * 3 + c]; n1[c] = a.nrm_s[q * 3 + 3 + c];
  }
  const float dir[3] = {a.rays_d[n * 3], a.rays_d[n * 3 + 1], a.rays_d[n * 3 + 2]};
  const float near = a.nears[n], far = a.fars[n];
  const float sample_dist = SF_DIV(SF_SUB(far, near), (float)T);
  const float span = SF_SUB(far, near);
  const float z_next = sf_shfl(z0, (int)((lane + 1) & 63));    // first sample of the next lane
  const float d0 = SF_SUB(z1, z0);
  const float d1 = (m0 + 2 < M) ? SF_SUB(z_next, z1) : sample_dist;
  const float a0 = live ? SF_SUB(1.0f, expf(SF_MUL(-d0, s0))) : 0.0f;
  const float a1 = live ? SF_SUB(1.0f, expf(SF_MUL(-d1, s1))) : 0.0f;
  const double f0 = live ? (double)SF_ADD(SF_SUB(1.0f, a0), 1e-15f) : 1.0;
  const double f1 = live ? (double)SF_ADD(SF_SUB(1.0f, a1), 1e-15f) : 1.0;
  double incl = f0 * f1;                                       // inclusive product scan over lanes
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double up = sf_shfl(incl, (int)((lane - d) & 63));
    if ((int)lane >= d) incl *= up;
  }
  double excl = sf_shfl(incl, (int)((lane - 1) & 63));
  if (lane == 0) excl = 1.0;
  const float w0 = SF_MUL(a0, (float)excl);
  const float w1 = SF_MUL(a1, (float)(excl * f0));
  if (a.w_s && live) { a.w_s[q] = w0; a.w_s[q + 1] = w1; }
  const float raw0 = SF_DIV(SF_SUB(z0, near), span), raw1 = SF_DIV(SF_SUB(z1, near), span);
  const float oz0 = (raw0 != raw0) ? raw0 : fminf(fmaxf(raw0, 0.0f), 1.0f);   // NaN (miss rays: 0/0) propagates like torch.clamp
  const float oz1 = (raw1 != raw1) ? raw1 : fminf(fmaxf(raw1, 0.0f), 1.0f);
  // orientation: (n * d).sum(-1).clamp(min=0) ** 2, the sum left to right
  const float nd0 = SF_ADD(SF_ADD(SF_MUL(n0[0], dir[0]), SF_MUL(n0[1], dir[1])), SF_MUL(n0[2], dir[2]));
  const float nd1 = SF_ADD(SF_ADD(SF_MUL(n1[0], dir[0]), SF_MUL(n1[1], dir[1])), SF_MUL(n1[2], dir[2]));
  const float k0 = (nd0 != nd0) ? nd0 : fmaxf(nd0, 0.0f), k1 = (nd1 != nd1) ? nd1 : fmaxf(nd1, 0.0f);
  float acc[9];
  acc[0] = live ? SF_ADD(w0, w1) : 0.0f;
  acc[1] = live ? SF_ADD(SF_MUL(w0, oz0), SF_MUL(w1, oz1)) : 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    acc[2 + c] = live ? SF_ADD(SF_MUL(w0, c0[c]), SF_MUL(w1, c1[c])) : 0.0f;
    acc[5 + c] = live ? SF_ADD(SF_MUL(w0, n0[c]), SF_MUL(w1, n1[c])) : 0.0f;
  }
  acc[8] = live ? SF_ADD(SF_MUL(w0, SF_MUL(k0, k0)), SF_MUL(w1, SF_MUL(k1, k1))) : 0.0f;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = SF_ADD(acc[k], sf_shfl_xor(acc[k], d));
  }
  if (lane == 0) {
    const float rest = SF_MUL(SF_SUB(1.0f, acc[0]), a.bg);
    a.image[n * 3 + 0] = SF_ADD(acc[2], rest); a.image[n * 3 + 1] = SF_ADD(acc[3], rest); a.image[n * 3 + 2] = SF_ADD(acc[4], rest);
    a.depth[n] = acc[1];
    a.weights_sum[n] = acc[0];
    if (a.normal_image) { a.normal_image[n * 3 + 0] = acc[5]; a.normal_image[n * 3 + 1] = acc[6]; a.normal_image[n * 3 + 2] = acc[7]; }
    if (a.orient) a.orient[n] = acc[8];
  }
}

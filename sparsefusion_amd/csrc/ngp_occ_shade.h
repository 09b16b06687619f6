// Lambertian-shaded occupancy-grid EVALUATION render (NeRFRenderer.run_cuda with shading='lambertian', eval mode;
// external/nerf/renderer_df.py:503-584 with NeRFNetwork.forward, external/nerf/network_grid.py:129-153): march + seven field
// evaluations + finite-difference normal + shading + composite in ONE launch, EIGHT LANES PER RAY.
//
// k_render_occ_eval (raymarch_occ.hip) is one ray per lane at ~207 VGPRs: two waves per SIMD, and a 128 x 128 view is 256 waves for
// 1024 SIMDs.  Shading multiplies the work per sample by seven (the centre and the six offset points of ngp_point_attrs.h) and leaves
// the number of rays alone, so the seven evaluations go ACROSS lanes: a group of 8 adjacent lanes owns one ray (8 rays per wave, 32 per
// 256-thread workgroup), lane e = lane & 7 of the group evaluates point e of ngp_point_attrs' numbering (e = 0 the sample, e = 1..6
// clamp(x +- eps e_a, -bound, bound), e = 7 nothing).  Every lane of a group carries the same Marcher state and takes the same
// steps -- the march is cheap next to the field.  Per occupied sample: one field evaluation per lane (the per-point code of
// k_ngp_field), sf_shfl brings the centre's sigma / albedo and the six offset sigmas to every lane of the group, each lane forms the
// gradient and the normal (ngp_fd_grad / ngp_fd_normal: the bits of sf_ngp_point_attrs), ngp_lambertian and albedo * lambertian, and
// accumulates exactly what k_render_occ_eval accumulates, operation for operation, plus sum w n.  Lane 0 of the group stores.
//
// CONVERGENCE.  A shuffle must not read a lane that is masked off, so the sample loop is WAVE-UNIFORM: while (any group of the wave is
// alive).  Each iteration every live group probes once, then either skips its empty cell or takes its sample; the evaluation and the
// accumulation sit under per-group / per-lane predicates, the shuffles and the loop vote sit outside them and are executed by all
// 64 lanes on every iteration (no lane returns before the loop ends: groups past N idle with alive = false).  A finished group idles
// until the wave's slowest ray ends, as it would under SIMT divergence anyway.
//
// Written against sf_dev.h / ngp_device.h so that tests/hostemu runs the same source on CPU fibers (tests/test_hostemu_occ_shade.py).
// FieldPtrs / load_weights_lds come from ngp_field_lds.h, a HIP-only header: the host harness supplies its own before this file.
#pragma once
#include "sf_dev.h"
#include "ngp_device.h"
#include "ngp_point_attrs.h"
#include "occ_marcher.h"
#ifndef SF_HOST_EMU
#include "ngp_field_lds.h"
#endif

struct OccShadeArgs {
  FieldPtrs f; NgpLevels lv;
  const float* rays_o; const float* rays_d; const float* nears; const float* fars;   // [N][3], [N][3], [N], [N]
  const uint8_t* grid;                                                               // density bitfield, C cascades of H^3 cells
  const float* noises;                                                               // [N] jitter of the first sample, or null
  const float* light_d;                                                              // [3] on the device
  float dt_gamma, T_thresh, ratio, eps;
  uint32_t max_steps, C, H, N;
  float* weights_sum; float* depth; float* image;                                    // [N], [N] un-normalised, [N][3] without background
  float* normal_image; uint32_t* n_samples;                                          // or null: [N][3] sum w n, [N] samples composited
};

SF_KERNEL(256) void k_render_occ_eval_shaded(OccShadeArgs a) {
  SF_SHARED __attribute__((aligned(16))) float W[NGP_WTOTAL];
  load_weights_lds(W, a.f);
  sf_sync();
  const uint32_t lane = threadIdx.x & 63, e = lane & 7, g0 = lane & ~7u;      // point of this lane, first lane of its group
  const uint32_t n = blockIdx.x * 32 + (threadIdx.x >> 3);
  const bool has_ray = n < a.N;
  const uint32_t nr = has_ray ? n : 0;                                         // groups past N read ray 0 (N >= 1) and never march
  const float l[3] = {a.light_d[0], a.light_d[1], a.light_d[2]};
  const float bound = a.f.bound;
  Marcher m;
  m.init(a.rays_o + (size_t)nr * 3, a.rays_d + (size_t)nr * 3, a.grid, bound, a.dt_gamma, a.max_steps, a.C, a.H);
  const float far = a.fars[nr];
  float t = a.nears[nr];
  if (a.noises) t = fmaf(m.step_size(t), a.noises[nr], t);
  float tc = a.nears[nr];                                  // the compositor's running depth (starts at rays_t = near)
  float last_t = t;
  float wsum = 0.0f, d = 0.0f, r = 0.0f, g = 0.0f, b = 0.0f, nsx = 0.0f, nsy = 0.0f, nsz = 0.0f;
  uint32_t step = 0;
  bool alive = has_ray && t < far && step < a.max_steps;
  const int axis = ((int)e - 1) >> 1;                      // -1 for the centre
  const float off = (e & 1) ? a.eps : -a.eps;
  while (sf_wave_any(alive)) {                             // wave-uniform: all 64 lanes run every iteration
    asm volatile("" ::: "memory");                         // keep the LDS weight reads inside the loop (see k_ngp_field)
    float x[3] = {0.0f, 0.0f, 0.0f}, dt = 0.0f, mb;
    int nx, ny, nz;
    bool take = false;
    if (alive) {
      take = m.probe(t, x[0], x[1], x[2], dt, nx, ny, nz, mb);
      if (!take) t = m.skip(t, x[0], x[1], x[2], nx, ny, nz, mb);
    }
    float s = 0.0f, alb[3] = {0.0f, 0.0f, 0.0f};
    if (take && e < 7) {                                   // one field evaluation per lane: point e of the sample
      float xe[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) xe[c] = e == 0 ? x[c] : ngp_clamp_sym(SF_ADD(x[c], c == axis ? off : 0.0f), bound);
      float x01[3], feat[NGP_FEAT], h1[NGP_HID], h2[NGP_HID], out[NGP_OUT];
      const bool inside = ngp_unit(xe, bound, x01);
      ngp_encode(a.lv, a.f.table, x01, inside, feat);
      ngp_mlp_forward(W, feat, h1, h2, out);
      s = expf(out[0] + ngp_blob(xe));
      alb[0] = ngp_sigmoid(out[1]);
      alb[1] = ngp_sigmoid(out[2]);
      alb[2] = ngp_sigmoid(out[3]);
    }
    // ---- all 64 lanes: the group's seven sigmas and the centre's albedo
    const float sigma = sf_shfl(s, (int)g0);
    const float a0 = sf_shfl(alb[0], (int)g0), a1 = sf_shfl(alb[1], (int)g0), a2 = sf_shfl(alb[2], (int)g0);
    const float sp0 = sf_shfl(s, (int)g0 + 1), sn0 = sf_shfl(s, (int)g0 + 2);
    const float sp1 = sf_shfl(s, (int)g0 + 3), sn1 = sf_shfl(s, (int)g0 + 4);
    const float sp2 = sf_shfl(s, (int)g0 + 5), sn2 = sf_shfl(s, (int)g0 + 6);
    if (take) {
      t += dt;
      const float gap = t - last_t;
      last_t = t;
      ++step;
      const float grad[3] = {ngp_fd_grad(sp0, sn0, a.eps), ngp_fd_grad(sp1, sn1, a.eps), ngp_fd_grad(sp2, sn2, a.eps)};
      float nrm[3];
      ngp_fd_normal(grad, nrm);
      const float lam = ngp_lambertian(nrm, l, a.ratio);
      const float alpha = 1.0f - sf_exp(-sigma * dt);
      const float T = 1.0f - wsum;
      const float weight = alpha * T;
      wsum += weight;
      tc += gap;
      d = fmaf(weight, tc, d);
      r = fmaf(weight, SF_MUL(a0, lam), r);
      g = fmaf(weight, SF_MUL(a1, lam), g);
      b = fmaf(weight, SF_MUL(a2, lam), b);
      nsx = fmaf(weight, nrm[0], nsx);
      nsy = fmaf(weight, nrm[1], nsy);
      nsz = fmaf(weight, nrm[2], nsz);
      if (T < a.T_thresh) alive = false;
    }
    alive = alive && t < far && step < a.max_steps;
  }
  if (has_ray && e == 0) {
    a.weights_sum[n] = wsum; a.depth[n] = d;
    a.image[(size_t)n * 3] = r; a.image[(size_t)n * 3 + 1] = g; a.image[(size_t)n * 3 + 2] = b;
    if (a.normal_image) { a.normal_image[(size_t)n * 3] = nsx; a.normal_image[(size_t)n * 3 + 1] = nsy; a.normal_image[(size_t)n * 3 + 2] = nsz; }
    if (a.n_samples) a.n_samples[n] = step;
  }
}

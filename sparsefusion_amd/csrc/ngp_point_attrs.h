// Point attributes of the Instant-NGP field for ONE point: sigma and albedo at the point, the central finite difference of sigma
// (NeRFNetwork.finite_difference_normal, external/nerf/network_grid.py:91-106) and its safe_normalize'd direction (normal,
// :155-164; safe_normalize, external/nerf/utils.py:41).  Plain C++ over ngp_device.h, so tests/hostemu compiles the same source
// for the CPU; the kernel and the host entry point (sf_ngp_point_attrs) are in mesh.hip.  See DESIGN.md section 9.
//
// Seven evaluations of the field, each the per-point code of k_ngp_field (ngp_unit / ngp_encode / ngp_mlp_forward / ngp_blob), so
// each is bit-identical to sf_ngp_density on the same fp32 point:
//   e = 0          the point itself, as given (not clamped, as common_forward does not clamp)
//   e = 1 .. 6     clamp(x + o, -bound, bound) with o = +eps e_a (odd e) or -eps e_a (even e), a = (e - 1) / 2: the add and the
//                  clamp in fp32 on ALL three coordinates (the reference adds a [1, 3] tensor whose other two entries are 0.0 and
//                  clamps the sum), NaN kept as torch.clamp keeps it
//   grad_a   = 0.5f * (sp_a - sn_a) / eps                      (IEEE division; written as computed: NaN / inf stay visible)
//   normal   = grad / sqrtf(fmaxf((gx gx + gy gy) + gz gz, 1e-20f)), NaN components -> 0   (no contraction)
// The evaluations run in a loop that is NOT unrolled, one after the other through the same registers: the register count is that
// of one evaluation (k_ngp_lattice's), and the latency of a level's eight gathers is hidden by the other waves of the SIMD.
#pragma once
#include "ngp_device.h"

struct NgpPointAttrs { float sigma; float albedo[3]; float grad[3]; float normal[3]; };

// torch.clamp(v, -b, b): NaN propagates (fminf / fmaxf alone would return the bound)
SF_HD float ngp_clamp_sym(float v, float b) { return (v != v) ? v : fminf(fmaxf(v, -b), b); }

// Offset point e = 1 .. 6 of x (the rule in the header comment).  One function for the forward (ngp_point_attrs below) and for the
// offset instantiations of the backward kernels (through ngp_sample_x01 below, or called by the kernel itself): the backward's point is
// the forward's fp32 point bit for bit.
SF_HD void ngp_offset_point(const float x[3], int e, float eps, float bound, float xe[3]) {
  const int axis = (e - 1) >> 1;
  const float o = (e & 1) ? eps : -eps;
#pragma unroll
  for (int d = 0; d < 3; ++d) xe[d] = ngp_clamp_sym(SF_ADD(x[d], d == axis ? o : 0.0f), bound);
}

// The point a backward kernel gathers from or scatters to, for the sorted sample at depth z of ray n: ngp_point, with OFF = 1 then offset
// point off_e = 1 .. 6 of it with step off_eps (OFF = 0 ignores both), then ngp_unit.  x: the world point, x01: its unit-cube image;
// returns whether it lies inside the grid.  Used by k_ngp_field_bwd_mfma_t (ngp_bwd_mfma.h), k_ngp_scatter_fine (ngp_scatter.h) and the
// references of tests/hostemu.  k_ngp_scatter (ngp_scatter.h) and k_ngp_bin_t (ngp_scatter_bin.h), the two scatter kernels of every
// teacher-field backward, restate these steps in their own text: that is the code their timing was measured on (the reasons are there).
template <int OFF>
SF_HD bool ngp_sample_x01(const float* __restrict__ rays_o, const float* __restrict__ rays_d, uint32_t n, float z, const float box[6],
                          float bound, uint32_t off_e, float off_eps, float x[3], float x01[3]) {
  const float o[3] = {rays_o[n * 3], rays_o[n * 3 + 1], rays_o[n * 3 + 2]};
  const float d[3] = {rays_d[n * 3], rays_d[n * 3 + 1], rays_d[n * 3 + 2]};
  ngp_point(o, d, z, box, x);
  if (OFF) {
    const float xc[3] = {x[0], x[1], x[2]};
    ngp_offset_point(xc, (int)off_e, off_eps, bound, x);
  }
  return ngp_unit(x, bound, x01);
}

// The finite-difference arithmetic, shared by ngp_point_attrs below and the eight-lanes-per-ray shaded render (ngp_occ_shade.h),
// whose normals are therefore the same bits: one component of the gradient from the sigmas at x + eps e_a and x - eps e_a ...
SF_HD float ngp_fd_grad(float sp, float sn, float eps) { return SF_DIV(SF_MUL(0.5f, SF_SUB(sp, sn)), eps); }
// ... and safe_normalize of the gradient, NaN components -> 0
SF_HD void ngp_fd_normal(const float g[3], float n[3]) {
  const float len = sqrtf(fmaxf(SF_ADD(SF_ADD(SF_MUL(g[0], g[0]), SF_MUL(g[1], g[1])), SF_MUL(g[2], g[2])), 1e-20f));
  const float nx = SF_DIV(g[0], len), ny = SF_DIV(g[1], len), nz = SF_DIV(g[2], len);
  n[0] = (nx != nx) ? 0.0f : nx;
  n[1] = (ny != ny) ? 0.0f : ny;
  n[2] = (nz != nz) ? 0.0f : nz;
}

// lambertian = ratio + (1 - ratio) * clamp(n @ (-l), min=0); the dot product left to right, nothing contracted
SF_HD float ngp_lambertian(const float n[3], const float l[3], float ratio) {
  const float dot = SF_ADD(SF_ADD(SF_MUL(n[0], -l[0]), SF_MUL(n[1], -l[1])), SF_MUL(n[2], -l[2]));
  const float lit = (dot != dot) ? dot : fmaxf(dot, 0.0f);       // torch.clamp keeps NaN
  return SF_ADD(ratio, SF_MUL(SF_SUB(1.0f, ratio), lit));
}

// n_eval = 7: everything; n_eval = 1: sigma and albedo only (grad and normal are left untouched); first_eval = 1: the centre is
// skipped (sigma and albedo are left untouched: the caller already holds that point's values -- k_ngp_shade, ngp_shade.h)
SF_HD void ngp_point_attrs(const NgpLevels& lv, const float* __restrict__ table, const float* __restrict__ W, float bound,
                           const float x[3], float eps, int n_eval, NgpPointAttrs& a, int first_eval = 0) {
  float sp = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f;
#pragma unroll 1
  for (int e = first_eval; e < n_eval; ++e) {
    // keeps the loop-invariant weight reads (LDS on the GPU) inside the loop: hoisted, they would be pinned in registers and spill
    asm volatile("" ::: "memory");
    const int axis = (e - 1) >> 1;                     // -1 for the centre
    float xe[3] = {x[0], x[1], x[2]};
    if (e != 0) ngp_offset_point(x, e, eps, bound, xe);
    float x01[3], feat[NGP_FEAT], h1[NGP_HID], h2[NGP_HID], out[NGP_OUT];
    const bool inside = ngp_unit(xe, bound, x01);
    ngp_encode(lv, table, x01, inside, feat);
    ngp_mlp_forward(W, feat, h1, h2, out);
    const float s = expf(out[0] + ngp_blob(xe));
    if (e == 0) {
      a.sigma = s;
      a.albedo[0] = ngp_sigmoid(out[1]);
      a.albedo[1] = ngp_sigmoid(out[2]);
      a.albedo[2] = ngp_sigmoid(out[3]);
    } else if (e & 1) {
      sp = s;
    } else {
      const float g = ngp_fd_grad(sp, s, eps);
      if (axis == 0) gx = g;
      else if (axis == 1) gy = g;
      else gz = g;
    }
  }
  if (n_eval < 7) return;
  a.grad[0] = gx;
  a.grad[1] = gy;
  a.grad[2] = gz;
  ngp_fd_normal(a.grad, a.normal);
}

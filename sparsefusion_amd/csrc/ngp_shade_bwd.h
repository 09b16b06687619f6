// Backward of the Lambertian shading of one sorted sample (k_ngp_shade, ngp_shade.h; NeRFNetwork.forward / finite_difference_normal /
// safe_normalize, external/nerf/network_grid.py:91-106,129-164; the orientation term, external/nerf/renderer_df.py:428-431).
// Runs between k_ngp_composite_bwd_wave (which leaves d(col) = dL / d(shaded colour) of every sample when it is given col_s) and the
// seven field-backward passes of sf_ngp_render_shaded_backward (ngp_render.hip).  With a = albedo, g = the un-normalised gradient
// (grad_s), G = g . g, len = sqrt(max(G, 1e-20)), n = g / len (normal_s, NaN components 0), l = light, d = ray direction:
//   lam   = ratio + (1 - ratio) max(n . -l, 0)                         (ngp_lambertian on normal_s: the forward's bits)
//   d(a)  = d(col) lam
//   d(n)  = (1 - ratio) [n . -l > 0] (a . d(col)) (-l)  +  g_orient w 2 max(n . d, 0) [n . d > 0] d       (the weight w is detached)
//   d(g)  = (d(n) - n (n . d(n))) / len   if G >= 1e-20,   d(n) / len   below (torch.clamp passes no gradient under its minimum)
//   d(s_e) = +- (0.5 / eps) d(g)_axis     e = 1 .. 6: + for odd e (x + eps e_axis), - for even e
// DEVIATION from torch, on purpose: a sample whose g has a non-finite component gets d(g) = 0 (torch would carry NaN into every
// parameter of the field).
// One thread per sorted sample; elementwise and memory-bound (76 bytes read, 36 written per sample; a wave's accesses are contiguous);
// SF_MUL / SF_ADD arithmetic, nothing contracted, as ngp_point_attrs.h.  Written against sf_dev.h / ngp_device.h: tests/hostemu runs
// the same source on CPU fibers (tests/test_hostemu_shade_bwd.py).
#pragma once
#include "sf_dev.h"
#include "ngp_device.h"
#include "ngp_point_attrs.h"

struct ShadeBwdArgs {
  const float* dcol;                                             // [P][3] d(shaded colour) (k_ngp_composite_bwd_wave's drgb on col_s)
  const float* rgb_s; const float* normal_s; const float* grad_s;   // [P][3] albedo, normal, un-normalised gradient (the forward's)
  const float* w_s;                                              // [P] weights (the forward's)
  const float* rays_d; const float* light_d;                     // [N][3]; [3] on the device
  const float* g_orient;                                         // [N] or null (= 0)
  uint32_t P, T2;
  float ratio, eps;
  float* dalb;                                                   // [P][3] d(albedo); may be dcol (every thread reads its row first)
  float* ds_off;                                                 // [6][P] d(sigma at offset point e), plane e - 1
};

SF_HD float ngp_dot3(const float a[3], const float b[3]) {      // left to right, nothing contracted
  return SF_ADD(SF_ADD(SF_MUL(a[0], b[0]), SF_MUL(a[1], b[1])), SF_MUL(a[2], b[2]));
}

// d(g) of one sample from d(n); g, n as the forward left them
SF_HD void ngp_fd_normal_bwd(const float g[3], const float n[3], const float dn[3], float dg[3]) {
  dg[0] = dg[1] = dg[2] = 0.0f;
  if (!(fabsf(g[0]) < INFINITY && fabsf(g[1]) < INFINITY && fabsf(g[2]) < INFINITY)) return;      // the deviation above
  const float G = ngp_dot3(g, g);
  const float len = sqrtf(fmaxf(G, 1e-20f));
  const float ndn = G >= 1e-20f ? ngp_dot3(n, dn) : 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) dg[c] = SF_DIV(SF_SUB(dn[c], SF_MUL(n[c], ndn)), len);
}

SF_KERNEL(256) void k_ngp_shade_bwd(ShadeBwdArgs a) {
  const float l[3] = {a.light_d[0], a.light_d[1], a.light_d[2]};
  const float ml[3] = {-l[0], -l[1], -l[2]};
  const float k = SF_DIV(0.5f, a.eps);
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.P; p += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = (uint32_t)(p / a.T2);
    float dc[3], alb[3], n[3], g[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      dc[c] = a.dcol[p * 3 + c]; alb[c] = a.rgb_s[p * 3 + c]; n[c] = a.normal_s[p * 3 + c]; g[c] = a.grad_s[p * 3 + c];
      d[c] = a.rays_d[r * 3 + c];
    }
    const float w = a.w_s[p];
    const float go = a.g_orient ? a.g_orient[r] : 0.0f;
    const float lam = ngp_lambertian(n, l, a.ratio);
    const float lit = ngp_dot3(n, ml), nd = ngp_dot3(n, d);
    const float s_lit = lit > 0.0f ? SF_MUL(SF_SUB(1.0f, a.ratio), ngp_dot3(alb, dc)) : 0.0f;
    const float s_ori = nd > 0.0f ? SF_MUL(SF_MUL(go, w), SF_MUL(2.0f, nd)) : 0.0f;
    float dn[3], dg[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) dn[c] = SF_ADD(SF_MUL(s_lit, ml[c]), SF_MUL(s_ori, d[c]));
    ngp_fd_normal_bwd(g, n, dn, dg);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      a.dalb[p * 3 + c] = SF_MUL(dc[c], lam);
      const float v = SF_MUL(k, dg[c]);
      a.ds_off[(size_t)(2 * c) * a.P + p] = v;                   // e = 2c + 1: x + eps e_c
      a.ds_off[(size_t)(2 * c + 1) * a.P + p] = -v;              // e = 2c + 2: x - eps e_c
    }
  }
}

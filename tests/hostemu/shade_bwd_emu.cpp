// CPU harness for the shaded render's backward (sparsefusion_amd/csrc/ngp_shade_bwd.h): k_ngp_shade_bwd and the offset instantiations
// of the field backward (k_ngp_field_bwd_mfma_t<1>, ngp_bwd_mfma.h) and of the binned scatter (k_ngp_bin_t<1>, ngp_scatter_bin.h) run on
// CPU fibers (hip_emu.h) from the SAME source the product compiles.  Driven by tests/test_hostemu_shade_bwd.py.  TEST INFRASTRUCTURE ONLY.
#ifndef SF_HOST_EMU
#define SF_HOST_EMU
#endif
#define HIPEMU_IMPLEMENTATION
#include "hip_emu.h"
#define NGP_EMU_FIELD_BWD
#include "ngp_emu_common.h"
#include "../../sparsefusion_amd/csrc/ngp_bwd_plan.h"
#include "../../sparsefusion_amd/csrc/ngp_scatter_bin.h"
#include "../../sparsefusion_amd/csrc/ngp_shade_bwd.h"

extern "C" void emu_shade_bwd(const float* dcol, const float* rgb_s, const float* normal_s, const float* grad_s, const float* w_s,
                              const float* rays_d, const float* light_d, const float* g_orient, uint32_t N, uint32_t T, float ratio,
                              float eps, uint32_t blocks, float* dalb, float* ds_off) {
  ShadeBwdArgs a{};
  a.dcol = dcol; a.rgb_s = rgb_s; a.normal_s = normal_s; a.grad_s = grad_s; a.w_s = w_s; a.rays_d = rays_d; a.light_d = light_d;
  a.g_orient = g_orient; a.P = N * 2 * T; a.T2 = 2 * T; a.ratio = ratio; a.eps = eps; a.dalb = dalb; a.ds_off = ds_off;
  hipemu::launch(blocks, 256, 0, [&] { k_ngp_shade_bwd(a); });
}

// the point every backward kernel derives for offset e of a sorted sample (ngp_sample_x01, ngp_point_attrs.h; e = 0: the sample itself)
static bool emu_sample_x01(const float* rays_o, const float* rays_d, uint32_t n, float z, const float* aabb, float bound, uint32_t e, float eps,
                           float x[3], float x01[3]) {
  return e ? ngp_sample_x01<1>(rays_o, rays_d, n, z, aabb, bound, e, eps, x, x01) : ngp_sample_x01<0>(rays_o, rays_d, n, z, aabb, bound, e, eps, x, x01);
}
extern "C" void emu_offset_points(const float* rays_o, const float* rays_d, const float* aabb, const float* z_s, uint32_t N, uint32_t T2,
                                  uint32_t e, float eps, float bound, float* xyz) {
  for (uint32_t p = 0; p < N * T2; ++p) {
    float x[3], x01[3];
    emu_sample_x01(rays_o, rays_d, p / T2, z_s[p], aabb, bound, e, eps, x, x01);
    for (int i = 0; i < 3; ++i) xyz[p * 3 + i] = x[i];
  }
}

// k_ngp_field_bwd_mfma_t<1> over all P points in one launch of `grid` workgroups, d(sigma) at the offset points in ds_e [P]; also the
// features, points and inside flags ngp_encode gives the offset points (what the kernel's re-gather loop computes)
extern "C" void emu_field_bwd_off(const float* table, const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                  const float* w0, const float* b0, const float* w1, const float* b1, const float* w2, const float* b2,
                                  float bound, const float* rays_o, const float* rays_d, const float* aabb, const float* z_s,
                                  const float* ds_e, uint32_t P, uint32_t T2, uint32_t grid, float thr, uint32_t e, float eps,
                                  float* g_w0, float* g_b0, float* g_w1, float* g_b1, float* g_w2, float* g_b2, float* dfeat, float* feat,
                                  float* xyz, float* inside_out) {
  NgpLevels lv;
  fill_levels(&lv, h_offsets, L, S, H, gridtype);
  EmuFixAcc acc(g_w0, g_b0, g_w1, g_b1, g_w2, g_b2);
  FBArgs a = emu_fb_args(lv, table, w0, b0, w1, b1, w2, b2, bound, acc, thr, rays_o, rays_d, aabb, z_s, ds_e, nullptr, dfeat, 0, P / T2, T2, P,
                         nullptr);
  a.P = P; a.off_e = e; a.off_eps = eps;
  hipemu::launch(grid, 256, FB_LDS_FLOATS * sizeof(float), [&] { k_ngp_field_bwd_mfma_t<1>(a); });
  acc.convert();
  for (uint32_t p = 0; p < P; ++p) {
    const uint32_t n = p / T2;
    float xe[3], x01[3];
    const bool inside = ngp_sample_x01<1>(rays_o, rays_d, n, z_s[p], aabb, bound, e, eps, xe, x01);
    ngp_encode(lv, table, x01, inside, feat + (size_t)p * NGP_FEAT);
    for (int i = 0; i < 3; ++i) xyz[p * 3 + i] = xe[i];
    inside_out[p] = inside ? 1.0f : 0.0f;
  }
}

// ---- references for the GPU test (tests/test_gpu_shaded_backward.py): no kernel runs here.
// The features, points and inside flags ngp_encode gives offset point e of every sorted sample (what the kernels' re-gather computes).
extern "C" void emu_offset_features(const float* table, const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                    float bound, const float* rays_o, const float* rays_d, const float* aabb, const float* z_s, uint32_t P,
                                    uint32_t T2, uint32_t e, float eps, float* feat, float* xyz, float* inside_out) {
  NgpLevels lv;
  fill_levels(&lv, h_offsets, L, S, H, gridtype);
  for (uint32_t p = 0; p < P; ++p) {
    const uint32_t n = p / T2;
    float xe[3], x01[3];
    const bool inside = ngp_sample_x01<1>(rays_o, rays_d, n, z_s[p], aabb, bound, e, eps, xe, x01);
    ngp_encode(lv, table, x01, inside, feat + (size_t)p * NGP_FEAT);
    for (int i = 0; i < 3; ++i) xyz[p * 3 + i] = xe[i];
    inside_out[p] = inside ? 1.0f : 0.0f;
  }
}

// The table gradient of ONE level from a level-major d(feat) image at offset e, in double: want[row][ch] = sum w_corner dfeat (the fp32
// corner weights ngp_cell gives, as the kernels compute them; the products and sums exact to 2^-53), sum_abs the same over magnitudes,
// count the number of addends per element.  want / sum_abs / count: [hsize][2] of that level.
// e == 0: the samples themselves, no offset.
extern "C" void emu_scatter_ref64(const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype, float bound,
                                  const float* rays_o, const float* rays_d, const float* aabb, const float* z_s, const float* dfeat, uint32_t P,
                                  uint32_t T2, uint32_t level, uint32_t e, float eps, double* want, double* sum_abs, double* count) {
  NgpLevels lv;
  fill_levels(&lv, h_offsets, L, S, H, gridtype);
  for (uint32_t p = 0; p < P; ++p) {
    const uint32_t n = p / T2;
    float x[3], x01[3];
    if (!emu_sample_x01(rays_o, rays_d, n, z_s[p], aabb, bound, e, eps, x, x01)) continue;
    NgpCell c;
    ngp_cell(lv, level, x01, c);
    for (int ch = 0; ch < 2; ++ch) {
      const double df = dfeat[((size_t)level * P + p) * 2 + ch];
      if (df == 0.0) continue;
      for (int i = 0; i < 8; ++i) {
        const size_t k = (size_t)c.row[i] * 2 + ch;
        want[k] += (double)c.w[i] * df; sum_abs[k] += fabs((double)c.w[i] * df); count[k] += 1.0;
      }
    }
  }
}

// k_ngp_bin_t<1> + k_ngp_bin_reduce at offset e against ngp_scatter (ngp_device.h) on the same offset points; as emu_bin_scatter of
// ngp_bwd_emu.cpp otherwise
extern "C" int emu_bin_scatter_off(const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype, float bound,
                                   const float* rays_o, const float* rays_d, const float* aabb, const float* z_s, const float* dfeat,
                                   uint32_t N, uint32_t T2, uint32_t first_level, uint32_t cap, uint32_t chunks, uint32_t grid, int use_ref,
                                   uint32_t e, float eps, float* gtable) {
  NgpLevels lv;
  fill_levels(&lv, h_offsets, L, S, H, gridtype);
  const uint32_t P = N * T2;
  if (use_ref) {
    for (uint32_t p = 0; p < P; ++p) {
      const uint32_t n = p / T2;
      float xe[3], x01[3], df[NGP_FEAT] = {0};
      const bool inside = ngp_sample_x01<1>(rays_o, rays_d, n, z_s[p], aabb, bound, e, eps, xe, x01);
      for (uint32_t l = first_level; l < L; ++l) { df[2 * l] = dfeat[((size_t)l * P + p) * 2]; df[2 * l + 1] = dfeat[((size_t)l * P + p) * 2 + 1]; }
      ngp_scatter(lv, gtable, x01, inside, df);
    }
    return 0;
  }
  SBArgs b{};
  SBRArgs r{};
  uint32_t tb = 0;
  for (uint32_t l = 0; l <= NGP_MAX_LEVELS; ++l) {
    b.bucket0[l] = r.bucket0[l] = tb;
    if (l >= first_level && l < L) {
      const uint32_t nb = (lv.hsize[l] + SB_ROWS - 1) >> SB_ROWS_LOG;
      if (nb > SB_MAX_BUCKETS) return 1;
      tb += nb;
    }
  }
  std::vector<uint32_t> cursor(tb, 0);
  std::vector<f32x4> ent((size_t)tb * cap);
  std::vector<long long> gacc((size_t)h_offsets[L] * 2, 0);
  b.lv = lv; b.bound = bound; b.aabb = aabb; b.dfeat = dfeat; b.gtable = gacc.data(); b.gtable_f = gtable; b.thr = sf_fix_thr(8.0 * 7.0 * P);
  b.cursor = cursor.data(); b.ent = ent.data(); b.T2 = T2; b.first_level = first_level; b.P_stride = P; b.cap = cap; b.off_e = e; b.off_eps = eps;
  r.lv = lv; r.gtable = gacc.data(); r.gtable_f = gtable; r.thr = b.thr; r.cursor = cursor.data(); r.ent = ent.data(); r.first_level = first_level; r.cap = cap;
  const uint32_t Nc = (N + chunks - 1) / chunks;
  for (uint32_t c = 0; c * Nc < N; ++c) {
    const uint32_t n0 = c * Nc, nn = n0 + Nc <= N ? Nc : N - n0;
    b.rays_o = rays_o + (size_t)n0 * 3; b.rays_d = rays_d + (size_t)n0 * 3; b.z_s = z_s + (size_t)n0 * T2; b.P = nn * T2; b.p_off = n0 * T2;
    hipemu::launch(grid, SB_THREADS, 0, [&] { k_ngp_bin_t<1>(b); });
    hipemu::launch(tb, SBR_THREADS, 0, [&] { k_ngp_bin_reduce(r); });
    for (uint32_t k = 0; k < tb; ++k) if (cursor[k]) return 2;
  }
  for (size_t i = 0; i < gacc.size(); ++i) gtable[i] += (float)((double)gacc[i] * SF_FIX_INV);
  return 0;
}

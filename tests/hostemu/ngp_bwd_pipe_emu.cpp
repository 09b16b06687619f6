// CPU harness for the pipelined field-backward kernel (sparsefusion_amd/csrc/ngp_bwd_pipe.h): k_ngp_field_bwd_pipe and
// k_ngp_field_bwd_mfma (ngp_bwd_mfma.h) run on CPU threads (hip_emu.h) over the same field cache, launched chunk by chunk the way
// sf_ngp_render_backward launches them; tests/test_hostemu_ngp_bwd_pipe.py compares d(feat) and the six MLP gradients with ==.
#ifndef SF_HOST_EMU
#define SF_HOST_EMU
#endif
#define HIPEMU_IMPLEMENTATION
#include "hip_emu.h"
#include <vector>
struct float2 { float x, y; };
#include "../../sparsefusion_amd/csrc/ngp_bwd_pipe.h"

static void fill_levels(NgpLevels* lv, const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype) {
  for (uint32_t l = 0; l < NGP_MAX_LEVELS; ++l) {
    const bool on = l < L;
    const float scale = on ? exp2f((float)l * S) * (float)H - 1.0f : 0.f;
    lv->scale[l] = scale;
    lv->resolution[l] = on ? (uint32_t)ceilf(scale) + 1 : 1;
    lv->offset[l] = on ? (uint32_t)h_offsets[l] : 0;
    lv->hsize[l] = on ? (uint32_t)(h_offsets[l + 1] - h_offsets[l]) : 1;
  }
  lv->L = L;
  lv->gridtype = gridtype;
}

// pipe: 1 = k_ngp_field_bwd_pipe, 0 = k_ngp_field_bwd_mfma.  The field cache holds the features ngp_encode gives every point behind
// some permutation of every ray's samples.  dfeat: [L][dfeat_P][2] with dfeat_P >= N * T2, or null.  Returns the number of points
// outside the unit cube.
extern "C" uint32_t emu_field_bwd_pipe(int pipe, const float* table, const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                       const float* w0, const float* b0, const float* w1, const float* b1, const float* w2, const float* b2,
                                       float bound, const float* rays_o, const float* rays_d, const float* aabb, const float* z_s,
                                       const float* dsig, const float* drgb, uint32_t N, uint32_t T2, uint32_t n_chunks, const uint32_t* start,
                                       const uint32_t* grids, float thr, uint32_t dfeat_P,
                                       float* g_w0, float* g_b0, float* g_w1, float* g_b1, float* g_w2, float* g_b2, float* dfeat) {
  const uint32_t P = N * T2, T = T2 / 2;
  NgpLevels lv;
  fill_levels(&lv, h_offsets, L, S, H, gridtype);
  std::vector<float> fc((size_t)N * T * NGP_FEAT, 0.f), ff((size_t)N * T * NGP_FEAT, 0.f);
  std::vector<uint32_t> perm((size_t)N * T2, 0);
  uint32_t n_out = 0;
  for (uint32_t p = 0; p < P; ++p) {
    const uint32_t n = p / T2, m = p - n * T2, src = (m * 7 + 3) % T2;       // (7 and T2 coprime: a permutation)
    perm[p] = src;
    float x[3], x01[3], feat[NGP_FEAT];
    ngp_point(rays_o + n * 3, rays_d + n * 3, z_s[p], aabb, x);
    const bool inside = ngp_unit(x, bound, x01);
    n_out += inside ? 0 : 1;
    ngp_encode(lv, table, x01, inside, feat);
    float* row = src < T ? &fc[((size_t)n * T + src) * NGP_FEAT] : &ff[((size_t)n * T + (src - T)) * NGP_FEAT];
    for (int i = 0; i < NGP_FEAT; ++i) row[i] = feat[i];
  }
  float* gout[6] = {g_w0, g_b0, g_w1, g_b1, g_w2, g_b2};
  const int glen[6] = {NGP_HID * NGP_FEAT, NGP_HID, NGP_HID * NGP_HID, NGP_HID, NGP_OUT * NGP_HID, NGP_OUT};
  std::vector<long long> gacc[6];
  for (int k = 0; k < 6; ++k) gacc[k].assign(glen[k], 0);
  for (uint32_t c = 0; c < n_chunks; ++c) {
    const uint32_t n0 = start[c], Nc = start[c + 1] - n0, P0 = n0 * T2;
    FBArgs a{};
    a.w0 = w0; a.b0 = b0; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.bound = bound;      // (table stays null: the cache path reads none)
    a.g_w0 = gacc[0].data(); a.g_b0 = gacc[1].data(); a.g_w1 = gacc[2].data(); a.g_b1 = gacc[3].data(); a.g_w2 = gacc[4].data(); a.g_b2 = gacc[5].data();
    a.f_w0 = g_w0; a.f_b0 = g_b0; a.f_w1 = g_w1; a.f_b1 = g_b1; a.f_w2 = g_w2; a.f_b2 = g_b2;
    a.thr = thr;
    a.lv = lv;
    a.rays_o = rays_o + (size_t)n0 * 3; a.rays_d = rays_d + (size_t)n0 * 3; a.aabb = aabb;
    a.z_s = z_s + P0; a.dsig = dsig + P0; a.drgb = drgb + (size_t)P0 * 3; a.dfeat_out = dfeat;
    a.P = Nc * T2; a.T2 = T2; a.dfeat_P = dfeat_P; a.p_off = P0;
    a.feat_c = fc.data(); a.feat_f = ff.data(); a.perm = perm.data();
    if (pipe) hipemu::launch(grids[c], 256, FB_LDS_FLOATS * sizeof(float), [&] { k_ngp_field_bwd_pipe(a); });
    else hipemu::launch(grids[c], 256, FB_LDS_FLOATS * sizeof(float), [&] { k_ngp_field_bwd_mfma(a); });
  }
  for (int k = 0; k < 6; ++k)
    for (int i = 0; i < glen[k]; ++i) gout[k][i] += (float)((double)gacc[k][i] * SF_FIX_INV);
  return n_out;
}

// What the NGP harnesses of tests/hostemu set up the same way: the level geometry, the packed weight block, the features of a set of
// points and a field cache holding them, and -- for the harnesses of the field backward, which define NGP_EMU_FIELD_BWD and get
// ngp_bwd_mfma.h with it -- the FBArgs of a launch and the fixed-point accumulators.  TEST INFRASTRUCTURE ONLY.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>
struct float2 { float x, y; };                     // ngp_device.h names it in a field helper
#include "../../sparsefusion_amd/csrc/ngp_device.h"
#include "../../sparsefusion_amd/csrc/ngp_point_attrs.h"       // ngp_sample_x01

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

static void pack_weights(std::vector<float>& W, const float* w0, const float* b0, const float* w1, const float* b1,
                         const float* w2, const float* b2) {
  W.resize(NGP_WTOTAL);
  memcpy(&W[NGP_W0], w0, sizeof(float) * NGP_HID * NGP_FEAT); memcpy(&W[NGP_B0], b0, sizeof(float) * NGP_HID);
  memcpy(&W[NGP_W1], w1, sizeof(float) * NGP_HID * NGP_HID);  memcpy(&W[NGP_B1], b1, sizeof(float) * NGP_HID);
  memcpy(&W[NGP_W2], w2, sizeof(float) * NGP_OUT * NGP_HID);  memcpy(&W[NGP_B2], b2, sizeof(float) * NGP_OUT);
}

// The features ngp_encode gives the P sorted samples of rays of T2 samples each: feat [P][32]; xyz [P][3] and inside [P] may be null.
// Returns the number of points outside the unit cube.
static uint32_t emu_encode_points(const NgpLevels& lv, const float* table, float bound, const float* rays_o, const float* rays_d,
                                  const float* aabb, const float* z_s, uint32_t P, uint32_t T2, float* feat, float* xyz, float* inside_out) {
  uint32_t n_out = 0;
  for (uint32_t p = 0; p < P; ++p) {
    const uint32_t n = p / T2;
    float x[3], x01[3];
    const bool inside = ngp_sample_x01<0>(rays_o, rays_d, n, z_s[p], aabb, bound, 0, 0.0f, x, x01);
    n_out += inside ? 0 : 1;
    ngp_encode(lv, table, x01, inside, feat + (size_t)p * NGP_FEAT);
    if (xyz)
      for (int i = 0; i < 3; ++i) xyz[p * 3 + i] = x[i];
    if (inside_out) inside_out[p] = inside ? 1.0f : 0.0f;
  }
  return n_out;
}

// A field cache as sf_ngp_render_forward leaves it, holding the given rows (feat_sorted [P][32], sorted order) behind some permutation
// of every ray's samples: perm = (m * 7 + 3) % T2 (7 and T2 coprime in every test: a permutation).
struct EmuFieldCache {
  std::vector<float> fc, ff;
  std::vector<uint32_t> perm;
  void build(const float* feat_sorted, uint32_t P, uint32_t T2) {
    const uint32_t T = T2 / 2, N = (P + T2 - 1) / T2;
    fc.assign((size_t)N * T * NGP_FEAT, 0.f); ff.assign((size_t)N * T * NGP_FEAT, 0.f); perm.assign((size_t)N * T2, 0);
    for (uint32_t p = 0; p < P; ++p) {
      const uint32_t n = p / T2, m = p - n * T2, src = (m * 7 + 3) % T2;
      perm[p] = src;
      float* row = src < T ? &fc[((size_t)n * T + src) * NGP_FEAT] : &ff[((size_t)n * T + (src - T)) * NGP_FEAT];
      for (int i = 0; i < NGP_FEAT; ++i) row[i] = feat_sorted[(size_t)p * NGP_FEAT + i];
    }
  }
};

#ifdef NGP_EMU_FIELD_BWD
#include "../../sparsefusion_amd/csrc/ngp_bwd_mfma.h"

// The six MLP gradients the way the product sums them: 64-bit fixed point (sf_dev.h), added to the float outputs at the end.
struct EmuFixAcc {
  std::vector<long long> acc[6];                   // w0, b0, w1, b1, w2, b2
  float* out[6];
  EmuFixAcc(float* g_w0, float* g_b0, float* g_w1, float* g_b1, float* g_w2, float* g_b2) : out{g_w0, g_b0, g_w1, g_b1, g_w2, g_b2} {
    const int len[6] = {NGP_HID * NGP_FEAT, NGP_HID, NGP_HID * NGP_HID, NGP_HID, NGP_OUT * NGP_HID, NGP_OUT};
    for (int k = 0; k < 6; ++k) acc[k].assign(len[k], 0);
  }
  void convert() {
    for (int k = 0; k < 6; ++k)
      for (size_t i = 0; i < acc[k].size(); ++i) out[k][i] += (float)((double)acc[k][i] * SF_FIX_INV);
  }
};

// FBArgs of the launch over rays [n0, n0 + Nc) of a set of dfeat_P / T2 or fewer rays, as sf_ngp_render_backward fills them: ray /
// sample pointers offset to the chunk, d(feat) in the layout of the whole set.  cache may be null (the re-gather path).
static FBArgs emu_fb_args(const NgpLevels& lv, const float* table, const float* w0, const float* b0, const float* w1, const float* b1,
                          const float* w2, const float* b2, float bound, EmuFixAcc& g, float thr, const float* rays_o, const float* rays_d,
                          const float* aabb, const float* z_s, const float* dsig, const float* drgb, float* dfeat, uint32_t n0, uint32_t Nc,
                          uint32_t T2, uint32_t dfeat_P, const EmuFieldCache* cache) {
  const uint32_t P0 = n0 * T2;
  FBArgs a{};
  a.table = table; a.w0 = w0; a.b0 = b0; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.bound = bound;
  a.g_w0 = g.acc[0].data(); a.g_b0 = g.acc[1].data(); a.g_w1 = g.acc[2].data(); a.g_b1 = g.acc[3].data(); a.g_w2 = g.acc[4].data(); a.g_b2 = g.acc[5].data();
  a.f_w0 = g.out[0]; a.f_b0 = g.out[1]; a.f_w1 = g.out[2]; a.f_b1 = g.out[3]; a.f_w2 = g.out[4]; a.f_b2 = g.out[5];
  a.thr = thr;
  a.lv = lv;
  a.rays_o = rays_o + (size_t)n0 * 3; a.rays_d = rays_d + (size_t)n0 * 3; a.aabb = aabb;
  a.z_s = z_s + P0; a.dsig = dsig + P0; a.drgb = drgb + (size_t)P0 * 3; a.dfeat_out = dfeat;
  a.P = Nc * T2; a.T2 = T2; a.dfeat_P = dfeat_P; a.p_off = P0;
  if (cache) { a.feat_c = cache->fc.data(); a.feat_f = cache->ff.data(); a.perm = cache->perm.data(); }
  return a;
}
#endif

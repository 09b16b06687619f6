// CPU harness for the pipelined field-backward kernel (sparsefusion_amd/csrc/ngp_bwd_pipe.h): k_ngp_field_bwd_pipe and
// k_ngp_field_bwd_mfma (ngp_bwd_mfma.h) run on CPU threads (hip_emu.h) over the same field cache, launched chunk by chunk the way
// sf_ngp_render_backward launches them; tests/test_hostemu_ngp_bwd_pipe.py compares d(feat) and the six MLP gradients with ==.
#ifndef SF_HOST_EMU
#define SF_HOST_EMU
#endif
#define HIPEMU_IMPLEMENTATION
#include "hip_emu.h"
#define NGP_EMU_FIELD_BWD
#include "ngp_emu_common.h"
#include "../../sparsefusion_amd/csrc/ngp_bwd_pipe.h"

// pipe: 1 = k_ngp_field_bwd_pipe, 0 = k_ngp_field_bwd_mfma.  The field cache holds the features ngp_encode gives every point behind
// some permutation of every ray's samples.  dfeat: [L][dfeat_P][2] with dfeat_P >= N * T2, or null.  Returns the number of points
// outside the unit cube.
extern "C" uint32_t emu_field_bwd_pipe(int pipe, const float* table, const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                       const float* w0, const float* b0, const float* w1, const float* b1, const float* w2, const float* b2,
                                       float bound, const float* rays_o, const float* rays_d, const float* aabb, const float* z_s,
                                       const float* dsig, const float* drgb, uint32_t N, uint32_t T2, uint32_t n_chunks, const uint32_t* start,
                                       const uint32_t* grids, float thr, uint32_t dfeat_P,
                                       float* g_w0, float* g_b0, float* g_w1, float* g_b1, float* g_w2, float* g_b2, float* dfeat) {
  const uint32_t P = N * T2;
  NgpLevels lv;
  fill_levels(&lv, h_offsets, L, S, H, gridtype);
  std::vector<float> feat((size_t)P * NGP_FEAT);
  const uint32_t n_out = emu_encode_points(lv, table, bound, rays_o, rays_d, aabb, z_s, P, T2, feat.data(), nullptr, nullptr);
  EmuFieldCache cache;
  cache.build(feat.data(), P, T2);
  EmuFixAcc acc(g_w0, g_b0, g_w1, g_b1, g_w2, g_b2);
  for (uint32_t c = 0; c < n_chunks; ++c) {
    // (table null: the cache path reads none)
    const FBArgs a = emu_fb_args(lv, nullptr, w0, b0, w1, b1, w2, b2, bound, acc, thr, rays_o, rays_d, aabb, z_s, dsig, drgb, dfeat, start[c],
                                 start[c + 1] - start[c], T2, dfeat_P, &cache);
    if (pipe) hipemu::launch(grids[c], 256, FB_LDS_FLOATS * sizeof(float), [&] { k_ngp_field_bwd_pipe(a); });
    else hipemu::launch(grids[c], 256, FB_LDS_FLOATS * sizeof(float), [&] { k_ngp_field_bwd_mfma(a); });
  }
  acc.convert();
  return n_out;
}

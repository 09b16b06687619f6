// CPU harness for the matrix-core field-forward kernel (sparsefusion_amd/csrc/ngp_field_mfma.h): the kernel source runs on CPU
// threads (hip_emu.h) and is compared by tests/test_hostemu_ngp_field_mfma.py, with ==, to the per-point math k_ngp_field runs
// (ngp_encode + ngp_mlp_forward + activations of ngp_device.h).
#ifndef SF_HOST_EMU
#define SF_HOST_EMU
#endif
#define HIPEMU_IMPLEMENTATION
#include "hip_emu.h"
#include "ngp_emu_common.h"
#include "../../sparsefusion_amd/csrc/ngp_field_mfma.h"

// mode 0: z from (nears, fars, lin, u) and written to z_out; mode 1: z read from z_in.  use_ref: the per-point math, serial.
// feat_out may be null.  P = N * T.
extern "C" void emu_field_fwd(int mode, const float* table, const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                              const float* w0, const float* b0, const float* w1, const float* b1, const float* w2, const float* b2,
                              float bound, const float* rays_o, const float* rays_d, const float* aabb, const float* nears,
                              const float* fars, const float* lin, const float* u, const float* z_in, uint32_t N, uint32_t T, uint32_t grid,
                              int use_ref, float* z_out, float* sigma, float* rgb, float* feat_out) {
  const uint32_t P = N * T;
  NgpLevels lv;
  fill_levels(&lv, h_offsets, L, S, H, gridtype);
  if (!use_ref) {
    FMArgs a{};
    a.table = table; a.w0 = w0; a.b0 = b0; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.bound = bound; a.lv = lv;
    a.rays_o = rays_o; a.rays_d = rays_d; a.aabb = aabb; a.nears = nears; a.fars = fars; a.lin = lin; a.u = u; a.z_in = z_in;
    a.P = P; a.T = T; a.z_out = z_out; a.sigma = sigma; a.rgb = rgb; a.feat_out = feat_out;
    if (mode == 0) hipemu::launch(grid, 256, FM_LDS_FLOATS * sizeof(float), [&] { k_ngp_field_mfma<0>(a); });
    else hipemu::launch(grid, 256, FM_LDS_FLOATS * sizeof(float), [&] { k_ngp_field_mfma<1>(a); });
    return;
  }
  std::vector<float> W;
  pack_weights(W, w0, b0, w1, b1, w2, b2);
  for (uint32_t p = 0; p < P; ++p) {                    // the body of k_ngp_field<0 / 1> (ngp_render.hip)
    const uint32_t n = p / T, k = p - n * T;
    float z;
    if (mode == 0) {
      z = ngp_coarse_z(nears[n], fars[n], lin[k], u ? u[p] : -1.0f, T);
      z_out[p] = z;
    } else {
      z = z_in[p];
    }
    float x[3], x01[3], feat[NGP_FEAT], h1[NGP_HID], h2[NGP_HID], out[NGP_OUT];
    ngp_point(rays_o + n * 3, rays_d + n * 3, z, aabb, x);
    const bool inside = ngp_unit(x, bound, x01);
    ngp_encode(lv, table, x01, inside, feat);
    if (feat_out)
      for (int i = 0; i < NGP_FEAT; ++i) feat_out[(size_t)p * NGP_FEAT + i] = feat[i];
    ngp_mlp_forward(W.data(), feat, h1, h2, out);
    sigma[p] = expf(out[0] + ngp_blob(x));
    rgb[p * 3 + 0] = ngp_sigmoid(out[1]);
    rgb[p * 3 + 1] = ngp_sigmoid(out[2]);
    rgb[p * 3 + 2] = ngp_sigmoid(out[3]);
  }
}

// number of sample points of the reference pass that fall outside the unit cube (features zero): the test wants some
extern "C" uint32_t emu_count_outside(float bound, const float* rays_o, const float* rays_d, const float* aabb, const float* z, uint32_t N,
                                      uint32_t T) {
  uint32_t c = 0;
  for (uint32_t p = 0; p < N * T; ++p) {
    float x[3], x01[3];
    ngp_point(rays_o + (p / T) * 3, rays_d + (p / T) * 3, z[p], aabb, x);
    c += ngp_unit(x, bound, x01) ? 0 : 1;
  }
  return c;
}

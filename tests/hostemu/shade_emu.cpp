// CPU harness for the shaded render's kernels (sparsefusion_amd/csrc/ngp_shade.h): k_ngp_shade and k_ngp_composite_sorted_wave run
// on CPU fibers (hip_emu.h) from the SAME source the product compiles, next to k_ngp_composite_wave (ngp_composite_wave.h), the
// albedo render's kernel they must agree with at ambient_ratio = 1.  The level geometry and the packed weight block's layout come
// from ngp_host.cpp, which this file includes.  Driven by tests/test_hostemu_shade.py.  TEST INFRASTRUCTURE ONLY.
#ifndef SF_HOST_EMU
#define SF_HOST_EMU
#endif
#define HIPEMU_IMPLEMENTATION
#include "hip_emu.h"
#include "ngp_host.cpp"
#include "../../sparsefusion_amd/csrc/sf_dev.h"

// ngp_field_lds.h (FieldPtrs, load_weights_lds) is a HIP-only header: the same struct and the same strided copy for the fibers
struct FieldPtrs {
  const float* table;
  const float* w0; const float* b0; const float* w1; const float* b1; const float* w2; const float* b2;
  float bound;
};
static inline void load_weights_lds(float* W, const FieldPtrs& f) {
  for (uint32_t i = threadIdx.x; i < NGP_HID * NGP_FEAT; i += blockDim.x) W[NGP_W0 + i] = f.w0[i];
  for (uint32_t i = threadIdx.x; i < NGP_HID * NGP_HID; i += blockDim.x) W[NGP_W1 + i] = f.w1[i];
  for (uint32_t i = threadIdx.x; i < NGP_OUT * NGP_HID; i += blockDim.x) W[NGP_W2 + i] = f.w2[i];
  for (uint32_t i = threadIdx.x; i < NGP_HID; i += blockDim.x) { W[NGP_B0 + i] = f.b0[i]; W[NGP_B1 + i] = f.b1[i]; }
  if (threadIdx.x < NGP_OUT) W[NGP_B2 + threadIdx.x] = f.b2[threadIdx.x];
}
#include "../../sparsefusion_amd/csrc/ngp_composite_wave.h"
#include "../../sparsefusion_amd/csrc/ngp_shade.h"

extern "C" void emu_shade(const float* table, const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                          const float* w0, const float* b0, const float* w1, const float* b1, const float* w2, const float* b2,
                          float bound, const float* rays_o, const float* rays_d, const float* aabb, const float* z_s,
                          const float* rgb_s, const float* light_d, uint32_t N, uint32_t T, float ratio, float eps, uint32_t blocks,
                          float* normal_s, float* rgb_shaded_s, float* xyz_s) {
  ShadeArgs a{};
  a.f = FieldPtrs{table, w0, b0, w1, b1, w2, b2, bound};
  fill_levels(&a.lv, h_offsets, L, S, H, gridtype);
  a.rays_o = rays_o; a.rays_d = rays_d; a.aabb = aabb; a.z_s = z_s; a.rgb_s = rgb_s; a.light_d = light_d;
  a.P = N * 2 * T; a.T2 = 2 * T; a.ratio = ratio; a.eps = eps;
  a.normal_s = normal_s; a.rgb_shaded_s = rgb_shaded_s; a.xyz_s = xyz_s;
  hipemu::launch(blocks, 256, 0, [&] { k_ngp_shade(a); });
}

extern "C" void emu_composite_sorted(const float* z_s, const float* sig_s, const float* col_s, const float* nrm_s, const float* rays_d,
                                     const float* nears, const float* fars, uint32_t N, uint32_t T, float bg, float* image,
                                     float* depth, float* ws, float* normal_image, float* orient) {
  CompositeSortedArgs a{z_s, sig_s, col_s, nrm_s, rays_d, nears, fars, N, T, bg, image, depth, ws, normal_image, orient};
  hipemu::launch((N + 3) / 4, 256, 0, [&] { k_ngp_composite_sorted_wave(a); });
}

extern "C" void emu_composite_wave(const float* z_c, const float* sig_c, const float* rgb_c, const float* z_f, const float* sig_f,
                                   const float* rgb_f, const float* nears, const float* fars, uint32_t N, uint32_t T, float bg,
                                   float* z_s, float* sig_s, float* rgb_s, float* image, float* depth, float* ws) {
  CompositeArgs a{z_c, sig_c, rgb_c, z_f, sig_f, rgb_f, nears, fars, N, T, bg, z_s, sig_s, rgb_s, image, depth, ws, nullptr};
  hipemu::launch((N + 3) / 4, 256, 4 * 5 * 2 * T * sizeof(float), [&] { k_ngp_composite_wave(a); });
}

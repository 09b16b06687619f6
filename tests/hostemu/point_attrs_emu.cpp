// Host emulation of k_ngp_point_attrs (sparsefusion_amd/csrc/mesh.hip): the SAME per-point device function
// (sparsefusion_amd/csrc/ngp_point_attrs.h) compiled with g++ and run thread by thread over the kernel's grid-stride schedule, so
// its logic can be checked against the oracle without a GPU.  The level geometry and the packed weight block come from
// ngp_host.cpp, which this file includes.  TEST INFRASTRUCTURE ONLY -- never loaded by the sparsefusion_amd package.
#include "ngp_host.cpp"
#include "../../sparsefusion_amd/csrc/ngp_point_attrs.h"

// blocks x 256 "threads" walk the points as the kernel does (base += blocks * 256, tail threads idle); null outputs are skipped
extern "C" void emu_point_attrs(const float* table, const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                                const float* b2, float bound, const float* xyz, uint32_t P, float eps, uint32_t blocks,
                                float* sigma, float* albedo, float* grad, float* normal) {
  NgpLevels lv; fill_levels(&lv, h_offsets, L, S, H, gridtype);
  std::vector<float> W; pack_weights(W, w0, b0, w1, b1, w2, b2);
  const int n_eval = (grad || normal) ? 7 : 1;
#pragma omp parallel for schedule(dynamic, 1)
  for (int64_t b = 0; b < (int64_t)blocks; ++b) {
    for (uint64_t base = (uint64_t)b * 256; base < P; base += (uint64_t)blocks * 256) {
      for (uint32_t t = 0; t < 256; ++t) {
        const uint64_t p = base + t;
        if (p >= P) continue;
        const float x[3] = {xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2]};
        NgpPointAttrs a;
        ngp_point_attrs(lv, table, W.data(), bound, x, eps, n_eval, a);
        if (sigma) sigma[p] = a.sigma;
        for (int c = 0; c < 3; ++c) {
          if (albedo) albedo[3 * p + c] = a.albedo[c];
          if (grad) grad[3 * p + c] = a.grad[c];
          if (normal) normal[3 * p + c] = a.normal[c];
        }
      }
    }
  }
}

// CPU harness for the atomic table-gradient scatter (sparsefusion_amd/csrc/ngp_scatter.h): k_ngp_scatter<1024, OFF> and
// k_ngp_scatter_fine<OFF> run on CPU fibers (hip_emu.h) from the SAME source the product compiles, launched the way
// ngp_bwd_field_scatter launches them.  Driven by tests/test_hostemu_ngp_scatter.py, which compares with the float64 corner sums of
// emu_scatter_ref64 (shade_bwd_emu.cpp).  TEST INFRASTRUCTURE ONLY.
#ifndef SF_HOST_EMU
#define SF_HOST_EMU
#endif
#define HIPEMU_IMPLEMENTATION
#include "hip_emu.h"
#include "ngp_emu_common.h"
#include "../../sparsefusion_amd/csrc/sf_dev.h"

// Which route every addend took, counted at the three calls the kernels make (the wrappers change nothing else):
//   [0] tag compare-and-swaps that found the slot free or holding the same row (the addend went to the LDS cache)
//   [1] ... that found another row (the addend fell through to the global table)
//   [2] fixed-point adds (the cache's flush to the table included), [3] addends sent to the fp32 table
static uint64_t g_route[4];
static inline uint32_t emu_counted_cas(uint32_t* p, uint32_t expect, uint32_t desired) {
  const uint32_t prev = sf_atomic_cas_u32(p, expect, desired);
  ++g_route[prev == expect || prev == desired ? 0 : 1];
  return prev;
}
static inline void emu_counted_global_add(float* p, float v) { ++g_route[3]; sf_global_add(p, v); }
static inline void emu_counted_fix_add(long long* p, long long v) { ++g_route[2]; sf_fix_add(p, v); }
static inline void emu_counted_grad_add(long long* acc, float* f32, float v, float thr) {
  ++g_route[fabsf(v) < thr ? 2 : 3];
  sf_grad_add(acc, f32, v, thr);
}
#define sf_atomic_cas_u32 emu_counted_cas
#define sf_global_add emu_counted_global_add
#define sf_fix_add emu_counted_fix_add
#define sf_grad_add emu_counted_grad_add
#include "../../sparsefusion_amd/csrc/ngp_scatter.h"
#undef sf_atomic_cas_u32
#undef sf_global_add
#undef sf_fix_add
#undef sf_grad_add

// kernel 0: k_ngp_scatter<1024, OFF> over all N rays, levels [0, levels) with [0, cached_levels) of them through the LDS cache.
// kernel 1: k_ngp_scatter_fine<OFF>, levels [levels, L), `chunks` launches over consecutive ray ranges of `grid` workgroups each (ray /
//           sample pointers offset to the chunk, d(feat) in the layout of the whole set).
// OFF = (e != 0).  dfeat: level-major [L][N * T2][2].  gtable [rows][2]: the fp32 table gradient, fixed-point sums converted at the end.
// stats [6]: the four route counts above, the largest table row any walked cell names, and 1 if one of them equals SC_EMPTY.
extern "C" int emu_ngp_scatter(const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype, float bound,
                               const float* rays_o, const float* rays_d, const float* aabb, const float* z_s, const float* dfeat,
                               uint32_t N, uint32_t T2, int kernel, uint32_t rays_per_row, uint32_t cached_levels, uint32_t levels,
                               uint32_t chunks, uint32_t grid, float thr, uint32_t e, float eps, float* gtable, uint64_t* stats) {
  NgpLevels lv;
  fill_levels(&lv, h_offsets, L, S, H, gridtype);
  const uint32_t P = N * T2;
  std::vector<long long> gacc((size_t)h_offsets[L] * 2, 0);           // fixed-point sums (sf_dev.h), added to gtable at the end
  for (int i = 0; i < 4; ++i) g_route[i] = 0;
  SCArgs s{};
  s.lv = lv; s.bound = bound; s.aabb = aabb; s.dfeat = dfeat; s.gtable = gacc.data(); s.gtable_f = gtable; s.thr = thr; s.T2 = T2;
  s.first_level = levels; s.P_stride = P; s.off_e = e; s.off_eps = eps;
  if (kernel == 0) {
    if (levels > L || cached_levels > levels) return 1;
    const uint32_t g = (N + SC_RAYS - 1) / SC_RAYS;
    auto k = e ? &k_ngp_scatter<1024, 1> : &k_ngp_scatter<1024, 0>;        // the argument order of ngp_bwd_field_scatter's launch
    hipemu::launch(g, 1024, SC_LDS_BYTES, [&] {
      k(lv, bound, gacc.data(), gtable, thr, rays_o, rays_d, aabb, z_s, dfeat, N, T2, rays_per_row, cached_levels, levels, SC_RUN, e, eps);
    });
  } else {
    if (levels >= L || chunks == 0) return 1;
    const uint32_t Nc = (N + chunks - 1) / chunks;
    for (uint32_t c = 0; c * Nc < N; ++c) {
      const uint32_t n0 = c * Nc, nn = n0 + Nc <= N ? Nc : N - n0;
      s.rays_o = rays_o + (size_t)n0 * 3; s.rays_d = rays_d + (size_t)n0 * 3; s.z_s = z_s + (size_t)n0 * T2; s.N = nn; s.p_off = n0 * T2;
      if (e) hipemu::launch(grid, 256, 0, [&] { k_ngp_scatter_fine<1>(s); });
      else hipemu::launch(grid, 256, 0, [&] { k_ngp_scatter_fine<0>(s); });
    }
  }
  for (size_t i = 0; i < gacc.size(); ++i) gtable[i] += (float)((double)gacc[i] * SF_FIX_INV);
  for (int i = 0; i < 4; ++i) stats[i] = g_route[i];
  // the rows the walked cells name (the reserved tag SC_EMPTY must not be among them)
  const uint32_t l0 = kernel == 0 ? 0 : levels, l1 = kernel == 0 ? levels : L;
  uint32_t max_row = 0, reserved = 0;
  for (uint32_t p = 0; p < P; ++p) {
    float x[3], x01[3];
    const bool inside = e ? ngp_sample_x01<1>(rays_o, rays_d, p / T2, z_s[p], aabb, bound, e, eps, x, x01)
                          : ngp_sample_x01<0>(rays_o, rays_d, p / T2, z_s[p], aabb, bound, e, eps, x, x01);
    if (!inside) continue;
    for (uint32_t l = l0; l < l1; ++l) {
      NgpCell c;
      ngp_cell(lv, l, x01, c);
      for (int i = 0; i < 8; ++i) {
        if (c.row[i] > max_row) max_row = c.row[i];
        if (c.row[i] == SC_EMPTY) reserved = 1;
      }
    }
  }
  stats[4] = max_row; stats[5] = reserved;
  return 0;
}

// out [3] for one level: rows, 1 if the level is wrapped (its (res + 1)^3 corners exceed the rows), 1 if z-dropped (ngp_z_dropped)
extern "C" void emu_level_kind(const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype, uint32_t level, uint32_t* out) {
  NgpLevels lv;
  fill_levels(&lv, h_offsets, L, S, H, gridtype);
  const uint64_t step = (uint64_t)lv.resolution[level] + 1;
  out[0] = lv.hsize[level];
  out[1] = step * step * step > lv.hsize[level] ? 1u : 0u;
  out[2] = ngp_z_dropped(lv, level) ? 1u : 0u;
}

// CPU harness for the mesh-export kernels (sparsefusion_amd/csrc/mesh_kernels.h): the kernel source runs on CPU fibers (hip_emu.h)
// with the launch geometry of mesh.hip's host entry points.  Host pointers.
#ifndef SF_HOST_EMU
#define SF_HOST_EMU
#endif
#define HIPEMU_IMPLEMENTATION
#include "hip_emu.h"
#include <vector>
#include "../../sparsefusion_amd/csrc/mesh_kernels.h"

static uint32_t div_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

// sf_gaussian3d: axis 0 in -> out, axis 1 out -> tmp, axis 2 tmp -> out (+ partial sums), statistics; returns 0, or 1 for bad taps
extern "C" int emu_gaussian3d(const float* in, float* out, uint32_t nx, uint32_t ny, uint32_t nz, float sigma, float truncate,
                              double* stats) {
  GaussTaps taps;
  if (!gs_make_taps(sigma, truncate, &taps)) return 1;
  const uint64_t N = (uint64_t)nx * ny * nz;
  std::vector<float> tmp(N);
  const uint64_t tiles = (uint64_t)nx * ny * div_up(nz, GS_NT);
  const uint32_t nwg = (uint32_t)(tiles < GS_STAT_WG ? tiles : GS_STAT_WG);
  std::vector<double> partial(2 * (size_t)nwg);
  float* t = tmp.data();
  hipemu::launch(div_up((uint64_t)div_up(nx, GS_SEG) * ny * nz, GS_NT), GS_NT, 0, [&] { k_gauss_strided(in, out, 1, nx, ny * nz, taps); });
  hipemu::launch(div_up((uint64_t)nx * div_up(ny, GS_SEG) * nz, GS_NT), GS_NT, 0, [&] { k_gauss_strided(out, t, nx, ny, nz, taps); });
  double* pp = stats ? partial.data() : nullptr;
  hipemu::launch(nwg, GS_NT, 0, [&] { k_gauss_rows(t, out, (uint64_t)nx * ny, nz, taps, pp); });
  if (stats) hipemu::launch(1, GS_NT, 0, [&] { k_gauss_stats(pp, nwg, N, stats); });
  return 0;
}

// sf_mc_count + sf_mc_emit in one call: counts2 = {V, F}; verts / faces are written when given (a first call with NULL sizes them)
extern "C" void emu_mc(const float* vol, uint32_t nx, uint32_t ny, uint32_t nz, float iso, uint32_t* counts2, float* verts, int32_t* faces) {
  const uint64_t N = (uint64_t)nx * ny * nz;
  const uint32_t nb = div_up(N, MC_BLOCK);
  std::vector<uint16_t> code(N);
  std::vector<uint32_t> vbase(N), bsum(2 * (size_t)nb), boff(2 * (size_t)nb);
  const McDims d{nx, ny, nz};
  hipemu::launch(nb, MC_NT, 0, [&] { k_mc_classify(vol, d, iso, code.data(), bsum.data()); });
  hipemu::launch(1, MC_NT, 0, [&] { k_mc_scan(bsum.data(), nb, boff.data(), counts2); });
  if (!verts || !faces) return;
  hipemu::launch(nb, MC_NT, 0, [&] { k_mc_emit_verts(vol, d, iso, code.data(), boff.data(), verts, vbase.data()); });
  hipemu::launch(nb, MC_NT, 0, [&] { k_mc_emit_faces(d, code.data(), boff.data(), vbase.data(), faces); });
}

// the kernel's tables, for the table-consistency test
extern "C" void emu_mc_tables(int8_t* tri, int8_t* edge_owner) {
  memcpy(tri, mc_tri, sizeof(mc_tri));
  memcpy(edge_owner, mc_edge_owner, sizeof(mc_edge_owner));
}

// CPU harness for the mesh clean-up kernels (sparsefusion_amd/csrc/mesh_clean.h): the kernel source runs on CPU fibers (hip_emu.h) in
// the launch order of mesh.hip's host entry points.  Host pointers.  The element-wise kernels are grid-stride, so the harness
// takes their workgroup size `nt` and a cap on the number of workgroups (0: one thread per element, as many workgroups as that needs);
// the scan kernels have the fixed geometry of marching cubes.  The kernels without workgroup barriers (hook, flatten, count) run
// with sf_emu_atomic_yield: the lanes of a wave advance one atomic at a time, so a lane's compare-and-swap does meet words that
// other lanes changed after it read them.
#ifndef SF_HOST_EMU
#define SF_HOST_EMU
#endif
#define HIPEMU_IMPLEMENTATION
#include "hip_emu.h"
#include <vector>
#include "../../sparsefusion_amd/csrc/mesh_clean.h"

static uint32_t div_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }
static uint32_t grid_of(uint64_t n, uint32_t nt, uint32_t max_blocks) {
  uint32_t g = div_up(n, nt);
  if (max_blocks && g > max_blocks) g = max_blocks;
  return g ? g : 1;
}

// sf_mesh_components; face_label may be NULL
extern "C" void emu_mesh_components(const int32_t* faces, uint32_t F, uint32_t V, int32_t* vertex_label, int32_t* face_label,
                                    uint32_t* faces_per_label, uint32_t* counts3, uint32_t nt, uint32_t max_blocks) {
  std::vector<uint32_t> parent(V);
  uint32_t* par = parent.data();
  const uint32_t gv = grid_of(V, nt, max_blocks), gf = grid_of(F, nt, max_blocks);
  hipemu::launch(gv, nt, 0, [&] { k_cc_init(par, faces_per_label, counts3, V); });
  sf_emu_atomic_yield = true;
  if (F && V) hipemu::launch(gf, nt, 0, [&] { k_cc_hook(faces, F, V, par); });
  if (V) hipemu::launch(gv, nt, 0, [&] { k_cc_flatten(par, V, vertex_label); });
  if (F) hipemu::launch(gf, nt, 0, [&] { k_cc_count(faces, F, V, vertex_label, face_label, faces_per_label, counts3); });
  sf_emu_atomic_yield = false;
  if (F && V) hipemu::launch(gv, nt, 0, [&] { k_cc_stats(faces_per_label, V, counts3); });
}

// sf_mesh_filter_count + sf_mesh_filter_emit in one call: counts2 = {V', F'}; the outputs are written when given (a first call with
// NULL sizes them)
extern "C" void emu_mesh_filter(const uint32_t* verts, const int32_t* faces, uint32_t F, uint32_t V, const int32_t* vertex_label,
                                const uint32_t* faces_per_label, const uint32_t* counts3, uint32_t min_faces, double min_fraction,
                                uint32_t* counts2, uint32_t* out_verts, int32_t* out_faces, int32_t* vertex_ids, int32_t* face_ids,
                                uint32_t nt, uint32_t max_blocks) {
  const uint32_t big = V > F ? V : F, nb = big ? div_up(big, MC_BLOCK) : 1;
  std::vector<uint8_t> vert_keep((size_t)V + 1, 7), face_keep((size_t)F + 1, 7);
  std::vector<uint32_t> remap((size_t)V + 1, 0xffffffffu), bsum(2 * (size_t)nb), boff(2 * (size_t)nb);
  uint8_t *vk = vert_keep.data(), *fk = face_keep.data();
  if (V) hipemu::launch(grid_of(V, nt, max_blocks), nt, 0, [&] { k_flt_zero(vk, V); });
  if (F) hipemu::launch(grid_of(F, nt, max_blocks), nt, 0, [&] {
    k_flt_flags(faces, F, V, vertex_label, faces_per_label, counts3, min_faces, min_fraction, fk, vk);
  });
  hipemu::launch(nb, MC_NT, 0, [&] { k_flt_bsum(vk, V, fk, F, bsum.data()); });
  hipemu::launch(1, MC_NT, 0, [&] { k_mc_scan(bsum.data(), nb, boff.data(), counts2); });
  if (!vertex_ids || !face_ids) return;
  if (V) hipemu::launch(div_up(V, MC_BLOCK), MC_NT, 0, [&] { k_flt_emit_verts(verts, V, vk, boff.data(), out_verts, vertex_ids, remap.data()); });
  if (F) hipemu::launch(div_up(F, MC_BLOCK), MC_NT, 0, [&] { k_flt_emit_faces(faces, F, fk, boff.data(), remap.data(), out_faces, face_ids); });
}

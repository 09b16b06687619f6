// Host emulation of k_ngp_texture_bake (sparsefusion_amd/csrc/mesh.hip): the SAME per-texel device function and the SAME layout /
// argument check (sparsefusion_amd/csrc/ngp_texture.h) compiled with g++ and run thread by thread over the kernel's grid-stride
// schedule, so its logic can be checked without a GPU.  The level geometry and the packed weight block come from ngp_host.cpp, which
// this file includes.  TEST INFRASTRUCTURE ONLY -- never loaded by the sparsefusion_amd package.
#include "ngp_host.cpp"
#include "../../sparsefusion_amd/csrc/ngp_texture.h"

// the layout and its argument check alone: the return code of ngp_atlas_make, G and c
extern "C" int emu_atlas_make(uint32_t F, uint32_t W, uint32_t* G, uint32_t* c) {
  NgpAtlas at;
  const int rc = ngp_atlas_make(F, W, &at);
  *G = at.G; *c = at.c;
  return rc;
}

// blocks x 256 "threads" walk the texels as the kernel does (base += blocks * 256, tail threads idle); null outputs are skipped.
// Returns the code of the argument check; on a refusal nothing is read or written.
extern "C" int emu_texture_bake(const float* table, const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                                const float* b2, float bound, const float* verts, uint32_t V, const int32_t* faces, uint32_t F,
                                uint32_t Wtex, uint32_t blocks, uint8_t* rgb8, float* albedo, float* xyz, int32_t* face_id) {
  NgpAtlas at;
  if (const int rc = ngp_atlas_make(F, Wtex, &at)) return rc;
  NgpLevels lv; fill_levels(&lv, h_offsets, L, S, H, gridtype);
  std::vector<float> W; pack_weights(W, w0, b0, w1, b1, w2, b2);
  const NgpTexOut o{rgb8, albedo, xyz, face_id};
  const uint64_t P = (uint64_t)Wtex * Wtex;
#pragma omp parallel for schedule(dynamic, 1)
  for (int64_t b = 0; b < (int64_t)blocks; ++b) {
    for (uint64_t base = (uint64_t)b * 256; base < P; base += (uint64_t)blocks * 256) {
      for (uint32_t t = 0; t < 256; ++t) {
        if (base + t >= P) continue;
        ngp_texture_texel(lv, table, W.data(), bound, at, verts, V, faces, F, (uint32_t)(base + t), o);
      }
    }
  }
  return 0;
}

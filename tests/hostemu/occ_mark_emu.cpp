// CPU harness for the camera-coverage culling of the density grid (sparsefusion_amd/csrc/occ_mark.h): k_occ_mark_untrained runs on CPU
// fibers (hip_emu.h) from the SAME source the product compiles -- one lane per Morton index, the camera chunks staged in `__shared__`
// storage between two __syncthreads(), the early-exit ballot and the n_marked reduction as whole-wave rendezvous (a lane that returned
// early, or a wave that skipped a barrier, aborts the run).  The grid is the one sf_occ_mark_untrained launches, or a smaller one.  Driven by
// tests/test_hostemu_occ_mark.py.  TEST INFRASTRUCTURE ONLY.
#ifndef SF_HOST_EMU
#define SF_HOST_EMU
#endif
#define HIPEMU_IMPLEMENTATION
#include "hip_emu.h"
struct float2 { float x, y; };                                  // ngp_device.h (SF_MUL / SF_ADD / ...) names it in a field helper
#include "../../sparsefusion_amd/csrc/occ_mark.h"

extern "C" void emu_occ_mark_untrained(const float* poses, const float* intrinsics, uint32_t B, float bound, uint32_t C, uint32_t H,
                                       float* density_grid, int32_t* count, uint32_t* n_marked, uint32_t max_blocks) {
  *n_marked = 0;                                                  // the entry's hipMemsetAsync
  OccMarkArgs a{};
  a.poses = poses; a.intrinsics = intrinsics; a.B = B; a.C = C; a.H = H; a.bound = bound;
  a.grid = density_grid; a.count = count; a.n_marked = n_marked;
  unsigned blocks = occ_mark_grid(H);                             // the grid sf_occ_mark_untrained launches ...
  if (max_blocks && max_blocks < blocks) blocks = max_blocks;     // ... or fewer workgroups, to stride over the tiles at a small H
  hipemu::launch(blocks, OCC_MARK_BLOCK, 0, [&] { k_occ_mark_untrained(a); });
}

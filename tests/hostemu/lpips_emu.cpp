// CPU harness for the small kernels of the perceptual-loss plans (sparsefusion_amd/csrc/lpips_kernels.h): max pooling forward /
// backward, the LPIPS heads, ReLU backward, the scaling layer.  The SAME kernel source runs on CPU fibers (hip_emu.h), launched from
// the SAME op decoding as the gfx950 dispatch (lpips_launch_of / LPIPS_DISPATCH), on host pointers.  Driven by tests/test_hostemu_lpips.py.
// TEST INFRASTRUCTURE ONLY.
#ifndef SF_HOST_EMU
#define SF_HOST_EMU
#endif
#define HIPEMU_IMPLEMENTATION
#include "hip_emu.h"
#include "../../sparsefusion_amd/csrc/lpips_kernels.h"

#define LPIPS_EMU_LAUNCH(kernel, ...) hipemu::launch(L.grid, L.block, 0, [&] { kernel(__VA_ARGS__); })

extern "C" int emu_lpips_plan_run(const sf_op* ops, uint32_t n_ops, char* err, int errn) {
  for (uint32_t k = 0; k < n_ops; ++k) {
    const sf_op& op = ops[k];
    LpipsLaunch L;
    if (const char* e = lpips_launch_of(op, L)) {
      snprintf(err, (size_t)errn, "op %u: %s (op type %d, flags %d)", k, e, op.type, op.flags);
      return 1;
    }
    LPIPS_DISPATCH(op, L, LPIPS_EMU_LAUNCH)
  }
  return 0;
}

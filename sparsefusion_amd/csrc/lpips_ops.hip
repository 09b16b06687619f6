// Extra plan ops for the perceptual-loss term of the distillation step:
// LPIPS(net='vgg') as called by external/external_utils.py:11-50 / sparsefusion/distillation.py:312-314.
// The VGG16 convs run on the conv kernels of unet_ops.hip (ReLU in the epilogue); what is left -- max pooling, the per-layer heads, ReLU
// backward, the scaling layer -- are the kernels of lpips_kernels.h, and this file is their host dispatch.

#include "sf_common.h"
#include "plan_ops.h"
#include "lpips_kernels.h"

#define LPIPS_GPU_LAUNCH(kernel, ...) kernel<<<L.grid, L.block, 0, st>>>(__VA_ARGS__)

int sf_plan_extra_op(const sf_op* opp, void* stream) {
  const sf_op& op = *opp;
  hipStream_t st = (hipStream_t)stream;
  if (op.type == SF_OP_POOL && op.flags == 2) return sf_plan_eft_op(opp, stream);          // 3x3 / 2 stem pooling (eft_ops.hip)
  LpipsLaunch L;
  if (const char* err = lpips_launch_of(op, L)) SF_FAIL(SF_ERR_INVALID, "%s (op type %d, flags %d)", err, op.type, op.flags);
  LPIPS_DISPATCH(op, L, LPIPS_GPU_LAUNCH)
  SF_CHECK_LAUNCH(L.name);
  return SF_OK;
}

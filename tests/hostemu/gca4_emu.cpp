// CPU harness for the 4x4-level compile-time-geometry kernels (sparsefusion_amd/csrc/fused_gca4.h) and the (256, 16) row of k_gca_net0_t next to
// the general kernels they replace, on the same ops: both kernel sources run on CPU threads (hip_emu.h), the op decoding and the "does the
// new kernel take this op" predicates are the product's (fused_host.h), the dispatch mirrors run_fconv / run_pool_rc_pair / run_gca of
// csrc/unet_fused.hip.  Test infrastructure only.
#ifndef SF_HOST_EMU
#define SF_HOST_EMU
#endif
#define HIPEMU_IMPLEMENTATION
#include "hip_emu.h"
#include "../../sparsefusion_amd/csrc/fused_host.h"

static int g_launches[4] = {0, 0, 0, 0};
extern "C" int emu_gca4_launches(int family) { return (family >= 0 && family < 4) ? g_launches[family] : 0; }

static int run_one(const sf_op* op, char* err, int errn) {
  if (op->type == SF_OP_FCONV) {
    FConvArgs a;
    int WM, WN;
    uint32_t grid, lds;
    if (fconv_setup(*op, a, WM, WN, grid, lds, err, (size_t)errn)) return 1;
    if (conv4_1x1_ok(*op, a, WM, WN, false)) {
      hipemu::launch(SF_CONV4_1X1_COUT / 16, 512, Conv41x1Geom<SF_CONV4_1X1_CIN, SF_CONV4_1X1_COUT>::LDS_BYTES,
                     [&] { k_conv4_1x1_t<SF_CONV4_1X1_CIN, SF_CONV4_1X1_COUT>(a); });
      ++g_launches[1];
      return 0;
    }
    if (WM != 1 || WN != 1 || a.norm != FNORM_NONE || a.s1.mode) { snprintf(err, errn, "gca4 emu: only the plain 16 x 16 tile"); return 1; }
    hipemu::launch(grid, SF_FCONV_WAVES * 64, lds, [&] { k_conv_fused<1, 1, 12, FNORM_NONE, 0, SF_FCONV_WAVES>(a); });
    return 0;
  }
  if (op->type == SF_OP_GCA) {
    GcaPoolArgs pa;
    GcaNetArgs na;
    GcaGateArgs ga;
    uint32_t grid;
    if (gca_setup(*op, pa, na, ga, grid, err, (size_t)errn)) return 1;
    if (op->flags == 1) {
      const int g4 = gca_pool4_groups(*op, pa);
      if (g4 == 5) hipemu::launch(grid, 256, 0, [&] { k_gca_pool4_t<SF_POOL4_C, 4>(pa); });
      else if (g4 == 1) hipemu::launch(grid, 256, 0, [&] { k_gca_pool4_t<SF_POOL4_C, 0>(pa); });
      else hipemu::launch(grid, 256, 0, [&] { k_gca_pool(pa); });
      if (g4) ++g_launches[0];
      return 0;
    }
    if (op->flags == 2) {
      if (!(op->i[5] & 1) && na.B == 1 && na.C == 256 && na.Kp == 256 && na.chunks > 8 && na.chunks <= 16) {
        hipemu::launch(grid, 256, 0, [&] { k_gca_net0_t<256, 16>(na); });
        ++g_launches[3];
        return 0;
      }
      if (na.chunks <= 8 || na.chunks > 16) { snprintf(err, errn, "gca4 emu: net0 with 9..16 chunks only"); return 1; }
      hipemu::launch(grid, 256, 0, [&] { k_gca_net0<16>(na); });
      return 0;
    }
  }
  snprintf(err, errn, "gca4 emu: op type %d stage %d not supported", op->type, op->flags);
  return 1;
}

static int run_pair(const sf_op* op1, const sf_op* op2, char* err, int errn) {
  FConvArgs b;
  int WM, WN;
  uint32_t gb, lds, gp;
  GcaPoolArgs pa;
  GcaNetArgs na;
  GcaGateArgs ga;
  if (op2->type != SF_OP_GCA || fconv_setup(*op1, b, WM, WN, gb, lds, err, (size_t)errn) || gca_setup(*op2, pa, na, ga, gp, err, (size_t)errn)) return 1;
  if (op2->flags != 1 || b.norm != FNORM_NONE || b.s1.mode || WM != 1 || WN != 1) { snprintf(err, errn, "pool || res_conv pair: bad operands"); return 1; }
  const int g4 = gca_pool4_groups(*op2, pa);
  if (g4 && conv4_1x1_ok(*op1, b, WM, WN, true) && pa.C == SF_CONV4_1X1_COUT) {
    constexpr uint32_t l4 = Conv41x1Geom<SF_CONV4_1X1_CIN, SF_CONV4_1X1_COUT>::LDS_BYTES;
    if (g4 == 5) hipemu::launch(gb + gp, 512, l4, [&] { k_gca_pool4_rc_t<SF_CONV4_1X1_CIN, SF_POOL4_C, 4>(pa, b, (int)gb); });
    else hipemu::launch(gb + gp, 512, l4, [&] { k_gca_pool4_rc_t<SF_CONV4_1X1_CIN, SF_POOL4_C, 0>(pa, b, (int)gb); });
    ++g_launches[2];
    return 0;
  }
  hipemu::launch(gb + gp, SF_FCONV_WAVES * 64, lds, [&] { k_gca_pool_rc<1, 1, 12, SF_FCONV_WAVES>(pa, b, (int)gb); });
  return 0;
}

extern "C" int emu_gca4_run(const sf_op* ops, uint32_t n, char* err, int errn) {
  err[0] = 0;
  for (uint32_t k = 0; k < n; ++k) {
    if (ops[k].type == SF_OP_FCONV && (ops[k].flags & 16)) {
      if (k + 1 >= n) { snprintf(err, errn, "gca4 emu: a paired fconv needs a successor"); return 1; }
      if (int rc = run_pair(&ops[k], &ops[k + 1], err, errn)) return rc;
      ++k;
      continue;
    }
    if (int rc = run_one(&ops[k], err, errn)) return rc;
  }
  return 0;
}

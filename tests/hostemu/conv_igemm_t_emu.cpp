// CPU harness for k_conv_igemm_t (sparsefusion_amd/csrc/conv_igemm_t.h) next to k_conv_igemm (conv_igemm.h) on the same ConvArgs: both
// kernel sources run on CPU threads (hip_emu.h).  A variant is named by its row in SF_IGEMM_T_VARIANTS; argument set-up mirrors run_conv
// of csrc/unet_ops.hip for tile codes < 256, one image.
#ifndef SF_HOST_EMU
#define SF_HOST_EMU
#endif
#define HIPEMU_IMPLEMENTATION
#include "hip_emu.h"
#include <algorithm>
using std::min;
using std::max;
#include "../../sparsefusion_amd/csrc/conv_igemm.h"
#include "../../sparsefusion_amd/csrc/conv_igemm_t.h"

template <int HL, int CIN, int COUT, int K, int S, int P, int UPS, int WM, int WN, int G, bool F32, int EPI>
static int go(int general, const void* in, const uint16_t* w, const float* bias, float* out, float* ws, float* slots) {
  ConvArgs a{};
  a.in = in; a.w = reinterpret_cast<const bf16x8*>(w); a.bias = bias; a.out = out; a.ws = ws; a.slots_out = slots;
  a.B = 1; a.H = a.W = 1 << HL; a.Cin = CIN; a.Ho = a.Wo = (a.H + 2 * P - K) / S + 1; a.Cout = COUT;
  a.pixshuf = EPI == SF_IGT_PIXSHUF; a.ldc = a.pixshuf ? COUT / 4 : COUT; a.co_off = 0;
  a.kh = a.kw = K; a.stride = S; a.pad = P; a.groups = G; a.ups = UPS;
  a.cchunks = CIN / 32;
  a.KS = K * K * a.cchunks;
  a.m_frags = (a.Ho * a.Wo + 15) / 16;
  a.n_frags = (COUT + 15) / 16;
  a.m_tiles = (a.m_frags + WM - 1) / WM;
  a.n_tiles = (a.n_frags + WN - 1) / WN;
  a.npad = a.n_frags * 16;
  a.steps_per_wave = (a.KS + G * 4 - 1) / (G * 4);
  const unsigned blocks = (unsigned)(a.m_tiles * a.n_tiles * G);
  if (general) hipemu::launch(blocks, 256, 0, [&] { k_conv_igemm<WM, WN, F32>(a); });
  else hipemu::launch(blocks, 256, 0, [&] { k_conv_igemm_t<HL, CIN, COUT, K, S, P, UPS, WM, WN, G, F32, EPI>(a); });
  return 0;
}

extern "C" int emu_igemm_t_run(int variant, int general, const void* in, const uint16_t* w, const float* bias, float* out, float* ws,
                               float* slots) {
  int row = 0;
#define SF_EMU_IGT(hl_, cin_, cout_, k_, s_, p_, ups_, wm_, wn_, g_, f32_, epi_) \
  if (row++ == variant) return go<hl_, cin_, cout_, k_, s_, p_, ups_, wm_, wn_, g_, (bool)f32_, epi_>(general, in, w, bias, out, ws, slots);
  SF_IGEMM_T_VARIANTS(SF_EMU_IGT)
#undef SF_EMU_IGT
  return 1;
}

// k_conv_igemm_t: k_conv_igemm (conv_igemm.h) with the geometry of ONE launch as template parameters -- the one-of-a-kind implicit
// GEMMs of the canonical B = 1 UNet eval (three Downsample convs, three Upsample 1x1 convs, the final 3x3 conv).  Same operands, same
// grid, same split of K over groups and waves, same k-step order inside a wave, same LDS reduction order and same epilogue arithmetic:
// output, split-K workspace and statistics slots are bit-identical to k_conv_igemm's (tests/test_hostemu_conv_igemm_t.py,
// tests/test_gpu_conv_igemm_t.py).  What changes is the instruction stream: pixel coordinates, tap and weight offsets are shifts, masks
// and immediates in 32 bits; a wave's k-steps are fully unrolled and their fragment loads requested at entry (all of them where they
// fit ~96 VGPRs, otherwise through a ring of compile-time depth -- the general kernel's pipeline re-reads its last trip, which for the
// 4 .. 8 steps of these launches doubles every load); the bias is requested at entry; the epilogue has no run-time branch.
// Written against sf_dev.h so that tests/hostemu runs the same source on CPU threads.
#pragma once
#include "sf_dev.h"
#include "conv_lds.h"          // ConvArgs

#define SF_IGT_SPLITK 0        // epilogue kinds: split-K partial tile -> workspace [grp][m][npad]
#define SF_IGT_PIXSHUF 1       //                 bias + SiLU + PixelShuffle(2) + statistics slots (ldc = Cout / 4, co_off = 0)

// (log2 H = log2 W, Cin, Cout, k, stride, pad, ups, WM, WN, split-K groups, A is fp32, epilogue kind); one image (B = 1).
// sparsefusion_amd/unet.py mirrors the table as IGEMM_T_VARIANTS (tests/test_plans_igemm_t_cpu.py compares the two).
#define SF_IGEMM_T_VARIANTS(X) \
  X(5, 256, 256, 4, 2, 1, 0, 2, 2, 4, 1, 0) \
  X(4, 256, 512, 4, 2, 1, 0, 1, 2, 8, 1, 0) \
  X(3, 512, 1024, 4, 2, 1, 0, 1, 1, 4, 1, 0) \
  X(2, 1024, 4096, 1, 1, 0, 0, 1, 1, 1, 1, 1) \
  X(3, 1024, 2048, 1, 1, 0, 0, 1, 1, 1, 1, 1) \
  X(4, 512, 1024, 1, 1, 0, 0, 1, 2, 1, 1, 1) \
  X(5, 256, 4, 3, 1, 1, 0, 1, 1, 4, 1, 0)

constexpr int sf_igt_log2(int v) { return v <= 1 ? 0 : 1 + sf_igt_log2(v >> 1); }

// Measurement aid (build.build_variant(tag, ["SF_IGT_KNOCKOUT=n"], sources=("unet_ops.hip",)); never defined in the product): 1 = no
// activation loads, 2 = no weight loads, 3 = no epilogue stores.  The results are garbage, the timing of everything else stands.
#ifndef SF_IGT_KNOCKOUT
#define SF_IGT_KNOCKOUT 0
#endif

template <int HL, int CIN, int COUT, int K, int STRIDE, int PAD, int UPS, int WM, int WN, int GROUPS, bool A_FP32, int EPI>
SF_KERNEL(256) void k_conv_igemm_t(ConvArgs a) {
  constexpr int H = 1 << HL, HO = (H + 2 * PAD - K) / STRIDE + 1, HOL = sf_igt_log2(HO), M = HO * HO;
  constexpr int CCH = CIN / 32, CCL = sf_igt_log2(CCH), KS = K * K * CCH, NF = (COUT + 15) / 16, NPAD = NF * 16;
  constexpr int MT = M / 16 / WM, NT = NF / WN, SPW = (KS + GROUPS * 4 - 1) / (GROUPS * 4);
  constexpr bool RAGGED = SPW * GROUPS * 4 != KS;      // (the final conv: 72 steps over 16 waves; the last waves hold fewer, wave-uniformly)
  constexpr int STEP_REGS = WM * (A_FP32 ? 8 : 4) + WN * 4;
  constexpr int D = SPW * STEP_REGS <= 96 ? SPW : (96 / STEP_REGS < 2 ? 2 : 96 / STEP_REGS);      // fragments in flight per wave: k-steps
  constexpr int LDC = COUT / 4;                                                                   // (pixel-shuffle form)
  static_assert((1 << HOL) == HO && (1 << CCL) == CCH && CIN % 32 == 0, "k_conv_igemm_t: power-of-two map and channel chunks");
  static_assert(M % (16 * WM) == 0 && NF % WN == 0, "k_conv_igemm_t: the tiles divide the output evenly (no clamped fragments)");
  static_assert(EPI == SF_IGT_SPLITK ? GROUPS > 1 : (GROUPS == 1 && COUT % 64 == 0 && M % 16 == 0), "k_conv_igemm_t: epilogue kind");
  static_assert(H * H * CIN < (1 << 28) && NF * KS * 64 < (1 << 27) && GROUPS * M * NPAD < (1 << 29), "k_conv_igemm_t: 32-bit offsets");

  sf_touch_kernarg<(int)sizeof(ConvArgs)>();        // all kernel-argument lines in one scalar-cache round trip (sf_dev.h)
  SF_SHARED __attribute__((aligned(16))) float red[3][WM * WN * 4 * 64];
  const int lane = threadIdx.x & 63, wave = sf_uniform((int)(threadIdx.x >> 6));
  const int tile = blockIdx.x % (MT * NT), grp = blockIdx.x / (MT * NT);
  const int nt = tile % NT, mt = tile / NT;
  const int k0 = (grp * 4 + wave) * SPW;
  const int cgrp = (lane >> 4) * 8;

  // bias of this lane's output columns: requested in front of everything else, first used in the epilogue
  float bq[WN];
#pragma unroll
  for (int ni = 0; ni < WN; ++ni) bq[ni] = EPI == SF_IGT_PIXSHUF ? a.bias[(nt * WN + ni) * 16 + (lane & 15)] : 0.0f;

  int py[WM], px[WM];
#pragma unroll
  for (int mi = 0; mi < WM; ++mi) {
    const int m = (mt * WM + mi) * 16 + (lane & 15);
    py[mi] = (m >> HOL) * STRIDE - PAD;
    px[mi] = (m & (HO - 1)) * STRIDE - PAD;
  }
  const float* in32 = reinterpret_cast<const float*>(a.in);
  const sf_opnd* in16 = reinterpret_cast<const sf_opnd*>(a.in);

  // the ring: slot s holds the raw fragments of one k-step (out-of-image taps read pixel 0 and are zeroed by a select at use)
  f32x4 ra[D][WM][2];
  bf16x8 rh[D][WM], rb[D][WN];
  bool ain[D][WM];
  auto request = [&](int i, int s) {
    int ks = k0 + i;
    if (RAGGED) ks = ks < KS ? ks : KS - 1;
    const int tap = ks >> CCL, cc = ks & (CCH - 1);
    const int ky = K == 1 ? 0 : tap / K, kx = K == 1 ? 0 : tap - ky * K;
#pragma unroll
    for (int ni = 0; ni < WN; ++ni)
      rb[s][ni] = SF_IGT_KNOCKOUT == 2 ? sf_zero8() : a.w[((nt * WN + ni) * KS + ks) * 64 + lane];
#pragma unroll
    for (int mi = 0; mi < WM; ++mi) {
      const int iy = py[mi] + ky, ix = px[mi] + kx;
      ain[s][mi] = PAD == 0 || ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)H);
      const int off = (ain[s][mi] ? ((iy >> UPS) * (H >> UPS) + (ix >> UPS)) * CIN : 0) + cc * 32 + cgrp;
      if (SF_IGT_KNOCKOUT == 1) {
        ra[s][mi][0] = ra[s][mi][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        rh[s][mi] = sf_zero8();
      } else if (A_FP32) {
        ra[s][mi][0] = *reinterpret_cast<const f32x4*>(in32 + off);
        ra[s][mi][1] = *reinterpret_cast<const f32x4*>(in32 + off + 4);
      } else {
        rh[s][mi] = *reinterpret_cast<const bf16x8*>(in16 + off);
      }
    }
  };
#pragma unroll
  for (int i = 0; i < D; ++i) request(i, i);

  f32x4 acc[WM][WN];
#pragma unroll
  for (int mi = 0; mi < WM; ++mi)
#pragma unroll
    for (int ni = 0; ni < WN; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int i = 0; i < SPW; ++i) {
    const int s = i % D;
    bf16x8 fa[WM], fb[WN];
#pragma unroll
    for (int ni = 0; ni < WN; ++ni) fb[ni] = rb[s][ni];
#pragma unroll
    for (int mi = 0; mi < WM; ++mi) {
      bf16x8 v;
      if (A_FP32) {
        const f32x4 lo = ra[s][mi][0], hi = ra[s][mi][1];
        v[0] = (sf_opnd)lo[0]; v[1] = (sf_opnd)lo[1]; v[2] = (sf_opnd)lo[2]; v[3] = (sf_opnd)lo[3];
        v[4] = (sf_opnd)hi[0]; v[5] = (sf_opnd)hi[1]; v[6] = (sf_opnd)hi[2]; v[7] = (sf_opnd)hi[3];
      } else {
        v = rh[s][mi];
      }
      fa[mi] = ain[s][mi] ? v : sf_zero8();
    }
    if (i + D < SPW) request(i + D, s);
    if (!RAGGED || k0 + i < KS) {
#pragma unroll
      for (int mi = 0; mi < WM; ++mi)
#pragma unroll
        for (int ni = 0; ni < WN; ++ni) acc[mi][ni] = sf_mfma16(fa[mi], fb[ni], acc[mi][ni]);
    }
  }

  // reduce the 4 K-slices of this workgroup through LDS (k_conv_igemm's order)
  if (wave > 0) {
#pragma unroll
    for (int mi = 0; mi < WM; ++mi)
#pragma unroll
      for (int ni = 0; ni < WN; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave - 1][((mi * WN + ni) * 4 + r) * 64 + lane] = acc[mi][ni][r];
  }
  sf_sync();
  if (wave != 0) return;
#pragma unroll
  for (int mi = 0; mi < WM; ++mi)
#pragma unroll
    for (int ni = 0; ni < WN; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int idx = ((mi * WN + ni) * 4 + r) * 64 + lane;
        acc[mi][ni][r] += red[0][idx] + red[1][idx] + red[2][idx];
      }
  if (SF_IGT_KNOCKOUT == 3) {
#ifndef SF_HOST_EMU
#pragma unroll
    for (int mi = 0; mi < WM; ++mi)
#pragma unroll
      for (int ni = 0; ni < WN; ++ni) asm volatile("" ::"v"(acc[mi][ni]), "v"(bq[ni]));      // keeps the stubbed-out values live
#endif
    return;
  }

#pragma unroll
  for (int mi = 0; mi < WM; ++mi) {
#pragma unroll
    for (int ni = 0; ni < WN; ++ni) {
      const int nf = nt * WN + ni;
      const int n = nf * 16 + (lane & 15);
      const int m0 = (mt * WM + mi) * 16 + (lane >> 4) * 4;
      if (EPI == SF_IGT_SPLITK) {                 // partial tile -> workspace [grp][m][npad] (padded columns included, as k_conv_igemm)
#pragma unroll
        for (int r = 0; r < 4; ++r) a.ws[(grp * M + m0 + r) * NPAD + n] = acc[mi][ni][r];
      } else {
        // out[2*oy+i, 2*ox+j, c] = silu(conv[oy, ox, c*4 + i*2 + j] + bias)   (PixelShuffle(2)); slots as k_conv_igemm files them
        float bv = bq[ni];
        SF_USE_FROM_HERE(bv);
        float v[4], sm = 0.0f, sq = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = sf_silu(acc[mi][ni][r] + bv);
          sm += v[r];
          sq = fmaf(v[r], v[r], sq);
        }
        sm = sf_wave_sum(sm);
        sq = sf_wave_sum(sq);
        if (lane == 0) {
          float* sl = a.slots_out + (((mt * WM + mi) * 4 + (nf & 3)) * (LDC >> 4) + (nf >> 2)) * 2;
          sl[0] = sm;
          sl[1] = sq;
        }
        const int c = n >> 2, ii = (n >> 1) & 1, jj = n & 1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + r, oy = m >> HOL, ox = m & (HO - 1);
          a.out[((2 * oy + ii) * (2 * HO) + 2 * ox + jj) * LDC + c] = v[r];
        }
      }
    }
  }
}

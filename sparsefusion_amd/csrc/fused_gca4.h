// The 4x4 level of a B = 1 eval on compile-time geometry: the GlobalContext pooling of its 16-pixel map and the plain 1x1 conv (res_conv)
// on the raw concat of that map.  Same operands, same arithmetic in the same order as gca_pool_body (fused_gca.h) and
// conv_fused_body<1, 1, 12, FNORM_NONE, 0, 8> (fused_kernels.h) -- results are bit-identical -- with what those keep generic made static,
// so that every global load of a launch is requested at entry and travels in ONE round trip:
//   * k_gca_pool: run-time C / CH / chunks / nparts / groups.  At 4x4 the chunk is the whole map; a thread sums its nparts / 16 logit parts
//     in two dependent trips of 8 loads, issues 4 x 8 slab loads of which 4 are live (the others are clamped copies), six block barriers;
//   * k_conv_fused<1, 1, 12, FNORM_NONE, 0, 8>: the 16 pixels x CIN channels are staged two float4 per thread at a time (software pipeline
//     with run-time trip counts: eight dependent L2 round trips in front of 8 MFMAs per wave).
#pragma once
#include "fused_kernels.h"
#include "fused_gca.h"

// ---- GlobalContext pooling: M = HW = CH = 16 (one chunk = the map), nparts = 4 * C / 16 logit parts (conv2 runs 4 input-channel slices),
// GROUPS = 4: h2 is still conv2's 4 split-K slabs (+ bias) with row stride C and is written back; GROUPS = 0: h2 is materialised.
// grid = (M / 16) * (C / 64); 256 threads = 16 channel float4 lanes x 16 pixel lanes.  Two block barriers (the 16 part lanes of a pixel's
// logit meet, the 16 pixel lanes of a pooled channel meet); every wave forms the softmax itself, e[p] travels by a shuffle.
// Summation orders of gca_pool_body kept: a thread's parts k = pl, pl + 16, ..; red[0..15]; the wave max / sum trees over lanes 0..15
// (-inf / 0 elsewhere); bias, slab 0..3 and the four clamped slab-3 terms with weight 0; the 16-row pooled reduction.
template <int C, int GROUPS>
SF_DEV void gca_pool4_body(const GcaPoolArgs& a, const int bid) {
  static_assert(C % 64 == 0 && (GROUPS == 0 || GROUPS == 4), "gca_pool4: 64-channel slabs, 4 split-K slabs or a materialised h2");
  constexpr int NP = C / 64;                                   // logit parts per thread
  constexpr int cslabs = C / 64;
  SF_SHARED float redl[16][17];
  SF_SHARED float redp[16][68];
  const int tid = threadIdx.x, lane = tid & 63;
  const int cs = bid % cslabs, bc = bid / cslabs;
  const long m0 = (long)bc * 16;
  const int c4 = tid & 15, pl = tid >> 4;
  const int c = cs * 64 + c4 * 4;
  // every load of the launch: the thread's logit parts (pixel c4, part lane pl), its pixel's float4 of h2 (or its 4 slabs + bias)
  float t[NP];
#pragma unroll
  for (int u = 0; u < NP; ++u) t[u] = a.logit_part[(long)(pl + u * 16) * a.M + m0 + c4];
  f32x4 sl[4], bq;
  if (GROUPS) {
    const float* ap = a.ws + (m0 + pl) * C + c;
    const long gstride = (long)a.M * C;
#pragma unroll
    for (int g = 0; g < 4; ++g) sl[g] = *reinterpret_cast<const f32x4*>(ap + g * gstride);
    bq = *reinterpret_cast<const f32x4*>(a.bias ? a.bias + c : ap);
  } else {
    sl[0] = *reinterpret_cast<const f32x4*>(a.h2 + (m0 + pl) * C + c);
  }
  // (1) logit of pixel c4: this thread's parts in k order, then the 16 part lanes in LDS
  float l = 0.0f;
#pragma unroll
  for (int u = 0; u < NP; ++u) l += t[u];
  redl[pl][c4] = l;
  sf_sync();
  float lq = 0.0f;
#pragma unroll
  for (int k = 0; k < 16; ++k) lq += redl[k][lane & 15];
  // (2) softmax numerators: lanes 0..15 of every wave hold the 16 pixels
  const bool on = lane < 16;
  const float mx = sf_wave_max(on ? lq : -INFINITY);
  const float ex = sf_exp(lq - mx);
  const float sm = sf_wave_sum(on ? ex : 0.0f);
  if (tid == 0 && cs == 0) { a.part_ms[(long)bc * 2] = mx; a.part_ms[(long)bc * 2 + 1] = sm; }
  const float ep = sf_shfl(ex, pl);                            // e of this thread's pixel
  // (3) un-normalised pooled slab; h2 is evaluated (and written back) from the slabs when lazy
  f32x4 v;
  if (GROUPS) {
    v = a.bias ? bq : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < 8; ++g) v += sl[g < 3 ? g : 3] * (g <= 3 ? 1.0f : 0.0f);      // (the general kernel's 8 slab terms, 4 of them clamped with weight 0)
    *reinterpret_cast<f32x4*>(a.h2 + (m0 + pl) * C + c) = v;
  } else {
    v = sl[0];
  }
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  acc += v * ep;
#pragma unroll
  for (int j = 0; j < 4; ++j) redp[pl][c4 * 4 + j] = acc[j];
  sf_sync();
  if (tid < 64) {
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += redp[k][tid];
    a.part_pool[(long)bc * C + cs * 64 + tid] = s;
  }
}

template <int C, int GROUPS>
SF_KERNEL(256) void k_gca_pool4_t(GcaPoolArgs a) {
  sf_touch_kernarg<(int)sizeof(GcaPoolArgs)>();
  gca_pool4_body<C, GROUPS>(a, (int)blockIdx.x);
}

// ---- the plain 1x1 conv of the 16-pixel map: one image, CIN = C1 + C2 channels of two plain sources (the second scaled), COUT outputs,
// no norm, no activation, one input-channel slice; final mode (bias, optional residual).  Workgroup = 8 waves = one 16-channel fragment of
// the output; every thread keeps ONE float4 channel chunk (or CIN / 2048 of them) of all 16 pixels.
template <int CIN, int COUT>
struct Conv41x1Geom {
  static constexpr int NT = 512, NW = 8;
  static constexpr int KS = CIN / 32, SPW = KS / NW;             // k-steps (32-channel chunks), k-steps per wave
  static constexpr int TC = CIN / 4 < NT ? CIN / 4 : NT;       // threads across the float4 channel chunks
  static constexpr int PPP = NT / TC, NPX = 16 / PPP;          // pixel lanes, pixels per thread
  static constexpr int PIX_STRIDE = CIN * 2 + 32;              // = fconv_pix_stride(CIN): 32 (mod 256)
  static constexpr int RED_OFF = 16 * PIX_STRIDE;
  static constexpr uint32_t LDS_BYTES = RED_OFF + 1024 * NW;
  static_assert(CIN % 256 == 0 && CIN / 4 <= NT && KS % NW == 0 && SPW <= 12 && COUT % 16 == 0, "conv4_1x1: geometry");
};

template <int CIN, int COUT>
SF_DEV void conv4_1x1_body(const FConvArgs& a, const int bid) {
  using G = Conv41x1Geom<CIN, COUT>;
  SF_DYN_LDS(lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nf = bid;                                          // n-tile = 16-channel fragment (one m-tile, one slice)
  // ---- every load of the launch.  Activations first (the first thing waited for), then this wave's weight fragments, then the epilogue's rows.
  const int tp = tid / G::TC, cl = (tid - tp * G::TC) * 4;
  const bool first = cl < a.s1.C;
  const float* srcp = first ? a.s1.p + cl : a.s2.p + (cl - a.s1.C);
  const int srcld = first ? a.s1.C : a.s2.C;
  const float sc = first ? a.s1.scale : a.s2.scale;
  f32x4 v[G::NPX];
#pragma unroll
  for (int u = 0; u < G::NPX; ++u) v[u] = *reinterpret_cast<const f32x4*>(srcp + (long)(tp + u * G::PPP) * srcld);
  const bf16x8* wbase = a.w + ((long)nf * G::KS + wave * G::SPW) * 64 + lane;
  bf16x8 fb[G::SPW];
#pragma unroll
  for (int u = 0; u < G::SPW; ++u) fb[u] = __builtin_nontemporal_load(&wbase[u * 64]);
  const int n = nf * 16 + (lane & 15);
  const int mrow = (lane >> 4) * 4;
  const float* fallback = a.s1.p;                               // any valid address for an absent operand (its value is never used)
  float bq = (a.bias ? a.bias : fallback)[a.bias ? n : 0];
  float rq[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) rq[r] = (a.resid ? a.resid : fallback)[a.resid ? (long)(mrow + r) * a.ldc + a.co_off + n : 0];
  // ---- fp32 -> operand type, [pixel][channel] (the scale is ONE fp32 product, as the general kernel's slope 1 * scale)
#pragma unroll
  for (int u = 0; u < G::NPX; ++u) {
    const f32x4 y = v[u] * sc;
    bf16x4 o;
    o[0] = (sf_opnd)y[0]; o[1] = (sf_opnd)y[1]; o[2] = (sf_opnd)y[2]; o[3] = (sf_opnd)y[3];
    *reinterpret_cast<bf16x4*>(lds + (tp + u * G::PPP) * G::PIX_STRIDE + cl * 2) = o;
  }
  sf_sync();
  // ---- this wave's k-steps [wave * SPW, (wave + 1) * SPW) in order
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  const char* abase = lds + (lane & 15) * G::PIX_STRIDE + (lane >> 4) * 16 + wave * G::SPW * 64;
#pragma unroll
  for (int u = 0; u < G::SPW; ++u) acc = sf_mfma16(*reinterpret_cast<const bf16x8*>(abase + u * 64), fb[u], acc);
  // ---- the 8 K-slices meet in LDS in wave order; wave 0 finalises
  float* red = reinterpret_cast<float*>(lds + G::RED_OFF);      // [wave][r][lane]
#pragma unroll
  for (int r = 0; r < 4; ++r) red[(wave * 4 + r) * 64 + lane] = acc[r];
  sf_sync();
  SF_USE_FROM_HERE(bq);
#pragma unroll
  for (int r = 0; r < 4; ++r) SF_USE_FROM_HERE(rq[r]);
  if (wave == 0) {
    const float bv = a.bias ? bq : 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float sacc = 0.0f;
#pragma unroll
      for (int w = 0; w < G::NW; ++w) sacc += red[r * 64 + lane + w * 256];
      const float rv = a.resid ? rq[r] : 0.0f;
      a.out[(long)(mrow + r) * a.ldc + a.co_off + n] = sacc + bv + rv;
    }
  }
}

template <int CIN, int COUT>
SF_KERNEL(512) void k_conv4_1x1_t(FConvArgs a) {
  sf_touch_kernarg<(int)sizeof(FConvArgs)>();
  conv4_1x1_body<CIN, COUT>(a, (int)blockIdx.x);
}

// res_conv || pooling of one 4x4 block in one launch, the launch shape of k_gca_pool_rc (fused_pipe.h): conv workgroups first, then the pooling
// workgroups, which retire their upper four waves at once.
template <int CIN, int C, int GROUPS>
SF_KERNEL(512) void k_gca_pool4_rc_t(GcaPoolArgs pa, FConvArgs b, int grid_b) {
  sf_touch_kernarg<(int)(sizeof(GcaPoolArgs) + sizeof(FConvArgs))>();
  if ((int)blockIdx.x < grid_b) conv4_1x1_body<CIN, C>(b, (int)blockIdx.x);
  else if (threadIdx.x < 256) gca_pool4_body<C, GROUPS>(pa, (int)blockIdx.x - grid_b);
}

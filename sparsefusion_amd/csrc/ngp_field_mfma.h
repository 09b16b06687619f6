// Field forward of the fused Instant-NGP render with the two hidden layers on the matrix cores (gfx950), fp32 in / fp32 out.
//
// What it computes: exactly what k_ngp_field<0> / <1> (ngp_render.hip) compute per sample point -- position, hash-grid features,
// the 32 -> 64 -> 64 -> 4 ReLU MLP, trunc_exp / sigmoid -- and, when asked, the 128-byte field-cache row of the point.
// k_ngp_field runs the MLP as one lane per point: 6 320 v_fmac_f32 per wave of 64 points behind broadcast LDS weight reads, 62 % of
// the kernel's VALU instructions.  Here one WAVE owns 32 points per trip, as the forward phases A -> B1 -> B2 -> C of
// k_ngp_field_bwd_mfma (ngp_bwd_mfma.h) do:
//   A   lane = (point, half): each half encodes 8 of the 16 levels with the calls and the per-level fmaf order of ngp_encode;
//       the features go to a wave-private LDS tile [32][33] (and to the cache row, four 16-byte stores per lane);
//   B1  H1 = relu(F W0^T + b0) and  B2  H2 = relu(H1 W1^T + b1) on v_mfma_f32_16x16x4_f32, the bias as the initial accumulator
//       and the k-steps in ascending order.  The f32 MFMA rounds once per product in k order, so every hidden value is bit for bit
//       the chain  a = bias; for k: a = fmaf(W[j][k], x[k], a)  of ngp_mlp_forward;
//   C   the 4-wide output layer on the VALU, two outputs per lane in the same k order, then the activations.
// The weight fragments of a lane do not depend on the trip.  The 64 W1 fragments are read once per wave into registers (staged
// through the tiles' LDS before the first trip); the 32 of W0 do not fit beside them at two waves per SIMD and are read from a
// padded LDS image, 32 conflict-free 4-byte reads per trip.  H2 is written over H1: a 16-row
// half of H1 is read only by the MFMAs that produce the same 16 rows of H2.  No workgroup barrier in the loop, no atomics: the
// four waves of a workgroup never exchange data.
#pragma once
#include "sf_dev.h"
#include "ngp_device.h"

#define FM_PTS 32
#define FM_SF 33                                   // feature row stride (floats): conflict-free 4-byte fragment reads
#define FM_SH 65                                   // hidden row stride
#define FM_WAVE_FLOATS (FM_PTS * FM_SF + FM_PTS * FM_SH)
#define FM_W2 0                                    // [4][64]
#define FM_B2 (FM_W2 + NGP_OUT * NGP_HID)          // [4]
#define FM_B0 (FM_B2 + 8)                           // [64]
#define FM_B1 (FM_B0 + NGP_HID)                    // [64]
#define FM_W0 (FM_B1 + NGP_HID)                    // [64][33]
#define FM_HEAD (FM_W0 + NGP_HID * FM_SF)
#define FM_LDS_FLOATS (FM_HEAD + 4 * FM_WAVE_FLOATS)      // 60 192 bytes; the W1 [64][65] staging image fits in the tiles

#ifndef FM_DEPTH
#define FM_DEPTH 1                                 // levels of gathers in flight per lane (see the encode loop); 2 measured the same
                                                   // (0.893 against 0.895-0.902 ms per render forward) at 256 instead of 200 registers
#endif

#ifdef SF_HOST_EMU
#define FM_SCHED_FENCE() do { } while (0)
#else
#define FM_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)      // no instruction is scheduled across this point
#endif

struct FMArgs {
  const float* table; const float* w0; const float* b0; const float* w1; const float* b1; const float* w2; const float* b2;
  float bound;
  NgpLevels lv;
  const float* rays_o; const float* rays_d; const float* aabb; const float* nears; const float* fars;
  const float* lin; const float* u;          // mode 0: linspace(0, 1, T) and the stratified jitter [P] (or null)
  const float* z_in;                         // mode 1: the depths [P]
  uint32_t P, T;
  float* z_out;                              // mode 0
  float* sigma; float* rgb;
  float* feat_out;                           // [P][32] field-cache rows, or null
};

// entry 0 of `m` = level ll (hi = 0) or 8 + ll (hi = 1) of `lv`; ll is a compile-time constant at every call
SF_DEV void fm_level(const NgpLevels& lv, uint32_t hi, int ll, NgpLevels& m) {
  m.scale[0] = hi ? lv.scale[8 + ll] : lv.scale[ll];
  m.resolution[0] = hi ? lv.resolution[8 + ll] : lv.resolution[ll];
  m.offset[0] = hi ? lv.offset[8 + ll] : lv.offset[ll];
  m.hsize[0] = hi ? lv.hsize[8 + ll] : lv.hsize[ll];
  m.gridtype = lv.gridtype;
}

// mode 0: z from the stratified coarse rule (writes z_out); mode 1: z read from z_in.
template <int MODE>
SF_KERNEL(256) void k_ngp_field_mfma(FMArgs a) {
  SF_DYN_LDS(lds_raw);
  float* W = reinterpret_cast<float*>(lds_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kq = lane >> 4;            // MFMA fragment coordinates of this lane
  // ---- the weights: W2 / b2 (broadcast reads of phase C) and the padded W0 image stay in LDS; W1 passes through a padded image
  // laid over the tiles into this lane's fragment registers
  float bw1[NGP_HID / 4][4];                           // W1 B fragments [k-step][column tile]
  {
    float* S1 = W + FM_HEAD;                           // [64][65]
    for (int i = tid; i < NGP_HID * NGP_FEAT; i += 256) W[FM_W0 + (i >> 5) * FM_SF + (i & 31)] = a.w0[i];
    for (int i = tid; i < NGP_HID * NGP_HID; i += 256) S1[(i >> 6) * FM_SH + (i & 63)] = a.w1[i];
    for (int i = tid; i < NGP_OUT * NGP_HID; i += 256) W[FM_W2 + i] = a.w2[i];
    if (tid < NGP_HID) { W[FM_B0 + tid] = a.b0[tid]; W[FM_B1 + tid] = a.b1[tid]; }
    if (tid < NGP_OUT) W[FM_B2 + tid] = a.b2[tid];
    sf_sync();
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
      for (int s = 0; s < NGP_HID / 4; ++s) bw1[s][nt] = S1[(nt * 16 + li) * FM_SH + 4 * s + kq];
    }
    sf_sync();                                         // every wave holds its fragments: the image's LDS becomes the tiles
  }
  float* F = W + FM_HEAD + wave * FM_WAVE_FLOATS;      // [32][33] features
  float* H = F + FM_PTS * FM_SF;                       // [32][65] h1, then h2
  float box[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) box[i] = a.aabb[i];

  const int pl = lane & 31, half = lane >> 5;
  const uint32_t n_trips = (a.P + FM_PTS - 1) / FM_PTS;
  for (uint32_t trip = blockIdx.x * 4 + wave; trip < n_trips; trip += gridDim.x * 4) {
    // ---- A: position + hash-grid features; lane = (point pl, half)
    const uint32_t p = trip * FM_PTS + pl;
    const bool live = p < a.P;                         // a dead lane forms no address: x01 = 0, outside, every store masked
    float x01[3] = {0.f, 0.f, 0.f}, blob = 0.0f;       // blob: ngp_blob of the position, for the density of phase C
    bool inside = false;
    if (live) {
      const uint32_t n = p / a.T;
      float z;
      if (MODE == 0) {
        z = ngp_coarse_z(a.nears[n], a.fars[n], a.lin[p - n * a.T], a.u ? a.u[p] : -1.0f, a.T);
        if (half == 0) a.z_out[p] = z;
      } else {
        z = a.z_in[p];
      }
      const float o[3] = {a.rays_o[n * 3], a.rays_o[n * 3 + 1], a.rays_o[n * 3 + 2]};
      const float d[3] = {a.rays_d[n * 3], a.rays_d[n * 3 + 1], a.rays_d[n * 3 + 2]};
      float x[3];
      ngp_point(o, d, z, box, x);
      inside = ngp_unit(x, a.bound, x01);
      blob = ngp_blob(x);
    }
    // No branch around a level (ngp_encode has one): the gathers of all 8 levels may be in flight together.  A lane that is outside
    // the grid (or dead) encodes the origin instead and drops the result; an unused level (l >= L) has resolution 1, one row at
    // offset 0 (sf_ngp_make_levels), so it reads row 0 of the table and drops that: every address stays inside the table.
    const float xe[3] = {inside ? x01[0] : 0.0f, inside ? x01[1] : 0.0f, inside ? x01[2] : 0.0f};
    // The geometry of this lane's 8 levels: the level tables sit in scalar registers (kernel arguments), a lane takes entry ll or
    // 8 + ll by a select, level by level (fm_level).  `hi` is made opaque once per trip: the compiler otherwise keeps ~90 registers
    // of per-level, per-lane constants across the trips and the kernel drops to one wave per SIMD.
    uint32_t hi = half;
    SF_USE_FROM_HERE(hi);
    // Software pipeline, FM_DEPTH levels deep: the gathers of a level are issued FM_DEPTH cell computations (some 300 VALU
    // instructions each) before their use; FM_SCHED_FENCE keeps the compiler from sinking a computation behind the use.
    f32x2 fv[FM_DEPTH][8];
    float w[FM_DEPTH][8];
    NgpCell c;
    NgpLevels m;
#pragma unroll
    for (int q = 0; q < FM_DEPTH; ++q) {
      fm_level(a.lv, hi, q, m);
      ngp_cell(m, 0, xe, c);
      const float* tab = a.table + (size_t)m.offset[0] * 2;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        fv[q][i] = *reinterpret_cast<const f32x2*>(tab + (size_t)c.row[i] * 2);
        w[q][i] = c.w[i];
      }
      FM_SCHED_FENCE();
    }
#pragma unroll
    for (int ll = 0; ll < 8; ++ll) {
      const uint32_t l = hi * 8 + ll;
      const int q = ll % FM_DEPTH;
      const float* tab = a.table;
      if (ll + FM_DEPTH < 8) {
        fm_level(a.lv, hi, ll + FM_DEPTH, m);
        ngp_cell(m, 0, xe, c);
        tab = a.table + (size_t)m.offset[0] * 2;
      }
      FM_SCHED_FENCE();
      float r0 = 0.0f, r1 = 0.0f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        r0 = fmaf(w[q][i], fv[q][i][0], r0);
        r1 = fmaf(w[q][i], fv[q][i][1], r1);
      }
      if (!(inside && l < a.lv.L)) r0 = r1 = 0.0f;
      F[pl * FM_SF + 2 * l] = r0;
      F[pl * FM_SF + 2 * l + 1] = r1;
      if (ll + FM_DEPTH < 8) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          fv[q][i] = *reinterpret_cast<const f32x2*>(tab + (size_t)c.row[i] * 2);
          w[q][i] = c.w[i];
        }
      }
      FM_SCHED_FENCE();
    }
    if (a.feat_out && live) {
      // the cache row: this lane's 16 floats back from the tile (its own stores; 16 registers less across the level loop)
      float* dst = a.feat_out + (size_t)p * NGP_FEAT + half * 16;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = F[pl * FM_SF + half * 16 + 4 * j + e];
        *reinterpret_cast<f32x4*>(dst + 4 * j) = v;
      }
    }
    sf_wave_sync();

    // ---- B1: H1 = relu(F W0^T + b0), 16 points at a time (four independent accumulators)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      f32x4 c[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const float bv = W[FM_B0 + nt * 16 + li];
        c[nt] = f32x4{bv, bv, bv, bv};
      }
#pragma unroll
      for (int s = 0; s < NGP_FEAT / 4; ++s) {
        const float av = F[(mt * 16 + li) * FM_SF + 4 * s + kq];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) c[nt] = sf_mfma4(av, W[FM_W0 + (nt * 16 + li) * FM_SF + 4 * s + kq], c[nt]);
      }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) H[(mt * 16 + 4 * kq + r) * FM_SH + nt * 16 + li] = fmaxf(c[nt][r], 0.0f);
    }
    sf_wave_sync();
    // ---- B2: H2 = relu(H1 W1^T + b1), written over H1 (rows mt*16 .. +15 of H1 are read by this mt only)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      f32x4 c[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const float bv = W[FM_B1 + nt * 16 + li];
        c[nt] = f32x4{bv, bv, bv, bv};
      }
#pragma unroll
      for (int s = 0; s < NGP_HID / 4; ++s) {
        const float av = H[(mt * 16 + li) * FM_SH + 4 * s + kq];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) c[nt] = sf_mfma4(av, bw1[s][nt], c[nt]);
      }
      sf_wave_sync();                                  // every lane has read its H1 fragments of these 16 rows
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) H[(mt * 16 + 4 * kq + r) * FM_SH + nt * 16 + li] = fmaxf(c[nt][r], 0.0f);
    }
    sf_wave_sync();
    // ---- C: output layer (4 wide, VALU) and activations: lane = (point pl, half) owns outputs 2*half, 2*half + 1
    {
      float o0 = W[FM_B2 + 2 * half], o1 = W[FM_B2 + 2 * half + 1];
#pragma unroll 8
      for (int k = 0; k < NGP_HID; ++k) {
        const float hk = H[pl * FM_SH + k];
        o0 = fmaf(W[FM_W2 + (2 * half) * NGP_HID + k], hk, o0);
        o1 = fmaf(W[FM_W2 + (2 * half + 1) * NGP_HID + k], hk, o1);
      }
      if (live) {
        if (half == 0) {
          a.sigma[p] = expf(o0 + blob);
          a.rgb[(size_t)p * 3 + 0] = ngp_sigmoid(o1);
        } else {
          a.rgb[(size_t)p * 3 + 1] = ngp_sigmoid(o0);
          a.rgb[(size_t)p * 3 + 2] = ngp_sigmoid(o1);
        }
      }
    }
    sf_wave_sync();                                    // before the next trip restages F / H
  }
}

// Field backward of the fused Instant-NGP render on the matrix cores, cache path, software-pipelined (gfx950), fp32 in / fp32 out.
//
// What it computes: exactly what k_ngp_field_bwd_mfma (ngp_bwd_mfma.h) computes from a field cache -- the same arguments, the same
// trips (32 points per wave and trip, wave 4b + w takes trips 4b + w + 4 grid i), the same LDS image, one register-resident
// accumulator set per wave flushed once through sf_grad_add -- with every MFMA and fmaf chain in the same k order from the same
// initial accumulator, so that d(feat) and the six per-wave addends are the same values.  What differs is when operands are asked for:
//   * global operands.  k_ngp_field_bwd_mfma pays its global round trips in full: rays / depth, perm, then the feature row behind
//     perm, then dsig / drgb in phase C.  Here a lane asks for perm two trips ahead and for the feature row, ray, depth and upstream
//     gradients of the NEXT trip right after it has stored those of the current one (28 registers); a lane with no next trip, or a
//     dead point, reads the launch's last valid point instead and masks the values where they are used;
//   * weight fragments.  The 64 W1 fragments of phase B2, the padded W2 fragments of C and E and the biases do not depend on the
//     trip: registers, read once per wave.  W0, and W1 as phase G reads it, stay in the padded LDS image: G's 64 fragments in
//     registers as well (FP_W1_REGS = 2) spill at 512 VGPRs (profiles/ngp_field_bwd_pipe_regs.log);
//   * tile fragments.  Every MFMA phase reads all its LDS fragments into registers first and then runs its MFMAs;
//   * phases C, D and E run on the matrix cores too, in forms with the same chains:
//       C   out = H2 W2^T + b2      [32x64][64x16], N padded 4 -> 16, the bias as the initial accumulator, k ascending;
//       D   dW2 += dout^T H2         [16x32][32x64], M padded, the points ascending into the running accumulator; db2 the same
//           A fragments against a column of ones (b + dv = fmaf(dv, 1, b));
//       E   dh2 = dout W2            [32x4][4x64], one K = 4 step from a zero accumulator (fmaf(w0, d0, +0) = w0 * d0 up to the sign
//           of a zero, which no later sum can see: an accumulator that starts at +0 never becomes -0);
//     relu(H1) and relu(H2) stay in the registers that produced them, so the masks of E and G read no LDS.
//   db1 / db0 keep their VALU chains (point-ascending adds), with the 32 reads of a chain issued together.
// No workgroup barrier in the loop and no spin-wait: the four waves of a workgroup never exchange data.
// The phases share two GEMM shapes, each written once below: the row GEMM (fp_row_*: B1, B2, C, E, G, I) and the points GEMM
// (fp_point_frags / fp_points_gemm: D, F, H); fp_store_dfeat is I's epilogue, fp_flush the flush after the last trip.
#pragma once
#include "ngp_bwd_mfma.h"                          // FBArgs and the LDS image (FB_*)

#ifndef SF_FIELD_BWD_PIPE_DEFAULT
#define SF_FIELD_BWD_PIPE_DEFAULT 1                // the start value of the process-wide switch sf_ngp_field_bwd_pipe (ngp_render.hip)
#endif
#ifndef FP_W1_REGS
#define FP_W1_REGS 1                               // W1's fragments in registers: 2 = those of B2 and of G (64 + 64; spills), 1 = B2's, 0 = none (LDS)
#endif
#ifndef FP_H1_REGS
#define FP_H1_REGS 1                               // 1: relu(h1) stays in registers from B1 to the mask of G (32); 0: G reads it back from LDS
#endif
#ifndef FP_PREFETCH
#define FP_PREFETCH 1                              // 1: global operands a trip ahead (perm two); 0: loaded by the trip that uses them (+0.05 ms per render)
#endif

// the global operands of one lane = (point pl, half) and trip
struct FPOps {
  f32x4 fv[4];                                     // the lane's 16 cached features
  float z, o[3], d[3];
  float g0, g1;                                    // half 0: dsig, drgb[0]; half 1: drgb[1], drgb[2]
};

// pc: a VALID point of this launch (callers clamp), src: perm of that point
SF_DEV void fp_load(const FBArgs& a, uint32_t pc, uint32_t src, int half, FPOps& q) {
  const uint32_t pg = a.p_off + pc, ng = pg / a.T2, T = a.T2 >> 1, n = pc / a.T2;
  const float* row = (src < T ? a.feat_c + ((size_t)ng * T + src) * NGP_FEAT : a.feat_f + ((size_t)ng * T + (src - T)) * NGP_FEAT) + half * 16;
#pragma unroll
  for (int j = 0; j < 4; ++j) q.fv[j] = *reinterpret_cast<const f32x4*>(row + 4 * j);
  q.z = a.z_s[pc];
#pragma unroll
  for (int i = 0; i < 3; ++i) { q.o[i] = a.rays_o[n * 3 + i]; q.d[i] = a.rays_d[n * 3 + i]; }
  q.g0 = half == 0 ? a.dsig[pc] : a.drgb[(size_t)pc * 3 + 1];
  q.g1 = half == 0 ? a.drgb[(size_t)pc * 3] : a.drgb[(size_t)pc * 3 + 2];
}

// ---- the two GEMM shapes of the kernel, on fragments of v_mfma_f32_16x16x4_f32: lane (li, kq) holds A[li][4s + kq] and B[4s + kq][li] of
// k-step s and rows 4 kq + r, column li of a 16 x 16 accumulator tile.  Every helper is reached by all 64 lanes (sf_mfma4 is a rendezvous
// of the wave under the emulation) and loads, multiplies and stores in fully unrolled loops: the arrays are registers.
//
// Row GEMM  c[mt][nt] = T[32][4 KS] B[4 KS][16 NT]  (+ the accumulators' initial value), T a wave-private tile of row stride ld: the A
// fragments of both 16-row halves, av[mt][s] = T[mt * 16 + li][4 s + kq]
template <int KS>
SF_DEV void fp_row_frags(const float* T, int ld, int li, int kq, float (&av)[2][KS]) {
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    av[0][s] = T[li * ld + 4 * s + kq];
    av[1][s] = T[(16 + li) * ld + 4 * s + kq];
  }
}
// the k-steps ascending into every accumulator; b(s, nt) is the B fragment: a register the caller loaded, or an LDS read
template <int KS, int NT, class BSrc>
SF_DEV void fp_row_gemm(const float (&av)[2][KS], BSrc b, f32x4 (&c)[2][NT]) {
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const float bv = b(s, nt);
      c[0][nt] = sf_mfma4(av[0][s], bv, c[0][nt]);
      c[1][nt] = sf_mfma4(av[1][s], bv, c[1][nt]);
    }
}
template <int NT>
SF_DEV void fp_row_fill(f32x4 (&c)[2][NT], const float* v) {        // every row of column tile nt starts at v[nt] (a bias)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) { c[0][nt] = f32x4{v[nt], v[nt], v[nt], v[nt]}; c[1][nt] = c[0][nt]; }
}
// the accumulator layout back into a tile: D[mt * 16 + 4 kq + r][nt * 16 + li] = val(mt, nt, r)
SF_DEV int fp_row_at(int ld, int li, int kq, int mt, int nt, int r) { return (mt * 16 + 4 * kq + r) * ld + nt * 16 + li; }
template <int NT, class Val>
SF_DEV void fp_row_store(float* D, int ld, int li, int kq, Val val) {
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) D[fp_row_at(ld, li, kq, mt, nt, r)] = val(mt, nt, r);
}
// Points GEMM  acc[jt][kt] += sum over the 4 KS points of T  A[p][16 jt ..] (x) B[p][16 kt ..], the points ascending into the running
// accumulator: the fragments v[s][t] = T[4 s + kq][t * 16 + li] of a block of points (T points at the block's first row)
template <int KS, int NT>
SF_DEV void fp_point_frags(const float* T, int ld, int li, int kq, float (&v)[KS][NT]) {
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int t = 0; t < NT; ++t) v[s][t] = T[(4 * s + kq) * ld + t * 16 + li];
}
template <int KS, int JT, int KT>
SF_DEV void fp_points_gemm(const float (&av)[KS][JT], const float (&bv)[KS][KT], f32x4 (&acc)[JT][KT]) {
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) acc[jt][kt] = sf_mfma4(av[s][jt], bv[s][kt], acc[jt][kt]);
}

// d(feat) of the trip at point p0, transposed through the F tile into the level-major [L][P][2] image, as k_ngp_field_bwd_mfma: lane =
// (level lane >> 2, quarter lane & 3) owns 8 consecutive points of one level = 64 contiguous bytes
SF_DEV void fp_store_dfeat(const FBArgs& a, const float* F, uint32_t p0, int lane) {
  const uint32_t l = lane >> 2, q0 = (lane & 3) * 8;
  if (l >= a.lv.L) return;
  float* dst = a.dfeat_out + ((size_t)l * a.dfeat_P + a.p_off + p0 + q0) * 2;
  if (p0 + FB_PTS <= a.P && !((a.dfeat_P | a.p_off) & 1)) {      // whole trip, 16-byte aligned rows
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 v;
      v[0] = F[(q0 + 2 * j) * FB_SF + 2 * l];     v[1] = F[(q0 + 2 * j) * FB_SF + 2 * l + 1];
      v[2] = F[(q0 + 2 * j + 1) * FB_SF + 2 * l]; v[3] = F[(q0 + 2 * j + 1) * FB_SF + 2 * l + 1];
      *reinterpret_cast<f32x4*>(dst + 4 * j) = v;
    }
  } else {                                         // ragged last trip (or an odd point count)
    for (int j = 0; j < 8; ++j)
      if (p0 + q0 + j < a.P) { dst[2 * j] = F[(q0 + j) * FB_SF + 2 * l]; dst[2 * j + 1] = F[(q0 + j) * FB_SF + 2 * l + 1]; }
  }
}

// this wave's gradient tiles as fixed-point integer adds: the same addends as k_ngp_field_bwd_mfma's waves
SF_DEV void fp_flush(const FBArgs& a, int lane, const f32x4 (&acc1)[4][4], const f32x4 (&acc0)[4][2], const f32x4 (&acc2)[1][4], const f32x4& accb2,
                     float accb1, float accb0) {
  const int li = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = jt * 16 + 4 * kq + r;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) sf_grad_add(a.g_w1 + j * NGP_HID + kt * 16 + li, a.f_w1 + j * NGP_HID + kt * 16 + li, acc1[jt][kt][r], a.thr);
      sf_grad_add(a.g_w0 + j * NGP_FEAT + li, a.f_w0 + j * NGP_FEAT + li, acc0[jt][0][r], a.thr);
      sf_grad_add(a.g_w0 + j * NGP_FEAT + 16 + li, a.f_w0 + j * NGP_FEAT + 16 + li, acc0[jt][1][r], a.thr);
    }
  if (kq == 0) {
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) sf_grad_add(a.g_w2 + r * NGP_HID + kt * 16 + li, a.f_w2 + r * NGP_HID + kt * 16 + li, acc2[0][kt][r], a.thr);
    if (li == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) sf_grad_add(a.g_b2 + r, a.f_b2 + r, accb2[r], a.thr);
    }
  }
  sf_grad_add(a.g_b1 + lane, a.f_b1 + lane, accb1, a.thr);
  sf_grad_add(a.g_b0 + lane, a.f_b0 + lane, accb0, a.thr);
}

// Requires the field cache (a.feat_c, a.feat_f, a.perm); the re-gather path is k_ngp_field_bwd_mfma's.
SF_KERNEL(256) void k_ngp_field_bwd_pipe(FBArgs a) {
  SF_DYN_LDS(lds_raw);
  float* W = reinterpret_cast<float*>(lds_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* F = W + FB_WTOT + wave * FB_WAVE_FLOATS;    // [32][33] features
  float* H1 = F + FB_PTS * FB_SF;                     // [32][65] h1, later dh1
  float* H2 = H1 + FB_PTS * FB_SH;                    // [32][65] h2, later dh2
  float* DO = H2 + FB_PTS * FB_SH;                    // [32][4]  out, then d(out)
  float* INS = DO + FB_PTS * 4;                       // [32]     1 = point inside the grid and live
  for (int i = tid; i < NGP_HID * NGP_FEAT; i += 256) W[FB_W0 + (i >> 5) * FB_SF + (i & 31)] = a.w0[i];
  for (int i = tid; i < NGP_HID * NGP_HID; i += 256) W[FB_W1 + (i >> 6) * FB_SH + (i & 63)] = a.w1[i];
  for (int i = tid; i < NGP_OUT * NGP_HID; i += 256) W[FB_W2 + i] = a.w2[i];
  if (tid < NGP_HID) { W[FB_B0 + tid] = a.b0[tid]; W[FB_B1 + tid] = a.b1[tid]; }
  if (tid < NGP_OUT) W[FB_B2 + tid] = a.b2[tid];
  float box[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) box[i] = a.aabb[i];
  sf_sync();

  const int li = lane & 15, kq = lane >> 4;            // MFMA fragment coordinates of this lane
  const int pl = lane & 31, half = lane >> 5;          // (point, half) coordinates of phases A and C
  // ---- trip-invariant fragments
#if FP_W1_REGS >= 1
  float bw1[NGP_HID / 4][4];                           // W1^T, the B operand of phase B2
#pragma unroll
  for (int s = 0; s < NGP_HID / 4; ++s)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) bw1[s][nt] = W[FB_W1 + (nt * 16 + li) * FB_SH + 4 * s + kq];
#endif
#if FP_W1_REGS >= 2
  float gw1[NGP_HID / 4][4];                           // W1, the B operand of phase G
#pragma unroll
  for (int s = 0; s < NGP_HID / 4; ++s)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) gw1[s][nt] = W[FB_W1 + (4 * s + kq) * FB_SH + nt * 16 + li];
#endif
  float cw2[NGP_HID / 4], ew2[4], bb0[4], bb1[4];      // W2^T padded to 16 columns (C), W2 (E), b0 / b1 by column tile
#pragma unroll
  for (int s = 0; s < NGP_HID / 4; ++s) {
    const float v = W[FB_W2 + (li & 3) * NGP_HID + 4 * s + kq];
    cw2[s] = li < NGP_OUT ? v : 0.0f;
  }
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    ew2[nt] = W[FB_W2 + kq * NGP_HID + nt * 16 + li];
    bb0[nt] = W[FB_B0 + nt * 16 + li];
    bb1[nt] = W[FB_B1 + nt * 16 + li];
  }
  const float cb2[1] = {li < NGP_OUT ? W[FB_B2 + (li & 3)] : 0.0f};
  const float zero4[4] = {0.0f, 0.0f, 0.0f, 0.0f};

  f32x4 acc1[4][4], acc0[4][2];                        // dW1[jt][kt], dW0[jt][ft] tiles (rows j = jt*16 + 4*kq + r, cols li)
  f32x4 acc2[1][4], accb2 = f32x4{0.f, 0.f, 0.f, 0.f}; // lanes kq == 0: dW2[o = r][k = kt*16 + li]; db2[o = r] (the same in every column)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc1[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc0[i][0] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc0[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc2[0][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float accb1 = 0.0f, accb0 = 0.0f;                    // db1[lane], db0[lane]

  const uint32_t n_trips = (a.P + FB_PTS - 1) / FB_PTS, stride = gridDim.x * 4;
  uint32_t trip = blockIdx.x * 4 + wave;
  // the point of trip t this lane reads: its own where that is a point of the launch, else the launch's last point (masked at use)
#define FP_POINT(t) ((t) < n_trips && (t) * FB_PTS + pl < a.P ? (t) * FB_PTS + pl : a.P - 1)
#if FP_PREFETCH
  FPOps cur;
  uint32_t perm_nxt = 0;
  if (trip < n_trips) {
    const uint32_t pc = FP_POINT(trip);
    fp_load(a, pc, a.perm[a.p_off + pc], half, cur);
    perm_nxt = a.perm[a.p_off + FP_POINT(trip + stride)];
  }
#endif
  for (; trip < n_trips; trip += stride) {
    const uint32_t p0 = trip * FB_PTS;
    const uint32_t p = p0 + pl;
    const bool live = p < a.P;
#if FP_PREFETCH
    FPOps nxt;
    fp_load(a, FP_POINT(trip + stride), perm_nxt, half, nxt);
    const uint32_t perm_nn = a.perm[a.p_off + FP_POINT(trip + 2 * stride)];
#else
    FPOps cur;
    {
      const uint32_t pc = FP_POINT(trip);
      fp_load(a, pc, a.perm[a.p_off + pc], half, cur);
    }
#endif
    // ---- A: position, the cached features into the F tile; lane = (point pl, half)
    float x[3] = {0.f, 0.f, 0.f}, x01[3] = {0.f, 0.f, 0.f};
    bool inside = false;
    if (live) {
      ngp_point(cur.o, cur.d, cur.z, box, x);
      inside = ngp_unit(x, a.bound, x01);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) F[pl * FB_SF + half * 16 + 4 * j + e] = live ? cur.fv[j][e] : 0.0f;
    if (half == 0) INS[pl] = inside ? 1.0f : 0.0f;
    sf_wave_sync();

    f32x4 h1r[2][4], h2r[2][4];                        // relu(h1), relu(h2) in the accumulator layout (rows mt*16 + 4*kq + r, cols nt*16 + li)
    // ---- B1: H1 = relu(F W0^T + b0)
    {
      float av[2][NGP_FEAT / 4], bv[NGP_FEAT / 4][4];
      fp_row_frags(F, FB_SF, li, kq, av);
#pragma unroll
      for (int s = 0; s < NGP_FEAT / 4; ++s)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) bv[s][nt] = W[FB_W0 + (nt * 16 + li) * FB_SF + 4 * s + kq];
      fp_row_fill(h1r, bb0);
      fp_row_gemm(av, [&](int s, int nt) { return bv[s][nt]; }, h1r);
      fp_row_store<4>(H1, FB_SH, li, kq, [&](int mt, int nt, int r) { return h1r[mt][nt][r] = fmaxf(h1r[mt][nt][r], 0.0f); });
    }
    sf_wave_sync();
    // ---- B2: H2 = relu(H1 W1^T + b1)
    {
      float av[2][NGP_HID / 4];
      fp_row_frags(H1, FB_SH, li, kq, av);
      fp_row_fill(h2r, bb1);
#if FP_W1_REGS >= 1
      fp_row_gemm(av, [&](int s, int nt) { return bw1[s][nt]; }, h2r);
#else
      fp_row_gemm(av, [&](int s, int nt) { return W[FB_W1 + (nt * 16 + li) * FB_SH + 4 * s + kq]; }, h2r);
#endif
      fp_row_store<4>(H2, FB_SH, li, kq, [&](int mt, int nt, int r) { return h2r[mt][nt][r] = fmaxf(h2r[mt][nt][r], 0.0f); });
    }
    sf_wave_sync();
    // ---- C: out = H2 W2^T + b2 on the matrix cores (lanes li < 4 hold out[point][o = li]), through DO to lane = (point pl, half),
    // which owns outputs 2*half, 2*half + 1 and turns them into d(out)
    {
      float av[2][NGP_HID / 4];
      fp_row_frags(H2, FB_SH, li, kq, av);
      f32x4 c[2][1];
      fp_row_fill(c, cb2);
      fp_row_gemm(av, [&](int s, int) { return cw2[s]; }, c);
      if (li < NGP_OUT) fp_row_store<1>(DO, 4, li, kq, [&](int mt, int, int r) { return c[mt][0][r]; });
      sf_wave_sync();
      const float o0 = DO[pl * 4 + 2 * half], o1 = DO[pl * 4 + 2 * half + 1];
      float d0 = 0.0f, d1 = 0.0f;
      if (live) {
        if (half == 0) {
          const float pre = o0 + ngp_blob(x);
          d0 = cur.g0 * expf(fminf(fmaxf(pre, -15.0f), 15.0f));               // trunc_exp backward
          const float sg = ngp_sigmoid(o1);
          d1 = cur.g1 * sg * (1.0f - sg);
        } else {
          const float s0 = ngp_sigmoid(o0), s1 = ngp_sigmoid(o1);
          d0 = cur.g0 * s0 * (1.0f - s0);
          d1 = cur.g1 * s1 * (1.0f - s1);
        }
      }
      DO[pl * 4 + 2 * half] = d0;                      // (the two elements only this lane has read)
      DO[pl * 4 + 2 * half + 1] = d1;
    }
    sf_wave_sync();
    // ---- D: dW2[o][k] += sum_p dout[p][o] h2[p][k] (A = dout^T, rows o >= 4 zero; B = h2; K = the 32 points, ascending);  db2
    // ---- E: dh2 = (dout W2) masked by h2 > 0, over h2
    {
      float da[FB_PTS / 4][1], hb[FB_PTS / 4][4], one[FB_PTS / 4][1], ea[2][1];
#pragma unroll
      for (int s = 0; s < FB_PTS / 4; ++s) {
        const float v = DO[(4 * s + kq) * 4 + (li & 3)];
        da[s][0] = li < NGP_OUT ? v : 0.0f;
        one[s][0] = 1.0f;
      }
      fp_point_frags(H2, FB_SH, li, kq, hb);
      fp_row_frags(DO, 4, li, kq, ea);
      f32x4 b[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}};
      fp_points_gemm(da, hb, acc2);
      fp_points_gemm(da, one, b);
#pragma unroll
      for (int r = 0; r < 4; ++r) accb2[r] += b[0][0][r];
      sf_wave_sync();                                    // every lane holds its h2 fragments: dh2 goes over h2
      f32x4 g[2][4];
      fp_row_fill(g, zero4);
      fp_row_gemm(ea, [&](int, int nt) { return ew2[nt]; }, g);
      fp_row_store<4>(H2, FB_SH, li, kq, [&](int mt, int nt, int r) { return h2r[mt][nt][r] > 0.0f ? g[mt][nt][r] : 0.0f; });
    }
    sf_wave_sync();
    // ---- F: dW1[j][k] += sum_p dh2[p][j] h1[p][k]   (A = dh2^T, B = h1; K = the 32 points);  db1[j = lane], points ascending
    {
      float b = 0.0f;
#pragma unroll
      for (int hs = 0; hs < 2; ++hs) {                   // 16 points at a time: 80 fragment registers instead of 160
        float av[FB_PTS / 8][4], bv[FB_PTS / 8][4], col[FB_PTS / 2];
        fp_point_frags(H2 + 16 * hs * FB_SH, FB_SH, li, kq, av);
        fp_point_frags(H1 + 16 * hs * FB_SH, FB_SH, li, kq, bv);
#pragma unroll
        for (int q = 0; q < FB_PTS / 2; ++q) col[q] = H2[(16 * hs + q) * FB_SH + lane];
        fp_points_gemm(av, bv, acc1);
#pragma unroll
        for (int q = 0; q < FB_PTS / 2; ++q) b += col[q];
      }
      accb1 += b;
    }
    // ---- G: dh1 = (dh2 W1) masked by h1 > 0, written over h1 (phase F holds its h1 fragments: wave barrier before the stores)
    {
      float av[2][NGP_HID / 4];
      fp_row_frags(H2, FB_SH, li, kq, av);
      f32x4 c[2][4];
      fp_row_fill(c, zero4);
#if FP_W1_REGS >= 2
      fp_row_gemm(av, [&](int s, int nt) { return gw1[s][nt]; }, c);
#else
      fp_row_gemm(av, [&](int s, int nt) { return W[FB_W1 + (4 * s + kq) * FB_SH + nt * 16 + li]; }, c);
#endif
      sf_wave_sync();
#if FP_H1_REGS
      fp_row_store<4>(H1, FB_SH, li, kq, [&](int mt, int nt, int r) { return h1r[mt][nt][r] > 0.0f ? c[mt][nt][r] : 0.0f; });
#else
      fp_row_store<4>(H1, FB_SH, li, kq, [&](int mt, int nt, int r) { return H1[fp_row_at(FB_SH, li, kq, mt, nt, r)] > 0.0f ? c[mt][nt][r] : 0.0f; });
#endif
    }
    sf_wave_sync();
    // ---- H: dW0[j][f] += sum_p dh1[p][j] feat[p][f];  db0[j = lane], points ascending
    {
      float av[FB_PTS / 4][4], bv[FB_PTS / 4][2], col[FB_PTS];
      fp_point_frags(H1, FB_SH, li, kq, av);
      fp_point_frags(F, FB_SF, li, kq, bv);
#pragma unroll
      for (int q = 0; q < FB_PTS; ++q) col[q] = H1[q * FB_SH + lane];
      fp_points_gemm(av, bv, acc0);
      float b = 0.0f;
#pragma unroll
      for (int q = 0; q < FB_PTS; ++q) b += col[q];
      accb0 += b;
    }
    // ---- I: d(feat) = dh1 W0 -> level-major [L][P][2] (zero for points outside the grid)
    if (a.dfeat_out) {
      float av[2][NGP_HID / 4], bv[NGP_HID / 4][2];
      fp_row_frags(H1, FB_SH, li, kq, av);
      fp_point_frags(W + FB_W0, FB_SF, li, kq, bv);
      f32x4 c[2][2];
      fp_row_fill(c, zero4);
      fp_row_gemm(av, [&](int s, int ft) { return bv[s][ft]; }, c);
      sf_wave_sync();                                    // phase H holds its F fragments
      fp_row_store<2>(F, FB_SF, li, kq, [&](int mt, int ft, int r) { return INS[mt * 16 + 4 * kq + r] != 0.0f ? c[mt][ft][r] : 0.0f; });
      sf_wave_sync();
      fp_store_dfeat(a, F, p0, lane);
    }
    sf_wave_sync();                                      // before the next trip restages F / H1 / H2 / DO / INS
#if FP_PREFETCH
    cur = nxt;
    perm_nxt = perm_nn;
#endif
  }
#undef FP_POINT

  fp_flush(a, lane, acc1, acc0, acc2, accb2, accb1, accb0);
}
